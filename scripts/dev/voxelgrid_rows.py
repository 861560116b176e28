"""Times of geometry::VoxelGrid, host wall time, each the median of 5 after a warm-up call:
  create_from_point_cloud of the bench cloud (10M points U[0,1)^3, seed 42) with colours at the voxel size of the
    VoxelDownSample row (2.154 n^(-1/3)), beside voxel_down_sample with colours on the same cloud and voxel size;
  carve_depth_map of a 256^3 dense grid with a 640x480 image, beside its byte floor (24 B read + up to 24 B written
    per voxel at 8 TB/s);
  check_if_included of 1M queries against a 1M-voxel grid, sorted and through the setter (sorted per call);
  create_from_occupancy_grid on the scene of scripts/dev/occgrid_rows.py.
Prints one line per row.

    python scripts/dev/voxelgrid_rows.py [--once] [--points N]   # --once: one call of each after the warm-up, for a kernel trace
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(fn, sync, n=5):
    fn()
    sync()
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def main():
    import torch
    from conftest import render_depth, small_pose
    from cupoch_amd import camera, geometry, utility
    n_rep = 1 if "--once" in sys.argv else 5
    n = int(sys.argv[sys.argv.index("--points") + 1]) if "--points" in sys.argv else 10_000_000
    sync = torch.cuda.synchronize
    F = np.float32

    rng = np.random.Generator(np.random.PCG64(42))
    pts = torch.from_numpy(rng.random((n, 3), dtype=F)).cuda()
    col = torch.from_numpy(np.random.Generator(np.random.PCG64(45)).random((n, 3), dtype=F)).cuda()
    cloud = geometry.PointCloud()
    cloud.points, cloud.colors = utility.Vector3fVector(pts), utility.Vector3fVector(col)
    vox = 2.154 * float(n) ** (-1.0 / 3.0)
    ms_down = median_ms(lambda: cloud.voxel_down_sample(vox), sync, n_rep)
    ms_grid = median_ms(lambda: geometry.VoxelGrid.create_from_point_cloud(cloud, vox), sync, n_rep)
    lo, hi = cloud.get_min_bound() - F(vox) * F(0.5), cloud.get_max_bound() + F(vox) * F(0.5)
    ms_within = median_ms(lambda: geometry.VoxelGrid.create_from_point_cloud_within_bounds(cloud, vox, lo, hi), sync, n_rep)
    g = geometry.VoxelGrid.create_from_point_cloud(cloud, vox)
    print("voxel_down_sample (colours)        %8.3f ms   %d points, voxel %.4g -> %d points" %
          (ms_down, n, vox, len(cloud.voxel_down_sample(vox).points)), flush=True)
    print("create_from_point_cloud            %8.3f ms   -> %d voxels (%.2fx; within given bounds %.3f ms)" %
          (ms_grid, len(g), ms_grid / ms_down, ms_within), flush=True)
    del cloud, pts, col, g

    side = 256
    dense = geometry.VoxelGrid.create_dense((0, 0, 0), 1.0 / side, 1.0, 1.0, 1.0)
    W, H, K4 = 640, 480, (525.0, 525.0, 319.5, 239.5)
    depth = np.full((H, W), 2.0, F) + (np.arange(W, dtype=F)[None, :] - 320) * F(0.0015)
    E = np.eye(4, dtype=F)
    E[:3, 3] = (-0.5, -0.5, 1.5)
    cam = camera.PinholeCameraParameters(camera.PinholeCameraIntrinsic(W, H, *K4), E)
    img = geometry.Image(torch.from_numpy(depth).cuda())
    kept = len(geometry.VoxelGrid(dense).carve_depth_map(img, cam))
    copy_ms = median_ms(lambda: geometry.VoxelGrid(dense), sync, n_rep)
    ms = median_ms(lambda: geometry.VoxelGrid(dense).carve_depth_map(img, cam), sync, n_rep)
    m = len(dense)
    print("carve_depth_map 256^3, 640x480     %8.3f ms   %d of %d voxels stay; floor %.4f ms (the copy it carves: %.3f ms of it)" %
          (ms, kept, m, (m * 24 + kept * 24) / 8e12 * 1e3, copy_ms), flush=True)
    del dense

    keys = np.stack(np.unravel_index(np.random.default_rng(1).permutation(128 ** 3)[:1_000_000], (128,) * 3), axis=1).astype(np.int32)
    keys = keys[np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))]
    q = torch.from_numpy(np.random.default_rng(2).random((1_000_000, 3), dtype=F)).cuda()
    g = geometry.VoxelGrid()
    g.voxel_size, g.origin = 1.0 / 128, np.zeros(3, F)
    g.voxels = (keys, np.ones((len(keys), 3), F))
    eng = g._eng()
    ms_unsorted = median_ms(lambda: eng.voxelgrid_query(g._keys, g.voxel_size, g.origin, q, keys_sorted=False), sync, n_rep)
    ms_sorted = median_ms(lambda: eng.voxelgrid_query(g._keys, g.voxel_size, g.origin, q, keys_sorted=True), sync, n_rep)
    hits = int(eng.voxelgrid_query(g._keys, g.voxel_size, g.origin, q, keys_sorted=True)[0].sum())
    print("check_if_included 1M in 1M voxels  %8.3f ms   sorted keys (%d included); %.3f ms when the keys are sorted first" %
          (ms_sorted, hits, ms_unsorted), flush=True)

    W, H, K4 = 640, 480, (525.0, 525.0, 319.5, 239.5)
    pose = small_pose()
    depth = render_depth(W, H, K4, pose, holes=0.02, seed=1)
    K = camera.PinholeCameraIntrinsic(W, H, *K4)
    scan = geometry.PointCloud.create_from_depth_image(torch.from_numpy(depth).cuda(), K, np.linalg.inv(pose).astype(F),
                                                       depth_scale=1.0, depth_trunc=100.0)
    occ = geometry.OccupancyGrid()
    occ.insert(scan.points.tensor, pose[:3, 3].astype(F), -1.0)
    ms = median_ms(lambda: geometry.VoxelGrid.create_from_occupancy_grid(occ), sync, n_rep)
    print("create_from_occupancy_grid         %8.3f ms   %d voxels" % (ms, len(geometry.VoxelGrid.create_from_occupancy_grid(occ))), flush=True)


if __name__ == "__main__":
    main()
