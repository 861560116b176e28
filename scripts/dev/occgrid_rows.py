"""Times of geometry::OccupancyGrid for the cloud of a 640x480 depth frame in the default grid (512^3 voxels of 0.05),
the viewpoint at the camera, each the median of 5 after a warm-up call: insert with max_range -1 and 3.0, the three
extractions and create_from_occupancy_grid.  Prints one line per row, with the number of distinct voxels an insert
updates and the floor it implies (updated voxels x 8 bytes, plus the mark bytes of the x-slabs swept, at 8 TB/s).

    python scripts/dev/occgrid_rows.py [--once]      # --once: one call of each after the warm-up, for a kernel trace
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
    from cupoch_amd import camera, geometry
    n_rep = 1 if "--once" in sys.argv else 5
    W, H, K4 = 640, 480, (525.0, 525.0, 319.5, 239.5)
    pose = small_pose()
    depth = render_depth(W, H, K4, pose, holes=0.02, seed=1)
    K = camera.PinholeCameraIntrinsic(W, H, *K4)
    cloud = geometry.PointCloud.create_from_depth_image(torch.from_numpy(depth).cuda(), K, np.linalg.inv(pose).astype(np.float32),
                                                        depth_scale=1.0, depth_trunc=100.0)
    viewpoint = pose[:3, 3].astype(np.float32)
    pts = cloud.points.tensor
    sync = torch.cuda.synchronize
    print("cloud: %d points, viewpoint %s" % (len(pts), viewpoint), flush=True)
    grid = geometry.OccupancyGrid()
    res = grid.resolution
    for max_range in (-1.0, 3.0):
        grid.clear()
        grid.insert(pts, viewpoint, max_range)
        updated = len(grid.extract_known_voxels())
        lo, hi = grid.min_bound, grid.max_bound
        swept = int(hi[0] - lo[0] + 1) * res * res
        ms = median_ms(lambda: grid.insert(pts, viewpoint, max_range), sync, n_rep)
        print("insert max_range %4.1f        %8.3f ms   %d voxels updated, %d x-slabs swept, floor %.4f ms" %
              (max_range, ms, updated, hi[0] - lo[0] + 1, (updated * 8 + swept) / 8e12 * 1e3), flush=True)
    for name, fn in (("extract_known_voxels", grid.extract_known_voxels), ("extract_free_voxels", grid.extract_free_voxels),
                     ("extract_occupied_voxels", grid.extract_occupied_voxels)):
        ms = median_ms(fn, sync, n_rep)
        print("%-28s %8.3f ms   %d voxels" % (name, ms, len(fn())), flush=True)
    ms = median_ms(lambda: geometry.PointCloud.create_from_occupancy_grid(grid), sync, n_rep)
    print("create_from_occupancy_grid   %8.3f ms   %d points" %
          (ms, len(geometry.PointCloud.create_from_occupancy_grid(grid).points)), flush=True)
    box = (grid.max_bound - grid.min_bound + 1).astype(np.int64)
    print("bounds box %s = %d voxels" % (box, int(box.prod())), flush=True)


if __name__ == "__main__":
    main()
