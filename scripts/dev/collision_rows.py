"""Times of collision.compute_intersection, host wall time, each the median of 5 after a warm-up call:
  a 1M-voxel grid (the bench cloud, 10M points U[0,1)^3, seed 42, at the voxel size of the VoxelDownSample row) against
    the same grid shifted by 0.37 voxel, sorted and through the setter (sorted per call);
  4096 segments that cross a 512^3 occupancy grid (a noisy sphere of 2M points seen from its centre) from face to face;
  1024 mixed primitives (boxes, spheres, capsules) against that grid, and that grid's voxels against them.
Prints one line per row.

    python scripts/dev/collision_rows.py [--once]   # --once: one call of each after the warm-up, for a kernel trace
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
    import collision_exact as ex
    from cupoch_amd import collision, geometry, utility
    n_rep = 1 if "--once" in sys.argv else 5
    sync = torch.cuda.synchronize
    F = np.float32

    n = 10_000_000
    rng = np.random.Generator(np.random.PCG64(42))
    cloud = geometry.PointCloud()
    cloud.points = utility.Vector3fVector(torch.from_numpy(rng.random((n, 3), dtype=F)).cuda())
    vox = 2.154 * float(n) ** (-1.0 / 3.0)
    a = geometry.VoxelGrid.create_from_point_cloud(cloud, vox)
    b = geometry.VoxelGrid(a)
    b.origin = (np.asarray(a.origin, F) + F(0.37 * vox)).astype(F)
    given = geometry.VoxelGrid()
    given.voxel_size, given.origin = a.voxel_size, a.origin
    given.voxels = a.voxels                                   # the setter: not known to be sorted
    del cloud
    res = {}
    ms = median_ms(lambda: res.__setitem__("vv", collision.compute_intersection(a, b)), sync, n_rep)
    ms_given = median_ms(lambda: collision.compute_intersection(given, b), sync, n_rep)
    # more than 65536 pairs: the two calls above compute the query twice (the count, then the pairs); with room given once
    ms_room = median_ms(lambda: collision.compute_intersection(a, b, first_capacity=len(b)), sync, n_rep)
    ms_given_room = median_ms(lambda: collision.compute_intersection(given, b, first_capacity=len(b)), sync, n_rep)
    print("voxels x voxels                    %8.3f ms   %d against %d voxels -> %d pairs (target through the setter: %.3f ms); "
          "with first_capacity = the enumerated count, one compute: %.3f ms (setter: %.3f ms)" %
          (ms, len(a), len(b), len(res["vv"].collision_index_pairs), ms_given, ms_room, ms_given_room), flush=True)
    del a, b, given

    rng = np.random.default_rng(7)
    vs, resolution = 0.02, 512
    half = vs * resolution / 2
    g = geometry.OccupancyGrid(vs, resolution)
    d = rng.normal(size=(2_000_000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    g.insert((d * (0.6 * half + rng.normal(size=(len(d), 1)) * 0.05)).astype(F), np.full(3, 0.001, F))
    occupied = len(g.extract_occupied_voxels())

    def on_faces(m):
        p = rng.uniform(-half, half, (m, 3))
        ax = rng.integers(0, 3, m)
        p[np.arange(m), ax] = rng.choice([-half, half], m)
        return p
    pts = np.concatenate([on_faces(4096), on_faces(4096)]).astype(F)
    pts[4096:] = np.where(np.abs(pts[:4096]) == F(half), -pts[:4096], pts[4096:])      # the other end on the opposite face
    ls = geometry.LineSet(pts, np.stack([np.arange(4096), np.arange(4096) + 4096], axis=1).astype(np.int32))
    ms = median_ms(lambda: res.__setitem__("ol", collision.compute_intersection(g, ls)), sync, n_rep)
    print("occupancy grid x 4096 segments     %8.3f ms   %d^3 grid, %d occupied -> %d pairs" %
          (ms, resolution, occupied, len(res["ol"].collision_index_pairs)), flush=True)

    prims = [p for p in ex.mixed_primitives(rng, 1100, np.full(3, -half), np.full(3, half)) if ex.primitive_live(p)][8:1032]
    arr = collision.PrimitiveArray()
    for P in prims:
        arr.append(collision.Box(P.param, P.transform) if P.type == ex.BOX else
                   collision.Sphere(P.param[0], P.transform[:3, 3]) if P.type == ex.SPHERE else
                   collision.Capsule(P.param[0], P.param[1], P.transform))
    ms = median_ms(lambda: res.__setitem__("op", collision.compute_intersection(g, arr)), sync, n_rep)
    ms_rev = median_ms(lambda: res.__setitem__("po", collision.compute_intersection(arr, g)), sync, n_rep)
    print("occupancy grid x %d primitives   %8.3f ms   -> %d pairs; primitives x grid (per occupied voxel) %.3f ms -> %d pairs" %
          (len(arr), ms, len(res["op"].collision_index_pairs), ms_rev, len(res["po"].collision_index_pairs)), flush=True)


if __name__ == "__main__":
    main()
