"""Times of geometry.Graph and planning.Pos3DPlanner, host wall time, each the median of 5 after a first call:
  dijkstra_paths on the 10x20x5 lattice of the reference's examples (the small regime: one launch);
  dijkstra_paths on a 128^3 lattice (the large regime), with its launches, host waits and rounds;
  find_path on the 10x20x5 lattice against a 128^3 VoxelGrid, split into collide, construct and search;
  scipy.sparse.csgraph.dijkstra on the host for the same graphs, as context only.
Prints one line per row.

    python scripts/dev/graph_rows.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


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


def scipy_ms(g, once=False):
    try:
        from scipy.sparse import csr_matrix
        from scipy.sparse.csgraph import dijkstra
    except Exception:
        return float("nan")
    l, w = g.edges.tensor.cpu().numpy(), g.edge_weights.cpu().numpy().astype(np.float64)
    n = len(g.points)
    mat = csr_matrix((w, (l[:, 0], l[:, 1])), shape=(n, n))
    if once:                                                  # (a large graph: one call, no warm-up)
        t0 = time.perf_counter()
        dijkstra(mat, directed=True, indices=0)
        return (time.perf_counter() - t0) * 1e3
    return median_ms(lambda: dijkstra(mat, directed=True, indices=0), lambda: None, 3)


def main():
    import torch
    from cupoch_amd import collision, geometry, planning
    sync = torch.cuda.synchronize
    F = np.float32
    res = {}

    small = geometry.Graph.create_from_axis_aligned_bounding_box((-1, -2, -0.5), (1, 2, 0.5), (10, 20, 5))
    ms = median_ms(lambda: res.__setitem__("s", small.dijkstra_paths(0, want_info=True)), sync)
    info = res["s"][2]
    print("dijkstra_paths 10x20x5             %8.3f ms   %d nodes, %d edges; regime %d, %d launch(es), %d wait(s), %d rounds; "
          "scipy on the host %.3f ms" % (ms, len(small.points), len(small.edges), info[0], info[1], info[2], info[3], scipy_ms(small)),
          flush=True)

    ms_make = median_ms(lambda: res.__setitem__("g", geometry.Graph.create_from_axis_aligned_bounding_box((0, 0, 0), (1, 1, 1), (128, 128, 128))), sync, 3)
    big = res["g"]
    ms = median_ms(lambda: res.__setitem__("b", big.dijkstra_paths(0, want_info=True)), sync)
    info = res["b"][2]
    ms_end = median_ms(lambda: res.__setitem__("e", big.dijkstra_paths(0, 128 * 128 * 20, want_info=True)), sync)
    print("dijkstra_paths 128^3               %8.3f ms   %d nodes, %d edges (lattice made in %.3f ms); regime %d, %d launches, %d waits, "
          "%d rounds; with an end 20 layers away %.3f ms (%d launches); scipy on the host %.1f ms" %
          (ms, len(big.points), len(big.edges), ms_make, info[0], info[1], info[2], info[3], ms_end, res["e"][2][1], scipy_ms(big, once=True)),
          flush=True)
    del big, res["g"], res["b"], res["e"]

    # a 128^3 VoxelGrid: a thick shell of cells around the roadmap's middle, open along one axis
    k = np.stack(np.meshgrid(*[np.arange(-64, 64)] * 3, indexing="ij"), axis=-1).reshape(-1, 3)
    r = np.linalg.norm((k + 0.5) * np.array([1.0, 0.5, 2.0]), axis=1)
    keys = k[(r > 20) & (r < 26) & (np.abs(k[:, 2]) > 8)].astype(np.int32)
    wall = geometry.VoxelGrid()
    wall.voxel_size, wall.origin = 1.0 / 32, np.zeros(3, F)
    wall.add_voxels((keys, np.ones((len(keys), 3), F)))
    planner = planning.Pos3DPlanner(small, 0.05, 0.5).add_obstacle(wall)
    start, goal = (-0.95, -1.9, -0.4), (0.05, 0.1, 0.0)
    ms = median_ms(lambda: res.__setitem__("p", planner.find_path(start, goal)), sync)
    g = geometry.Graph(small)
    g.add_node_and_connect(start, 0.5, True)
    ms_construct = median_ms(lambda: geometry.Graph(g).add_node_and_connect(goal, 0.5, False), sync)
    g.add_node_and_connect(goal, 0.5, False)
    ms_collide = median_ms(lambda: res.__setitem__("c", collision.compute_intersection(wall, g, 0.05, first_capacity=len(g.edges))), sync)
    planner._remove_collision_edges(g)
    n = len(small.points)
    ms_search = median_ms(lambda: g.dijkstra_path(n, n + 1), sync)
    print("find_path 10x20x5 vs 128^3 grid    %8.3f ms   %d voxels, %d of %d edges collide, path of %d points; copy + two nodes + construct "
          "%.3f ms, collide %.3f ms, search with the path read back %.3f ms" %
          (ms, len(keys), len(res["c"].collision_index_pairs), len(g.edges), len(res["p"]), ms_construct, ms_collide, ms_search), flush=True)


if __name__ == "__main__":
    main()
