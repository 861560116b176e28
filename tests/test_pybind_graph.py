"""geometry.Graph and the planning submodule of the reference's pybind11 module (cupoch_amd/cpp/src/pybind_module.cpp)
with the reference's Python names and defaults: names on the CPU, and on the GPU the five-node graph, the zero-weight
trap and the wall with a window, exactly as the numpy restatement has them (tests/graph_exact.py).  Skips only where
there is nothing to build the module with."""
import re

import numpy as np
import pytest

import graph_exact as gx

F = np.float32


def module():
    import importlib.util
    import shutil
    missing = [n for n in ("make", "g++") if shutil.which(n) is None] + ([] if importlib.util.find_spec("pybind11") else ["pybind11"])
    if missing:                 # nothing to build the module with: the only reason to skip
        pytest.skip("cupoch_pybind cannot be built here: no %s" % ", ".join(missing))
    from cupoch_amd import pybind as cph        # (a build or an import that breaks is a failure)
    return cph


def test_graph_and_planning_rows_have_the_references_names():
    cph = module()
    G = cph.geometry.Graph
    assert issubclass(G, cph.geometry.LineSet)
    for name in ("edges", "edge_weights", "edge_index_offsets", "node_colors", "is_directed", "has_weights", "has_node_colors",
                 "is_constructed", "construct_graph", "connect_to_nearest_neighbors", "add_node_and_connect", "add_edge", "add_edges",
                 "remove_edge", "remove_edges", "paint_edge_color", "paint_edges_color", "paint_node_color", "paint_nodes_color",
                 "set_edge_weights_from_distance", "set_edge_weights", "dijkstra_paths", "dijkstra_path", "to_edges_dlpack",
                 "from_edges_dlpack", "create_from_axis_aligned_bounding_box", "points", "lines"):
        assert hasattr(G, name), name
    assert not hasattr(G, "create_from_triangle_mesh") and not hasattr(cph.geometry, "Graph2D")
    def default(fn, name, value):            # "name: <the type, as this pybind11 spells it> = value"
        return re.search(r"\b%s: [^,)]*= %s[,)]" % (name, re.escape(value)), fn.__doc__) is not None
    assert default(G.construct_graph, "set_edge_weights_from_distance", "True")
    assert default(G.connect_to_nearest_neighbors, "max_num_edges", "30")
    assert default(G.add_node_and_connect, "max_edge_distance", "0.0") and default(G.add_node_and_connect, "lazy_add", "False")
    assert default(G.add_edge, "weight", "1.0") and default(G.dijkstra_paths, "end_node_index", "-1")
    P = cph.planning.Pos3DPlanner
    for name in ("add_obstacle", "update_graph", "find_path", "get_graph", "object_radius", "max_edge_distance"):
        assert hasattr(P, name), name
    assert default(P.__init__, "object_radius", "0.1") and default(P.__init__, "max_edge_distance", "1.0")


@pytest.mark.gpu
def test_five_nodes_trap_and_dlpack():
    cph = module()
    import torch
    g = cph.geometry.Graph(np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [2, 2, 0]], F))
    assert not g.is_directed and not g.is_constructed()
    for e, w in (((0, 1), 1.0), ((0, 2), 2.0), ((1, 3), 1.0), ((2, 3), 1.0), ((3, 4), 1.0)):
        g.add_edge(np.array(e, np.int32), w)
    n, lines, w, start = gx.small_cases()["five"]
    assert np.array_equal(np.asarray(g.edges.cpu()), lines) and list(g.edge_index_offsets) == [0, 2, 4, 6, 9, 10]
    assert np.array_equal(np.asarray(g.edge_weights), w) and g.is_constructed() and g.has_weights()
    dist, prev = g.dijkstra_paths(0)
    want = gx.sssp(lines, w, n, 0)
    assert dist.tobytes() == want[0].tobytes() and np.array_equal(prev, want[1])
    assert g.dijkstra_path(0, 4) == ([0, 1, 3, 4], 3.0) and g.dijkstra_path(2, 2) == ([2], 0.0)
    d3, p3 = g.dijkstra_paths(0, 3)
    want = gx.sssp(lines, w, n, 0, 3)
    assert d3.tobytes() == want[0].tobytes() and np.array_equal(p3, want[1])
    t = torch.from_dlpack(g.to_edges_dlpack())
    assert t.dtype == torch.int32 and t.is_cuda and np.array_equal(t.cpu().numpy(), lines)
    n, lines, w, start = gx.small_cases()["zero_pair_trap"]
    trap = cph.geometry.Graph(np.zeros((n, 3), F))
    trap.is_directed = True
    trap.from_edges_dlpack(torch.from_numpy(lines).cuda().__dlpack__())
    assert not trap.is_constructed() and np.array_equal(np.asarray(trap.edges.cpu()), lines)
    trap.edge_weights = w
    trap.construct_graph(False)
    dist, prev = trap.dijkstra_paths(start)
    want = gx.sssp(lines, w, n, start)
    assert dist.tobytes() == want[0].tobytes() and prev.tolist() == want[1].tolist() == [3, 3, 1, 3]
    assert trap.dijkstra_path(0, 3) == ([], float("inf"))
    trap.remove_edges(cph.utility.Vector2iVector(np.array([[3, 0]], np.int32)))
    assert np.array_equal(np.asarray(trap.edges.cpu()), gx.remove_edges(lines, n, [[3, 0]], True)[0])


@pytest.mark.gpu
def test_wall_with_a_window():
    cph = module()
    from test_gpu_planning import GOAL, RADIUS, REACH, START, VS, wall_keys
    pts, lat, _, off = gx.lattice((-1, -1, -1), (1, 1, 1), (10, 10, 10))
    g = cph.geometry.Graph.create_from_axis_aligned_bounding_box(np.array([-1, -1, -1], F), np.array([1, 1, 1], F), np.array([10, 10, 10], np.int32))
    assert np.asarray(g.points.cpu()).tobytes() == pts.tobytes() and np.array_equal(np.asarray(g.edges.cpu()), lat)
    assert np.array_equal(np.asarray(g.edge_index_offsets), off)

    def wall(window):
        v = cph.geometry.VoxelGrid()
        v.voxel_size, v.origin = VS, np.zeros(3, F)
        v.add_voxels([cph.geometry.Voxel(k) for k in wall_keys(window)])
        return v
    planner = cph.planning.Pos3DPlanner(g, RADIUS, REACH).add_obstacle(wall(True))
    path = planner.find_path(np.array(START, F), np.array(GOAL, F))
    want, _, _ = gx.find_path(pts, lat, START, GOAL, [("voxel", wall_keys(True), VS, np.zeros(3, F))], RADIUS, REACH)
    assert path.dtype == F and path.tobytes() == want.tobytes() and len(path) >= 4
    shut = cph.planning.Pos3DPlanner(g, RADIUS, REACH).add_obstacle(wall(False))
    assert shut.find_path(np.array(START, F), np.array(GOAL, F)).shape == (0, 3)
    w = np.asarray(planner.update_graph().get_graph().edge_weights)
    assert 0 < np.isinf(w).sum() < len(w) and np.isfinite(np.asarray(g.edge_weights)).all()
    free = cph.planning.Pos3DPlanner(g)
    assert (free.object_radius, free.max_edge_distance) == (pytest.approx(0.1), 1.0)
    far = free.find_path(np.array([-1.0, -0.5, -0.2], F), np.array([0.8, 0.9, 0.7], F))      # src/tests/planning/planner.cpp
    assert far.tobytes() == gx.find_path(pts, lat, (-1.0, -0.5, -0.2), (0.8, 0.9, 0.7), [], 0.1, 1.0)[0].tobytes()
