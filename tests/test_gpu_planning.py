"""planning.Pos3DPlanner on the GPU against the restatement of find_path (tests/graph_exact.py, segments by
tests/collision_exact.py): a 10x10x10 roadmap over [-1, 1]^3, a wall at x in [0, 0.1] with one 0.5-wide window, as a
VoxelGrid and as an OccupancyGrid.  The path equals the restatement's point for point, collides nowhere, and is empty
when the window is closed."""
import numpy as np
import pytest

import graph_exact as gx

pytestmark = pytest.mark.gpu
F = np.float32
VS, RES = 0.1, 32
RADIUS, REACH = 0.1, 0.45
START, GOAL = (-0.9, -0.5, -0.2), (0.75, 0.62, 0.33)


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def wall_keys(window):
    """the cells of the plane x = [0, 0.1] over [-1, 1]^2, without the 5 x 5 cells y, z in [-0.2, 0.3] when `window`"""
    y, z = np.meshgrid(np.arange(-10, 10), np.arange(-10, 10), indexing="ij")
    keys = np.stack([np.zeros_like(y), y, z], axis=-1).reshape(-1, 3)
    if window:
        keys = keys[~((np.abs(keys[:, 1]) <= 2) & (np.abs(keys[:, 2]) <= 2))]
    return np.ascontiguousarray(keys, np.int32)


@pytest.fixture(scope="module")
def roadmap():
    from cupoch_amd import geometry
    g = geometry.Graph.create_from_axis_aligned_bounding_box((-1, -1, -1), (1, 1, 1), (10, 10, 10))
    pts, lines, w, off = gx.lattice((-1, -1, -1), (1, 1, 1), (10, 10, 10))
    assert to_np(g.points.tensor).tobytes() == pts.tobytes() and np.array_equal(to_np(g.edges.tensor), lines)
    return g, pts, lines


def voxel_obstacle(keys):
    from cupoch_amd import geometry
    v = geometry.VoxelGrid()
    v.voxel_size, v.origin = VS, np.zeros(3, F)
    v.add_voxels((keys, np.ones((len(keys), 3), F)))
    return v, ("voxel", to_np(v.voxels.grid_index), VS, np.zeros(3, F))


def occ_obstacle(keys):
    from cupoch_amd import geometry
    o = geometry.OccupancyGrid(VS, RES, (0.0, 0.0, 0.0))
    o.add_voxels(keys + RES // 2, True)
    idx = to_np(o.extract_occupied_voxels().grid_index)
    assert len(idx) == len(keys)
    return o, ("occ", idx, RES, VS, np.zeros(3, F))


@pytest.fixture(scope="module")
def expected(roadmap):
    """the restatement's answers, computed once: {window: (path, lines, weights)} -- the two obstacle kinds hold the same cells"""
    _, pts, lines = roadmap
    out = {}
    for window in (True, False):
        side = ("voxel", wall_keys(window), VS, np.zeros(3, F))
        out[window] = gx.find_path(pts, lines, START, GOAL, [side], RADIUS, REACH)
    return out


@pytest.mark.parametrize("kind", ["voxel", "occ"])
def test_path_through_the_window_equals_the_restatement(roadmap, expected, kind):
    from cupoch_amd import collision, geometry, planning
    g, pts, lines = roadmap
    make = voxel_obstacle if kind == "voxel" else occ_obstacle
    wall, side = make(wall_keys(True))
    want, _, _ = gx.find_path(pts, lines, START, GOAL, [side], RADIUS, REACH) if kind == "occ" else expected[True]
    assert np.array_equal(want, expected[True][0])
    planner = planning.Pos3DPlanner(g, RADIUS, REACH)
    planner.add_obstacle(wall)
    path = planner.find_path(START, GOAL)
    assert path.dtype == F and path.shape == want.shape and len(path) >= 4
    assert path.tobytes() == want.tobytes()
    assert np.array_equal(path[0], np.array(START, F)) and np.array_equal(path[-1], np.array(GOAL, F))
    assert (path[:, 0] < 0).any() and (path[:, 0] > 0.1).any()                      # it crosses the wall's plane ...
    k = len(path)
    segs = geometry.LineSet(path, np.stack([np.arange(k - 1), np.arange(1, k)], 1).astype(np.int32))
    assert not collision.compute_intersection(wall, segs, RADIUS).is_collided()     # ... and touches nothing
    crossing = path[(path[:, 0] >= -0.2) & (path[:, 0] <= 0.3)]
    assert (np.abs(crossing[:, 1:]) < 0.3).all()                                    # through the window
    assert len(g.points) == 1000 and len(planner.get_graph().points) == 1000        # the planner's graph is untouched
    closed, _ = make(wall_keys(False))
    planner2 = planning.Pos3DPlanner(g, RADIUS, REACH).add_obstacle(closed)
    none = planner2.find_path(START, GOAL)
    assert none.shape == (0, 3) and none.dtype == F and expected[False][0].shape == (0, 3)


def test_without_obstacles_and_with_the_reference_unit_test_arguments(roadmap):
    from cupoch_amd import planning
    g, pts, lines = roadmap
    planner = planning.Pos3DPlanner(g)
    assert planner.object_radius == 0.1 and planner.max_edge_distance == 1.0
    start, goal = (-1.0, -0.5, -0.2), (0.8, 0.9, 0.7)                               # src/tests/planning/planner.cpp
    path = planner.find_path(start, goal)
    want, _, _ = gx.find_path(pts, lines, start, goal, [], 0.1, 1.0)
    assert path.tobytes() == want.tobytes() and len(path) >= 3
    a, b = (0.07, 0.03, 0.01), (0.31, 0.12, -0.05)                                   # goal within reach of the start, off the lattice: one hop
    near = planner.find_path(a, b)
    assert near.shape == (2, 3) and near.tobytes() == gx.find_path(pts, lines, a, b, [], 0.1, 1.0)[0].tobytes()
    far = planning.Pos3DPlanner(g, 0.1, 0.05).find_path((5.0, 5.0, 5.0), goal)        # nothing within reach
    assert far.shape == (0, 3)


def test_update_graph_keeps_both_directions_equal(roadmap):
    from cupoch_amd import planning
    g, pts, lines = roadmap
    wall, side = voxel_obstacle(wall_keys(True))
    planner = planning.Pos3DPlanner(g, RADIUS, REACH).add_obstacle(wall)
    assert planner.update_graph() is planner
    got = planner.get_graph()
    w = to_np(got.edge_weights)
    l = to_np(got.edges.tensor)
    assert np.array_equal(l, lines)
    import collision_exact as cx
    pairs = cx.compute_intersection(side, ("lines", pts, lines), RADIUS)
    want = gx.set_edge_weights(lines, gx.weights_from_distance(pts, lines), lines[pairs[:, 1]], np.inf, True)
    assert w.tobytes() == want.tobytes() and 0 < np.isinf(w).sum() < len(w)
    n = len(pts)
    key = l[:, 0].astype(np.int64) * n + l[:, 1]
    rev = l[:, 1].astype(np.int64) * n + l[:, 0]
    pos = np.searchsorted(key, rev)
    assert np.array_equal(key[pos], rev)                      # every edge has its reverse ...
    assert w[pos].tobytes() == w.tobytes()                    # ... at the same weight: the predicate is symmetric in the end points
    assert np.isfinite(to_np(g.edge_weights)).all()           # the caller's graph is a copy apart


def test_unsupported_obstacle_is_logged_not_fatal(roadmap, capfd):
    from cupoch_amd import geometry, planning
    g, pts, lines = roadmap
    planner = planning.Pos3DPlanner(g, RADIUS, REACH)
    planner.add_obstacle(geometry.PointCloud(np.zeros((3, 3), F)))
    path = planner.find_path(START, GOAL)
    assert "Unsupported obstacle type." in capfd.readouterr().err
    want, _, _ = gx.find_path(pts, lines, START, GOAL, [], RADIUS, REACH)
    assert path.tobytes() == want.tobytes() and len(path) >= 3
