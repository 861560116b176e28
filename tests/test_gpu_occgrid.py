"""geometry::OccupancyGrid on the GPU against the numpy fp32 restatement of its contract (tests/occgrid_exact.py): the
reference's four unit tests at the default 512^3 (through queries and counts only), then after every call of every scene
the whole log-odds plane, the bounds, the three extractions and the occupied cloud bit for bit; determinism, two grids on
one context, a registration in between, and the error returns."""
import ctypes as C

import numpy as np
import pytest

import occgrid_exact as ox

pytestmark = pytest.mark.gpu
F = np.float32


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def same(a, b):
    """bit-equal arrays of float32, NaN positions included"""
    a, b = np.ascontiguousarray(to_np(a), F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def gpu_grid(res):
    from cupoch_amd import geometry
    return geometry.OccupancyGrid(ox.VOXEL, res, ox.ORIGINS[res])


def apply(grid, op):
    if op[0] == "insert":
        grid.insert(op[1], op[2], op[3])
    elif op[0] == "free":
        grid.set_free_area(op[1], op[2])
    elif op[0] == "add":
        grid.add_voxels(op[1], op[2])
    else:
        for k, v in op[1].items():
            setattr(grid, k, v)


def check(grid, ref):
    """plane, bounds, the three extractions (count, order, indices, values) and the occupied cloud"""
    from cupoch_amd import geometry
    got = to_np(grid.get_voxels())
    assert same(got, ref.prob), "the plane differs at %d voxels" % int((got.view(np.uint32) != ref.prob.view(np.uint32)).sum())
    assert np.array_equal(grid.min_bound, ref.min_bound) and np.array_equal(grid.max_bound, ref.max_bound)
    assert same(grid.get_min_bound(), ox.get_min_bound(ref)) and same(grid.get_max_bound(), ox.get_max_bound(ref))
    for which, fn in ((ox.KNOWN, grid.extract_known_voxels), (ox.FREE, grid.extract_free_voxels),
                      (ox.OCCUPIED, grid.extract_occupied_voxels)):
        ijk, p, _ = ox.extract(ref, which)
        gi, gp = fn().cpu()
        assert gi.shape == ijk.shape and np.array_equal(gi, ijk) and same(gp, p)
    ijk, p, pts = ox.extract(ref, ox.OCCUPIED)
    cloud = geometry.PointCloud.create_from_occupancy_grid(grid)
    assert len(cloud.points) == len(pts) and same(cloud.points.tensor, pts)
    col = to_np(cloud.colors.tensor)
    assert col.shape == pts.shape and (col == np.array([0, 0, 1], F)).all()
    assert repr(grid) == "geometry::OccupancyGrid with %d voxels." % len(ox.extract(ref, ox.KNOWN)[0])


# ---- the reference's four unit tests (src/tests/geometry/occupancygrid.cpp) at the default 512^3 ------------------------
@pytest.fixture(scope="module")
def grid512():
    from cupoch_amd import geometry
    g = geometry.OccupancyGrid()
    yield g
    del g


def fresh(g):
    g.clear()
    g.voxel_size, g.origin = 0.05, np.zeros(3, F)
    return g


def test_reference_bounds(grid512):
    g = fresh(grid512)
    assert F(g.voxel_size) == F(0.05) and g.resolution == 512
    g.voxel_size = 5.0
    g.add_voxel([0, 0, 0])
    g.add_voxel([511, 511, 511])
    assert np.array_equal(g.get_min_bound(), np.full(3, -1280.0, F))
    assert np.array_equal(g.get_max_bound(), np.full(3, 1280.0, F))
    assert np.array_equal(g.get_center(), np.zeros(3, F))


def test_reference_get_voxel(grid512):
    g = fresh(grid512)
    g.voxel_size = 1.0
    h = 256
    want = F(0.0)
    for occupied in (True, True, False):
        g.add_voxel([h + 1, h, h], occupied)
        want = F(want + (F(0.85) if occupied else F(-0.4)))
        known, v = g.get_voxel([1.5, 0.0, 0.0])
        assert known and F(v.prob_log) == want and tuple(v.grid_index) == (h + 1, h, h)
        assert tuple(v.color) == (0.0, 0.0, 1.0)
    assert g.is_occupied([1.5, 0, 0]) and not g.is_unknown([1.5, 0, 0]) and g.is_unknown([2.5, 0, 0])
    # outside the grid on ONE axis: unknown (the linear index alone would alias into another voxel)
    assert g.is_unknown([1.5, 256.5, 0.0]) and not g.get_voxel([1.5, -300.0, 0.0])[0]
    out = to_np(g.get_prob_log(np.array([[1.5, 0, 0], [2.5, 0, 0], [1.5, 256.5, 0], [np.nan, 0, 0]], F)))
    assert F(out[0]) == want and np.isnan(out[1:]).all()


def test_reference_insert(grid512):
    g = fresh(grid512)
    g.origin, g.voxel_size = np.array([-0.5, -0.5, 0.0], F), 1.0
    g.insert(np.array([[0.0, 0.0, 3.5]], F), np.zeros(3, F))
    assert len(g.extract_known_voxels()) == 4 and repr(g) == "geometry::OccupancyGrid with 4 voxels."
    for z in (0.5, 1.5, 2.5, 3.5):
        assert g.get_voxel([0.0, 0.0, z])[0]
    assert not g.get_voxel([0.0, 0.0, 4.5])[0]
    assert len(g.extract_free_voxels()) == 3 and len(g.extract_occupied_voxels()) == 1
    assert g.is_occupied([0, 0, 3.5]) and not g.is_occupied([0, 0, 2.5])
    ref = ox.Grid(1.0, 512, (-0.5, -0.5, 0.0), dense=False)
    ox.insert(ref, [[0.0, 0.0, 3.5]], [0, 0, 0])
    ijk, p, _ = ox.extract(ref, ox.KNOWN)
    gi, gp = g.voxels.cpu()
    assert np.array_equal(gi, ijk) and same(gp, p)
    assert np.array_equal(g.min_bound, ref.min_bound) and np.array_equal(g.max_bound, ref.max_bound)


def test_reference_set_free_area(grid512):
    g = fresh(grid512)
    g.set_free_area([0, 0, 0], [0.1, 0.1, 0.1])
    assert len(g.extract_free_voxels()) == 27 and len(g.extract_occupied_voxels()) == 0
    ref = ox.Grid(dense=False)
    ox.set_free_area(ref, [0, 0, 0], [0.1, 0.1, 0.1])
    gi, gp = g.extract_known_voxels().cpu()
    ijk, p, _ = ox.extract(ref, ox.KNOWN)
    assert np.array_equal(gi, ijk) and same(gp, p)      # (the voxel's position, where the reference reports (0,0,0))


# ---- bit-equal planes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ox.COUNTS)
@pytest.mark.parametrize("res", ox.RESOLUTIONS)
@pytest.mark.parametrize("name", ox.SCENES)
def test_scene_equals_the_restatement(name, res, n):
    grid, ref, stats = gpu_grid(res), ox.new_grid(res), []
    check(grid, ref)
    for op in ox.scene(name, res, n):
        ox.apply(ref, op, stats)
        apply(grid, op)
        check(grid, ref)
    # not vacuous
    assert sum(s["free"] for s in stats) > 0 and sum(s["free"] + s["occupied"] for s in stats) > 0
    if n == 5000:
        assert sum(s["occupied"] for s in stats) > 0 and sum(s["both"] for s in stats) > 0
        assert sum(s["left_box"] for s in stats) > 0       # a walk leaves the box of its end voxels
        if name == "b":
            assert sum(s["left_grid"] for s in stats) > 0  # a walk emits voxels outside the grid
            assert (ref.min_bound == 0).all() and (ref.max_bound == res - 1).all()
        if name == "e":
            known = ref.prob[~np.isnan(ref.prob)]
            assert known.min() == F(-2.0) and known.max() == F(3.5)          # both clamps bind
        if name == "g":
            assert np.nanmin(ref.prob) < F(-0.4)                              # the free area, then a walked miss: unclamped sums
    # clear() keeps the grid usable: every voxel unknown, the bounds at the centre
    grid.clear()
    ref.clear()
    check(grid, ref)


def test_skipped_points_and_empty_input():
    res = 33
    grid, ref = gpu_grid(res), ox.new_grid(res)
    op = ox.scene("a", res, 257)[0]
    pts = op[1].copy()
    pts[3, 1], pts[100, 0], pts[200, 2] = np.nan, np.inf, -np.inf
    grid.insert(pts, op[2], op[3])
    ox.insert(ref, pts, op[2], op[3])
    check(grid, ref)
    grid.insert(np.zeros((0, 3), F), op[2])                                   # empty: a no-op
    grid.add_voxels(np.zeros((0, 3), np.int32), True)
    check(grid, ref)
    grid.insert(np.full((5, 3), np.nan, F), op[2])                            # nothing left after skipping
    check(grid, ref)


def test_attributes_are_read_at_call_time_and_reconstruct():
    grid, ref = gpu_grid(16), ox.new_grid(16)
    op = ox.scene("a", 16, 257)[0]
    apply(grid, op)
    ox.apply(ref, op)
    grid.translate([0.05, -0.02, 0.01])
    grid.scale(1.5)
    ref.origin = (ref.origin + np.array([0.05, -0.02, 0.01], F)).astype(F)
    ref.voxel_size = F(ref.voxel_size * F(1.5))
    assert same(grid.origin, ref.origin) and F(grid.voxel_size) == ref.voxel_size
    apply(grid, op)
    ox.apply(ref, op)
    check(grid, ref)
    with pytest.raises(RuntimeError):
        grid.transform(np.eye(4))
    with pytest.raises(RuntimeError):
        grid.rotate(np.eye(3))
    grid.reconstruct(0.2, 33)
    ref = ox.Grid(0.2, 33, ref.origin)
    check(grid, ref)
    pts = (op[1] * F(2.0)).astype(F)
    grid.insert(pts, op[2])
    ox.insert(ref, pts, op[2])
    check(grid, ref)
    grid.resolution = 16                                                      # a changed resolution rebuilds the grid
    ref = ox.Grid(0.2, 16, ref.origin)
    check(grid, ref)


# ---- determinism, neighbours ----------------------------------------------------------------------------------------
def test_two_runs_two_grids_and_a_registration_in_between():
    from conftest import make_pair
    from cupoch_amd import _lib, geometry
    res = 64
    ops = ox.scene("b", res, 5000) + ox.scene("h", res, 5000)
    a, b = gpu_grid(res), gpu_grid(res)
    other = geometry.OccupancyGrid(0.07, 33, (0.3, 0.1, -0.2))                # a second grid on the same context
    other_ops = ox.scene("a", 33, 257)
    for op in ops:
        apply(a, op)
        apply(other, other_ops[0])
    plane_other = to_np(other.get_voxels()).copy()
    d = make_pair(3000, seed=5)
    eng = geometry.get_engine()
    eng.set_target(d["tgt"], d["tgt_nrm"])
    eng.set_source(d["src"])
    eng.registration_icp(_lib.EST_POINT_TO_PLANE, d["max_dist"], None, 1e-6, 1e-6, 5, -1.0)
    for op in ops:
        apply(b, op)
    pa, pb = to_np(a.get_voxels()), to_np(b.get_voxels())
    assert same(pa, pb) and np.array_equal(a.min_bound, b.min_bound) and np.array_equal(a.max_bound, b.max_bound)
    for fa, fb in ((a.extract_known_voxels, b.extract_known_voxels), (a.extract_occupied_voxels, b.extract_occupied_voxels)):
        (ia, va), (ib, vb) = fa().cpu(), fb().cpu()
        assert np.array_equal(ia, ib) and same(va, vb)
    assert same(other.get_voxels(), plane_other)                              # the registration and the other grids left it alone
    ref = ox.new_grid(res)
    for op in ops:
        ox.apply(ref, op)
    check(a, ref)


# ---- error returns: status codes, never faults ------------------------------------------------------------------------
def test_error_returns_change_nothing():
    from cupoch_amd import MiIcpError, geometry
    from cupoch_amd.engine import Engine
    with pytest.raises(MiIcpError):
        geometry.OccupancyGrid(0.1, 1).get_voxels()                          # resolution < 2
    with pytest.raises(MiIcpError):
        geometry.OccupancyGrid(0.1, 1025).get_voxels()                       # above MI_ICP_OCCGRID_MAX_RESOLUTION
    res = 16
    grid, ref = gpu_grid(res), ox.new_grid(res)
    op = ox.scene("a", res, 257)[0]
    apply(grid, op)
    ox.apply(ref, op)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        grid.voxel_size = bad
        with pytest.raises(MiIcpError):
            grid.insert(op[1], op[2])
        with pytest.raises(MiIcpError):
            grid.set_free_area([0, 0, 0], [1, 1, 1])
    grid.voxel_size = ox.VOXEL
    check(grid, ref)
    far = op[1].copy()
    far[17] = (ox.VOXEL * (ox.MAX_NDIV + 2), 0.0, 0.0)                        # n_div above the cap
    with pytest.raises(MiIcpError, match="voxels along an axis"):
        grid.insert(far, op[2])
    with pytest.raises(ox.Refused):
        ox.insert(ref, far, op[2])
    check(grid, ref)
    near = op[1].copy()
    near[17] = (op[2][0] + F(ox.VOXEL * (ox.MAX_NDIV - 1)), op[2][1], op[2][2])   # just below it: accepted
    grid.insert(near, op[2])
    ox.insert(ref, near, op[2])
    check(grid, ref)
    for idx in ([[3, 4, 5], [16, 0, 0]], [[0, -1, 0]], [[1, 2, 3], [1, 2, 1 << 20]]):
        with pytest.raises(MiIcpError, match="occupancy grid range"):
            grid.add_voxels(np.array(idx, np.int32), True)
    with pytest.raises(MiIcpError):
        grid.insert(op[1], [np.nan, 0, 0])
    check(grid, ref)

    # a grid of another context is refused; the capacity rule: too little room writes nothing and reports the need
    import torch
    eng, L = grid._eng, grid._eng._L
    other = Engine(0)
    try:
        p = eng.occgrid_params(ox.VOXEL, ox.ORIGINS[res], -2.0, 3.5, 0.85, -0.4, 0.0)
        m = C.c_int64(-7)
        assert L.mi_icp_occgrid_extract(other._ctx, grid._grid, C.byref(p), 0, None, None, None, 0, C.byref(m)) == -1
        assert L.mi_icp_occgrid_reset(other._ctx, grid._grid) == -1
        assert L.mi_icp_occgrid_destroy(other._ctx, grid._grid) == -1
        assert L.mi_icp_occgrid_insert(other._ctx, grid._grid, C.byref(p), None, 0, None, -1.0) == -1
    finally:
        other.close()
    need = len(ox.extract(ref, ox.KNOWN)[0])
    assert need > 8
    idx = torch.full((need, 3), -5, dtype=torch.int32, device="cuda")
    prob = torch.full((need,), -5.0, dtype=torch.float32, device="cuda")
    for cap in (0, need - 1):
        m = C.c_int64(0)
        assert L.mi_icp_occgrid_extract(eng._ctx, grid._grid, C.byref(p), 0, C.c_void_p(idx.data_ptr()),
                                        C.c_void_p(prob.data_ptr()), None, cap, C.byref(m)) == 0
        eng.synchronize()
        assert m.value == need and bool((idx == -5).all()) and bool((prob == -5.0).all())
    assert L.mi_icp_occgrid_extract(eng._ctx, grid._grid, C.byref(p), 0, C.c_void_p(idx.data_ptr()),
                                    C.c_void_p(prob.data_ptr()), None, need, C.byref(m)) == 0
    eng.synchronize()
    ijk, pr, _ = ox.extract(ref, ox.KNOWN)
    assert np.array_equal(to_np(idx), ijk) and same(prob, pr)
    assert L.mi_icp_occgrid_extract(eng._ctx, grid._grid, C.byref(p), 3, None, None, None, 0, C.byref(m)) == -1
    assert L.mi_icp_occgrid_extract(eng._ctx, grid._grid, C.byref(p), 0, None, None, None, -1, C.byref(m)) == -1
    check(grid, ref)


def test_free_area_beside_the_grid_is_empty():
    res = 16
    grid, ref = gpu_grid(res), ox.new_grid(res)
    for lo, hi in (([5.0, 0, 0], [6.0, 0.1, 0.1]), ([-0.2, -0.2, -9.0], [0.2, 0.2, -7.0])):
        grid.set_free_area(lo, hi)
        ox.set_free_area(ref, lo, hi)
        check(grid, ref)
        assert len(grid.extract_known_voxels()) == 0
    op = ox.scene("a", res, 65)[0]
    apply(grid, op)
    ox.apply(ref, op)
    check(grid, ref)


# ---- a bounds box whose three extents differ, through everything that decodes it ----------------------------------------
def test_a_box_with_three_different_extents_through_every_consumer():
    """The occupancy input of the other tests is a shell seen from its centre: a bounds box that is nearly a cube, which
    a decode with two extents swapped would pass.  Here the box is 5 x 11 x 23 voxels, (3, 9, 5) .. (7, 19, 27)."""
    import collision_exact as cx
    from cupoch_amd import collision, geometry
    res, origin, lo, hi = 32, ox.ORIGINS[33], np.array([3, 9, 5]), np.array([7, 19, 27])
    grid, ref = geometry.OccupancyGrid(ox.VOXEL, res, origin), ox.Grid(ox.VOXEL, res, origin)

    def centre(ijk):
        return ((np.asarray(ijk, F) + F(0.5 - res // 2)) * F(ox.VOXEL) + np.asarray(origin, F)).astype(F)
    rng = np.random.default_rng(5)
    inner = np.stack([rng.integers(lo[k], hi[k] + 1, 40) for k in range(3)], 1)
    corners = np.array([[3, 9, 5], [7, 19, 27], [3, 19, 5], [7, 9, 27]])
    for op in (("free", centre(lo), centre(hi)), ("add", np.concatenate([inner, corners]).astype(np.int32), True)):
        apply(grid, op)
        ox.apply(ref, op)
    assert np.array_equal(ref.min_bound, lo) and np.array_equal(ref.max_bound, hi)
    e, g, p = grid._call()
    for which, count in ((ox.KNOWN, 1265), (ox.FREE, 1221), (ox.OCCUPIED, 44)):
        ijk, prob, pts = ox.extract(ref, which)
        assert len(ijk) == count
        gi, gp, gx = e.occgrid_extract(g, p, which, want_points=True)
        assert np.array_equal(to_np(gi), ijk) and same(gp, prob) and same(gx, pts)
    check(grid, ref)
    occupied = ox.extract(ref, ox.OCCUPIED)[0]

    d = geometry.DistanceTransform.create_from_occupancy_grid(grid)
    near, dist = d.voxels.cpu()
    near1, dist1 = geometry.DistanceTransform(ox.VOXEL, res, origin).compute_edt(occupied).voxels.cpu()
    assert np.array_equal(near, near1) and same(dist, dist1)
    assert np.count_nonzero(dist) == res ** 3 - 44 and np.isfinite(dist).all()

    v = geometry.VoxelGrid.create_from_occupancy_grid(grid)
    assert np.array_equal(to_np(v.voxels.grid_index), occupied)

    # a small VoxelGrid in a frame of its own, with a voxel over each of two corners and two voxels beside the box
    vs_q, origin_q = ox.VOXEL, np.asarray(origin, F) + F(0.037)
    keys = np.array(sorted(map(tuple, [corners[0] - 16, corners[1] - 16, corners[2] - 16 + [0, 1, 0], [9, 9, 9]])), np.int32)
    q = geometry.VoxelGrid()
    q.voxel_size, q.origin = float(vs_q), origin_q
    q.add_voxels((keys, np.ones((len(keys), 3), F)))
    assert np.array_equal(to_np(q.voxels.grid_index), keys)
    oside, qside = ("occ", occupied, res, ox.VOXEL, np.asarray(origin, F)), ("voxel", keys, vs_q, origin_q)
    for a, b, sa, sb in ((grid, q, oside, qside), (q, grid, qside, oside)):
        want = cx.compute_intersection(sa, sb, 0.0)
        got = collision.compute_intersection(a, b, 0.0).get_collision_index_pairs()
        assert np.array_equal(got, want) and len(want) >= 2
