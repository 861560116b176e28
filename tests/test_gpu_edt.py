"""geometry::DistanceTransform on the GPU against the numpy restatement of its contract (tests/edt_exact.py), through the
Python mirror and the C ABI.  Unless a case says otherwise the whole plane is compared: the distances bit for bit with
sqrt(float32(d2)) * float32(voxel_size), the nearest indices with valid_nearest (a site, at the field's minimum)."""
import numpy as np
import pytest

import edt_exact as ex

pytestmark = pytest.mark.gpu
F = np.float32
VS = 0.1


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def same(a, b):
    a, b = np.ascontiguousarray(to_np(a), F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def transform(res, vs=VS, origin=(0.0, 0.0, 0.0)):
    from cupoch_amd import geometry
    return geometry.DistanceTransform(vs, res, origin)


def planes(d):
    near, dist = d.voxels.cpu()
    return near, dist


def check_plane(d, cells):
    """the whole plane of `d` is the exact field of the cells inside its grid"""
    res = int(d.resolution)
    sites, _ = ex.site_set(cells, res)
    d2 = ex.field(sites, res)
    near, dist = planes(d)
    assert near.shape == (res ** 3, 3) and near.dtype == np.int32
    want = ex.distance(d2, d.voxel_size)
    assert same(dist, want), "%d distances differ" % int((dist.view(np.uint32) != want.view(np.uint32)).sum())
    ok, msg = ex.valid_nearest(near, sites, d2, res=res)
    assert ok, msg
    return near, dist


# ---- tiny grids: a single site at each corner in turn -------------------------------------------------------------------
@pytest.mark.parametrize("res", [2, 3, 8])
def test_tiny_grids_one_corner_site(res):
    d = transform(res)
    for corner in range(8):
        c = [[(res - 1) * ((corner >> k) & 1) for k in (2, 1, 0)]]
        near, _ = check_plane(d.compute_edt(np.array(c, np.int32)), c)
        assert (near == np.array(c)).all()


# ---- densities at a full wave, one over, and a size that is no multiple of 8 ---------------------------------------------
@pytest.mark.parametrize("res", [64, 65, 67])
@pytest.mark.parametrize("density", ["one", "five", "0.1%", "5%", "50%", "all"])
def test_densities(res, density):
    rng = np.random.default_rng(res * 7 + len(density))
    if density == "all":
        cells = ex.grid_cells(res)
    else:
        n = {"one": 1, "five": 5, "0.1%": res ** 3 // 1000, "5%": res ** 3 // 20, "50%": res ** 3 // 2}[density]
        lin = rng.choice(res ** 3, n, replace=False)
        cells = np.stack([lin // (res * res), (lin // res) % res, lin % res], axis=1)
    check_plane(transform(res).compute_edt(cells.astype(np.int32)), cells)


# ---- degenerate sets: whole lines of a pass see no site and "none" must propagate ---------------------------------------
def _degenerate(res):
    a = np.arange(res)
    u, v = [m.ravel() for m in np.meshgrid(a, a, indexing="ij")]
    c = np.full(res * res, 11)
    out = {"plane x": np.stack([c, u, v], 1), "plane y": np.stack([u, c, v], 1), "plane z": np.stack([u, v, c], 1)}
    k5, k20 = np.full(res, 5), np.full(res, 20)
    out.update({"line x": np.stack([a, k5, k20], 1), "line y": np.stack([k5, a, k20], 1), "line z": np.stack([k5, k20, a], 1)})
    out["corners"] = np.array([[(res - 1) * ((i >> k) & 1) for k in (2, 1, 0)] for i in range(8)])
    out["face"] = np.stack([u, v, np.full(res * res, res - 1)], 1)
    return out


@pytest.mark.parametrize("name", ["plane x", "plane y", "plane z", "line x", "line y", "line z", "corners", "face"])
def test_degenerate_sets(name):
    cells = _degenerate(33)[name]
    check_plane(transform(33).compute_edt(cells.astype(np.int32)), cells)


def test_no_sites():
    d = transform(17)
    for cells in (np.zeros((0, 3), np.int32), np.array([[17, 0, 0], [-1, 3, 3]], np.int32)):
        near, dist = planes(d.compute_edt(cells))
        assert np.isposinf(dist).all() and (near == -1).all()
    inside, v = d.get_voxel((0.0, 0.0, 0.0))
    assert inside and tuple(v.nearest_index) == (-1, -1, -1) and np.isposinf(v.distance)
    fresh = transform(9)                                    # a transform nothing was computed in has no sites either
    near, dist = planes(fresh)
    assert np.isposinf(dist).all() and (near == -1).all()


# ---- set semantics ----------------------------------------------------------------------------------------------------
def test_a_pure_function_of_the_site_set():
    import torch
    res = 40
    rng = np.random.default_rng(5)
    cells = rng.integers(0, res, (3000, 3)).astype(np.int32)
    d = transform(res)
    near0, dist0 = check_plane(d.compute_edt(cells), cells)
    again = np.concatenate([cells, cells[rng.integers(0, len(cells), 900)]])      # 30 % duplicates, another order
    again = again[rng.permutation(len(again))]
    near1, dist1 = planes(d.compute_edt(torch.from_numpy(again).cuda()))          # a device tensor is read in place
    assert np.array_equal(near0, near1) and same(dist0, dist1)
    other = transform(res)                                                          # and on a transform of its own
    near2, dist2 = planes(other.compute_voronoi_diagram(again[::-1].copy()))
    assert np.array_equal(near0, near2) and same(dist0, dist2)


def test_cells_outside_are_dropped_and_counted():
    res = 20
    rng = np.random.default_rng(6)
    cells = rng.integers(-3, res + 3, (4000, 3)).astype(np.int32)
    sites, dropped = ex.site_set(cells, res)
    assert 0 < dropped < len(cells)
    d = transform(res)
    assert d.compute_edt(cells).dropped is None
    check_plane(d, cells)
    assert d.compute_edt(cells, count_dropped=True).dropped == dropped
    check_plane(d, cells)
    assert d.compute_edt(sites.astype(np.int32), count_dropped=True).dropped == 0


def test_each_compute_replaces_the_site_set_and_reconstruct():
    from cupoch_amd import MiIcpError
    rng = np.random.default_rng(7)
    d = transform(30)
    big = rng.integers(0, 30, (2000, 3)).astype(np.int32)
    check_plane(d.compute_edt(big), big)
    small = np.array([[29, 0, 15]], np.int32)
    near, _ = check_plane(d.compute_edt(small), small)                             # nothing of the first set is left
    assert (near == small[0]).all()
    assert d.reconstruct(0.25, 21) is d and d.resolution == 21 and d.voxel_size == 0.25
    near, dist = planes(d)
    assert len(dist) == 21 ** 3 and np.isposinf(dist).all() and (near == -1).all()
    cells = rng.integers(0, 21, (50, 3)).astype(np.int32)
    check_plane(d.compute_edt(cells), cells)
    d.resolution = 2000                                                            # refused: the transform stays as it was
    handle = d._dt
    with pytest.raises(MiIcpError) as err:
        d.compute_edt(cells)
    assert err.value.code == -1 and d._dt is handle
    d.resolution = 21
    check_plane(d, cells)
    d.resolution = 35                                                              # the public member, read at the next call
    cells = rng.integers(0, 35, (50, 3)).astype(np.int32)
    check_plane(d.compute_edt(cells), cells)
    assert d.clear() is d and np.isposinf(planes(d)[1]).all()


# ---- the reference's unit test (src/tests/geometry/distancetransform.cpp) ---------------------------------------------------
def test_reference_unit_test():
    from cupoch_amd import geometry
    grid = geometry.VoxelGrid()
    grid.voxel_size = 1.0
    grid.add_voxel(geometry.Voxel([5, 5, 5]))
    d = geometry.DistanceTransform(1.0, 512)
    assert d.compute_voronoi_diagram(grid) is d
    inside, v = d.get_voxel((0.0, 0.0, 0.0))
    assert inside and tuple(v.nearest_index) == (261, 261, 261)
    assert v.distance == float(np.sqrt(F(3 * 5 * 5)))
    assert d.get_distance((5.5, 5.5, 5.5)) == 0.0


# ---- form 2: a VoxelGrid ----------------------------------------------------------------------------------------------
def _cloud_grid():
    from cupoch_amd import geometry
    rng = np.random.default_rng(8)
    pts = (rng.normal(0.0, 0.6, (3000, 3))).astype(F)
    lo = np.array([-2.013, -1.987, -2.041], F)                                     # no multiple of the voxel size
    return geometry.VoxelGrid.create_from_point_cloud_within_bounds(geometry.PointCloud(pts), VS, lo, -lo)


def test_voxelgrid_form_equals_the_restatement():
    grid = _cloud_grid()
    keys = grid.voxels.cpu()[0]
    assert len(keys) > 500
    res, origin = 48, (0.31, -0.17, 0.052)
    d = transform(res, VS, origin)
    assert d.compute_edt(grid, count_dropped=True) is d
    cells = ex.cells_of_keys(keys, VS, grid.origin, origin, res)
    sites, dropped = ex.site_set(cells, res)
    assert d.dropped == dropped and 0 < dropped < len(keys) and len(sites) > 200
    check_plane(d, cells)
    # ... and it is form 1 of exactly those cells
    near, dist = planes(d)
    near1, dist1 = planes(transform(res, VS, origin).compute_edt(cells.astype(np.int32)))
    assert np.array_equal(near, near1) and same(dist, dist1)


def test_voxel_size_mismatch_changes_nothing(capfd):
    from cupoch_amd import MiIcpError
    grid = _cloud_grid()
    cells = np.array([[3, 4, 5], [20, 1, 9]], np.int32)
    d = transform(24, VS).compute_edt(cells)
    near0, dist0 = planes(d)
    d.voxel_size = float(F(VS) + F(1e-6))                                          # |difference| > FLT_EPSILON
    capfd.readouterr()
    assert d.compute_edt(grid) is d
    assert "Unsupport computing Voronoi diagrams from different voxel size." in capfd.readouterr().err
    d.voxel_size = VS
    near1, dist1 = planes(d)
    assert np.array_equal(near0, near1) and same(dist0, dist1)
    e, h = d._call()                                                               # the C ABI refuses it itself
    with pytest.raises(MiIcpError, match="different voxel size"):
        e.dt_compute_voxelgrid(h, VS, d.origin, grid.voxels.cpu()[0], VS * 2, grid.origin)
    with pytest.raises(MiIcpError):
        e.dt_compute_voxelgrid(h, float("nan"), d.origin, grid.voxels.cpu()[0], VS, grid.origin)
    near1, dist1 = planes(d)
    assert np.array_equal(near0, near1) and same(dist0, dist1)


# ---- form 3: an OccupancyGrid -----------------------------------------------------------------------------------------
def test_occupancy_grid_form():
    from cupoch_amd import geometry, MiIcpError
    rng = np.random.default_rng(9)
    dirs = rng.normal(size=(1500, 3))
    pts = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True) * rng.uniform(1.0, 2.5, (1500, 1))).astype(F)
    occ = geometry.OccupancyGrid(VS, 64, (0.05, -0.02, 0.01))
    occ.insert(pts, (0.0, 0.0, 0.0))
    idx = occ.extract_occupied_voxels().cpu()[0]
    assert len(idx) > 300
    d = geometry.DistanceTransform.create_from_occupancy_grid(occ)
    assert (d.voxel_size, d.resolution) == (occ.voxel_size, 64) and np.array_equal(d.origin, occ.origin)
    near, dist = check_plane(d, idx)
    assert np.count_nonzero(dist) == 64 ** 3 - len(idx) and np.isfinite(dist).all()     # computed, not merely marked
    near1, dist1 = planes(transform(64, VS, occ.origin).compute_edt(idx.astype(np.int32)))
    assert np.array_equal(near, near1) and same(dist, dist1)
    occ.occ_prob_thres_log = 1.0                                                    # the threshold is read at the call
    idx2 = occ.extract_occupied_voxels().cpu()[0]
    assert 0 < len(idx2) < len(idx) or len(idx2) == 0
    if len(idx2):
        check_plane(d.compute_edt(occ), idx2)
    small = transform(32)
    e, h = small._call()
    with pytest.raises(MiIcpError, match="resolutions differ"):
        e.dt_compute_occgrid(h, occ._call()[1], 0.0)


# ---- queries -----------------------------------------------------------------------------------------------------------
def test_queries():
    res, vs, origin = 16, 0.5, np.array([0.25, -1.0, 2.0], F)
    rng = np.random.default_rng(10)
    cells = rng.integers(0, res, (12, 3)).astype(np.int32)
    d = transform(res, vs, origin).compute_edt(cells)
    near, dist = planes(d)
    lim = res * vs / 2
    q = np.concatenate([
        (rng.uniform(-lim, lim, (500, 3)) + origin).astype(F),                      # inside
        (rng.integers(-res // 2, res // 2, (200, 3)) * F(vs) + origin).astype(F),   # exactly on cell boundaries
        origin + np.array([[lim, 0, 0], [0, lim, 0], [0, 0, lim], [-lim - 0.01, 0, 0], [0, -lim - 0.01, 0],
                           [0, 0, -lim - 0.01], [1e9, 0, 0], [np.nan, 0, 0]], F)]).astype(F)   # outside on each axis
    c = ex.cells_of_points(q, vs, origin, res)
    ins = ex.inside(c, res)
    assert ins[:700].all() and not ins[700:].any()
    got_d, got_n = [to_np(t) for t in d.get_nearest_indices(q)]
    lin = (c[ins, 0] * res + c[ins, 1]) * res + c[ins, 2]
    assert same(got_d[ins], dist[lin]) and np.array_equal(got_n[ins], near[lin])
    assert np.isnan(got_d[~ins]).all() and (got_n[~ins] == -1).all()
    assert same(d.get_distances(q), got_d)
    for i in (0, 500, 650, 700, 707):
        one = d.get_distance(q[i])
        assert (np.isnan(one) and np.isnan(got_d[i])) or F(one) == got_d[i]
    assert d.get_voxel(q[703])[0] is False
    # scale(2): every finite distance doubles bit for bit
    qi = q[:700].copy()
    before = to_np(d.get_distances(qi))
    cells_before = ex.cells_of_points(qi, vs, origin, res)
    d.scale(2.0)
    q2 = ((qi - origin) * F(2.0) + origin).astype(F)                                # the same cells at twice the size
    assert np.array_equal(ex.cells_of_points(q2, vs * 2, origin, res), cells_before)
    assert same(d.get_distances(q2), before * F(2.0)) and same(planes(d)[1], dist * F(2.0))
    d.scale(0.5)
    # translate: the same world point maps to the shifted cell
    shift = np.array([vs * 3, -vs * 2, vs], F)
    d.translate(shift)
    moved = ex.cells_of_points(qi, vs, origin + shift, res)
    ok = ex.inside(moved, res)
    assert 0 < ok.sum() < len(qi)
    got_d, got_n = [to_np(t) for t in d.get_nearest_indices(qi)]
    lin = (moved[ok, 0] * res + moved[ok, 1]) * res + moved[ok, 2]
    assert same(got_d[ok], dist[lin]) and np.array_equal(got_n[ok], near[lin]) and np.isnan(got_d[~ok]).all()


# ---- the largest grid: where 32-bit arithmetic breaks ----------------------------------------------------------------------
def test_resolution_1024():
    from cupoch_amd import MiIcpError
    res = 1024
    rng = np.random.default_rng(11)
    corners = np.array([[(res - 1) * ((i >> k) & 1) for k in (2, 1, 0)] for i in range(8)])
    sites = np.concatenate([corners, rng.integers(0, res, (24, 3))]).astype(np.int32)
    d = transform(res, 1.0)
    try:
        d._call()
    except MiIcpError as e:                 # create itself could not have the two planes (8 GiB): MI_ICP_ERR_HIP
        if e.code == -3:
            pytest.skip("mi_icp_dt_create: %s" % e)
        raise
    d.compute_edt(sites, count_dropped=True)
    assert d.dropped == 0
    mid = res // 2
    a = np.arange(res)
    m = np.full(res, mid)
    lines = np.concatenate([np.stack([a, m, m], 1), np.stack([m, a, m], 1), np.stack([m, m, a], 1)])
    faces = np.array([[0, mid, mid], [res - 1, mid, mid], [mid, 0, mid], [mid, res - 1, mid], [mid, mid, 0], [mid, mid, res - 1]])
    cells = np.concatenate([rng.integers(0, res, (200000, 3)), corners, faces, lines]).astype(np.int64)
    q = (cells - mid + 0.5).astype(F)                                               # cell centres: exact in fp32
    assert np.array_equal(ex.cells_of_points(q, 1.0, (0, 0, 0), res), cells)
    got_d, got_n = [to_np(t) for t in d.get_nearest_indices(q)]
    d2 = ex.d2_brute(sites, cells)
    assert d2.max() > 500 * 500
    assert same(got_d, ex.distance(d2, 1.0))
    ok, msg = ex.valid_nearest(got_n, sites, d2, cells=cells)
    assert ok, msg
