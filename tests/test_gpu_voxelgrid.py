"""geometry::VoxelGrid on the GPU against the numpy fp32 restatement of its contract (tests/voxelgrid_exact.py): keys and
their order array_equal, colours bit-equal unless a test says otherwise; voxelisation at every size and key width, merges
in both modes, dense grids and the carvings, queries on sorted and unsorted grids, bounds and centre, the occupancy-grid
factory, selections and paint, refusals that change nothing, and a registration on the same context around it."""
import numpy as np
import pytest

import voxelgrid_exact as vx

pytestmark = pytest.mark.gpu
F = np.float32


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def same(a, b):
    a, b = np.ascontiguousarray(to_np(a), F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def cloud(points, colors=None):
    from cupoch_amd import geometry, utility
    pc = geometry.PointCloud()
    pc.points = utility.Vector3fVector(np.ascontiguousarray(points, F))
    if colors is not None:
        pc.colors = utility.Vector3fVector(np.ascontiguousarray(colors, F))
    return pc


def grid_of(keys, colors, voxel_size=1.0, origin=(0, 0, 0)):
    from cupoch_amd import geometry
    g = geometry.VoxelGrid()
    g.voxel_size, g.origin = float(voxel_size), np.asarray(origin, F)
    g.voxels = (np.asarray(keys, np.int32).reshape(-1, 3), np.asarray(colors, F).reshape(-1, 3))
    return g


def got(g):
    k, c = g.voxels.cpu()
    return k, c


def check(g, keys, colors):
    k, c = got(g)
    assert k.shape == keys.shape and np.array_equal(k, keys)
    assert same(c, colors), "colours differ at %d of %d voxels" % (int((c.view(np.uint32) != colors.view(np.uint32)).any(axis=1).sum()), len(c))
    assert repr(g) == "geometry::VoxelGrid with %d voxels." % len(keys)


def within(points, colors, vs, lo, hi):
    from cupoch_amd import geometry
    return geometry.VoxelGrid.create_from_point_cloud_within_bounds(cloud(points, colors), vs, lo, hi)


# ---- from_points -------------------------------------------------------------------------------------------------------
def dyadic(rng, n):
    return (rng.integers(0, 1025, (n, 3)) / 1024.0).astype(F)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 20000])
def test_from_points_sizes(n):
    rng = np.random.default_rng(n + 1)
    pts = rng.random((n, 3)).astype(F)
    col = dyadic(rng, n)                        # every fp64 sum exact in any order: bit-equal for any correct code
    lo, hi = np.array([0.3, 0.4, 0.2], F), np.array([1, 1, 1], F)   # min_bound inside the cloud: negative keys
    vs = 0.11
    g = within(pts, col, vs, lo, hi)
    k, c = vx.from_points(pts, col, vs, lo, hi)
    check(g, k, c)
    assert g.voxel_size == float(F(vs)) and same(g.origin, lo)
    if n > 1:
        assert k.min() < 0
    g2 = within(pts, None, vs, lo, hi)          # no colours: (1, 1, 1)
    check(g2, k, np.ones_like(c))


def test_from_points_one_voxel_holds_the_cloud_and_one_point_per_voxel():
    rng = np.random.default_rng(7)
    n = 20000
    pts = (rng.random((n, 3)) * 0.9).astype(F)
    col = dyadic(rng, n)
    g = within(pts, col, 1.0, (0, 0, 0), (1, 1, 1))
    k, c = vx.from_points(pts, col, 1.0, (0, 0, 0), (1, 1, 1))
    assert len(k) == 1
    check(g, k, c)
    ijk = np.stack(np.unravel_index(rng.permutation(32 ** 3)[:n], (32, 32, 32)), axis=1)
    pts = ((ijk + 0.5) / 32.0).astype(F)
    g = within(pts, col, 1.0 / 32.0, (0, 0, 0), (1, 1, 1))
    k, c = vx.from_points(pts, col, 1.0 / 32.0, (0, 0, 0), (1, 1, 1))
    assert len(k) == n
    check(g, k, c)


def test_from_points_random_colours_within_one_ulp_and_repeatable():
    """an fp64 sum of n <= 2e4 fp32 values errs by less than n * 2^-53 relative in any order, far below half an fp32 ulp:
    two orders can only round to neighbouring floats"""
    rng = np.random.default_rng(8)
    n = 20000
    pts = rng.random((n, 3)).astype(F)
    col = rng.random((n, 3)).astype(F)
    for vs in (1.0, 0.26, 0.05):              # one run of 20000, runs of hundreds, short runs
        g = within(pts, col, vs, (0, 0, 0), (1, 1, 1))
        k, c = vx.from_points(pts, col, vs, (0, 0, 0), (1, 1, 1))
        gk, gc = got(g)
        assert np.array_equal(gk, k)
        d = vx.ulp_distance(gc, c)
        print("voxel_size %g: %d voxels, colours off by one ulp: %d, max %d" % (vs, len(k), int((d == 1).sum()), int(d.max())))
        assert d.max() <= 1
        g2 = within(pts, col, vs, (0, 0, 0), (1, 1, 1))
        assert np.array_equal(got(g2)[0], gk) and same(got(g2)[1], gc)


def test_from_points_wide_keys_and_skipped_points():
    rng = np.random.default_rng(9)
    a = rng.random((300, 3)).astype(F)
    col = dyadic(rng, 600)
    for shift, bits in (((3.0e6, 3.0e6, 0.0), None), ((3.0e6, 3.0e6, 3.0e6), 66)):   # one 64-bit key; two sorts
        pts = np.concatenate([a, a + np.array(shift, F)]).astype(F)
        lo, hi = np.zeros(3, F), np.full(3, 4.0e6, F)
        k, c = vx.from_points(pts, col, 1.0, lo, hi)
        assert vx.key_span_bits(k) > 32 and (bits is None or vx.key_span_bits(k) == bits)
        check(within(pts, col, 1.0, lo, hi), k, c)
    corners = np.array([[-2e9, -2e9, -2e9], [2e9, 2e9, 2e9], [0, 0, 0], [2e9, 2e9, 2e9]], F)   # held at +-1e9: 93 bits
    k, c = vx.from_points(corners, col[:4], 1.0, (0, 0, 0), (1, 1, 1))
    assert len(k) == 3 and vx.key_span_bits(k) > 64
    check(within(corners, col[:4], 1.0, (0, 0, 0), (1, 1, 1)), k, c)
    pts = rng.random((1000, 3)).astype(F)
    pts[::7, 0] = np.nan
    pts[3::11, 2] = np.inf
    pts[5::13, 1] = -np.inf
    col = dyadic(rng, 1000)
    k, c = vx.from_points(pts, col, 0.2, (0, 0, 0), (1, 1, 1))
    check(within(pts, col, 0.2, (0, 0, 0), (1, 1, 1)), k, c)
    allbad = np.full((70, 3), np.nan, F)
    assert len(within(allbad, None, 0.2, (0, 0, 0), (1, 1, 1)).voxels) == 0


def test_create_from_point_cloud_takes_the_cloud_bounds():
    from cupoch_amd import geometry
    rng = np.random.default_rng(10)
    pts = (rng.random((5000, 3)) * 2 - 1).astype(F)
    col = dyadic(rng, 5000)
    vs = F(0.13)
    g = geometry.VoxelGrid.create_from_point_cloud(cloud(pts, col), float(vs))
    lo, hi = pts.min(axis=0) - vs * F(0.5), pts.max(axis=0) + vs * F(0.5)
    k, c = vx.from_points(pts, col, vs, lo, hi)
    assert same(g.origin, lo)
    check(g, k, c)


# ---- merge -------------------------------------------------------------------------------------------------------------
def two_grids(rng, na, nb, lo_b):
    ka = np.unique(rng.integers(-8, 8, (na, 3)), axis=0).astype(np.int32)
    kb = np.unique(rng.integers(lo_b, lo_b + 16, (nb, 3)), axis=0).astype(np.int32)
    return ka, dyadic(rng, len(ka)), kb, dyadic(rng, len(kb))


@pytest.mark.parametrize("case", ["disjoint", "identical", "half", "empty_a", "empty_b"])
def test_merge_average(case):
    rng = np.random.default_rng(11)
    ka, ca, kb, cb = two_grids(rng, 700, 700, {"disjoint": 100, "half": 0}.get(case, -8))
    if case == "identical":
        kb, cb = ka.copy(), dyadic(rng, len(ka))
    if case == "empty_a":
        ka, ca = np.zeros((0, 3), np.int32), np.zeros((0, 3), F)
    if case == "empty_b":
        kb, cb = np.zeros((0, 3), np.int32), np.zeros((0, 3), F)
    a, b = grid_of(ka, ca, 0.5, (1, 2, 3)), grid_of(kb, cb, 0.5, (1, 2, 3))
    k, c = vx.merge(ka, ca, kb, cb, vx.AVERAGE)
    s = a + b
    check(s, k, c)
    assert s.voxel_size == 0.5 and same(s.origin, np.array([1, 2, 3], F))
    check(a, *vx.merge(ka, ca, ka[:0], ca[:0], vx.AVERAGE))                  # + leaves its operands alone
    a += b
    check(a, k, c)
    if case == "half":
        both = len(ka) + len(kb) - len(k)
        assert 0 < both < min(len(ka), len(kb))


def test_merge_average_with_duplicates_inside_an_operand_and_refusals():
    rng = np.random.default_rng(12)
    ka = rng.integers(0, 4, (300, 3)).astype(np.int32)                        # many duplicates, unsorted (the setter)
    kb = rng.integers(0, 4, (200, 3)).astype(np.int32)
    ca, cb = dyadic(rng, 300), dyadic(rng, 200)
    a, b = grid_of(ka, ca), grid_of(kb, cb)
    check(a, ka, ca)                                                          # the setter takes what it is given
    k, c = vx.merge(ka, ca, kb, cb, vx.AVERAGE)
    check(a + b, k, c)
    b.voxel_size = 2.0
    with pytest.raises(RuntimeError, match="voxel_size differs"):
        a += b
    b.voxel_size, b.origin = 1.0, np.array([0, 0, 1], F)
    with pytest.raises(RuntimeError, match="origin differs"):
        a + b
    check(a, ka, ca)


def test_add_voxels_keep_first_and_the_reference_bounds():
    from cupoch_amd import geometry
    V = geometry.Voxel
    g = geometry.VoxelGrid()
    g.voxel_size = 5.0
    for idx in ([1, 0, 0], [0, 2, 0], [0, 0, 3]):                            # the reference's Bounds test
        g.add_voxel(V(idx, [0, 0, 0]))
    assert same(g.get_min_bound(), np.zeros(3, F)) and same(g.get_max_bound(), np.array([10, 15, 20], F))
    assert np.array_equal(got(g)[0], [[0, 0, 3], [0, 2, 0], [1, 0, 0]])
    g.add_voxel(V([0, 2, 0], [1, 0.5, 0.25]))                                 # an existing voxel beats an added one
    assert same(got(g)[1], np.zeros((3, 3), F))
    g.add_voxels([V([5, 5, 5], [0.5, 0, 0]), V([5, 5, 5], [0, 0.5, 0]), V([-1, 0, 0], [0, 0, 0.5])])   # the first listed wins
    k, c = got(g)
    assert np.array_equal(k, [[-1, 0, 0], [0, 0, 3], [0, 2, 0], [1, 0, 0], [5, 5, 5]])
    assert same(c, np.array([[0, 0, 0.5], [0, 0, 0], [0, 0, 0], [0, 0, 0], [0.5, 0, 0]], F))
    rng = np.random.default_rng(13)
    ka, ca, kb, cb = two_grids(rng, 500, 500, -4)
    kb = np.concatenate([kb, kb[::3]])
    cb = np.concatenate([cb, dyadic(rng, len(kb) - len(cb))])
    a = grid_of(ka, ca)
    a.add_voxels((kb, cb))
    check(a, *vx.merge(ka, ca, kb, cb, vx.KEEP_FIRST))


# ---- dense + carve -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def dense_grid():
    from cupoch_amd import geometry
    g = geometry.VoxelGrid.create_dense(vx.DENSE_ORIGIN, vx.DENSE_VS, vx.DENSE_SIDE, vx.DENSE_SIDE, vx.DENSE_SIDE)
    k, c = vx.dense(32, 32, 32)
    check(g, k, c)
    g.paint_indexed_color(np.arange(0, len(k), 5), (0.25, 0.5, 0.75))          # colours that tell voxels apart
    return g


def camera_of(intr, E):
    from cupoch_amd import camera
    return camera.PinholeCameraParameters(camera.PinholeCameraIntrinsic(vx.IMG_W, vx.IMG_H, *intr), E)


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", ["front", "inside", "partial", "silhouette"])
def test_carve_equals_the_restatement(dense_grid, name, keep):
    from cupoch_amd import geometry
    intr, E, img = vx.carve_scenes()[name]
    k0, c0 = got(dense_grid)
    g = geometry.VoxelGrid(dense_grid)
    fn = g.carve_silhouette if name == "silhouette" else g.carve_depth_map
    assert fn(geometry.Image(img), camera_of(intr, E), keep) is g
    k, c = vx.carve(k0, c0, vx.DENSE_VS, vx.DENSE_ORIGIN, img, intr, E, keep)
    assert 0.05 * len(k0) <= len(k) <= 0.95 * len(k0)
    check(g, k, c)
    check(dense_grid, k0, c0)


def test_carve_other_image_formats_and_dense_shapes(dense_grid):
    from cupoch_amd import MiIcpError, geometry
    intr, E, _ = vx.carve_scenes()["front"]
    k0, c0 = got(dense_grid)
    for img in (np.ones((vx.IMG_H, vx.IMG_W), np.uint16), np.ones((vx.IMG_H, vx.IMG_W, 3), F)):
        g = geometry.VoxelGrid(dense_grid).carve_depth_map(geometry.Image(img), camera_of(intr, E))   # the default: keep = False
        assert len(g.voxels) == 0 and g.is_empty()
        g = geometry.VoxelGrid(dense_grid).carve_depth_map(geometry.Image(img), camera_of(intr, E), True)
        check(g, k0, c0)
    with pytest.raises(RuntimeError, match="not compatible"):
        geometry.VoxelGrid(dense_grid).carve_depth_map(geometry.Image(np.ones((10, 10), F)), camera_of(intr, E))
    g = geometry.VoxelGrid.create_dense((1, 2, 3), 0.5, 1.0, 2.6, 1.7)         # round(2), round(5.2), round(3.4)
    check(g, *vx.dense(2, 5, 3))
    assert geometry.VoxelGrid.create_dense((0, 0, 0), 0.5, 0.0, 1.0, 1.0).is_empty()
    assert geometry.VoxelGrid.create_dense((0, 0, 0), 0.5, -1.0, 1.0, 1.0).is_empty()
    with pytest.raises(MiIcpError, match="more than 2\\^31 - 1"):
        geometry.VoxelGrid.create_dense((0, 0, 0), 1.0, 2048.0, 2048.0, 512.0)


# ---- query -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 65, 10000])
@pytest.mark.parametrize("m", [0, 1, 1000])
def test_check_if_included(m, nq):
    rng = np.random.default_rng(100 * m + nq)
    vs, o = F(0.25), np.array([0.1, -0.2, 0.3], F)
    keys = np.unique(rng.integers(-12, 12, (4 * m, 3)), axis=0)[:m].astype(np.int32) if m else np.zeros((0, 3), np.int32)
    keys = keys[np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))]
    q = ((rng.random((nq, 3)) * 8 - 4)).astype(F)
    if m:
        inside = keys[rng.integers(0, m, nq // 2)]
        q[:nq // 2] = ((inside + rng.random((nq // 2, 3)) * 0.9 + 0.05) * vs + o).astype(F)   # voxel interiors of the grid
        face = keys[rng.integers(0, m, max(nq // 8, 1))].astype(F) * vs + o                    # exactly on voxel faces
        nf = min(len(face), nq - nq // 2)
        q[nq // 2:nq // 2 + nf] = face[:nf]
    if nq > 3:
        q[-1] = [np.nan, 0, 0]
        q[-2] = [0, np.inf, 0]
    inc, _ = vx.query(keys, vs, o, q)
    g = grid_of(keys, np.ones((len(keys), 3), F), vs, o)                       # through the setter: taken as unsorted
    assert np.array_equal(g.check_if_included(q), inc)
    if m:
        assert inc[:nq // 2].all() or nq == 1
        rev = g.select_by_index(np.arange(m - 1, -1, -1))                     # reversed: unsorted in fact
        assert np.array_equal(got(rev)[0], keys[::-1])
        assert np.array_equal(rev.check_if_included(q), inc)
        srt = rev + grid_of(keys[:0], np.zeros((0, 3), F), vs, o)            # a merge sorts: the binary search alone
        assert np.array_equal(got(srt)[0], keys) and np.array_equal(srt.check_if_included(q), inc)
        k0 = keys[m // 2]
        assert same(g.get_voxel_center_coordinate(k0), (k0.astype(F) + F(0.5)) * vs + o)
        assert same(g.get_voxel_center_coordinate([99, 99, 99]), np.zeros(3, F))
        assert np.array_equal(g.get_voxel(q[0]), vx.point_keys(q[:1], vs, o)[0][0])


# ---- bounds / centre -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 257, 20000])
def test_bounds_and_centre(m):
    rng = np.random.default_rng(m)
    keys = rng.integers(-300, 500, (m, 3)).astype(np.int32)
    vs, o = F(0.037), np.array([0.5, -1.25, 2.0], F)
    g = grid_of(keys, np.ones((m, 3), F), vs, o)
    lo, hi, ce = vx.bounds(keys, vs, o)
    assert same(g.get_min_bound(), lo) and same(g.get_max_bound(), hi)
    box = g.get_axis_aligned_bounding_box()
    assert same(box.get_min_bound(), lo) and same(box.get_max_bound(), hi)
    d = vx.ulp_distance(g.get_center(), ce)
    print("centre off by", d)
    assert d.max() <= 1


def test_empty_grid_bounds():
    from cupoch_amd import geometry
    g = geometry.VoxelGrid()
    g.voxel_size, g.origin = 0.5, np.array([1, 2, 3], F)
    assert same(g.get_min_bound(), g.origin) and same(g.get_max_bound(), g.origin) and same(g.get_center(), np.zeros(3, F))
    assert g.check_if_included(np.zeros((3, 3), F)).tolist() == [False] * 3


# ---- the occupancy grid's occupied space, selections, paint -------------------------------------------------------------
def test_create_from_occupancy_grid():
    from cupoch_amd import geometry
    rng = np.random.default_rng(21)
    occ = geometry.OccupancyGrid(0.05, 64, (0.1, 0.2, 0.3))
    pts = (rng.random((3000, 3)) * 2.4 - 1.2).astype(F)
    occ.insert(pts, np.array([0.1, 0.2, 0.3], F))
    idx, _ = occ.extract_occupied_voxels().cpu()
    assert len(idx) > 100
    g = geometry.VoxelGrid.create_from_occupancy_grid(occ)
    check(g, idx, np.tile(np.array([0, 0, 1], F), (len(idx), 1)))
    assert g.voxel_size == occ.voxel_size and same(g.origin, occ.origin)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))
    assert np.array_equal(order, np.arange(len(idx)))                          # already ascending
    q = ((idx[:50].astype(F) + F(0.5)) * F(0.05) + np.array([0.1, 0.2, 0.3], F)).astype(F)
    assert np.array_equal(g.check_if_included(q), vx.query(idx, 0.05, (0.1, 0.2, 0.3), q)[0])


def test_select_by_index_and_paint():
    from cupoch_amd import MiIcpError
    rng = np.random.default_rng(22)
    m = 1000
    keys, cols = rng.integers(-50, 50, (m, 3)).astype(np.int32), rng.random((m, 3)).astype(F)
    g = grid_of(keys, cols, 0.5, (1, 1, 1))
    idx = rng.integers(0, m, 300)
    s = g.select_by_index(idx)
    check(s, keys[idx], cols[idx])
    assert s.voxel_size == 0.5 and same(s.origin, np.ones(3, F))
    mask = np.ones(m, bool)
    mask[idx] = False                                                          # a repeated index counts once
    check(g.select_by_index(idx, invert=True), keys[mask], cols[mask])
    check(g.select_by_index([], invert=True), keys, cols)
    assert g.select_by_index([]).is_empty()
    for bad in ([m], [-1], [0, 5, m + 7]):
        with pytest.raises(MiIcpError, match="out of range"):
            g.select_by_index(bad)
        with pytest.raises(MiIcpError, match="out of range"):
            g.select_by_index(bad, invert=True)
        with pytest.raises(MiIcpError, match="out of range"):
            g.paint_indexed_color(bad, (1, 0, 0))
    check(g, keys, cols)                                                       # the refused paint painted nothing
    want = cols.copy()
    want[idx] = (0.25, 0.5, 1.0)
    assert g.paint_indexed_color(idx, (0.25, 0.5, 1.0)) is g
    check(g, keys, want)
    g.paint_uniform_color((0.5, 0.125, 0.0))
    check(g, keys, np.tile(np.array([0.5, 0.125, 0.0], F), (m, 1)))


# ---- refusals change nothing; the context's scratch is shared with a registration ------------------------------------------
def test_refusals_leave_outputs_untouched():
    import ctypes as C
    import torch
    from cupoch_amd import MiIcpError, geometry
    eng = geometry.get_engine()
    pts = np.random.default_rng(23).random((500, 3)).astype(F)
    for vs in (0.0, -0.5, float("nan"), float("inf")):
        with pytest.raises(MiIcpError):
            within(pts, None, vs, (0, 0, 0), (1, 1, 1))
    with pytest.raises(MiIcpError, match="too small"):
        within(pts, None, 1e-12, (0, 0, 0), (1, 1, 1))
    # at the C boundary: the outputs keep their bytes and *m is 0
    dev = torch.device("cuda", eng.device)
    p = torch.from_numpy(pts).to(dev)
    keys = torch.full((500, 3), 77, dtype=torch.int32, device=dev)
    cols = torch.full((500, 3), 0.5, dtype=torch.float32, device=dev)
    m = C.c_int64(99)
    lo, hi = (C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1)
    for vs in (0.0, -1.0, float("nan"), 1e-12):
        rc = eng._L.mi_icp_voxelgrid_from_points(eng._ctx, C.c_void_p(p.data_ptr()), None, 500, vs, lo, hi,
                                                 C.c_void_p(keys.data_ptr()), C.c_void_p(cols.data_ptr()), 500, C.byref(m))
        assert rc == -1 and m.value == 0
    rc = eng._L.mi_icp_voxelgrid_dense(eng._ctx, 2048, 2048, 512, C.c_void_p(keys.data_ptr()), C.c_void_p(cols.data_ptr()), 500, C.byref(m))
    assert rc == -1 and m.value == 0
    # the capacity rule: the count comes back, nothing is written
    rc = eng._L.mi_icp_voxelgrid_from_points(eng._ctx, C.c_void_p(p.data_ptr()), None, 500, 0.1, lo, hi,
                                             C.c_void_p(keys.data_ptr()), C.c_void_p(cols.data_ptr()), 3, C.byref(m))
    assert rc == 0 and m.value == len(vx.from_points(pts, None, 0.1, (0, 0, 0), (1, 1, 1))[0]) > 3
    eng.synchronize()
    assert bool((keys == 77).all()) and bool((cols == 0.5).all())


def test_registration_before_and_after_a_voxelisation():
    from conftest import make_pair
    from cupoch_amd import _lib, geometry
    d = make_pair(3000, seed=5)
    eng = geometry.get_engine()

    def register():
        eng.set_target(d["tgt"], d["tgt_nrm"])
        eng.set_source(d["src"])
        r = eng.registration_icp(_lib.EST_POINT_TO_PLANE, d["max_dist"], None, 1e-6, 1e-6, 5, -1.0)
        return np.array(list(r.transformation), F)

    before = register()
    rng = np.random.default_rng(24)
    pts, col = rng.random((20000, 3)).astype(F), dyadic(rng, 20000)
    g = within(pts, col, 0.05, (0, 0, 0), (1, 1, 1))
    check(g, *vx.from_points(pts, col, 0.05, (0, 0, 0), (1, 1, 1)))
    g.check_if_included(pts[:100])
    after = register()
    assert same(before, after)
