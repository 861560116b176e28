"""GPU: PointCloud::RemoveStatisticalOutliers / RemoveRadiusOutliers / SelectByIndex / UniformDownSample
(include/mi_icp.h, csrc/select.h, knn_normals_kernel<2 | 3>) held to the CPU restatement of tests/outlier_exact.py.

On dyadic clouds (tests/knn_exact.py) every squared distance and every fp64 sum of them is exact, so the per-point
statistic must equal the restatement bit for bit and the radius counts exactly, at every candidate-list capacity
(k = 1 ... 100 covers 32 / 64 / 104 slots and their edges).  Kept index sets may differ only at points whose statistic
lies on the threshold (within 1e-9 of it) or with a neighbour on the search sphere."""
import numpy as np
import pytest
import torch

import knn_exact as kx
import outlier_exact as ox

pytestmark = pytest.mark.gpu

F32 = np.float32
KS = [1, 8, 20, 32, 33, 64, 65, 100]
CLOUDS = {"volume": kx.cloud_volume, "graded": kx.cloud_graded, "sheet": kx.cloud_sheet, "outliers": kx.cloud_outliers}


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a, b):
    """bit equality of two float32 arrays of any shape (tells -0 from +0)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def _check_stat_indices(case, idx, avg_gpu, avg_ref, thr, keep_ref, max_loose=10):
    """kept indices equal the restatement's except points within 1e-9 of the threshold (or within the two statistics'
    difference of it); that set must be tiny"""
    slack = np.maximum(1e-9 * abs(thr), np.abs(avg_gpu.astype(np.float64) - avg_ref.astype(np.float64)))
    loose = (np.abs(avg_ref.astype(np.float64) - thr) <= slack) & (avg_ref > 0)   # (avg = 0 is removed whatever thr is)
    got = np.zeros(len(avg_ref), bool)
    got[_np(idx)] = True
    bad = np.flatnonzero((got != keep_ref) & ~loose)
    assert not len(bad), "%s: %d points kept / removed wrongly, first %d (avg %r, thr %r)" % (
        case, len(bad), bad[0], avg_ref[bad[0]], thr)
    assert loose.sum() <= max_loose, (case, int(loose.sum()))


# ---- per-point exactness on dyadic clouds ---------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("cloud", sorted(CLOUDS))
def test_statistical_avg_bit_exact_on_dyadic_clouds(eng, cloud, k):
    pts = CLOUDS[cloud](40_000, seed=k + 7)
    kx.assert_exact_cumulants(pts, k)
    p, _, _, idx, avg = eng.remove_statistical_outliers(_dev(pts), k, 2.0)
    avg_ref, thr, keep = ox.statistical(pts, k, 2.0)
    assert _bits(_np(avg), avg_ref), "%s k=%d: avg_d2 differs" % (cloud, k)
    _check_stat_indices("%s k=%d" % (cloud, k), idx, _np(avg), avg_ref, thr, keep)
    assert np.array_equal(_np(p), pts[_np(idx)])


@pytest.mark.parametrize("nb", [k - 1 for k in KS if k > 1] + [1])
@pytest.mark.parametrize("cloud", ["graded", "volume", "sheet"])
def test_radius_counts_exact_on_dyadic_clouds(eng, cloud, nb):
    pts = CLOUDS[cloud](40_000, seed=nb + 3)
    steps = int(round(((nb + 1) / (0.008 * 4.19)) ** (1.0 / 3.0)))
    r = kx.dyadic_radius(steps)
    r2 = np.float64(F32(r) * F32(r)) / kx.SCALE ** 2
    assert r2 % 1.0 == 0.25                               # the library's fp32 r*r equals no lattice d2
    p, _, _, idx, cnt = eng.remove_radius_outliers(_dev(pts), nb, r)
    cnt_ref, keep = ox.radius(pts, nb, r)
    assert np.array_equal(_np(cnt), cnt_ref), "%s nb=%d: counts differ" % (cloud, nb)
    assert np.array_equal(_np(idx), np.flatnonzero(keep))


# ---- real data ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fragment():
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fragment_every3rd.npz"))
    return d["points"].astype(F32), d["normals"].astype(F32)


@pytest.mark.parametrize("k,ratio", [(20, 2.0)])
def test_statistical_on_the_fragment(eng, fragment, k, ratio):
    pts, _ = fragment
    _, _, _, idx, avg = eng.remove_statistical_outliers(_dev(pts), k, ratio)
    avg_ref, thr, keep = ox.statistical(pts, k, ratio)
    np.testing.assert_allclose(_np(avg), avg_ref, rtol=1e-5, atol=0)
    _check_stat_indices("fragment k=%d" % k, idx, _np(avg), avg_ref, thr, keep)
    assert np.all(np.diff(_np(idx)) > 0)


@pytest.mark.parametrize("nb,r", [(10, 0.1), (16, 0.05)])
def test_radius_on_the_fragment(eng, fragment, nb, r):
    pts, _ = fragment
    _, _, _, idx, cnt = eng.remove_radius_outliers(_dev(pts), nb, r)
    cnt_ref, keep = ox.radius(pts, nb, r)
    lo, _ = ox.radius(pts, nb, r * (1 - 1e-6))
    hi, _ = ox.radius(pts, nb, r * (1 + 1e-6))
    loose = lo != hi                                       # a neighbour on the sphere
    assert np.array_equal(_np(cnt)[~loose], cnt_ref[~loose])
    got = np.zeros(len(pts), bool)
    got[_np(idx)] = True
    assert np.array_equal(got[~loose], keep[~loose])
    assert loose.sum() <= 10


# ---- attributes, layout, memory kinds -------------------------------------------------------------------------------
def _attr_cloud(n, seed):
    rng = np.random.default_rng(seed)
    pts = rng.random((n, 3), dtype=F32)
    far = rng.choice(n, n // 100, replace=False)
    pts[far] += F32(3.0) * rng.random((len(far), 3), dtype=F32) + F32(2.0)
    return pts, rng.standard_normal((n, 3)).astype(F32), rng.random((n, 3), dtype=F32)


@pytest.mark.parametrize("which", ["statistical", "radius"])
def test_attributes_follow_the_points_on_both_memory_kinds(eng, which):
    pts, nrm, col = _attr_cloud(50_000, 5)
    call = (lambda *a: eng.remove_statistical_outliers(a[0], 20, 2.0, a[1], a[2])) if which == "statistical" else \
        (lambda *a: eng.remove_radius_outliers(a[0], 16, 0.04, a[1], a[2]))
    dp, dn, dc, di, ds = [_np(x) for x in call(_dev(pts), _dev(nrm), _dev(col))]
    hp, hn, hc, hi, hs = call(pts, nrm, col)
    assert isinstance(hp, np.ndarray) and isinstance(hi, np.ndarray)
    for a, b in ((dp, hp), (dn, hn), (dc, hc), (di, hi), (ds, hs)):
        assert _bits(a, b) if a.dtype == F32 else (a.shape == b.shape and np.array_equal(a, b))
    assert 0 < len(di) < len(pts) and np.all(np.diff(di) > 0)
    assert np.array_equal(dp, pts[di]) and np.array_equal(dn, nrm[di]) and np.array_equal(dc, col[di])


# ---- SelectByIndex / UniformDownSample ------------------------------------------------------------------------------
def test_select_by_index_gathers_in_the_order_given(eng):
    pts, nrm, col = _attr_cloud(1000, 1)
    sel = [98, 3, 3, 999, 0, 47, 47, 47, 10]
    for side in (_dev, lambda a: a):
        p, n, c = eng.select_by_index(side(pts), sel if side is not _dev else torch.tensor(sel).cuda(), False,
                                      side(nrm), side(col))
        assert np.array_equal(_np(p), pts[sel]) and np.array_equal(_np(n), nrm[sel]) and np.array_equal(_np(c), col[sel])


def test_select_by_index_inverted_counts_repeats_once(eng):
    pts, nrm, col = _attr_cloud(1000, 2)
    sel = np.array([5, 5, 999, 0, 512, 5, 0])
    want = ox.select(1000, sel, invert=True)
    for side in (_dev, lambda a: a):
        p, n, c = eng.select_by_index(side(pts), sel, True, side(nrm), side(col))
        assert len(_np(p)) == 1000 - 4
        assert np.array_equal(_np(p), pts[want]) and np.array_equal(_np(n), nrm[want]) and np.array_equal(_np(c), col[want])


def test_select_by_index_empty_lists(eng):
    pts, _, _ = _attr_cloud(100, 3)
    p, _, _ = eng.select_by_index(_dev(pts), np.zeros(0, np.int64), False)
    assert len(_np(p)) == 0
    p, _, _ = eng.select_by_index(_dev(pts), np.zeros(0, np.int64), True)
    assert np.array_equal(_np(p), pts)


@pytest.mark.parametrize("bad", [[0, 100], [-1], [5, 1 << 40]])
@pytest.mark.parametrize("invert", [False, True])
def test_select_by_index_out_of_range_is_an_error(eng, bad, invert):
    from cupoch_amd._lib import MiIcpError
    pts, _, _ = _attr_cloud(100, 4)
    with pytest.raises(MiIcpError, match="out of range"):
        eng.select_by_index(_dev(pts), bad, invert)
    p, _, _ = eng.select_by_index(_dev(pts), [1, 2], invert)   # the context is fine afterwards
    assert len(_np(p)) == (98 if invert else 2)


@pytest.mark.parametrize("n,k", [(1000, 7), (1000, 1), (10, 11), (999, 999)])
def test_uniform_downsample(eng, n, k):
    pts, nrm, col = _attr_cloud(n, 6)
    want = ox.uniform(n, k)
    for side in (_dev, lambda a: a):
        p, nn, c = eng.uniform_downsample(side(pts), k, side(nrm), side(col))
        assert len(_np(p)) == n // k
        assert np.array_equal(_np(p), pts[want]) and np.array_equal(_np(nn), nrm[want]) and np.array_equal(_np(c), col[want])


# ---- errors, limits, empty clouds -----------------------------------------------------------------------------------
def test_illegal_parameters_are_errors(eng):
    from cupoch_amd._lib import MiIcpError
    pts = _dev(_attr_cloud(100, 7)[0])
    for call in (lambda: eng.remove_statistical_outliers(pts, 0, 2.0),
                 lambda: eng.remove_statistical_outliers(pts, 20, 0.0),
                 lambda: eng.remove_statistical_outliers(pts, 20, -1.0),
                 lambda: eng.remove_radius_outliers(pts, 0, 0.1),
                 lambda: eng.remove_radius_outliers(pts, 10, 0.0),
                 lambda: eng.remove_radius_outliers(pts, 10, -0.5),
                 lambda: eng.uniform_downsample(pts, 0)):
        with pytest.raises(MiIcpError):
            call()
    with pytest.raises(MiIcpError, match="100"):
        eng.remove_statistical_outliers(pts, 101, 2.0)
    with pytest.raises(MiIcpError, match="100"):
        eng.remove_radius_outliers(pts, 100, 0.1)
    eng.remove_statistical_outliers(pts, 100, 2.0)        # the limits themselves are fine
    eng.remove_radius_outliers(pts, 99, 0.1)


def test_empty_and_tiny_clouds(eng):
    empty = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
    for res in (eng.remove_statistical_outliers(empty, 20, 2.0), eng.remove_radius_outliers(empty, 10, 0.1)):
        assert len(_np(res[0])) == 0 and len(_np(res[3])) == 0
    one = _dev(np.array([[1.0, 2.0, 3.0]], F32))
    p, _, _, idx, avg = eng.remove_statistical_outliers(one, 20, 2.0)
    assert len(_np(p)) == 0 and _np(avg).tolist() == [0.0]
    dup = _dev(np.repeat(np.array([[0.5, 0.5, 0.5]], F32), 50, axis=0))
    p, _, _, idx, avg = eng.remove_statistical_outliers(dup, 8, 2.0)
    assert len(_np(p)) == 0 and (_np(avg) == 0).all()


# ---- context isolation, determinism ---------------------------------------------------------------------------------
def test_the_callers_target_survives_the_filters(eng):
    a = kx.cloud_volume(20_000, seed=1)
    b = kx.cloud_graded(30_000, seed=2)
    q = kx.cloud_sheet(5_000, seed=3)
    eng.set_target(_dev(a))
    i0, d0 = [_np(x) for x in eng.search_knn(_dev(q), 8)[1:]]
    eng.remove_statistical_outliers(_dev(b), 20, 2.0)
    eng.remove_radius_outliers(b, 16, 0.02)
    i1, d1 = [_np(x) for x in eng.search_knn(_dev(q), 8)[1:]]
    assert np.array_equal(i0, i1) and _bits(d0, d1)


def test_outputs_are_deterministic_across_calls_and_contexts(eng):
    from cupoch_amd.engine import Engine
    pts, nrm, col = _attr_cloud(200_000, 9)
    runs = [eng.remove_statistical_outliers(_dev(pts), 20, 2.0, _dev(nrm), _dev(col)) for _ in range(2)]
    fresh = Engine(0)
    try:
        runs.append(fresh.remove_statistical_outliers(_dev(pts), 20, 2.0, _dev(nrm), _dev(col)))
    finally:
        fresh.close()
    ref = [_np(x) for x in runs[0]]
    for r in runs[1:]:
        for a, b in zip(ref, [_np(x) for x in r]):
            assert a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- scale ----------------------------------------------------------------------------------------------------------
def test_two_million_points_with_far_outliers(eng):
    rng = np.random.default_rng(2024)
    n, nfar = 2_000_000, 2_000
    core = rng.random((n, 3), dtype=F32)
    d = rng.standard_normal((nfar, 3))
    far = (0.5 + d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(3.0, 8.0, (nfar, 1))).astype(F32)
    pts = np.concatenate([core, far])
    perm = rng.permutation(len(pts))
    pts = np.ascontiguousarray(pts[perm])
    is_far = np.zeros(len(pts), bool)
    is_far[np.argsort(perm)[n:]] = True                  # positions of the injected points after the shuffle
    _, _, _, idx, avg = eng.remove_statistical_outliers(_dev(pts), 20, 2.0)
    idx, avg = _np(idx), _np(avg)
    assert not is_far[idx].any()
    avg_ref, thr, keep = ox.statistical(pts, 20, 2.0)
    _check_stat_indices("2M statistical", idx, avg, avg_ref, thr, keep)
    r = 2.5 * len(pts) ** (-1.0 / 3.0)
    _, _, _, idx, cnt = eng.remove_radius_outliers(_dev(pts), 16, r)
    idx, cnt = _np(idx), _np(cnt)
    assert not is_far[idx].any()
    cnt_ref, keep = ox.radius(pts, 16, r)
    lo, _ = ox.radius(pts, 16, r * (1 - 1e-6))
    hi, _ = ox.radius(pts, 16, r * (1 + 1e-6))
    loose = lo != hi
    got = np.zeros(len(pts), bool)
    got[idx] = True
    assert np.array_equal(got[~loose], keep[~loose]) and np.array_equal(cnt[~loose], cnt_ref[~loose])
    assert loose.sum() <= 100


# ---- both front ends: the reference's outlier example ---------------------------------------------------------------
def _example_flow(geometry_mod, utility_mod, pts, nrm, ulong):
    pcd = geometry_mod.PointCloud()
    pcd.points = utility_mod.Vector3fVector(pts)
    pcd.normals = utility_mod.Vector3fVector(nrm)
    voxel = pcd.voxel_down_sample(voxel_size=0.02)
    uni = voxel.uniform_down_sample(every_k_points=5)
    out = {}
    for name, (cl, ind) in (("stat", voxel.remove_statistical_outlier(nb_neighbors=20, std_ratio=2.0)),
                            ("radius", voxel.remove_radius_outlier(nb_points=16, radius=0.05))):
        inl = voxel.select_by_index(ind)
        outl = voxel.select_by_index(ind, invert=True)
        out[name] = dict(cl=np.asarray(cl.points.cpu()), ind=np.asarray(ind.cpu()), inl=np.asarray(inl.points.cpu()),
                         inl_n=np.asarray(inl.normals.cpu()), outl=np.asarray(outl.points.cpu()))
        assert len(ind) == len(out[name]["ind"])
    out["voxel"] = np.asarray(voxel.points.cpu())
    out["uni"] = np.asarray(uni.points.cpu())
    out["uni_n"] = np.asarray(uni.normals.cpu())
    return out


def test_the_outlier_example_through_both_front_ends(fragment):
    from cupoch_amd import geometry, pybind as cph, utility
    pts, nrm = fragment
    a = _example_flow(geometry, utility, pts, nrm, utility.ULongVector)
    b = _example_flow(cph.geometry, cph.utility, pts, nrm, cph.utility.ULongVector)
    assert a.keys() == b.keys()
    for key in ("voxel", "uni", "uni_n"):
        assert np.array_equal(a[key], b[key]), key
    v = a["voxel"]
    assert np.array_equal(a["uni"], v[::5][:len(v) // 5])
    for name in ("stat", "radius"):
        for key in a[name]:
            assert np.array_equal(a[name][key], b[name][key]), (name, key)
        r = a[name]
        assert r["ind"].dtype == np.int64 and np.all(np.diff(r["ind"]) > 0) and 0 < len(r["ind"]) < len(v)
        assert np.array_equal(r["cl"], v[r["ind"]]) and np.array_equal(r["inl"], v[r["ind"]])
        both = np.concatenate([r["inl"], r["outl"]])   # inliers and outliers partition the cloud
        assert len(both) == len(v) and np.array_equal(np.unique(both, axis=0), np.unique(v, axis=0))


def test_select_by_index_takes_every_index_form():
    from cupoch_amd import geometry, utility
    pts = _attr_cloud(300, 8)[0]
    pcd = geometry.PointCloud(pts)
    sel = [7, 3, 250, 3]
    for ind in (sel, np.array(sel), torch.tensor(sel), torch.tensor(sel).cuda(), utility.ULongVector(sel)):
        assert np.array_equal(np.asarray(pcd.select_by_index(ind).points.cpu()), pts[sel])
    v = utility.ULongVector(sel)
    assert len(v) == 4 and v.cpu().dtype == np.int64 and np.asarray(v).tolist() == sel
