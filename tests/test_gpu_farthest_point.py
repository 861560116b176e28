"""GPU: PointCloud::FarthestPointDownSample (include/mi_icp.h mi_icp_farthest_point_downsample, csrc/farthest_point.h)
held to the CPU restatement of tests/filters_exact.py.

The selection is compared at EVERY position, exactly: given the fp32 d2 of the header, min and compare are exact, and
ties go to the lowest index -- there is no undecided set."""
import os

import numpy as np
import pytest
import torch

import filters_exact as fx
import knn_exact as kx

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


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


def _check(eng, pts, k, case, device=True):
    p, n, c, idx = eng.farthest_point_downsample(_dev(pts) if device else pts, k)
    idx = _np(idx)
    want = fx.fps(pts, k)
    assert idx.dtype == np.int64 and idx.shape == (k,), case
    bad = np.flatnonzero(idx != want)
    assert not len(bad), "%s: %d of %d selections differ, first at position %d (%d vs %d)" % (
        case, len(bad), k, bad[0], idx[bad[0]], want[bad[0]])
    assert np.array_equal(_np(p), pts[want]) and n is None and c is None, case
    return idx


@pytest.mark.parametrize("cloud", ["volume", "sheet", "duplicates", "outliers"])
def test_dyadic_clouds(eng, cloud):
    make = {"volume": kx.cloud_volume, "sheet": kx.cloud_sheet, "duplicates": kx.cloud_duplicates, "outliers": kx.cloud_outliers}[cloud]
    pts = make(20_000, seed=11)
    _check(eng, pts, 500, cloud)


def test_lattice_where_most_steps_tie(eng):
    pts = fx.lattice(16, seed=3)                     # 4096 sites
    idx = _check(eng, pts, 1500, "lattice")
    assert len(set(idx.tolist())) == 1500
    # the ties are real: at most steps more than one point holds the largest distance
    import outlier_exact as ox
    dist = np.full(len(pts), np.inf, F32)
    ties = 0
    for t in range(300):
        dist = np.minimum(dist, ox.d2_f32(pts, pts[idx[t]][None, :]))
        ties += int((dist == dist.max()).sum() > 1)
    assert ties > 150


def test_duplicates_repeat_index_zero(eng):
    base = np.random.default_rng(2).random((40, 3), dtype=F32)
    pts = np.repeat(base, 5, axis=0)
    idx = _check(eng, pts, 70, "five copies of 40 points")
    assert len(set(idx[:40].tolist())) == 40 and (idx[40:] == 0).all()


@pytest.mark.parametrize("k", [1, 2, 64, 1000])
def test_fragment_scan(eng, k):
    pts = np.load(os.path.join(GOLDEN, "fragment_every3rd.npz"))["points"].astype(F32)
    _check(eng, pts, k, "fragment k=%d" % k)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000, 262_144 + 77])
def test_sizes_around_the_wave_and_the_block(eng, n):
    pts = np.random.default_rng(n).random((n, 3), dtype=F32)
    for k in sorted({1, min(2, n), min(n, 40), n - 1 if n < 2000 else 40} - {0}):
        _check(eng, pts, k, "n=%d k=%d" % (n, k))


def test_two_million_points(eng):
    rng = np.random.default_rng(7)
    centres = rng.uniform(-40, 40, (300, 3))
    pts = np.concatenate([centres[rng.integers(0, 300, 1_900_000)] + rng.normal(0, 0.8, (1_900_000, 3)),
                          rng.uniform(-45, 45, (100_000, 3))]).astype(F32)
    pts = pts[rng.permutation(len(pts))]
    _check(eng, pts, 256, "2M blobs")


def test_all_none_and_too_many(eng):
    from cupoch_amd._lib import MiIcpError
    rng = np.random.default_rng(4)
    pts, nrm, col = (rng.random((3001, 3), dtype=F32) for _ in range(3))
    p, n, c, idx = eng.farthest_point_downsample(_dev(pts), 3001, _dev(nrm), _dev(col))
    assert np.array_equal(_np(idx), np.arange(3001)) and np.array_equal(_np(p), pts)
    assert np.array_equal(_np(n), nrm) and np.array_equal(_np(c), col)
    p, n, c, idx = eng.farthest_point_downsample(_dev(pts), 0, _dev(nrm))
    assert len(p) == 0 and len(n) == 0 and c is None and len(idx) == 0
    p, _, _, idx = eng.farthest_point_downsample(np.zeros((0, 3), F32), 0)
    assert len(p) == 0 and len(idx) == 0
    for k in (3002, 10 ** 9, -1):
        with pytest.raises(MiIcpError):
            eng.farthest_point_downsample(_dev(pts), k)
    with pytest.raises(MiIcpError):
        eng.farthest_point_downsample(np.zeros((0, 3), F32), 1)
    _check(eng, pts, 10, "after the refusals")


def test_attributes_memory_kinds_determinism_and_the_callers_target(eng):
    from cupoch_amd.engine import Engine
    rng = np.random.default_rng(9)
    pts = np.load(os.path.join(GOLDEN, "fragment_every3rd.npz"))["points"].astype(F32)
    nrm, col = rng.random(pts.shape, dtype=F32), rng.random(pts.shape, dtype=F32)
    tgt, q = rng.random((20_000, 3), dtype=F32), rng.random((3000, 3), dtype=F32)
    eng.set_target(_dev(tgt))
    before = eng.search_knn(_dev(q), 8)
    want = fx.fps(pts, 300)
    d = eng.farthest_point_downsample(_dev(pts), 300, _dev(nrm), _dev(col))
    h = eng.farthest_point_downsample(pts, 300, nrm, col)
    after = eng.search_knn(_dev(q), 8)
    for x, y in zip(before, after):
        assert np.array_equal(_np(x), _np(y))
    assert all(t.is_cuda for t in d) and all(isinstance(a, np.ndarray) for a in h)
    d2 = eng.farthest_point_downsample(_dev(pts), 300, _dev(nrm), _dev(col))
    e2 = Engine(0)
    try:
        d3 = e2.farthest_point_downsample(_dev(pts), 300, _dev(nrm), _dev(col))
    finally:
        e2.close()
    for got in (d, h, d2, d3):
        assert np.array_equal(_np(got[3]), want)
        assert np.array_equal(_np(got[0]), pts[want]) and np.array_equal(_np(got[1]), nrm[want])
        assert np.array_equal(_np(got[2]), col[want])
    p, n, c, _ = eng.farthest_point_downsample(_dev(pts), 50, colors=_dev(col))
    assert n is None and np.array_equal(_np(c), col[want[:50]])


def test_non_finite_coordinates_terminate_with_indices_in_range(eng):
    pts = np.random.default_rng(5).random((5000, 3), dtype=F32)
    pts[[17, 400], 1] = np.nan
    pts[3000, 0] = np.inf
    _, _, _, idx = eng.farthest_point_downsample(_dev(pts), 64)
    idx = _np(idx)
    assert idx[0] == 0 and (idx >= 0).all() and (idx < 5000).all()
    assert (idx[1:] == 17).all()                  # the header: the lowest index with a non-finite coordinate, every time


def test_both_front_ends(eng):
    from cupoch_amd import geometry, pybind, utility
    pts = np.load(os.path.join(GOLDEN, "fragment_every3rd.npz"))["points"].astype(F32)
    rng = np.random.default_rng(2)
    nrm, col = rng.random(pts.shape, dtype=F32), rng.random(pts.shape, dtype=F32)
    want = fx.fps(pts, 200)
    for mod, util in ((geometry, utility), (pybind.geometry, pybind.utility)):
        pcl = mod.PointCloud()
        pcl.points = util.Vector3fVector(pts)
        pcl.normals = util.Vector3fVector(nrm)
        pcl.colors = util.Vector3fVector(col)
        out = pcl.farthest_point_down_sample(200)
        assert np.array_equal(np.asarray(out.points.cpu()), pts[want])
        assert np.array_equal(np.asarray(out.normals.cpu()), nrm[want]) and np.array_equal(np.asarray(out.colors.cpu()), col[want])
        assert len(pcl.farthest_point_down_sample(0).points) == 0
        assert len(pcl.farthest_point_down_sample(len(pts) + 1).points) == 0          # logged, empty
        small = mod.PointCloud()
        small.points = util.Vector3fVector(pts[:100])
        assert np.array_equal(np.asarray(small.farthest_point_down_sample(100).points.cpu()), pts[:100])
