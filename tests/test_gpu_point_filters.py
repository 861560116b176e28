"""GPU: PointCloud::PassThroughFilter, Crop(AxisAlignedBoundingBox) and RemoveNoneFinitePoints (include/mi_icp.h
mi_icp_pass_through_filter / mi_icp_crop_aabb / mi_icp_remove_none_finite, csrc/select.h), exactly against numpy."""
import numpy as np
import pytest
import torch

import filters_exact as fx

pytestmark = pytest.mark.gpu

F32 = np.float32
BAD = {3: (np.nan, 0), 1000: (np.inf, 1), 1001: (-np.inf, 2), 77_000: (np.nan, 2), 99_999: (np.inf, 0), 100_002: (np.nan, 1)}


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


def _cloud(n=100_003, seed=5, bad=True):
    rng = np.random.default_rng(seed)
    pts, nrm, col = (rng.random((n, 3), dtype=F32) for _ in range(3))
    if bad:
        for i, (v, axis) in BAD.items():
            pts[i, axis] = v
    return pts, nrm, col


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()          # (NaN payloads included)


def _check(got, keep, pts, nrm, col, case):
    p, n, c, idx = got
    want = np.flatnonzero(keep)
    assert np.array_equal(_np(idx), want), case
    assert _same(_np(p), pts[want]), case
    assert (n is None) == (nrm is None) and (c is None) == (col is None), case
    if nrm is not None:
        assert _same(_np(n), nrm[want]), case
    if col is not None:
        assert _same(_np(c), col[want]), case


@pytest.mark.parametrize("device", [True, False])
def test_pass_through(eng, device):
    pts, nrm, col = _cloud()
    put = _dev if device else (lambda a: a)
    lo, hi = float(pts[10, 1]), float(pts[20, 1])                       # bounds that occur in the cloud: inclusive
    lo, hi = min(lo, hi), max(lo, hi)
    for axis, a, b in [(1, lo, hi), (0, 0.25, 0.5), (2, -1.0, 2.0), (2, 0.7, 0.6), (0, float("-inf"), float("inf")),
                       (1, float("nan"), 0.5)]:
        keep = fx.pass_through(pts, axis, a, b)
        _check(eng.pass_through_filter(put(pts), axis, a, b, put(nrm), put(col)), keep, pts, nrm, col, (axis, a, b))
    keep = fx.pass_through(pts, 1, lo, hi)
    assert keep[10] and keep[20] and keep[100_002] and not keep.all()    # the bounds' own points and a NaN are kept
    _check(eng.pass_through_filter(put(pts), 1, lo, hi), keep, pts, None, None, "points alone")
    _check(eng.pass_through_filter(put(pts), 1, lo, hi, colors=put(col)), keep, pts, None, col, "colours alone")
    assert fx.pass_through(pts, 2, 0.7, 0.6).sum() == 1                  # none kept but the NaN of that axis


@pytest.mark.parametrize("device", [True, False])
def test_crop(eng, device):
    pts, nrm, col = _cloud()
    put = _dev if device else (lambda a: a)
    lo, hi = np.minimum(pts[30], pts[40]), np.maximum(pts[30], pts[40])  # two corners that are points of the cloud
    for a, b in [(lo, hi), ([0.1, 0.2, 0.3], [0.6, 0.7, 0.8]), ([-1, -1, -1], [2, 2, 2]), ([5, 5, 5], [6, 6, 6])]:
        keep = fx.crop(pts, a, b)
        _check(eng.crop_aabb(put(pts), a, b, put(nrm), put(col)), keep, pts, nrm, col, (a, b))
    keep = fx.crop(pts, lo, hi)
    assert keep[30] and keep[40] and not keep.all()
    assert fx.crop(pts, [-1, -1, -1], [2, 2, 2]).sum() == len(pts) - 3   # all but the three infinite ones: NaN is kept
    assert fx.crop(pts, [5, 5, 5], [6, 6, 6]).sum() == 0
    _check(eng.crop_aabb(put(pts), lo, hi, normals=put(nrm)), keep, pts, nrm, None, "normals alone")


@pytest.mark.parametrize("device", [True, False])
def test_remove_none_finite(eng, device):
    pts, nrm, col = _cloud()
    put = _dev if device else (lambda a: a)
    for rn, ri in [(True, True), (True, False), (False, True), (False, False)]:
        keep = fx.none_finite(pts, rn, ri)
        assert len(pts) - keep.sum() == 3 * rn + 3 * ri
        _check(eng.remove_none_finite(put(pts), rn, ri, put(nrm), put(col)), keep, pts, nrm, col, (rn, ri))
    clean, _, _ = _cloud(bad=False)
    _check(eng.remove_none_finite(put(clean)), np.ones(len(clean), bool), clean, None, None, "all kept")
    allbad = np.full((1000, 3), np.nan, F32)
    _check(eng.remove_none_finite(put(allbad)), np.zeros(1000, bool), allbad, None, None, "none kept")


def test_empty_clouds_and_refusals(eng):
    from cupoch_amd._lib import MiIcpError
    e = np.zeros((0, 3), F32)
    for got in (eng.pass_through_filter(e, 0, 0.0, 1.0), eng.crop_aabb(e, [0, 0, 0], [1, 1, 1]), eng.remove_none_finite(e),
                eng.pass_through_filter(_dev(e), 0, 0.0, 1.0)):
        assert len(got[0]) == 0 and len(got[3]) == 0
    pts = _dev(np.random.default_rng(0).random((500, 3), dtype=F32))
    for axis in (-1, 3, 7):
        with pytest.raises(MiIcpError):
            eng.pass_through_filter(pts, axis, 0.0, 1.0)
    for a, b in [([0, 0, 0], [1, 1, 0]), ([0, 0, 0], [1, 1, -1]), ([0, 0, 0], [0, 0, 0]), ([0, 0, 0], [1, float("nan"), 1])]:
        with pytest.raises(MiIcpError):
            eng.crop_aabb(pts, a, b)
    assert len(eng.crop_aabb(pts, [0, 0, 0], [1, 1, 1])[0]) == 500


def test_both_front_ends_and_the_in_place_removal(eng):
    from cupoch_amd import geometry, pybind, utility
    pts, nrm, col = _cloud(n=20_011, seed=8, bad=False)
    pts[[5, 900], 0] = np.nan
    pts[12_000, 2] = np.inf
    for mod, util in ((geometry, utility), (pybind.geometry, pybind.utility)):
        pcl = mod.PointCloud()
        pcl.points = util.Vector3fVector(pts)
        pcl.normals = util.Vector3fVector(nrm)
        pcl.colors = util.Vector3fVector(col)
        keep = fx.pass_through(pts, 2, 0.2, 0.4)
        out = pcl.pass_through_filter(2, 0.2, 0.4)
        assert _same(np.asarray(out.points.cpu()), pts[keep]) and _same(np.asarray(out.normals.cpu()), nrm[keep])
        assert _same(np.asarray(out.colors.cpu()), col[keep])
        assert len(pcl.pass_through_filter(3, 0.0, 1.0).points) == 0                     # logged, empty
        box = mod.AxisAlignedBoundingBox(np.array([0.1, 0.1, 0.1], F32), np.array([0.5, 0.9, 0.7], F32))
        keep = fx.crop(pts, [0.1, 0.1, 0.1], [0.5, 0.9, 0.7])
        out = pcl.crop(box)
        assert _same(np.asarray(out.points.cpu()), pts[keep]) and _same(np.asarray(out.colors.cpu()), col[keep])
        assert len(pcl.crop(mod.AxisAlignedBoundingBox(np.zeros(3, F32), np.array([1, 0, 1], F32))).points) == 0
        assert len(pcl.points) == len(pts)
        keep = fx.none_finite(pts)
        back = pcl.remove_none_finite_points()
        assert back is pcl or len(back.points) == len(pcl.points)
        assert len(pcl.points) == len(pts) - 3
        assert _same(np.asarray(pcl.points.cpu()), pts[keep]) and _same(np.asarray(pcl.normals.cpu()), nrm[keep])
        assert _same(np.asarray(pcl.colors.cpu()), col[keep])
        pcl.remove_none_finite_points(False, False)
        assert len(pcl.points) == len(pts) - 3
        whole = pcl.crop(pcl.get_axis_aligned_bounding_box())          # the bounds are inclusive: the cloud's own box keeps it
        assert _same(np.asarray(whole.points.cpu()), pts[keep])
