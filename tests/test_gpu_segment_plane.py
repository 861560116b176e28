"""GPU: PointCloud::SegmentPlane (include/mi_icp.h mi_icp_segment_plane, csrc/segment_plane.h) held to the CPU restatement
of tests/segment_plane_exact.py.

The winner's iteration, its count, its plane and the inlier list are integers or single fp32 roundings fixed by the
contract: they must EQUAL the restatement's.  Two things carry a bound, both set by the contract and not by what the
kernels give: the tie-break between hypotheses of equal count compares fp64 sums taken in different orders (relative
count * 2^-53, the worst case for non-negative terms), and the refit plane is an fp64 computation rounded to fp32
(2^-22 per component of the unit normal, 2^-22 * max(1, |d|) for d).

Real data (tests/golden/fragment_points.npz, segment_plane(0.02, 3, 1000, seed 0)): the restatement's winner is iteration
484 with 82,355 of the 113,662 points, an inlier share of 0.72456."""
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import knn_exact as kx
import segment_plane_exact as sx
from conftest import ROOT

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIVE = np.array([[1, 1, -1], [2, 2, -5], [-1, -1, 1], [-2, -2, 3], [10, 10, -21]], F32)
REFIT_BOUND = 2.0 ** -22
refit_deviation = {}        # case -> the largest deviation seen (printed by the last test; DESIGN.md records the figure)


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


# ---- scenes -----------------------------------------------------------------------------------------------------------
def _rotation(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    return q


def slab_clutter(n, seed, clutter=0.3, noise=0.004, half=2.0):
    """a tilted slab (Gaussian noise across it) and uniform clutter, shuffled"""
    rng = np.random.default_rng(seed)
    k = int(n * clutter)
    slab = np.column_stack([rng.uniform(-half, half, (n - k, 2)), rng.normal(0, noise, n - k)]) @ _rotation(rng).T
    pts = np.concatenate([slab + rng.uniform(-0.5, 0.5, 3), rng.uniform(-half, half, (k, 3))])
    return pts[rng.permutation(n)].astype(F32)


def two_slabs(n, seed):
    """two parallel slabs of nearly equal support, and a tenth of clutter"""
    rng = np.random.default_rng(seed)
    a = n * 45 // 100
    b = a - max(1, n // 500)
    def sheet(m, z):
        return np.column_stack([rng.uniform(-2, 2, (m, 2)), z + rng.normal(0, 0.004, m)])
    pts = np.concatenate([sheet(a, 0.0), sheet(b, 0.7), rng.uniform(-2, 2, (n - a - b, 3))]) @ _rotation(rng).T
    return pts[rng.permutation(n)].astype(F32)


def one_plane(n, seed):
    """every point on z = x / 2 + y / 4 - 1/8 exactly (dyadic coordinates)"""
    rng = np.random.default_rng(seed)
    xy = np.unique(rng.integers(-512, 513, (n + n // 4 + 8, 2)), axis=0)
    xy = xy[rng.permutation(len(xy))[:n]] * 4
    m = np.column_stack([xy, xy[:, 0] // 2 + xy[:, 1] // 4 - 64])
    return (m * 2.0 ** -9).astype(F32)


# ---- the comparison ---------------------------------------------------------------------------------------------------
def _check(eng, pts, thr, iters, seed, case, ransac_n=3, refit=False, exact=False):
    plane, idx, ransac, best, count = eng.segment_plane(_dev(pts), thr, ransac_n, iters, seed)
    idx = _np(idx)
    r = sx.run(pts, thr, ransac_n, iters, seed, exact=exact)
    print("%s: n=%d iters=%d seed=%d -> best %d (restated %d) count %d (%d) tied %d inliers %d (%d)"
          % (case, len(pts), iters, seed, best, r.best, count, r.count, len(r.tied), len(idx), len(r.inliers)))
    assert idx.dtype == np.int64 and plane.dtype == F32 and plane.shape == (4,)
    assert count == r.count, case
    want = r
    if len(r.tied) > 1:
        # equal counts: the winner reaches the count, its error sum is the smallest up to the order of an fp64 sum of
        # non-negative terms, and where the restated sums are further apart than that the iteration is the restated one
        assert best in r.tied, (case, best, r.tied[:8])
        bound = r.count * 2.0 ** -53
        smin = min(r.sums)
        s_best = r.sums[r.tied.index(best)]
        print("   tie: %d hypotheses, sums %.17g .. %.17g, winner's %.17g" % (len(r.tied), smin, max(r.sums), s_best))
        assert s_best <= smin * (1.0 + bound), (case, s_best, smin)
        rest = [s for t, s in zip(r.tied, r.sums) if t != r.best]
        if smin == 0.0 or min(rest) > smin * (1.0 + bound):
            assert best == r.best, (case, best, r.best)
        if best != r.best:
            want = sx.Result()
            want.ransac = r.planes[best]
            want.inliers = np.flatnonzero(sx.inlier_mask(want.ransac, pts, thr, exact)).astype(np.int64)
    else:
        assert best == r.best, (case, best, r.best)
    assert np.array_equal(ransac, want.ransac), (case, ransac, want.ransac)
    assert len(idx) == len(want.inliers) and np.array_equal(idx, want.inliers), \
        "%s: inlier lists differ (%d vs %d)" % (case, len(idx), len(want.inliers))
    if best >= 0:
        assert count == len(idx), case       # counted and listed under one rounding
    if refit:
        ref = sx.refit(pts, idx)
        dev = np.abs(plane.astype(np.float64) - ref)
        dev[3] /= max(1.0, abs(ref[3]))
        print("   refit: largest deviation %.3g (2^%.1f)" % (dev.max(), np.log2(max(dev.max(), 1e-300))))
        refit_deviation[case] = max(refit_deviation.get(case, 0.0), float(dev.max()))
        assert abs(np.linalg.norm(ref[:3]) - 1) < 1e-12 and ref[np.argmax(np.abs(ref[:3]))] > 0
        assert dev.max() <= REFIT_BOUND, (case, plane, ref)
    return plane, idx, ransac, best, count


# ---- exact ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("iters", [1, 3, 100, 1000, 4097])
def test_slab_and_clutter_at_every_tile_boundary(eng, iters):
    for n, seed in [(1000, 1), (5000, 2)]:
        _check(eng, slab_clutter(n, seed), 0.02, iters, seed, "slab", refit=True)


@pytest.mark.parametrize("n", [3, 5, 1000, 113662])
def test_sizes(eng, n):
    pts = slab_clutter(n, 7) if n > 5 else slab_clutter(50, 7)[:n]
    for seed in (0, 5):
        _check(eng, pts, 0.02, 100, seed, "size %d" % n, refit=n >= 1000)
    if n == 113662:
        _check(eng, pts, 0.02, 4097, 3, "size %d, 4097 iterations" % n, refit=True)


def test_two_million_points(eng):
    pts = slab_clutter(2_000_000, 11, half=4.0)
    _check(eng, pts, 0.02, 100, 1, "2M slab", refit=True)


def test_two_slabs_of_nearly_equal_support(eng):
    for seed in (0, 1, 2):
        _check(eng, two_slabs(20_000, 20 + seed), 0.015, 100, seed, "two slabs", refit=True)


def test_a_cloud_that_is_one_plane(eng):
    pts = one_plane(200, 3)          # (every hypothesis ties: the restatement sums them all with exact rationals)
    for iters in (100, 2049):
        plane, idx, ransac, best, count = _check(eng, pts, 0.01, iters, 2, "one plane", refit=True, exact=True)
        assert count == 200 and len(idx) == 200


@pytest.mark.parametrize("cloud", ["sheet", "volume"])
def test_dyadic_clouds(eng, cloud):
    pts = (kx.cloud_sheet if cloud == "sheet" else kx.cloud_volume)(30_000, seed=5)
    for seed, iters in [(0, 100), (9, 1000)]:
        _check(eng, pts, 0.02, iters, seed, cloud, refit=cloud == "sheet")


# ---- ties -------------------------------------------------------------------------------------------------------------
def test_ties_take_the_smallest_error_sum(eng):
    # small integers: a 9 x 9 grid on z = x + 2 y with two points off the plane, threshold 0.75.  Every valid triple
    # inside the grid holds the 81 grid points; k (1, 2, -1) normalises to planes that differ in the last place with k, so
    # the error sums (rounding residue, 3e-6 to 2e-5 in the restatement) differ too and several hypotheses share each
    g = np.arange(-4, 5)
    grid = np.array([[x, y, x + 2 * y] for x in g for y in g], F32)
    pts = np.concatenate([grid, np.array([[0, 0, 3], [1, 2, -5]], F32)])
    ran = 0
    for seed in range(6):
        plane, idx, ransac, best, count = _check(eng, pts, 0.75, 50, seed, "grid ties", exact=True)
        r = sx.run(pts, 0.75, 3, 50, seed, exact=True)
        ran += len(r.tied) > 1 and len(set(r.sums)) > 1
        assert count == 81
    assert ran == 6
    # the reference's five points: every valid hypothesis holds all five
    for seed in range(6):
        _check(eng, FIVE, 0.01, 10, seed, "five points", exact=True)


# ---- degenerate -------------------------------------------------------------------------------------------------------
def test_degenerate_runs(eng):
    line = np.outer(np.arange(40), [1, 2, -1]).astype(F32)            # collinear: every hypothesis invalid
    plane, idx, ransac, best, count = _check(eng, line, 0.01, 50, 1, "collinear")
    assert best == -1 and count == 0 and len(idx) == 40 and not ransac.any() and not plane.any()
    dup = np.tile(np.array([[1, 2, 3]], F32), (30, 1))                 # duplicates only
    plane, idx, ransac, best, count = _check(eng, dup, 0.01, 20, 1, "duplicates")
    assert best == -1 and len(idx) == 30 and not plane.any()
    pts = slab_clutter(2000, 3)
    plane, idx, ransac, best, count = _check(eng, pts, 0.02, 0, 1, "no iterations", refit=True)
    assert best == -1 and len(idx) == 2000
    plane, idx, ransac, best, count = _check(eng, pts, 0.02, -3, 1, "negative iterations")
    assert best == -1 and len(idx) == 2000
    plane, idx, ransac, best, count = _check(eng, pts, 0.0, 50, 1, "threshold 0")     # strict <: nothing
    assert best == -1 and len(idx) == 0 and not plane.any()
    for ransac_n, cloud in [(2, pts), (0, pts), (3, pts[:2]), (5, pts[:4]), (3, pts[:0])]:
        plane, idx, ransac, best, count = _check(eng, cloud, 0.02, 50, 1, "ransac_n %d, n %d" % (ransac_n, len(cloud)),
                                                 ransac_n=ransac_n)
        assert best == -1 and len(idx) == 0 and not plane.any()
    a = _check(eng, pts, 0.02, 50, 1, "ransac_n 5", ransac_n=5)         # still three points per hypothesis
    b = _check(eng, pts, 0.02, 50, 1, "ransac_n 3")
    assert a[3] == b[3] and np.array_equal(a[1], b[1])


def test_errors(eng):
    from cupoch_amd._lib import MiIcpError
    pts = _dev(slab_clutter(100, 1))
    with pytest.raises(MiIcpError):
        eng.segment_plane(pts, 0.02, 3, 65537, 0)
    plane, idx, ransac, best, count = eng.segment_plane(pts, 0.02, 3, 65536, 0)
    assert best >= 0


# ---- real data --------------------------------------------------------------------------------------------------------
def test_fragment_scan(eng):
    pts = np.load(os.path.join(GOLDEN, "fragment_points.npz"))["points"].astype(F32)
    assert len(pts) == 113662
    plane, idx, ransac, best, count = _check(eng, pts, 0.02, 1000, 0, "fragment", refit=True)
    r = sx.run(pts, 0.02, 3, 1000, 0)
    print("fragment: winner %d, %d inliers, share %.5f" % (r.best, r.count, r.count / len(pts)))
    assert (best, count) == (r.best, r.count) == (484, 82355) and round(count / len(pts), 5) == 0.72456


# ---- properties -------------------------------------------------------------------------------------------------------
def test_same_seed_same_result_and_seeds_matter(eng):
    from cupoch_amd.engine import Engine
    pts = slab_clutter(50_000, 8)
    a = eng.segment_plane(_dev(pts), 0.02, 3, 100, 4)
    b = eng.segment_plane(_dev(pts), 0.02, 3, 100, 4)
    e2 = Engine(0)
    try:
        c = e2.segment_plane(_dev(pts), 0.02, 3, 100, 4)
    finally:
        e2.close()
    for x in (b, c):
        assert a[0].tobytes() == x[0].tobytes() and _np(a[1]).tobytes() == _np(x[1]).tobytes() and a[3:] == x[3:]
    winners = {eng.segment_plane(_dev(pts), 0.02, 3, 3, s)[3] for s in range(8)}
    planes = {eng.segment_plane(_dev(pts), 0.02, 3, 3, s)[2].tobytes() for s in range(8)}
    assert len(planes) > 1 and winners


def test_inliers_lie_within_the_threshold_of_the_ransac_plane(eng):
    from cupoch_amd import geometry, utility
    pts = slab_clutter(40_000, 9)
    plane, idx, ransac, best, count = eng.segment_plane(_dev(pts), 0.02, 3, 100, 1)
    pcd = geometry.PointCloud()
    pcd.points = utility.Vector3fVector(pts)
    sel = np.asarray(pcd.select_by_index(utility.ULongVector(_np(idx))).points.cpu())
    rest = np.asarray(pcd.select_by_index(utility.ULongVector(_np(idx)), invert=True).points.cpu())
    assert len(sel) == count and len(sel) + len(rest) == len(pts)
    assert (sx.distances(ransac, sel, exact=True) < F32(0.02)).all()
    assert (sx.distances(ransac, rest, exact=True) >= F32(0.02)).all()


def test_host_device_and_pinned_memory_agree(eng):
    pts = slab_clutter(30_000, 10)
    d = eng.segment_plane(_dev(pts), 0.02, 3, 100, 2)
    h = eng.segment_plane(pts, 0.02, 3, 100, 2)
    p = eng.segment_plane(torch.from_numpy(pts).pin_memory(), 0.02, 3, 100, 2)
    assert isinstance(h[1], np.ndarray) and h[1].dtype == np.int64 and d[1].is_cuda and d[1].dtype == torch.int64
    for x in (h, p):
        assert d[0].tobytes() == x[0].tobytes() and np.array_equal(_np(d[1]), _np(x[1])) and d[2].tobytes() == x[2].tobytes()
        assert d[3:] == x[3:]


def test_the_callers_target_survives(eng):
    rng = np.random.default_rng(9)
    tgt = rng.random((20_000, 3), dtype=F32)
    q = rng.random((3000, 3), dtype=F32)
    eng.set_target(_dev(tgt))
    before = eng.search_knn(_dev(q), 8)
    eng.segment_plane(_dev(slab_clutter(40_000, 3)), 0.02, 3, 100, 1)
    after = eng.search_knn(_dev(q), 8)
    for x, y in zip(before, after):
        assert np.array_equal(_np(x), _np(y))


# ---- both front ends --------------------------------------------------------------------------------------------------
def test_both_front_ends_on_the_references_test_and_a_ported_pipeline():
    from cupoch_amd import geometry, pybind, utility
    scene = np.concatenate([slab_clutter(20_000, 12, clutter=0.0, noise=0.002),
                            np.random.default_rng(1).normal(0, 0.03, (3000, 3)) + [0.3, 0.2, 0.6]]).astype(F32)
    for mod in (geometry, pybind.geometry):
        ut = utility if mod is geometry else pybind.utility
        pcd = mod.PointCloud()
        pcd.points = ut.Vector3fVector(FIVE)
        plane, inliers = pcd.segment_plane(0.01, 3, 10)
        assert type(inliers).__name__ == "ULongVector" and np.asarray(plane).shape == (4,) and np.asarray(plane).dtype == F32
        assert np.array_equal(np.asarray(pcd.select_by_index(inliers).points.cpu()), FIVE)
        assert len(np.asarray(pcd.select_by_index(inliers, invert=True).points.cpu())) == 0
        plane, inliers = pcd.segment_plane(distance_threshold=0.01, ransac_n=2, num_iterations=10)
        assert not np.asarray(plane).any() and len(np.asarray(inliers.cpu())) == 0
        # remove the floor, cluster the rest
        pcd = mod.PointCloud()
        pcd.points = ut.Vector3fVector(scene)
        plane, idx = pcd.segment_plane(0.01, 3, 100)
        rest = pcd.select_by_index(idx, invert=True)
        labels = np.array(rest.cluster_dbscan(0.02, 10).cpu())
        assert len(np.asarray(idx.cpu())) > 15_000 and len(labels) == len(scene) - len(np.asarray(idx.cpu()))
        assert labels.max() >= 0
    pcd = geometry.PointCloud()
    pcd.points = utility.Vector3fVector(scene)
    a, b = pcd.segment_plane(0.01, 3, 50, seed=5), pcd.segment_plane(0.01, 3, 50, seed=5)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(np.asarray(a[1].cpu()), np.asarray(b[1].cpu()))


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_segment_plane")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_segment_plane.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["five_points_all_seeds"] and r["select_equals_points"] and r["plane_is_x_eq_y"]
    assert r["same_srand_same_result"] and r["ransac_n_2_empty"] and r["too_few_points_empty"]
    assert r["slab_inliers"] > 0.6 * r["slab_points"] and r["slab_normal_z"] > 0.999
    assert "ransac_n should be set to higher than or equal to 3." in out.stderr


def test_zz_report_refit_deviation(eng):
    _check(eng, slab_clutter(20_000, 30), 0.02, 100, 0, "slab", refit=True)      # (so the table is never empty)
    for case, d in sorted(refit_deviation.items()):
        print("refit deviation %-28s %.3g (2^%.1f)" % (case, d, np.log2(max(d, 1e-300))))
    assert refit_deviation and max(refit_deviation.values()) <= REFIT_BOUND
