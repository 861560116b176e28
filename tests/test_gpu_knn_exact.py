"""GPU: the k-NN kernels (csrc/knn_normals.h) held to exact references at every point, at every candidate-list
capacity (32 / 64 / 104 slots) and at sizes where the per-XCD index slab hands rows to a second owner (more than
10,304 x 64 = 659,456 queries or points on a 256-CU MI355X).

EstimateNormals on dyadic clouds is compared BIT FOR BIT with the restatement of knn_exact.py on every point whose
neighbour set is unambiguous; colour gradients per point against the fp64 reference; KDTreeFlann rows against the
oracle's.  No case allows a percentage of wrong points."""
import numpy as np
import pytest
import torch

import knn_exact as kx
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

F32 = np.float32
BIG = 700_000                  # > 659,456: every capacity's slab is reused within one launch
STATS = []                     # (case, points, ambiguous) -- printed at the end of the module (pytest -s)


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()
    for row in STATS:
        print("knn-exact %-40s points %8d  ambiguous %7d  checked %.4f" % (row[0], row[1], row[2], 1 - row[2] / max(row[1], 1)))


def radius_steps(max_nn):
    """lattice steps at which cloud_graded's core holds about max_nn neighbours"""
    return int(round((max_nn / (0.008 * 4.19)) ** (1.0 / 3.0)))


def check_normals(case, got, pts, k, radius=None, extra=0, min_checked=0.0):
    """bit-exact on every unambiguous point (the ambiguous rest: finite); at least min_checked of them unambiguous"""
    got = np.asarray(got.cpu().numpy() if isinstance(got, torch.Tensor) else got, F32)
    idx, cnt, _, amb = kx.neighbour_sets(pts, k, radius=radius, extra=extra)
    want = kx.restated_normals(pts, idx, cnt, device=0)
    same = kx.bits_equal(got, want)
    bad = np.flatnonzero(~same & ~amb)
    assert not len(bad), "%s: %d unambiguous points differ, first %d: got %s want %s (count %d)" % (
        case, len(bad), bad[0], got[bad[0]], want[bad[0]], cnt[bad[0]])
    assert (1 - amb.mean()) >= min_checked, (case, float(amb.mean()))
    assert np.isfinite(got).all()
    STATS.append((case, len(pts), int(amb.sum())))
    return cnt


# ---- EstimateNormals(Radius) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_nn", [16, 32, 33, 64, 65, 100])
@pytest.mark.parametrize("n", [30_000, BIG])
def test_radius_normals_bit_exact(eng, max_nn, n):
    pts = kx.cloud_graded(n, seed=max_nn + n)
    kx.assert_exact_cumulants(pts, max_nn)
    r = kx.dyadic_radius(radius_steps(max_nn))
    got = eng.estimate_normals_radius(torch.from_numpy(pts).cuda(), r, max_nn)
    cnt = check_normals("radius n=%d max_nn=%d" % (n, max_nn), got, pts, max_nn, radius=r)
    assert (cnt < 3).any() and (cnt == max_nn).any()            # the fallback and full lists both happen
    got = got.cpu().numpy()
    assert (got[cnt < 3] == F32([0, 0, 1])).all()


def test_radius_normals_on_a_sheet(eng):
    pts = kx.cloud_sheet(30_000, seed=3)
    for max_nn, steps in ((16, 6), (65, 12)):
        r = kx.dyadic_radius(steps)
        check_normals("sheet radius max_nn=%d" % max_nn, eng.estimate_normals_radius(pts, r, max_nn), pts, max_nn,
                      radius=r)


# ---- EstimateNormals(KNN) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 30, 32, 33, 64, 65, 100])
def test_knn_normals_bit_exact(eng, k):
    pts = kx.cloud_volume(BIG, seed=100 + k)
    kx.assert_exact_cumulants(pts, k)
    got = eng.estimate_normals_knn(torch.from_numpy(pts).cuda(), k)
    check_normals("knn n=%d k=%d" % (BIG, k), got, pts, k, min_checked=0.5)


# ---- edge shapes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 7, 63, 64, 65, 511, 513, 64 * 10938 - 1, 64 * 10938 + 1])
def test_knn_normals_edge_sizes(eng, n):
    pts = kx.cloud_volume(n, seed=n)
    for k in ((3, 30, 100) if n < 1000 else (33,)):
        check_normals("edge n=%d k=%d" % (n, k), eng.estimate_normals_knn(pts, k), pts, k)


def test_fewer_points_than_neighbours(eng):
    pts = kx.cloud_volume(50, seed=50)
    for k in (64, 100):
        got = eng.estimate_normals_knn(pts, k)
        check_normals("n=50 k=%d" % k, got, pts, k)
        got = eng.estimate_normals_radius(pts, kx.dyadic_radius(300), k)
        check_normals("n=50 radius max_nn=%d" % k, got, pts, k, radius=kx.dyadic_radius(300))


def test_exact_duplicates(eng):
    pts = kx.cloud_duplicates(200_000, seed=7)
    for k in (3, 30, 65, 100):
        check_normals("duplicates k=%d" % k, eng.estimate_normals_knn(pts, k), pts, k, extra=4, min_checked=0.5)


@pytest.mark.parametrize("k", [30, 100])
def test_outliers_walk_alone(eng, k):
    """far points around a dense core: their lanes leave the packet's walk (knn_walks_alone) or the whole packet does
    (knn_packet_reaches_too_far) and walk alone -- their normals are the exact ones all the same"""
    pts = kx.cloud_outliers(300_000, seed=k)
    check_normals("outliers k=%d" % k, eng.estimate_normals_knn(pts, k), pts, k, min_checked=0.5)


# ---- colour gradients -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_nn,n", [(5, 200_000), (30, 200_000), (33, BIG), (64, BIG), (100, BIG)])
def test_colour_gradients_every_point(eng, max_nn, n):
    pts, nrm, col, radius = kx.gradient_cloud(n, max_nn, seed=max_nn)
    eng.set_target(pts, nrm)
    eng.set_source(pts[:10])
    eng.set_target_colors(col)
    eng.set_source_colors(col[:10])
    got = np.asarray(eng.compute_color_gradients(radius, max_nn), np.float64)
    idx, cnt, _, amb = kx.neighbour_sets(pts, max_nn, radius=radius)
    ref, tol, zero = kx.gradient_reference(pts, nrm, orc.intensity(col), idx, cnt)
    assert np.array_equal((got == 0).all(1), zero), "fewer than four others -> exactly zero: the sets differ"
    assert zero.any() and not zero.all()
    err = np.abs(got - ref).max(1) / tol
    err[amb] = 0.0                                     # (a tie at the max_nn-th distance: either set is valid)
    assert err.max() <= 1.0, (float(err.max()), int(err.argmax()), got[err.argmax()], ref[err.argmax()])
    STATS.append(("gradients n=%d max_nn=%d" % (len(pts), max_nn), len(pts), int(amb.sum())))


# ---- KDTreeFlann at slab-reuse scale ----------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 32, 33, 64, 65, 100])
def test_search_knn_at_slab_reuse_scale(eng, k):
    rng = np.random.default_rng(k)
    tgt = rng.random((400_000, 3), dtype=F32)
    qry = (rng.random((BIG, 3), dtype=F32) * F32(1.1) - F32(0.05)).astype(F32)
    eng.set_target(tgt)
    found, idx, d2 = eng.search_knn(qry, k)
    assert found == BIG * k
    tree = orc.Tree(tgt)
    try:
        for s in range(0, BIG, 100_000):
            _, oi, od = tree.search_knn(qry[s:s + 100_000], k)
            kx.rows_equal_up_to_ties(idx[s:s + 100_000], d2[s:s + 100_000], oi, od, tgt, qry[s:s + 100_000])
    finally:
        tree.close()
    STATS.append(("search knn k=%d" % k, BIG, 0))


def test_search_radius_at_slab_reuse_scale(eng):
    rng = np.random.default_rng(9)
    tgt = rng.random((400_000, 3), dtype=F32)
    qry = tgt[rng.integers(0, len(tgt), BIG)] + rng.normal(0, 0.003, (BIG, 3)).astype(F32)
    radius, max_nn = 0.04, 100
    eng.set_target(tgt)
    found, idx, d2 = eng.search_knn(qry, max_nn, radius)
    tree = orc.Tree(tgt)
    total = 0
    try:
        for s in range(0, BIG, 100_000):
            r, oi, od = tree.search_radius(qry[s:s + 100_000], radius, max_nn)
            total += r
            kx.rows_equal_up_to_ties(idx[s:s + 100_000], d2[s:s + 100_000], oi, od, tgt, qry[s:s + 100_000])
    finally:
        tree.close()
    assert found == total
    n_found = np.isfinite(d2).sum(1)
    assert (n_found == max_nn).any() and (n_found < max_nn).any()
    STATS.append(("search radius max_nn=%d" % max_nn, BIG, 0))


# ---- no state carried between calls -----------------------------------------------------------------------------
def test_no_state_carried_between_calls(eng):
    """one engine runs normals and searches at k = 100, 30, 64 and 100 again on other data; every result is bit-equal
    to the same call on a fresh engine (stale slab rows or staging would show)"""
    from cupoch_amd.engine import Engine
    seq = [(100, 1), (30, 2), (64, 3), (100, 4)]
    clouds = {s: kx.cloud_volume(400_000, seed=1000 + s) for _, s in seq}
    qry = {s: kx.cloud_volume(200_000, seed=2000 + s) for _, s in seq}
    warm = []
    for k, s in seq:
        nrm = eng.estimate_normals_knn(clouds[s], k)
        eng.set_target(clouds[s])
        warm.append((nrm, eng.search_knn(qry[s], k)))
    for (k, s), (nrm, (found, idx, d2)) in zip(seq, warm):
        e = Engine(0)
        try:
            n2 = e.estimate_normals_knn(clouds[s], k)
            e.set_target(clouds[s])
            f2, i2, q2 = e.search_knn(qry[s], k)
        finally:
            e.close()
        assert kx.bits_equal(nrm, n2).all(), k
        assert found == f2 and np.array_equal(idx, i2) and np.array_equal(d2.view(np.uint32), q2.view(np.uint32)), k
