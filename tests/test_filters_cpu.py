"""CPU: the restatements of tests/filters_exact.py against brute force on small clouds (no GPU)."""
import numpy as np

import filters_exact as fx
import knn_exact as kx
import outlier_exact as ox

F32 = np.float32


def _fps_literal(pts, k):
    """the contract, point by point: O(n k) Python"""
    n = len(pts)
    if k == n:
        return list(range(n))
    D = ox.brute_d2(pts)
    sel, dist = [0] if k else [], [np.inf] * n
    for t in range(k - 1):
        s = sel[t]
        best, arg = -1.0, -1
        for i in range(n):
            dist[i] = min(dist[i], float(D[i, s]))
            if dist[i] > best:              # strictly: the first largest stays
                best, arg = dist[i], i
        sel.append(arg)
    return sel


def test_fps_against_the_literal_loop():
    rng = np.random.default_rng(0)
    for n, k in [(1, 1), (2, 1), (2, 2), (50, 7), (200, 64), (333, 100)]:
        pts = rng.random((n, 3), dtype=F32)
        assert fx.fps(pts, k).tolist() == _fps_literal(pts, k), (n, k)
    assert len(fx.fps(rng.random((10, 3), dtype=F32), 0)) == 0


def test_fps_ties_go_to_the_lowest_index_on_a_lattice():
    pts = fx.lattice(6, seed=1)                                   # 216 sites: distances are exact, most steps tie
    sel = fx.fps(pts, 100)
    assert sel.tolist() == _fps_literal(pts, 100)
    dist = np.full(len(pts), np.inf, F32)
    ties = 0
    for t in range(99):
        dist = np.minimum(dist, ox.d2_f32(pts, pts[sel[t]][None, :]))
        top = np.flatnonzero(dist == dist.max())
        ties += len(top) > 1
        assert sel[t + 1] == top[0]
    assert ties > 50
    assert len(set(sel.tolist())) == 100


def test_fps_duplicates_repeat_index_zero_once_distances_are_spent():
    base = np.random.default_rng(2).random((5, 3), dtype=F32)
    pts = np.repeat(base, 4, axis=0)                               # 20 points, 5 distinct
    sel = fx.fps(pts, 12)
    assert sel.tolist() == _fps_literal(pts, 12)
    assert len(set(sel[:5].tolist())) == 5 and (sel[5:] == 0).all()
    assert (sel[:5] % 4 == 0).all()                                # the first copy of every distinct point


def test_fps_all_points_is_the_identity():
    pts = np.random.default_rng(3).random((17, 3), dtype=F32)
    assert fx.fps(pts, 17).tolist() == list(range(17))


def _gaussian_brute(pts, r, sigma2, max_nn, attrs, dtype):
    D = ox.brute_d2(pts)
    r2 = F32(r) * F32(r)
    out = [np.zeros((len(pts), 3), dtype) for _ in attrs]
    cnt = np.zeros(len(pts), np.int32)
    for i in range(len(pts)):
        row = sorted((float(D[i, j]), j) for j in range(len(pts)) if D[i, j] < r2)[:max_nn]
        cnt[i] = len(row)
        total = dtype(0)
        acc = [np.zeros(3, dtype) for _ in attrs]
        for d2, j in row:
            w = np.exp(dtype(-0.5) * dtype(F32(d2)) / dtype(F32(sigma2)))
            total = dtype(total + w)
            for a, src in zip(acc, attrs):
                a += w * src[j].astype(dtype)
        for o, a in zip(out, acc):
            o[i] = a / total
    return out, cnt


def test_gaussian_against_brute_force_rows():
    rng = np.random.default_rng(4)
    pts = kx.cloud_duplicates(300, seed=5)
    nrm, col = rng.random((300, 3), dtype=F32), rng.random((300, 3), dtype=F32)
    for max_nn in (1, 3, 5, 40):
        r, sigma2 = 24 * kx.SCALE, 0.002
        for dt in (np.float64, F32):
            got, cnt = fx.gaussian(pts, r, sigma2, max_nn, nrm, col, dt)
            want, wcnt = _gaussian_brute(pts, r, sigma2, max_nn, [pts, nrm, col], dt)
            assert np.array_equal(cnt, wcnt)
            for g, w in zip(got, want):
                assert g.dtype == dt
                np.testing.assert_allclose(g, w, rtol=1e-12 if dt is np.float64 else 2e-6)
        if max_nn == 1:                                            # the point alone: itself
            assert np.array_equal(fx.gaussian(pts, r, sigma2, 1, dtype=F32)[0][0], pts)
        elif max_nn < 40:                                          # some rows are truncated, some are not
            assert cnt.max() == max_nn and (cnt < max_nn).any()
        else:
            assert 5 < cnt.max() < 40
    p_only, _ = fx.gaussian(pts, 24 * kx.SCALE, 0.002, 40)
    assert p_only[1] is None and p_only[2] is None


def test_predicates_and_their_nan_rule():
    pts = np.array([[0, 0, 0], [1, 2, 3], [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf], [1, 1, 1], [2, 2, 2]], F32)
    assert fx.pass_through(pts, 0, 0, 1).tolist() == [True, True, True, True, True, True, False]     # NaN is kept
    assert fx.pass_through(pts, 1, 1, 2).tolist() == [False, True, False, False, False, True, True]  # inclusive bounds
    assert fx.pass_through(pts, 2, 5, 4).tolist() == [False] * 7
    assert fx.crop(pts, [0, 0, 0], [1, 2, 3]).tolist() == [True, True, True, False, False, True, False]
    assert fx.none_finite(pts).tolist() == [True, True, False, False, False, True, True]
    assert fx.none_finite(pts, True, False).tolist() == [True, True, False, True, True, True, True]
    assert fx.none_finite(pts, False, True).tolist() == [True, True, True, False, False, True, True]
    assert fx.none_finite(pts, False, False).all()
