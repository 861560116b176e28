"""CPU restatement of the outlier filters and the index selections (geometry/down_sample.cu:40-62,110-129,275-438 of
the reference; the engine's form is described in include/mi_icp.h): numpy + scipy.spatial.cKDTree.

  statistical(pts, k, ratio)  -> (avg, thr, keep):  avg = mean of the k smallest squared distances (the point itself
                                 included, fewer when the cloud is smaller), each distance as the kernel forms it in
                                 fp32, summed in fp64, divided in fp64, rounded once to fp32; mean / std in fp64 in the
                                 reference's own form (the sum of squares over avg > 0 only); keep = avg > 0 & avg < thr
  radius(pts, nb, r)          -> (count, keep):     count = #{d2 < r*r in fp32} capped at nb + 1; keep = count == nb + 1
  select(n, idx, invert)      -> the indices the selection yields (a gather, or the complement ascending)
  brute_*                     the same from a full O(n^2) distance matrix (small clouds only)

This is a helper module of the suite, not a conftest: tests import it by name."""
import numpy as np
from scipy.spatial import cKDTree

F32 = np.float32
CHUNK = 1 << 16


def d2_f32(q, p):
    """the kernel's squared distance (device_utils.h sq3: fma(dz, dz, fma(dy, dy, dx * dx)) in fp32), restated with
    the products exact in fp64 and one rounding per fma"""
    d = (q.astype(F32) - p.astype(F32)).astype(np.float64)
    a = (d[..., 0] * d[..., 0]).astype(F32).astype(np.float64)
    a = (d[..., 1] * d[..., 1] + a).astype(F32).astype(np.float64)
    return (d[..., 2] * d[..., 2] + a).astype(F32)


def mean_d2(d2_rows, cnt):
    """fp32 [n, k] squared distances (the first cnt[i] of row i used) -> fp32 mean, fp64 sum divided in fp64"""
    k = d2_rows.shape[1]
    used = np.arange(k)[None, :] < cnt[:, None]
    s = np.where(used, d2_rows.astype(np.float64), 0.0).sum(1)
    return np.where(cnt > 0, s / np.maximum(cnt, 1), 0.0).astype(F32)


def threshold(avg, ratio):
    """down_sample.cu:395-418: mean over all points, the sum of squares over avg > 0, std over n - 1"""
    n = len(avg)
    if n < 2:
        return -np.inf
    a = avg.astype(np.float64)
    mean = a.sum() / n
    sq = ((a[a > 0] - mean) ** 2).sum()
    return mean + float(ratio) * np.sqrt(sq / (n - 1))


def _knn_rows(pts, k):
    """the k nearest of every point (itself included) as fp32 squared distances [n, k'] with k' = min(k, n)"""
    pts = np.ascontiguousarray(pts, F32)
    k = min(k, len(pts))
    tree = cKDTree(pts.astype(np.float64))
    out = np.empty((len(pts), k), F32)
    for s in range(0, len(pts), CHUNK):
        q = pts[s:s + CHUNK]
        _, idx = tree.query(q.astype(np.float64), k)
        idx = np.asarray(idx).reshape(len(q), k)
        out[s:s + len(q)] = np.sort(d2_f32(q[:, None, :], pts[idx]), axis=1)
    return out


def statistical(pts, k, ratio):
    n = len(pts)
    if n == 0:
        return np.zeros(0, F32), -np.inf, np.zeros(0, bool)
    rows = _knn_rows(pts, k)
    avg = mean_d2(rows, np.full(n, rows.shape[1]))
    thr = threshold(avg, ratio)
    return avg, thr, (avg > 0) & (avg.astype(np.float64) < thr)


def radius(pts, nb, r):
    """counts of points with fp32 d2 < fp32 r*r (itself included), capped at nb + 1"""
    pts = np.ascontiguousarray(pts, F32)
    n, K = len(pts), nb + 1
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, bool)
    r2 = F32(r) * F32(r)
    tree = cKDTree(pts.astype(np.float64))
    kk = min(K, n)
    cnt = np.empty(n, np.int32)
    for s in range(0, n, CHUNK):
        q = pts[s:s + CHUNK]
        dist, idx = tree.query(q.astype(np.float64), kk, distance_upper_bound=float(r) * 1.001 + 1e-12)
        dist, idx = np.asarray(dist).reshape(len(q), kk), np.asarray(idx).reshape(len(q), kk)
        have = np.isfinite(dist)
        d2 = d2_f32(q[:, None, :], pts[np.where(have, idx, 0)])
        cnt[s:s + len(q)] = (have & (d2 < r2)).sum(1)
    return cnt, cnt >= K


def select(n, idx, invert=False):
    idx = np.asarray(idx, np.int64).reshape(-1)
    if not invert:
        return idx
    keep = np.ones(n, bool)
    keep[idx] = False
    return np.flatnonzero(keep)


def uniform(n, k):
    return np.arange(n // k, dtype=np.int64) * k


# ---- O(n^2) restatements (small clouds) ------------------------------------------------------------------------------
def brute_d2(pts):
    pts = np.asarray(pts, F32)
    return d2_f32(pts[:, None, :], pts[None, :, :])


def brute_statistical(pts, k, ratio):
    n = len(pts)
    if n == 0:
        return np.zeros(0, F32), -np.inf, np.zeros(0, bool)
    D = np.sort(brute_d2(pts), axis=1)[:, :min(k, n)]
    avg = np.array([np.float64(sum(float(v) for v in row)) / len(row) for row in D], np.float64).astype(F32)
    thr = threshold(avg, ratio)
    return avg, thr, (avg > 0) & (avg.astype(np.float64) < thr)


def brute_radius(pts, nb, r):
    r2 = F32(r) * F32(r)
    cnt = np.minimum((brute_d2(pts) < r2).sum(1), nb + 1).astype(np.int32)
    return cnt, cnt >= nb + 1


def near_threshold(avg, thr, rel=1e-9):
    """points whose statistic lies within rel of the threshold: their keep flag may go either way"""
    return np.abs(avg.astype(np.float64) - thr) <= rel * abs(thr)
