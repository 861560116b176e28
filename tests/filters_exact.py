"""CPU restatements of PointCloud::FarthestPointDownSample, GaussianFilter, PassThroughFilter, Crop and
RemoveNoneFinitePoints (geometry/pointcloud.cu of the reference), written from the contracts in include/mi_icp.h: numpy.

  fps(pts, k)                          sel[0] = 0; dist = min(dist, d2(., sel[t])); sel[t + 1] = np.argmax(dist) -- the FIRST
                                       maximum, which is the contract's tie rule
  gaussian(pts, r, sigma2, max_nn, normals, colors, dtype)
                                       the weighted means over iss_exact.rows, in float32 or float64; the weights come
                                       from the fp32 d2 the row was chosen by; sums run over a row in its (d2, index) order
  pass_through / crop / none_finite    the keep masks of the three predicates
  lattice(n_side, seed)                every site of an integer lattice, shuffled: most farthest-point steps are exact ties

This is a helper module of the suite, not a conftest: tests import it by name."""
import numpy as np

import iss_exact as ix
import knn_exact as kx
import outlier_exact as ox

F32 = np.float32


def fps(pts, k):
    pts = np.ascontiguousarray(pts, F32)
    n, k = len(pts), int(k)
    assert 0 <= k <= n
    if k == n:
        return np.arange(n, dtype=np.int64)
    sel = np.zeros(k, np.int64)
    dist = np.full(n, np.inf, F32)
    for t in range(k - 1):
        dist = np.minimum(dist, ox.d2_f32(pts, pts[sel[t]][None, :]))
        sel[t + 1] = np.argmax(dist)
    return sel


def gaussian(pts, r, sigma2, max_nn, normals=None, colors=None, dtype=np.float64):
    """([points, normals or None, colors or None] as dtype, counts int32)"""
    pts = np.ascontiguousarray(pts, F32)
    n, dt = len(pts), dtype
    pad, cnt = ix.padded(*ix.rows(pts, r, max_nn), max_nn)
    attrs = [pts, normals, colors]
    total = np.zeros(n, dt)
    sums = [None if a is None else np.zeros((n, 3), dt) for a in attrs]
    for t in range(pad.shape[1]):
        use = t < cnt
        if not use.any():
            break
        j = np.where(use, pad[:, t], 0)
        d2 = ox.d2_f32(pts, pts[j]).astype(dt)
        w = np.where(use, np.exp(dt(-0.5) * d2 / dt(F32(sigma2))), dt(0)).astype(dt)
        total += w
        for s, a in zip(sums, attrs):
            if s is not None:
                s += w[:, None] * np.asarray(a, F32)[j].astype(dt)
    with np.errstate(divide="ignore", invalid="ignore"):
        return [None if s is None else s / total[:, None] for s in sums], cnt


def pass_through(pts, axis_no, min_bound, max_bound):
    v = np.asarray(pts, F32)[:, axis_no]
    return ~((v < F32(min_bound)) | (F32(max_bound) < v))


def crop(pts, min_bound, max_bound):
    p = np.asarray(pts, F32)
    return ~((p < np.asarray(min_bound, F32)) | (p > np.asarray(max_bound, F32))).any(1)


def none_finite(pts, remove_nan=True, remove_infinite=True):
    p = np.asarray(pts, F32)
    drop = (bool(remove_nan) & np.isnan(p).any(1)) | (bool(remove_infinite) & np.isinf(p).any(1))
    return ~drop


def lattice(n_side, seed):
    g = np.stack(np.meshgrid(*[np.arange(n_side)] * 3, indexing="ij"), -1).reshape(-1, 3) - n_side // 2
    return (g[np.random.default_rng(seed).permutation(len(g))] * kx.SCALE).astype(F32)
