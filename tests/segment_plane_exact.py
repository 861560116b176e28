"""CPU restatement of PointCloud::SegmentPlane as include/mi_icp.h states it (mi_icp_segment_plane), written from the
header alone: numpy for the fp32 steps, Python integers for the sampler, fractions.Fraction where a rounding could be
taken twice.

  u(seed, j), below(u, k), triple(seed, t, n)   the sampler, in uint64 arithmetic
  triangle_planes(pts, tri)                     ComputeTrianglePlane in fp32, one rounding per operation -> planes, valid
  distances(plane, pts)                         |fma(c, z, fma(b, y, fma(a, x, d)))| in fp32: every product is exact in
                                                fp64, so each fma is "one fp64 add, rounded to fp32"; that rounds twice,
                                                which can differ from the single rounding of a real fma only in the
                                                last place of one step.  Every point whose distance comes within
                                                2^-21 * (|a x| + |b y| + |c z| + |d|) of the threshold -- far more than
                                                three such slips can move it -- is recomputed with exact rationals,
                                                rounded once per fma.
  run(pts, thr, ransac_n, iters, seed)          counts, the selection rule (error sums by math.fsum), the ascending
                                                inlier list, the refit in fp64
  refit(pts, idx)                               GetPlaneFromPoints in fp64

This is a helper module of the suite, not a conftest: tests import it by name."""
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
MASK = (1 << 64) - 1


# ---- the sampler ------------------------------------------------------------------------------------------------------
def u(seed, j):
    z = (seed + (j + 1) * 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def below(x, k):
    return (x * k) >> 64


def triple(seed, t, n):
    seed &= MASK
    i0 = below(u(seed, 3 * t), n)
    i1 = below(u(seed, 3 * t + 1), n - 1)
    if i1 >= i0:
        i1 += 1
    i2 = below(u(seed, 3 * t + 2), n - 2)
    if i2 >= min(i0, i1):
        i2 += 1
    if i2 >= max(i0, i1):
        i2 += 1
    return i0, i1, i2


def triples(seed, iters, n):
    return np.array([triple(seed, t, n) for t in range(iters)], np.int64).reshape(-1, 3)


# ---- the plane of a triple ----------------------------------------------------------------------------------------------
def triangle_planes(pts, tri):
    """pts fp32 [n, 3], tri int [H, 3] -> (planes fp32 [H, 4], valid bool [H]); invalid planes are zero"""
    pts = np.ascontiguousarray(pts, F32)
    p0, p1, p2 = pts[tri[:, 0]], pts[tri[:, 1]], pts[tri[:, 2]]
    with np.errstate(all="ignore"):
        e0, e1 = p1 - p0, p2 - p0
        a = e0[:, 1] * e1[:, 2] - e0[:, 2] * e1[:, 1]
        b = e0[:, 2] * e1[:, 0] - e0[:, 0] * e1[:, 2]
        c = e0[:, 0] * e1[:, 1] - e0[:, 1] * e1[:, 0]
        norm = np.sqrt((a * a + b * b) + c * c)
        assert norm.dtype == F32
        valid = (norm > 0) & (norm < np.inf)
        safe = np.where(valid, norm, F32(1))
        a, b, c = a / safe, b / safe, c / safe
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
    planes = np.stack([a, b, c, d], 1).astype(F32)
    planes[~valid] = 0
    return planes, valid


# ---- the distance -------------------------------------------------------------------------------------------------------
def _round_f32(q):
    """a rational rounded to the nearest fp32 (ties to even), returned as a rational"""
    if q == 0:
        return Fraction(0)
    sign, q = (-1 if q < 0 else 1), abs(q)
    e = q.numerator.bit_length() - q.denominator.bit_length()
    if Fraction(2) ** e > q:
        e -= 1
    ue = max(e - 23, -149)
    m = q / Fraction(2) ** ue
    r = m.numerator // m.denominator
    frac = m - r
    if frac > Fraction(1, 2) or (frac == Fraction(1, 2) and r % 2 == 1):
        r += 1
    return sign * r * Fraction(2) ** ue


def distance_exact(plane, p):
    a, b, c, d = (Fraction(float(v)) for v in plane)
    x, y, z = (Fraction(float(v)) for v in p)
    s = _round_f32(a * x + d)
    s = _round_f32(b * y + s)
    s = _round_f32(c * z + s)
    return F32(float(abs(s)))


def distances(plane, pts, thr=None, exact=False):
    """fp32 distances of all points; those near `thr` (all of them with exact=True) by exact rationals"""
    pts = np.ascontiguousarray(pts, F32)
    a, b, c, d = (np.float64(v) for v in np.asarray(plane, F32))
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))
    s = (a * x + d).astype(F32).astype(np.float64)
    s = (b * y + s).astype(F32).astype(np.float64)
    dist = np.abs((c * z + s).astype(F32))
    if exact:
        redo = np.arange(len(pts))
    elif thr is None:
        return dist
    else:
        mag = np.abs(a * x) + np.abs(b * y) + np.abs(c * z) + abs(d)
        redo = np.flatnonzero(np.abs(dist.astype(np.float64) - float(F32(thr))) <= mag * 2.0 ** -21)
    for i in redo:
        dist[i] = distance_exact(plane, pts[i])
    return dist


def inlier_mask(plane, pts, thr, exact=False):
    return distances(plane, pts, thr, exact) < F32(thr)


# ---- the refit ----------------------------------------------------------------------------------------------------------
def refit(pts, idx):
    """GetPlaneFromPoints of pts[idx] in fp64 -> float64 [4] (not rounded to fp32)"""
    if len(idx) == 0:
        return np.zeros(4)
    q = np.asarray(pts, F32)[idx].astype(np.float64)
    cen = np.array([math.fsum(q[:, k]) for k in range(3)]) / len(q)
    r = q - cen
    xx, xy, xz = math.fsum(r[:, 0] * r[:, 0]), math.fsum(r[:, 0] * r[:, 1]), math.fsum(r[:, 0] * r[:, 2])
    yy, yz, zz = math.fsum(r[:, 1] * r[:, 1]), math.fsum(r[:, 1] * r[:, 2]), math.fsum(r[:, 2] * r[:, 2])
    det_x, det_y, det_z = yy * zz - yz * yz, xx * zz - xz * xz, xx * yy - xy * xy
    if det_x > det_y and det_x > det_z:
        abc = np.array([det_x, xz * yz - xy * zz, xy * yz - xz * yy])
    elif det_y > det_z:
        abc = np.array([xz * yz - xy * zz, det_y, xy * xz - yz * xx])
    else:
        abc = np.array([xy * yz - xz * yy, xy * xz - yz * xx, det_z])
    norm = math.sqrt((abc[0] * abc[0] + abc[1] * abc[1]) + abc[2] * abc[2])
    if not (0 < norm < math.inf):
        return np.zeros(4)
    abc = abc / norm
    return np.array([abc[0], abc[1], abc[2], -((abc[0] * cen[0] + abc[1] * cen[1]) + abc[2] * cen[2])])


# ---- the whole call -----------------------------------------------------------------------------------------------------
class Result:
    pass


def run(pts, thr, ransac_n=3, iters=100, seed=0, exact=False):
    """-> Result with .best (iteration or -1), .count, .inliers (int64 ascending), .ransac (fp32 [4]), .plane (the fp64
    refit), .counts [H], .valid [H], .planes [H, 4], .tied (iterations at the largest count), .sums (their error sums)"""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 3)
    n = len(pts)
    res = Result()
    res.best, res.count, res.ransac = -1, 0, np.zeros(4, F32)
    res.inliers, res.plane = np.zeros(0, np.int64), np.zeros(4)
    res.counts, res.valid, res.planes, res.tied, res.sums = np.zeros(0, np.int64), np.zeros(0, bool), np.zeros((0, 4), F32), [], []
    if ransac_n < 3 or n < ransac_n:
        return res
    H = max(int(iters), 0)
    res.planes, res.valid = triangle_planes(pts, triples(seed, H, n))
    res.counts = np.zeros(H, np.int64)
    for t in range(H):
        if res.valid[t]:
            res.counts[t] = int(inlier_mask(res.planes[t], pts, thr, exact).sum())
    ok = res.valid & (res.counts >= 1)
    if ok.any():
        top = int(res.counts[ok].max())
        res.tied = [int(t) for t in np.flatnonzero(ok & (res.counts == top))]
        res.best = res.tied[0]
        if len(res.tied) > 1:
            for t in res.tied:
                dist = distances(res.planes[t], pts, thr, exact)
                res.sums.append(math.fsum(float(v) for v in dist[dist < F32(thr)]))
            res.best = res.tied[int(np.argmin(res.sums))]      # (argmin keeps the first of equals: the lowest iteration)
        res.count = top
        res.ransac = res.planes[res.best].copy()
    res.inliers = np.flatnonzero(inlier_mask(res.ransac, pts, thr, exact)).astype(np.int64)
    res.plane = refit(pts, res.inliers)
    return res
