"""CPU restatement of geometry::keypoint::ComputeISSKeypoints (geometry/iss_keypoints.cu of the reference), written from
the contract in include/mi_icp.h (mi_icp_iss_keypoints): numpy + scipy.

  resolution(pts)                      the model resolution and the two radii derived from it
  rows(pts, r, max_neighbors)          CSR (indptr, idx): SearchRadius(r, max_neighbors) of every point, fp32 d2 < r*r,
                                       the max_neighbors smallest by (d2, index) (dbscan_exact.rows: the same convention)
  cumulants / covariance / eigenvalues steps 3 of the contract in the arithmetic asked for: dtype float32 or float64,
                                       coordinates relative to the query point (the engine's form) or raw (the reference's)
  gates(eig, cnt, ...)                 step 4 in numpy float32 (or float64) from given eigenvalues and counts
  suppress(sal, indptr, idx)           step 5 from a given saliency array
  iss(pts, ...)                        the whole detector; a dict of mask, saliency, eig, counts, radii and both rows
  undecided(res, ...)                  the points whose mask an fp32 rounding may decide either way

The fp32 sums run over a row in its (d2, index) order; the contract leaves the engine's order open, so fp32 eigenvalues
are compared within a tolerance and everything discrete is checked from the engine's own eigenvalues.

This is a helper module of the suite, not a conftest: tests import it by name."""
import numpy as np
from scipy.spatial import cKDTree

import dbscan_exact as dx
import outlier_exact as ox

F32 = np.float32
ZERO_TOL = 1.0e-5            # Eigen's isZero() at fp32: every |c_ij| <= 1e-5, absolute
TWO_THIRDS_PI = 2.09439510239319549


# ---- radii ----------------------------------------------------------------------------------------------------------
def resolution(pts):
    """(resolution, salient_radius, non_max_radius) as float32: sqrt of the mean, in fp64, of the fp32 squared distance
    to the nearest other entry of a k = 2 search; 6 and 4 times it in fp32"""
    pts = np.ascontiguousarray(pts, F32)
    n = len(pts)
    k = min(4, n)
    _, j = cKDTree(pts.astype(np.float64)).query(pts.astype(np.float64), k=k)
    j = j.reshape(n, k)
    d2 = np.sort(ox.d2_f32(pts[:, None, :], pts[j]), axis=1)[:, :2]        # (fp32 ties may reorder fp64's nearest)
    res = F32(np.sqrt(d2.astype(np.float64).sum() / n))
    return res, F32(6.0) * res, F32(4.0) * res


# ---- rows -----------------------------------------------------------------------------------------------------------
def rows(pts, r, max_neighbors):
    n = len(pts)
    if n == 0 or not F32(r) * F32(r) > 0:
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int64)
    return dx.rows(pts, r, int(max_neighbors) - 1)


def padded(indptr, idx, width):
    """CSR rows -> ([n, width] int64 padded with -1, counts)"""
    n = len(indptr) - 1
    cnt = np.diff(indptr)
    pad = np.full((n, max(width, 1)), -1, np.int64)
    src = np.repeat(np.arange(n), cnt)
    pad[src, np.arange(len(idx)) - indptr[src]] = idx
    return pad, cnt.astype(np.int32)


# ---- step 3 ---------------------------------------------------------------------------------------------------------
def cumulants(pts, pad, cnt, dtype, centred):
    """the nine sums over every row, slot after slot (products rounded, then added: nothing fused)"""
    P = pts.astype(dtype)
    n, K = pad.shape
    cum = np.zeros((n, 9), dtype)
    for t in range(K):
        use = t < cnt
        if not use.any():
            break
        q = P[np.where(use, pad[:, t], 0)]
        if centred:
            q = q - P
        q = np.where(use[:, None], q, dtype(0))
        x, y, z = q[:, 0], q[:, 1], q[:, 2]
        for e, v in enumerate((x, y, z, x * x, x * y, x * z, y * y, y * z, z * z)):
            cum[:, e] += v
    return cum


def covariance(cum, cnt, dtype):
    with np.errstate(divide="ignore", invalid="ignore"):
        c = cum / cnt.astype(dtype)[:, None]
    C = np.empty((len(c), 3, 3), dtype)
    C[:, 0, 0] = c[:, 3] - c[:, 0] * c[:, 0]
    C[:, 1, 1] = c[:, 6] - c[:, 1] * c[:, 1]
    C[:, 2, 2] = c[:, 8] - c[:, 2] * c[:, 2]
    C[:, 0, 1] = C[:, 1, 0] = c[:, 4] - c[:, 0] * c[:, 1]
    C[:, 0, 2] = C[:, 2, 0] = c[:, 5] - c[:, 0] * c[:, 2]
    C[:, 1, 2] = C[:, 2, 1] = c[:, 7] - c[:, 1] * c[:, 2]
    return C


def is_zero(C):
    return (np.abs(C) <= C.dtype.type(F32(ZERO_TOL))).all(axis=(1, 2))


def eigenvalues(C):
    """FastEigen3x3Val in C's dtype, operation by operation: the eigenvalues of C / C.max() in the general branch (never
    scaled back), C's diagonal when C / C.max() has no off-diagonal entry, zeros when C.max() == 0; (min, mid, max)"""
    dt = C.dtype.type
    n = len(C)
    mc = C.reshape(n, 9).max(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        S = C / mc[:, None, None]
        s00, s11, s22, s01, s02, s12 = S[:, 0, 0], S[:, 1, 1], S[:, 2, 2], S[:, 0, 1], S[:, 0, 2], S[:, 1, 2]
        norm = s01 * s01 + s02 * s02 + s12 * s12
        q = (s00 + s11 + s22) / dt(3)
        b00, b11, b22 = s00 - q, s11 - q, s22 - q
        p = np.sqrt((b00 * b00 + b11 * b11 + b22 * b22 + norm * dt(2)) / dt(6))
        c00 = b11 * b22 - s12 * s12
        c01 = s01 * b22 - s12 * s02
        c02 = s01 * s12 - b11 * s02
        det = (b00 * c00 - s01 * c01 + s02 * c02) / (p * p * p)
        half = np.minimum(np.maximum(det * dt(0.5), dt(-1)), dt(1))
        angle = np.arccos(half) / dt(3)
        beta2 = np.cos(angle) * dt(2)
        beta0 = np.cos(angle + dt(TWO_THIRDS_PI)) * dt(2)
        beta1 = -(beta0 + beta2)
        v = np.stack([q + p * beta0, q + p * beta1, q + p * beta2], 1)
    diag = np.stack([C[:, 0, 0], C[:, 1, 1], C[:, 2, 2]], 1)
    v = np.where((norm > 0)[:, None], v, diag)
    v = np.where((mc == 0)[:, None], dt(0), v).astype(C.dtype)
    mn, mx = v.min(1), v.max(1)
    return np.stack([mn, ((v[:, 0] + v[:, 1]) + v[:, 2]) - mn - mx, mx], 1)


def eig_of_rows(pts, pad, cnt, min_neighbors, dtype, centred):
    """step 3: [n, 3] eigenvalues, (-1, -1, -1) for too few neighbours or a zero covariance"""
    C = covariance(cumulants(pts, pad, cnt, dtype, centred), np.maximum(cnt, 0), dtype)
    with np.errstate(invalid="ignore"):
        e = eigenvalues(C)
    e[(cnt < min_neighbors) | is_zero(C)] = -1
    return e


# ---- steps 4 and 5 --------------------------------------------------------------------------------------------------
def gates(eig, cnt, min_neighbors, gamma_21, gamma_32):
    """saliency from given eigenvalues and counts, in eig's dtype (IEEE divisions, NaN compares false)"""
    dt = eig.dtype.type
    e0, e1, e2 = eig[:, 0], eig[:, 1], eig[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        ok = (e2 > 0) & (e1 / e2 < dt(F32(gamma_21))) & (e0 / e1 < dt(F32(gamma_32))) & (cnt >= min_neighbors)
    return np.where(ok, e0, dt(-1)).astype(eig.dtype)


def suppress(sal, indptr, idx):
    """mask[i] = sal[i] >= 0 and no row entry l has sal[i] < sal[l]"""
    n = len(sal)
    src = np.repeat(np.arange(n), np.diff(indptr))
    beaten = np.bincount(src[sal[src] < sal[idx]], minlength=n) > 0
    return (sal >= 0) & ~beaten


# ---- the whole detector ---------------------------------------------------------------------------------------------
def iss(pts, salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5,
        max_neighbors=100, dtype=np.float64, centred=True):
    pts = np.ascontiguousarray(pts, F32)
    rs, rn = F32(salient_radius), F32(non_max_radius)
    if len(pts) and (rs == 0 or rn == 0):
        _, rs, rn = resolution(pts)
    srow = rows(pts, rs, max_neighbors)
    nrow = rows(pts, rn, max_neighbors)
    pad, cnt = padded(*srow, max_neighbors)
    eig = eig_of_rows(pts, pad, cnt, min_neighbors, dtype, centred)
    sal = gates(eig, cnt, min_neighbors, gamma_21, gamma_32)
    return dict(mask=suppress(sal, *nrow), saliency=sal, eig=eig, counts=cnt, radii=(float(rs), float(rn)),
                salient_rows=srow, non_max_rows=nrow)


def undecided(res, gamma_21=0.975, gamma_32=0.975, ratio_tol=1e-4, tie_tol=1e-4):
    """the points an fp32 rounding may flip: the point itself or a point of its non-maximum row has e1/e2 or e0/e1
    within ratio_tol (absolute) of its gamma, or its saliency lies within tie_tol (relative) of a row neighbour's"""
    e, sal = res["eig"].astype(np.float64), res["saliency"].astype(np.float64)
    indptr, idx = res["non_max_rows"]
    n = len(sal)
    with np.errstate(divide="ignore", invalid="ignore"):
        near = (np.abs(e[:, 1] / e[:, 2] - float(F32(gamma_21))) <= ratio_tol) | \
               (np.abs(e[:, 0] / e[:, 1] - float(F32(gamma_32))) <= ratio_tol)
    near &= (e != -1).any(1)
    src = np.repeat(np.arange(n), np.diff(indptr))
    other = idx != src
    close = other & (sal[src] >= 0) & (sal[idx] >= 0) & \
        (np.abs(sal[src] - sal[idx]) <= tie_tol * np.maximum(np.abs(sal[src]), np.abs(sal[idx])))
    flag = near[src] | near[idx] | close
    return (np.bincount(src[flag], minlength=n) > 0) | near
