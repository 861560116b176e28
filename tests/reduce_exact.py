"""Clouds on which every term the ICP reduction (csrc/reduce.h) adds is exactly representable, and the integer-arithmetic
sums they must give: shared by tests/test_reduce_exact_cpu.py (which holds the construction) and
tests/test_gpu_reduce_exact.py (which holds the kernels to it, bit for bit).

TARGET   the 16^3 lattice i/16 (4096 points); normals are integer vectors from {-1,0,1}^3 without the zero vector (the
         engine never normalises them); covariances are diagonal with entries from {0.5, 1, 2}; all from one seeded rng.
SOURCE   n points; point i is a target point chosen at random plus an offset whose components are multiples of 2^-8 in
         [-7/256, 7/256], never all zero: shorter than half a spacing per axis, so the nearest neighbour is that target
         point, and no other is as near (held by brute force in the CPU file).  Source normals come from the same integer
         set; the source covariance is its target's (Cs = Ct, GICP).
MISSES   about one eighth of the points are moved by 5 along one axis, at least 4 beyond the lattice: no target within
         MAX_DIST = 1/16 (strict <).  They are moved in the POSITIVE direction of the frame the source is STORED in, so that in the engine's spatial order
         -- Morton codes over the source's box -- every miss comes behind every matched point: the element the kernels
         re-read past the end, sorted element 0, is then always a matched one with a non-zero offset and a non-zero
         normal (moved in the negative direction a miss would have been first, and a leak of it would add nothing).
         Original element 0 and the last one are matched too; the source is shuffled with the seeded rng.
TRANSFORMS  the identity, and a quarter turn about z with a dyadic translation: for the second the source is stored as
         the exact pre-image (a signed permutation of coordinates, minus a dyadic vector), normals and covariances
         likewise, so xform_point, rotate and rotate_cov run on non-trivial matrices and still round nowhere.  The
         transformed source -- hence every reference below -- is the same for both.

Everything is held in integers: coordinates in units of 1/256 (Q), normals in units of 1.  The references are sums of
integer products, converted once (an int below 2^53 over a power of two is an exact double).  Nothing here relies on a
bit count done by hand: self_check() evaluates every row in float32 the way reduce.h does, operation by operation,
compares it with the integer value, and bounds the sums.  The float32 mirror rounds after every operation where the
kernel uses fused multiply-adds; where the mirror equals the integer value, that value is representable, and the fused
form, which rounds the same exact value once, returns it too.
"""
import functools
import itertools

import numpy as np

P2P, PT2PL, SYM, COLORED, GICP = 1, 2, 3, 4, 5
EST_NAMES = {P2P: "p2p", PT2PL: "pt2pl", SYM: "sym", COLORED: "colored", GICP: "gicp"}
GRID = 16
NT = GRID ** 3
Q = 256                         # coordinates are integers in units of 1/Q
MAX_DIST = 1.0 / 16
GRADIENT_RADIUS = 1.1 / 16       # colour gradients over the six face neighbours: finite on this lattice (CPU file)
MISS_SHIFT = 5 * Q                  # lands at least 4 beyond the lattice's far face

# the smallest n that puts a kernel in each regime (grid = max(min(256, ceil(n/256)), min(1024, ceil(n/4096))),
# point-to-plane capped at 512 blocks, four elements in flight below 4 Mi points and two from there)
SIZES = [1, 63, 255, 256, 257,                # one wave, one block, the first second block
         32512, 32768, 32769,                 # 127 / 128 / 129 rows for the finishing block
         65536, 65537,                        # 256 blocks, one trip; the first second trip
         262144, 262145,                      # kU = 4: one full batch; a second outer trip with one live lane
         1048576, 1048577,                    # 16 trips on 256 blocks; the first 257-row grid
         2097153]                             # generic grid 513, point-to-plane capped at 512
BIG_SIZES = [4194303, 4194304, 4194305]       # the last kU = 4; the first kU = 2 and generic grid 1024; the 17th trip

T_IDENTITY = np.eye(4, dtype=np.float32)
T_ROT90Z = np.array([[0, -1, 0, 0.25], [1, 0, 0, -0.5], [0, 0, 1, 0.125], [0, 0, 0, 1]], np.float32)
TRANSFORMS = {"identity": T_IDENTITY, "rot90z": T_ROT90Z}

_DIRS = np.array([v for v in itertools.product((-1, 0, 1), repeat=3) if any(v)], np.int64)      # the 26 normals


def grid_of(n, pt2pl=False):
    """launch_reduce's grid for n elements"""
    g = max(min(256, -(-n // 256)), min(1024, -(-n // 4096)))
    return min(g, 512) if pt2pl else g


@functools.lru_cache(maxsize=1)
def target():
    """the lattice: points (float32), integer points / normals, covariance diagonals"""
    rng = np.random.default_rng(4096)
    g = np.arange(GRID, dtype=np.int64)
    pts_i = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3) * (Q // GRID)
    pts_i = np.ascontiguousarray(pts_i[rng.permutation(NT)])
    nrm_i = _DIRS[rng.integers(0, len(_DIRS), NT)]
    cov_k = rng.integers(0, 3, (NT, 3))                                     # diagonal entry 2^(k - 1): 0.5, 1, 2
    cov_d = np.ldexp(np.float32(0.5), cov_k).astype(np.float32)
    # dyadic intensities, otherwise arbitrary (colored ICP): colours (v, v, v) have the intensity v exactly
    inten = (rng.integers(0, 65, NT) / 64.0).astype(np.float32)
    return {"pts_i": pts_i, "nrm_i": nrm_i, "cov_k": cov_k,
            "pts": (pts_i / Q).astype(np.float32), "nrm": nrm_i.astype(np.float32), "cov": diag_cov(cov_d),
            "colors": np.repeat(inten[:, None], 3, 1)}


def diag_cov(d):
    c = np.zeros((len(d), 3, 3), np.float32)
    for k in range(3):
        c[:, k, k] = d[:, k]
    return c


@functools.lru_cache(maxsize=3)
def case(n):
    """the source of n points in the TRANSFORMED frame, as integers, in its final (shuffled) order"""
    tg = target()
    rng = np.random.default_rng(1000003 + n)
    tix = rng.integers(0, NT, n)
    off = rng.integers(-7, 8, (n, 3))
    zero = ~off.any(1)
    off[zero, 0] = 1 + tix[zero] % 7                                        # never all zero
    miss = rng.random(n) < 0.125
    miss[0] = miss[-1] = False
    axis = rng.integers(0, 3, n)
    nrm_i = _DIRS[rng.integers(0, len(_DIRS), n)]
    inten = (rng.integers(0, 65, n) / 64.0).astype(np.float32)
    perm = rng.permutation(n)
    tix, off, miss, axis, nrm_i, inten = tix[perm], off[perm], miss[perm], axis[perm], nrm_i[perm], inten[perm]
    ends = np.flatnonzero((perm == 0) | (perm == n - 1))                    # where the original ends went
    q_i = tg["pts_i"][tix] + off
    nn = np.where(miss, -1, tix).astype(np.int32)
    m = ~miss
    return {"n": n, "tix": tix, "off_i": off, "miss": miss, "axis": axis, "q_i": q_i, "nrm_i": nrm_i, "nn": nn,
            "ends": ends, "count": int(m.sum()), "d2": np.where(miss, np.inf, (off * off).sum(1) / float(Q * Q)).astype(np.float32),
            "colors": np.repeat(inten[:, None], 3, 1),
            # the matched rows, which is all the references need
            "vs": q_i[m], "vt": tg["pts_i"][tix[m]], "d": off[m], "nt": tg["nrm_i"][tix[m]], "ns": nrm_i[m],
            "ck": tg["cov_k"][tix[m]]}


def stored(n, tname):
    """what the engine is given for transform `tname`: float32 points, normals and covariances whose images under the
    transform are case(n)'s (the misses moved by +5 along an axis of THIS frame)"""
    c, tg = case(n), target()
    T = TRANSFORMS[tname].astype(np.float64)
    R = np.rint(T[:3, :3]).astype(np.int64)
    t_i = np.rint(T[:3, 3] * Q).astype(np.int64)
    p_i = (c["q_i"] - t_i) @ R                                              # R^T (q - t), row vectors
    rows = np.flatnonzero(c["miss"])
    p_i[rows, c["axis"][rows]] += MISS_SHIFT
    nrm = (c["nrm_i"] @ R).astype(np.float32)
    cov_d = np.ldexp(np.float32(0.5), tg["cov_k"][c["tix"]]).astype(np.float32) @ np.abs(R).astype(np.float32)   # diag of R^T C R
    pts = (p_i / Q).astype(np.float32)
    assert np.array_equal(pts.astype(np.float64) * Q, p_i)
    return {"pts": pts, "nrm": nrm, "cov": diag_cov(cov_d), "p_i": p_i}


def pairs_of(n):
    """case(n)'s correspondences as (source, target) pairs in source order"""
    c = case(n)
    rows = np.flatnonzero(~c["miss"])
    return np.stack([rows, c["tix"][rows]], 1).astype(np.int32)


def oracle_inputs(n):
    """what oracle.compute_system takes: the TRANSFORMED source (exact in float32), its normals and covariances"""
    c, tg = case(n), target()
    src_cov = diag_cov(np.ldexp(np.float32(0.5), tg["cov_k"][c["tix"]]).astype(np.float32))
    return {"src": (c["q_i"] / Q).astype(np.float32), "src_nrm": c["nrm_i"].astype(np.float32), "src_cov": src_cov,
            "tgt": tg["pts"], "tgt_nrm": tg["nrm"], "tgt_cov": tg["cov"], "cor": pairs_of(n)}


# --------------------------------------------------------------------------- integer rows
def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _exact(total, scale):
    """an integer total in units of 1/scale (a power of two) as a double; refuses what 53 bits cannot hold"""
    total = int(total)
    assert abs(total) < 2 ** 53, "the sum leaves 53 bits"
    return total / float(scale)


def _rows(rows, est):
    """integer Jacobian rows: J (m, 6) with columns 0..2 in units of 1/Q and 3..5 in units of 1; r (m) in units of 1/Q"""
    vs, vt, d, nt, ns = rows["vs"], rows["vt"], rows["d"], rows["nt"], rows["ns"]
    if est in (PT2PL, COLORED):
        return np.concatenate([_cross(vs, nt), nt], 1), (d * nt).sum(1)
    if est == SYM:
        nn = ns + nt
        return np.concatenate([_cross(vs + vt, nn), nn], 1), (d * nn).sum(1)
    raise ValueError(est)


def _gicp_rows(rows, dtype=np.int64):
    """S = (Ct + Cs)^-1 = diag(2^-k) in units of 1/4; P = S A (units 1/(4Q)), Qm = A^T S A (1/(4Q^2)), Sd (1/(4Q)),
    g = A^T S d (1/(4Q^2)), d^T S d (1/(4Q^2)) with A = [0 z -y; -z 0 x; y -x 0] of the transformed source point: formed
    the way gicp_rows forms them, from full matrices"""
    vs, d = rows["vs"].astype(dtype), rows["d"].astype(dtype)
    s4 = (4 >> rows["ck"]).astype(dtype)                                    # (m, 3): 4, 2, 1
    Sm = s4[:, :, None] * np.eye(3, dtype=dtype)                            # rows S_r
    P = _cross(vs[:, None, :], Sm)                                          # P[r][c] = (vs x S_r)_c
    Qm = _cross(vs[:, None, :], P.transpose(0, 2, 1)).transpose(0, 2, 1)    # Qm[:, c] = vs x P[:, c]
    Sd = s4 * d
    return Sm, P, Qm, Sd, _cross(vs, Sd), (d * Sd).sum(1)


def _gicp_words(rows):
    """the 28 GICP words per correspondence for a DIAGONAL S = diag(a, b, c), written out (self_check holds them against
    _gicp_rows): [(word, per-row integers, units)]"""
    x, y, z = rows["vs"].T
    d = rows["d"]
    a, b, c = (4 >> rows["ck"]).T
    u2, u1 = 4 * Q * Q, 4 * Q
    zero = np.zeros_like(x)
    Sd = [a * d[:, 0], b * d[:, 1], c * d[:, 2]]
    w = [(b * z * z + c * y * y, u2), (-c * x * y, u2), (-b * x * z, u2), (zero, u1), (-b * z, u1), (c * y, u1),
         (a * z * z + c * x * x, u2), (-a * y * z, u2), (a * z, u1), (zero, u1), (-c * x, u1),
         (a * y * y + b * x * x, u2), (-a * y, u1), (b * x, u1), (zero, u1),
         (a, 4), (zero, 4), (zero, 4), (b, 4), (zero, 4), (c, 4),
         (y * Sd[2] - z * Sd[1], u2), (z * Sd[0] - x * Sd[2], u2), (x * Sd[1] - y * Sd[0], u2),
         (Sd[0], u1), (Sd[1], u1), (Sd[2], u1), (d[:, 0] * Sd[0] + d[:, 1] * Sd[1] + d[:, 2] * Sd[2], u2)]
    return w


def rows_for(n, src):
    """the rows of explicit pairs (src[k], case(n)'s match of src[k]); sources may repeat, none may be a miss"""
    c, tg = case(n), target()
    src = np.asarray(src, np.int64)
    assert not c["miss"][src].any()
    t = c["tix"][src]
    return {"vs": c["q_i"][src], "vt": tg["pts_i"][t], "d": c["off_i"][src], "nt": tg["nrm_i"][t], "ns": c["nrm_i"][src],
            "ck": tg["cov_k"][t]}


def reference(n, est, rows=None):
    """compute_system(est)[:30] on case(n) -- or on the given matched rows -- as exact doubles"""
    rows = case(n) if rows is None else rows
    out = np.zeros(30, np.float64)
    d = rows["d"]
    out[28] = _exact((d * d).sum(), Q * Q)
    out[29] = float(len(d))
    if est == P2P:
        vs, vt = rows["vs"], rows["vt"]
        for p in range(3):
            out[p] = _exact(vs[:, p].sum(), Q)
            out[3 + p] = _exact(vt[:, p].sum(), Q)
        M = vs.T @ vt
        for p in range(3):
            for q in range(3):
                out[6 + 3 * p + q] = _exact(M[p, q], Q * Q)
        out[27] = out[28]
        return out
    if est == GICP:
        for k, (v, unit) in enumerate(_gicp_words(rows)):
            out[k] = _exact(v.sum(), unit)
        return out
    J, r = _rows(rows, est)
    js = [Q, Q, Q, 1, 1, 1]
    JJ, Jr = J.T @ J, J.T @ r
    k = 0
    for a in range(6):
        for b in range(a, 6):
            out[k] = _exact(JJ[a, b], js[a] * js[b])
            k += 1
    for a in range(6):
        out[21 + a] = _exact(Jr[a], js[a] * Q)
    out[27] = _exact((r * r).sum(), Q * Q)
    return out


def reference_error_sum(n, est, rows=None):
    """word [27] of the MODE 1 reduction (the estimator's ComputeRMSE sum); COLORED: at lambda_geometric = 1 only"""
    rows = case(n) if rows is None else rows
    d = rows["d"]
    if est == P2P:
        return _exact((d * d).sum(), Q * Q)
    _, r = _rows(rows, est)
    if est == SYM:                                                          # squared twice
        return _exact((r ** 4).sum(), Q ** 4)
    return _exact((r * r).sum(), Q * Q)


def reference_rmse(n, est, rows=None):
    """mi_icp_compute_rmse: sqrtf((float)sum / (float)count) in float32 -- for COLORED the plain sum as a float"""
    rows = case(n) if rows is None else rows
    s, cnt = np.float32(reference_error_sum(n, est, rows)), np.float32(len(rows["d"]))
    if est == COLORED:
        return float(s)
    return float(np.sqrt(s / cnt)) if cnt > 0 else 0.0


def reference_stats(n):
    """(count, fitness, inlier_rmse) as stats_from_system forms them in float32"""
    c = case(n)
    sd2 = _exact((c["d"] * c["d"]).sum(), Q * Q)
    cnt = np.float32(c["count"])
    return c["count"], float(cnt / np.float32(n)), float(np.sqrt(np.float32(sd2) / cnt))


# --------------------------------------------------------------------------- the float32 mirror
def _f32(a):
    return np.asarray(a, np.float32)


def _mirror_points(n, tname):
    """xform_point on the stored matched points, operation by operation in float32"""
    c, st = case(n), stored(n, tname)
    m = ~c["miss"]
    T = TRANSFORMS[tname]
    p = st["pts"][m]

    def rot(v):
        o = []
        for r in range(3):
            a = T[r, 0] * v[:, 0]
            a = T[r, 1] * v[:, 1] + a
            o.append(T[r, 2] * v[:, 2] + a)
        return o
    vs = np.stack([o + T[r, 3] for r, o in enumerate(rot(p))], 1)
    ns = np.stack(rot(st["nrm"][m]), 1)
    assert vs.dtype == np.float32 and ns.dtype == np.float32
    return vs, ns, st, m


def _same(f32, ints, scale, what):
    assert f32.dtype == np.float32, what
    assert np.array_equal(f32.astype(np.float64) * scale, ints), "%s is not exact in float32" % what


def _dot3(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def self_check(n, tname, est, eigen3_host=None):
    """every per-row term of reduce.h's rows for `est` (MODE 0 and MODE 1), formed in float32 as the kernel forms it,
    equals the integer value; and every one of the 30 sums stays below 2^53 units even with all signs alike.
    GICP needs eigen3_host(A (m, 3, 3) float32) -> S (m, 3, 3): eigen3.h gicp_weight on the host."""
    c, tg = case(n), target()
    vs, ns, st, m = _mirror_points(n, tname)
    _same(vs, c["vs"], Q, "the transformed point")
    vt = tg["pts"][c["tix"][m]]
    d = vs - vt
    _same(d, c["d"], Q, "d")
    d2 = d[:, 0] * d[:, 0]
    d2 = d[:, 1] * d[:, 1] + d2
    d2 = d[:, 2] * d[:, 2] + d2
    _same(d2, (c["d"] * c["d"]).sum(1), Q * Q, "sq3(d)")
    cnt = c["count"]
    if est == P2P:
        _same(_dot3(d, d), (c["d"] * c["d"]).sum(1), Q * Q, "dot3(d, d)")
        assert cnt * int(np.abs(c["vs"]).max()) * int(np.abs(c["vt"]).max()) < 2 ** 53
        return
    if est == GICP:
        R = TRANSFORMS[tname][:3, :3]
        C = st["cov"][m]                                                    # row-major == column-major: diagonal
        RC = np.zeros_like(C)
        Cs = np.zeros_like(C)
        for cc in range(3):
            for r in range(3):
                a = R[r, 0] * C[:, 0, cc]
                a = R[r, 1] * C[:, 1, cc] + a
                RC[:, r, cc] = R[r, 2] * C[:, 2, cc] + a
        for cc in range(3):
            for r in range(3):
                a = RC[:, r, 0] * R[cc, 0]
                a = RC[:, r, 1] * R[cc, 1] + a
                Cs[:, r, cc] = RC[:, r, 2] * R[cc, 2] + a
        Ct = tg["cov"][c["tix"][m]]
        assert np.array_equal(Cs, Ct), "R Cs R^T is not the target's covariance"
        M = Ct + Cs
        c00 = M[:, 1, 1] * M[:, 2, 2] - M[:, 1, 2] * M[:, 2, 1]            # inverse3 by cofactors: M is diagonal
        det = M[:, 0, 0] * c00 + M[:, 0, 1] * 0 + M[:, 0, 2] * 0
        inv = np.float32(1.0) / det
        Mi = np.zeros_like(M)
        Mi[:, 0, 0] = c00 * inv
        Mi[:, 1, 1] = (M[:, 0, 0] * M[:, 2, 2] - M[:, 0, 2] * M[:, 2, 0]) * inv
        Mi[:, 2, 2] = (M[:, 0, 0] * M[:, 1, 1] - M[:, 1, 0] * M[:, 0, 1]) * inv
        Sm, P, Qm, Sd, g, dSd = _gicp_rows(c, np.int32)
        k = 0
        words = _gicp_words(c)
        for p_ in range(6):                                                 # the written-out words are gicp_rows' words
            for q_ in range(p_, 6):
                v = Qm[:, p_, q_] if q_ < 3 else (P[:, q_ - 3, p_] if p_ < 3 else Sm[:, p_ - 3, q_ - 3])
                assert np.array_equal(v, words[k][0])
                k += 1
        for p_ in range(3):
            assert np.array_equal(g[:, p_], words[21 + p_][0]) and np.array_equal(Sd[:, p_], words[24 + p_][0])
        assert np.array_equal(dSd, words[27][0])
        _same(Mi, Sm, 4, "(Ct + Cs)^-1")
        assert eigen3_host is not None, "GICP needs eigen3.h's gicp_weight on the host"
        assert np.array_equal(eigen3_host(Mi), Mi), "gicp_weight changes a dyadic diagonal matrix"
        S = Mi
        Sdf = np.stack([S[:, r, 0] * d[:, 0] + S[:, r, 1] * d[:, 1] + S[:, r, 2] * d[:, 2] for r in range(3)], 1)
        _same(Sdf, Sd, 4 * Q, "S d")
        x, y, z = vs[:, 0], vs[:, 1], vs[:, 2]
        Pf = np.stack([np.stack([S[:, r, 2] * y - S[:, r, 1] * z, S[:, r, 0] * z - S[:, r, 2] * x,
                                 S[:, r, 1] * x - S[:, r, 0] * y], 1) for r in range(3)], 1)
        _same(Pf, P, 4 * Q, "P = S A")
        Qf = np.stack([y[:, None] * Pf[:, 2] - z[:, None] * Pf[:, 1], z[:, None] * Pf[:, 0] - x[:, None] * Pf[:, 2],
                       x[:, None] * Pf[:, 1] - y[:, None] * Pf[:, 0]], 1)
        _same(Qf, Qm, 4 * Q * Q, "Q = A^T S A")
        gf = np.stack([y * Sdf[:, 2] - z * Sdf[:, 1], z * Sdf[:, 0] - x * Sdf[:, 2], x * Sdf[:, 1] - y * Sdf[:, 0]], 1)
        _same(gf, g, 4 * Q * Q, "g = A^T S d")
        _same(_dot3(d, Sdf), dSd, 4 * Q * Q, "d^T S d")
        assert cnt * int(max(np.abs(Qm).max(), np.abs(g).max(), np.abs(dSd).max())) < 2 ** 53
        return
    nt = tg["nrm"][c["tix"][m]]
    if est == SYM:
        _same(ns, c["ns"], 1, "the rotated source normal")
        nvec = ns + nt
        lever = vs + vt
    else:
        nvec, lever = nt, vs
    r = _dot3(d, nvec)
    Jf = np.concatenate([np.stack([lever[:, 1] * nvec[:, 2] - lever[:, 2] * nvec[:, 1],
                                   lever[:, 2] * nvec[:, 0] - lever[:, 0] * nvec[:, 2],
                                   lever[:, 0] * nvec[:, 1] - lever[:, 1] * nvec[:, 0]], 1), nvec], 1)
    if est == COLORED:                                                      # lambda_geometric = 1: times sqrtf(1) = 1
        Jf, r = np.float32(1.0) * Jf, np.float32(1.0) * r
    J, ri = _rows(c, est)
    _same(Jf[:, :3], J[:, :3], Q, "J[0..2]")
    _same(Jf[:, 3:], J[:, 3:], 1, "J[3..5]")
    _same(r, ri, Q, "r")
    e2 = r * r
    _same(e2, ri * ri, Q * Q, "r * r")
    if est == SYM:
        _same(e2 * e2, ri ** 4, Q ** 4, "(r * r)^2")
        assert cnt * int(np.abs(ri).max()) ** 4 < 2 ** 53
    # the accumulators take fp64 products of two float32 values (exact: 48 bits); their sums, all signs alike:
    big = int(max(np.abs(J[:, :3]).max(), np.abs(ri).max()))
    assert cnt * big * big < 2 ** 53


def eigen3_host(A):
    """eigen3.h gicp_weight on the host (mi_icp_debug_eigen3, device -1): S for each 3x3 of A"""
    from cupoch_amd import _lib
    A = np.ascontiguousarray(A, np.float32).reshape(-1, 9)
    S = np.zeros_like(A)
    rc = _lib.load().mi_icp_debug_eigen3(-1, A.ctypes.data, len(A), None, None, S.ctypes.data)
    assert rc == 0, rc
    return S.reshape(-1, 3, 3)
