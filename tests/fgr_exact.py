"""CPU restatement of feature matching and FastGlobalRegistration as include/mi_icp.h states them ("feature matching and
FastGlobalRegistration"), written from the header alone: numpy for the fp32 steps, Python integers for the sampler,
fractions.Fraction where a rounding could be taken twice.

  scene(dim, ...)                          the test scene: two overlapping, permuted, moved copies of 440 points
  dist64(Q, R)                             the squared distances in fp64 (from the fp32 features)
  chain_exact(q, r)                        D(i, j) as the header defines it: exact rationals, one rounding per step
  neighbours(D) / undecided(D, dim)        smallest distance, smallest index among equals; the rows the band leaves open
  reciprocal_pairs / tuples                the pairs and the cut tuple list, integers throughout
  normalize / optimize / back_map / fgr    the optimiser, in fp64 throughout or with the stated fp32 steps
  par_schedule                             the line-process parameter after every iteration

This is a helper module of the suite, not a conftest: tests import it by name."""
from fractions import Fraction

import numpy as np

from segment_plane_exact import _round_f32, below, u

F32 = np.float32
F64 = np.float64
MIN_CORRES = 10


class Option:
    """registration::FastGlobalRegistrationOption (fast_global_registration.h) with its defaults"""

    def __init__(self, division_factor=1.4, use_absolute_scale=False, decrease_mu=True, maximum_correspondence_distance=0.025,
                 iteration_number=64, tuple_scale=0.95, maximum_tuple_count=1000):
        self.division_factor = division_factor
        self.use_absolute_scale = use_absolute_scale
        self.decrease_mu = decrease_mu
        self.maximum_correspondence_distance = maximum_correspondence_distance
        self.iteration_number = iteration_number
        self.tuple_scale = tuple_scale
        self.maximum_tuple_count = maximum_tuple_count


# ---- the scene ----------------------------------------------------------------------------------------------------------
def rotation(angle, axis):
    ax = np.asarray(axis, F64) / np.linalg.norm(axis)
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def scene(dim, seed=0, desc_sigma=0.05, point_noise=0.0):
    """440 base points uniform in a 4 x 2 x 1 box away from the origin, a standard-normal descriptor each; the source is
    a permutation of points 0-359, the target one of 0-299 and 360-439 moved by 1.1 rad about (1, 2, 3) and (0.7, -1.3,
    0.4); both copies' descriptors carry noise.  T_gt maps source to target."""
    rng = np.random.default_rng(seed)
    base = rng.uniform([3.0, 1.0, 2.0], [7.0, 3.0, 3.0], (440, 3))
    desc = rng.standard_normal((440, dim))
    si = rng.permutation(360)
    ti = np.concatenate([np.arange(300), np.arange(360, 440)])[rng.permutation(380)]
    R, t = rotation(1.1, (1, 2, 3)), np.array([0.7, -1.3, 0.4])
    src = base[si] + point_noise * rng.standard_normal((360, 3))
    tgt = base[ti] @ R.T + t + point_noise * rng.standard_normal((380, 3))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return dict(src=np.ascontiguousarray(src, F32), tgt=np.ascontiguousarray(tgt, F32),
                sfeat=np.ascontiguousarray(desc[si] + desc_sigma * rng.standard_normal((360, dim)), F32),
                tfeat=np.ascontiguousarray(desc[ti] + desc_sigma * rng.standard_normal((380, dim)), F32),
                T_gt=T, src_base=si, tgt_base=ti)


# ---- the distance -------------------------------------------------------------------------------------------------------
def dist64(Q, R):
    Q, R = np.asarray(Q, F32).astype(F64), np.asarray(R, F32).astype(F64)
    D = np.zeros((len(Q), len(R)))
    with np.errstate(all="ignore"):
        for k in range(Q.shape[1]):
            e = Q[:, k, None] - R[None, :, k]
            D += e * e
    return D


def chain_exact(q, r):
    """acc = 0; for k in order: e = fl(q_k - r_k), acc = fl(e * e + acc) -- each fl one rounding to fp32"""
    acc = Fraction(0)
    for a, b in zip(np.asarray(q, F32), np.asarray(r, F32)):
        e = _round_f32(Fraction(float(a)) - Fraction(float(b)))
        acc = _round_f32(e * e + acc)
    return F32(float(acc))


def neighbours(D):
    """per row the column of the smallest distance (the smallest column of equals), -1 where every distance is a NaN"""
    D = np.asarray(D)
    if D.shape[1] == 0:
        return np.full(len(D), -1, np.int32)
    nan = np.isnan(D)
    idx = np.argmin(np.where(nan, np.inf, D), axis=1).astype(np.int32)
    idx[nan.all(axis=1)] = -1
    return idx


def band(dim):
    """one rounding for the difference, doubled by the square, one per fma, on sums of non-negative terms: (dim + 2)
    2^-24 relative per candidate, two candidates"""
    return 2.0 * (dim + 2) * 2.0 ** -24


def undecided(D, dim):
    """rows whose best and second-best distance the fp32 chain cannot be trusted to order: second - best <= band * best"""
    D = np.asarray(D, F64)
    if D.shape[1] < 2:
        return np.zeros(len(D), bool)
    two = np.partition(D, 1, axis=1)[:, :2]
    return two[:, 1] - two[:, 0] <= band(dim) * two[:, 0]


# ---- pairs and tuples ---------------------------------------------------------------------------------------------------
def reciprocal_pairs(s_idx, t_idx):
    s_idx, t_idx = np.asarray(s_idx, np.int64), np.asarray(t_idx, np.int64)
    rows = [(i, j) for i, j in enumerate(s_idx) if 0 <= j < len(t_idx) and t_idx[j] == i]
    return np.array(rows, np.int32).reshape(-1, 2)


def side2(a, b):
    d = a - b
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def trial_pairs(seed, trials, ncorr):
    seed &= (1 << 64) - 1
    return np.array([below(u(seed, j), ncorr) for j in range(3 * trials)], np.int64).reshape(-1, 3)


def tuples(pairs, src, tgt, tuple_scale, maximum_tuple_count, seed):
    """-> (cut list int32 [m, 2], number of passing trials)"""
    pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
    ncorr = len(pairs)
    if ncorr == 0 or maximum_tuple_count <= 0:
        return np.zeros((0, 2), np.int32), 0
    src, tgt = np.asarray(src, F32), np.asarray(tgt, F32)
    a = trial_pairs(seed, 100 * ncorr, ncorr)
    s2 = F32(tuple_scale) * F32(tuple_scale)
    p = [src[pairs[a[:, m], 0]] for m in range(3)]
    q = [tgt[pairs[a[:, m], 1]] for m in range(3)]
    ok = np.ones(len(a), bool)
    for m in range(3):
        li, lj = side2(p[m], p[(m + 1) % 3]), side2(q[m], q[(m + 1) % 3])
        assert li.dtype == F32 and lj.dtype == F32
        ok &= (li * s2 < lj) & (lj * s2 < li)
    rows = pairs[a[ok]].reshape(-1, 2)                  # trial order, its three pairs in order
    return np.ascontiguousarray(rows[:maximum_tuple_count], np.int32), int(ok.sum())


# ---- the optimiser ------------------------------------------------------------------------------------------------------
def normalize(src, tgt, use_absolute_scale, fp32=True):
    """-> (source', target', means [2, 3], scale_global, largest norm); the means are fp64 sums rounded to fp32"""
    W = F32 if fp32 else F64
    out, means, top = [], [], W(0)
    for pts in (src, tgt):
        pts = np.asarray(pts, F32)
        mean = (pts.astype(F64).sum(axis=0) / len(pts)).astype(F32)
        c = pts.astype(W) - mean.astype(W)
        n2 = (c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1]) + c[:, 2] * c[:, 2]
        top = max(top, n2.max())
        out.append(c)
        means.append(mean)
    scale = np.sqrt(W(top))
    sg = W(1) if use_absolute_scale else scale
    with np.errstate(all="ignore"):
        return out[0] / sg, out[1] / sg, np.array(means), sg, scale


def vector6_to_matrix4(x, W=F32):
    """utility::TransformVector6fToMatrix4f in the working precision"""
    x = np.asarray(x, W)
    T = np.eye(4, dtype=W)
    T[:3, 3] = x[3:]
    th = np.sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2])
    if th == 0:
        return T
    w = x[:3] / th
    c, s = np.cos(th), np.sin(th)
    T[0, 0], T[0, 1], T[0, 2] = c + w[0] * w[0] * (1 - c), w[0] * w[1] * (1 - c) - w[2] * s, w[1] * s + w[0] * w[2] * (1 - c)
    T[1, 0], T[1, 1], T[1, 2] = w[2] * s + w[0] * w[1] * (1 - c), c + w[1] * w[1] * (1 - c), -w[0] * s + w[1] * w[2] * (1 - c)
    T[2, 0], T[2, 1], T[2, 2] = -w[1] * s + w[0] * w[2] * (1 - c), w[0] * s + w[1] * w[2] * (1 - c), c + w[2] * w[2] * (1 - c)
    return T.astype(W)


TRIU = np.triu_indices(6)


def step_sums(p, q, par, fp32=True):
    """the 27 sums of one iteration (21 of JTJ's upper triangle, row-major, then JTr) in fp64, and per entry the sum of
    the terms' magnitudes.  fp32: r and the weight are formed in fp32 as the header states; else all in fp64."""
    W = F32 if fp32 else F64
    p, q, par = np.asarray(p, W), np.asarray(q, W), W(par)
    r = p - q
    t = par / (((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]) + par)
    w = (t * t).astype(F64)
    q, r = q.astype(F64), r.astype(F64)
    n, z, o = len(q), np.zeros(len(q)), np.ones(len(q))
    rows = [(np.stack([z, -q[:, 2], q[:, 1], -o, z, z], 1), r[:, 0]),
            (np.stack([q[:, 2], z, -q[:, 0], z, -o, z], 1), r[:, 1]),
            (np.stack([-q[:, 1], q[:, 0], z, z, z, -o], 1), r[:, 2])]
    sums, mags = np.zeros(27), np.zeros(27)
    for J, res in rows:
        JJ = J[:, :, None] * J[:, None, :] * w[:, None, None]
        Jr = J * (res * w)[:, None]
        sums[:21] += JJ.sum(axis=0)[TRIU]
        mags[:21] += np.abs(JJ).sum(axis=0)[TRIU]
        sums[21:] += Jr.sum(axis=0)
        mags[21:] += np.abs(Jr).sum(axis=0)
    return sums, mags


def par_next(par, itr, opt, W=F32):
    if opt.decrease_mu and itr % 4 == 0 and par > W(opt.maximum_correspondence_distance):
        par = W(par) / W(opt.division_factor)
    return par


def par_schedule(par0, iterations, opt):
    out, par = [], F32(par0)
    for itr in range(iterations):
        par = par_next(par, itr, opt)
        out.append(par)
    return np.array(out, F32)


def optimize(src, tgt, corr, par0, opt, fp32=True, iterations=None):
    """-> (trans [4, 4] in the working precision, the last iteration's 27 sums, par after the last iteration)"""
    W = F32 if fp32 else F64
    corr = np.asarray(corr, np.int64).reshape(-1, 2)
    iters = opt.iteration_number if iterations is None else iterations
    trans, sums, par = np.eye(4, dtype=W), np.zeros(27), W(par0)
    if len(corr) < MIN_CORRES or iters <= 0:
        return trans, sums, par
    p, q = np.asarray(src, W)[corr[:, 0]], np.asarray(tgt, W)[corr[:, 1]].copy()
    for itr in range(iters):
        sums, _ = step_sums(p, q, par, fp32)
        S = sums.astype(W).astype(F64)                  # (the solve works on the rounded sums)
        A = np.zeros((6, 6))
        A[TRIU] = S[:21]
        A = A + A.T - np.diag(np.diag(A))
        x = np.linalg.solve(-A, S[21:])
        delta = vector6_to_matrix4(x.astype(W), W)
        trans = (delta @ trans).astype(W)
        d = delta
        q = np.stack([((d[k, 0] * q[:, 0] + d[k, 1] * q[:, 1]) + d[k, 2] * q[:, 2]) + d[k, 3] for k in range(3)], 1).astype(W)
        par = par_next(par, itr, opt, W)
    return trans, sums, par


def back_map(trans, means, scale_global, W=F32):
    """GetInvTransformationOriginalScale: v = (-(R m_tgt) + t * scale_global) + m_src, T = [R^T, -(R^T v)]"""
    trans = np.asarray(trans, W)
    R, t = trans[:3, :3], trans[:3, 3]
    m0, m1 = np.asarray(means[0], W), np.asarray(means[1], W)
    rm = (R[:, 0] * m1[0] + R[:, 1] * m1[1]) + R[:, 2] * m1[2]
    v = (-rm + t * W(scale_global)) + m0
    Rt = R.T
    T = np.eye(4, dtype=W)
    T[:3, :3] = Rt
    T[:3, 3] = -((Rt[:, 0] * v[0] + Rt[:, 1] * v[1]) + Rt[:, 2] * v[2])
    return T


class Result:
    pass


def fgr(src, tgt, sfeat, tfeat, opt=None, seed=0, fp32=True, nn=None):
    """the whole call up to the transformation -> Result with .T, .pairs, .corr, .passing, .s_idx, .t_idx, .D.
    nn = (s_idx, t_idx): take these neighbour lists instead of the fp64 ones."""
    opt = Option() if opt is None else opt
    res = Result()
    if nn is None:
        res.D = dist64(sfeat, tfeat)
        res.s_idx, res.t_idx = neighbours(res.D), neighbours(res.D.T)
    else:
        res.D, (res.s_idx, res.t_idx) = None, nn
    res.pairs = reciprocal_pairs(res.s_idx, res.t_idx)
    res.corr, res.passing = tuples(res.pairs, src, tgt, opt.tuple_scale, opt.maximum_tuple_count, seed)
    W = F32 if fp32 else F64
    ns_, nt_, res.means, sg, res.scale = normalize(src, tgt, opt.use_absolute_scale, fp32)
    res.trans, res.sums, res.par = optimize(ns_, nt_, res.corr, sg, opt, fp32)      # (par starts at scale_global: the kept quirk)
    res.T = back_map(res.trans, res.means, sg, W)
    return res


# ---- the cases the GPU tests of the matching use (tests/test_fgr_cpu.py asserts that none has an undecided row) ---------
MATCH_SIZES = [(1, 1), (1, 63), (63, 1), (64, 65), (65, 64), (127, 129), (128, 128), (129, 127)]
MATCH_DIMS = [1, 32, 33, 352, 512]
MATCH_LARGE = [(257, 1000, 33), (257, 1000, 512), (1000, 257, 352), (1000, 1000, 32), (1000, 1000, 1)]


def match_cases():
    """(nq, nr, dim): the small size pairs -- 1, the wave 63 / 64 / 65, the tile edge 127 / 128 / 129 -- at every
    dimension -- 1, the staging trip's multiple 32, 33, 352, the limit 512 -- and five with several tiles"""
    return [(nq, nr, dim) for dim in MATCH_DIMS for nq, nr in MATCH_SIZES] + MATCH_LARGE


def match_case(nq, nr, dim):
    """descriptor-like data: the smaller side holds the originals, the larger side noisy copies of them, copy number c
    of an original with noise 0.01 * 2^c -- so that a row's best and second-best distance differ by a factor, as they
    do between real descriptors, instead of concentrating as distances between independent high-dimensional rows do"""
    rng = np.random.default_rng(1000003 * nq + 1009 * nr + dim)
    scale = 10.0 if dim in (33, 352) else 1.0                   # (histogram-like magnitudes at the two descriptor sizes)
    small, large = min(nq, nr), max(nq, nr)
    orig = rng.standard_normal((small, dim)) * scale
    k = np.arange(large)
    copies = orig[k % small] + rng.standard_normal((large, dim)) * (scale * 0.01 * 2.0 ** (k // small))[:, None]
    copies = copies[rng.permutation(large)]
    Q, R = (orig, copies) if nq <= nr else (copies, orig)
    return np.ascontiguousarray(Q, F32), np.ascontiguousarray(R, F32)


def duplicate_case():
    """exactly duplicated rows on both sides: many rows whose best distance (0, or a repeated value) is reached by
    several columns with the same bits"""
    rng = np.random.default_rng(77)
    base = rng.standard_normal((40, 33)).astype(F32)
    Q = base[np.concatenate([np.arange(40), np.arange(0, 40, 2), np.arange(10)])]
    R = base[np.concatenate([np.arange(5, 40), np.arange(20), np.arange(5, 40), np.arange(30, 40)])]
    return np.ascontiguousarray(Q), np.ascontiguousarray(R)


# ---- the scenes the GPU tests of the whole call use ---------------------------------------------------------------------
def fgr_scenes():
    """name -> (scene, Option): both descriptor sizes in both scale modes, and the noisier variant"""
    out = {}
    for dim in (33, 352):
        for absolute in (False, True):
            out["d%d_%s" % (dim, "abs" if absolute else "rel")] = (scene(dim, seed=1), Option(use_absolute_scale=absolute))
    out["noisy"] = (scene(33, seed=2, desc_sigma=0.6, point_noise=0.002), Option())
    return out
