"""Exact references for the k-NN kernels (csrc/knn_normals.h): EstimateNormals (KNN and Radius), Colored ICP's colour
gradients and KDTreeFlann search, checked point by point.

The idea: on DYADIC clouds -- integer coordinates m in [-362, 362] times 2^-9 -- every square, product and partial sum
of up to 100 terms is an integer below 2^24 in units of 2^-18, so the nine fp32 cumulant sums of a neighbour set are
exact in any order, and so are the squared distances.  For a given neighbour set the kernel's 3x3 matrix A (phase C of
knn_normals_kernel: cum / cnt, then A = c_ij - c_i * c_j, each one correctly rounded fp32 operation) is then restated
here bit for bit; fed to the same eigen3.h (mi_icp_debug_eigen3) and selected as phase C selects, it gives the kernel's
normal bit for bit.  The oracle's neighbour sets are the kernel's wherever the set is unambiguous (`neighbour_sets`).

This is a helper module of the suite, not a conftest: tests import it by name."""
import numpy as np

from oracle import oracle as orc

F32 = np.float32
SCALE = 2.0 ** -9       # lattice step
M_MAX = 362             # |m| <= 362: m^2 * 100 < 2^24
CHUNK = 1 << 16         # queries per oracle search / gather (k = 100: ~160 MB of fp64 gathers)


# ---- dyadic clouds ------------------------------------------------------------------------------------------------
def _finish(m, rng, unique=True):
    """integer lattice points -> float32 coordinates (unique rows, shuffled)"""
    m = np.asarray(m, np.int64)
    assert np.abs(m).max(initial=0) <= M_MAX
    if unique:
        m = np.unique(m, axis=0)
    m = m[rng.permutation(len(m))]
    return (m * SCALE).astype(F32)


def _draw_unique(rng, n, draw):
    """n distinct lattice points from draw(count) -> (count, 3) int array"""
    m = np.unique(draw(n + n // 8 + 16), axis=0)
    while len(m) < n:
        m = np.unique(np.concatenate([m, draw(n - len(m) + 64)]), axis=0)
    return m[rng.permutation(len(m))[:n]]


def cloud_volume(n, seed):
    """n distinct points uniform over the whole lattice cube"""
    rng = np.random.default_rng(seed)
    return _finish(_draw_unique(rng, n, lambda c: rng.integers(-M_MAX, M_MAX + 1, (c, 3))), rng)


def cloud_graded(n, seed):
    """three quarters of the points in a sub-cube about 0.008 points per lattice site dense, the rest over the whole
    cube (~20 times sparser at 700k points): neighbourhood counts within one radius run from none to many"""
    rng = np.random.default_rng(seed)
    core = min(2 * M_MAX - 24, int(round((0.75 * n / 0.008) ** (1.0 / 3.0))))

    def draw(c):
        dense = rng.integers(-core // 2, core // 2 + 1, (c, 3))
        wide = rng.integers(-M_MAX, M_MAX + 1, (c, 3))
        return np.where((np.arange(c) < (3 * c) // 4)[:, None], dense, wide)
    return _finish(_draw_unique(rng, n, draw), rng)


def cloud_sheet(n, seed):
    """a tilted, gently curved sheet three lattice steps thick"""
    rng = np.random.default_rng(seed)

    def draw(c):
        xy = rng.integers(-M_MAX, M_MAX + 1, (c, 2))
        z = (xy[:, 0] // 3 + xy[:, 1] // 5 + (xy[:, 0] * xy[:, 0]) // 2000 - 30 + rng.integers(-1, 2, c))
        return np.column_stack([xy, np.clip(z, -M_MAX, M_MAX)])
    return _finish(_draw_unique(rng, n, draw), rng)


def cloud_duplicates(n, seed, copies=3):
    """n points: distinct sites, each repeated 1..copies times (exact duplicates, shuffled)"""
    rng = np.random.default_rng(seed)
    base = _draw_unique(rng, n, lambda c: rng.integers(-M_MAX // 2, M_MAX // 2 + 1, (c, 3)))
    rep = rng.integers(1, copies + 1, len(base))
    m = np.repeat(base, rep, axis=0)[:n]
    return _finish(m, rng, unique=False)


def cloud_outliers(n, seed, far=1000, core=200):
    """a dense core (a ball of `core` lattice steps) plus `far` points scattered over the whole cube: the far ones'
    k-th neighbours lie across the cloud, so they leave their packets (knn_walks_alone / knn_packet_reaches_too_far)"""
    rng = np.random.default_rng(seed)

    def draw_core(c):
        m = rng.integers(-core, core + 1, (2 * c, 3))
        return m[(m * m).sum(1) <= core * core][:c]
    core = _draw_unique(rng, n - far, draw_core)
    wide = rng.integers(-M_MAX, M_MAX + 1, (far, 3))
    return _finish(np.concatenate([core, wide]), rng, unique=False)


def dyadic_radius(steps):
    """a radius of (steps + 1/2) lattice steps: r^2 = (steps^2 + steps + 1/4) * 2^-18 in fp32 exactly, a quarter step
    off every squared distance of the lattice, so no point lies on the sphere"""
    r = F32((steps + 0.5) * SCALE)
    r2 = r * r
    assert float(r2) == (steps + 0.5) ** 2 * SCALE * SCALE
    return float(r)


def assert_exact_cumulants(pts, k):
    """the premise: sums of up to k coordinates, squares and products of this cloud are exact in fp32 (integers below
    2^24 in units of the lattice)"""
    m = pts.astype(np.float64) / SCALE
    assert np.array_equal(m, np.round(m)), "not on the dyadic lattice"
    a = np.abs(m).max(initial=0)
    assert k * a * a < 2 ** 24 and k * a < 2 ** 24
    assert 3 * (2 * a) ** 2 < 2 ** 24    # squared distances


# ---- neighbour sets and the ambiguity classifier ------------------------------------------------------------------
def neighbour_sets(pts, k, radius=None, extra=0, queries=None):
    """The oracle's k nearest (within `radius` when given, KDTreeSearchParamRadius) of every query -- the cloud's own
    points by default -- and whether that set is the only valid one.

    Returns (idx[n, k] int32 ascending by (d2, index), -1 padded; cnt[n]; d2[n, k]; ambiguous[n] bool).  The oracle is
    asked for k + 1 + extra: a set is unambiguous when it holds every point in range (cnt <= k), when its k-th and
    (k+1)-th distances differ, or when every point tied at the k-th distance has the same coordinates (that needs the
    whole tie group inside the k + 1 + extra returned)."""
    pts = np.ascontiguousarray(pts, F32)
    qry = pts if queries is None else np.ascontiguousarray(queries, F32)
    K = k + 1 + extra
    n = len(qry)
    idx_o, cnt_o, d2_o = np.empty((n, k), np.int32), np.empty(n, np.int64), np.empty((n, k), F32)
    amb = np.zeros(n, bool)
    tree = orc.Tree(pts)
    try:
        for s in range(0, n, CHUNK):
            q = qry[s:s + CHUNK]
            if radius is None:
                _, idx, d2 = tree.search_knn(q, K)
            else:
                _, idx, d2 = tree.search_radius(q, radius, K)
            have = (idx >= 0).sum(1)
            cnt_o[s:s + len(q)] = np.minimum(have, k)
            idx_o[s:s + len(q)] = idx[:, :k]
            d2_o[s:s + len(q)] = d2[:, :k]
            over = have > k
            if not over.any():
                continue
            rows = np.flatnonzero(over)
            D = d2[rows, k - 1]
            tie = d2[rows, k] == D
            rows, D = rows[tie], D[tie]
            if not len(rows):
                continue
            group = d2[rows] == D[:, None]
            open_end = group[:, -1] & (have[rows] == K)        # the group may go on beyond what was returned
            P = pts[np.maximum(idx[rows], 0)]
            same = ((P == pts[idx[rows, k - 1]][:, None, :]).all(2) | ~group).all(1)
            amb[s + rows] = open_end | ~same
    finally:
        tree.close()
    return idx_o, cnt_o, d2_o, amb


# ---- phase C restated ---------------------------------------------------------------------------------------------
def restated_A(pts, idx, cnt):
    """the kernel's covariance A (knn_normals.h phase C) of each neighbour set, as float32 [n, 3, 3]: the nine sums are
    exact (fp64 here, then cast), every later step is one fp32 operation in the kernel's order"""
    P = pts.astype(np.float64)
    n, k = idx.shape
    cum = np.zeros((n, 9), np.float64)
    for s in range(0, n, CHUNK):
        ii = idx[s:s + CHUNK]
        use = (np.arange(k)[None, :] < cnt[s:s + CHUNK, None]) & (ii >= 0)
        g = P[np.maximum(ii, 0)] * use[..., None]
        x, y, z = g[..., 0], g[..., 1], g[..., 2]
        cum[s:s + CHUNK] = np.stack([x.sum(1), y.sum(1), z.sum(1), (x * x).sum(1), (x * y).sum(1), (x * z).sum(1),
                                     (y * y).sum(1), (y * z).sum(1), (z * z).sum(1)], 1)
    c32 = cum.astype(F32)
    assert np.array_equal(c32.astype(np.float64), cum), "cumulant sums are not exact in fp32"
    with np.errstate(divide="ignore", invalid="ignore"):
        c = c32 / np.maximum(cnt, 1).astype(F32)[:, None]
    A = np.empty((n, 3, 3), F32)
    A[:, 0, 0] = c[:, 3] - c[:, 0] * c[:, 0]
    A[:, 1, 1] = c[:, 6] - c[:, 1] * c[:, 1]
    A[:, 2, 2] = c[:, 8] - c[:, 2] * c[:, 2]
    A[:, 0, 1] = A[:, 1, 0] = c[:, 4] - c[:, 0] * c[:, 1]
    A[:, 0, 2] = A[:, 2, 0] = c[:, 5] - c[:, 0] * c[:, 2]
    A[:, 1, 2] = A[:, 2, 1] = c[:, 7] - c[:, 1] * c[:, 2]
    return A


def eigen3(A, device):
    """eigen3.h fast_eigen3x3 through mi_icp_debug_eigen3: device >= 0 on that GPU, -1 on the host.
    Returns eval [n, 3] and evec [n, 3, 3] with eigenvector j in COLUMN j."""
    from cupoch_amd import _lib
    A = np.ascontiguousarray(A, F32)
    n = len(A)
    ev, vec = np.empty((n, 3), F32), np.empty((n, 3, 3), F32)
    if n:
        rc = _lib.load().mi_icp_debug_eigen3(device, A.ctypes.data, n, ev.ctypes.data, vec.ctypes.data, None)
        assert rc == 0, rc
    return ev, vec


def select_normal(ev, vec, cnt):
    """phase C's choice: the lowest eigenvalue, strict < in index order; (0, 0, 1) for fewer than 3 neighbours or an
    eigenvector of zero / NaN length"""
    n = len(ev)
    mi = np.zeros(n, np.int64)
    mi = np.where(ev[:, 1] < ev[np.arange(n), mi], 1, mi)
    mi = np.where(ev[:, 2] < ev[np.arange(n), mi], 2, mi)
    v = vec[np.arange(n), :, mi]
    l2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    fall = (cnt < 3) | (l2 == 0) | np.isnan(l2)
    out = np.where(fall[:, None], np.array([0, 0, 1], F32), v).astype(F32)
    return out


def restated_normals(pts, idx, cnt, device):
    """the kernel's normal of each given neighbour set"""
    ev, vec = eigen3(restated_A(pts, idx, cnt), device)
    return select_normal(ev, vec, cnt)


def bits_equal(a, b):
    """row-wise bit equality of two float32 arrays (tells -0 from +0, NaN equals its own bits)"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return (a.view(np.uint32) == b.view(np.uint32)).all(1)


# ---- colour gradients ---------------------------------------------------------------------------------------------
def gradient_reference(pts, nrm, inten, idx, cnt):
    """InitializePointCloudForColoredICP in fp64 (colored_icp.cu:88-120): the least-squares intensity gradient in the
    tangent plane over the neighbours after the nearest (the point itself), as the 3x3 normal equations of
    [v; (nn-1) n; 1e-3 I] g = [di; 0].  Returns (ref[n, 3], tol[n], zero[n]): zero marks fewer than four others, where
    the gradient is exactly 0; tol is the per-point bound of test_gpu_outside_checks.py's lstsq check,
    3e-7 * cond * max(|ref|, 1e-4) + 1e-7, made to hold for every point of large clouds in the fp32 formulation
    itself (the oracle's, test_knn_exact_cpu.py): cond becomes l2^2 / (l0 l1) -- the cofactor inverse's determinant
    cancels when TWO eigenvalues are small, as with four neighbours -- times |p| / |v| (fp32 forms the tangent offsets
    from coordinates), and 3e-7 becomes 4e-6."""
    P, N, I = pts.astype(np.float64), nrm.astype(np.float64), inten.astype(np.float64)
    n, k = idx.shape
    ref, tol = np.zeros((n, 3)), np.full(n, np.inf)
    nn = np.maximum(cnt - 1, 0)
    zero = nn < 4
    for s in range(0, n, CHUNK):
        e = min(n, s + CHUNK)
        nb = idx[s:e, 1:]
        use = ((np.arange(1, k)[None, :] < cnt[s:e, None]) & (nb >= 0)).astype(np.float64)
        nbc = np.maximum(nb, 0)
        Ni = N[s:e]
        dd = P[nbc] - P[s:e, None, :]
        v = (dd - (dd @ Ni[:, :, None]) * Ni[:, None, :]) * use[..., None]
        di = (I[nbc] - I[s:e, None]) * use
        w = (nn[s:e] - 1.0) ** 2
        M = np.einsum("nki,nkj->nij", v, v) + w[:, None, None] * np.einsum("ni,nj->nij", Ni, Ni)
        b = np.einsum("nki,nk->ni", v, di)
        # fp32 forms v from coordinates, not offsets: its rounding is relative to |p| / |v|, not to |v|
        mag = np.maximum(1.0, np.abs(P[s:e]).max(1) / np.maximum(np.sqrt((v * v).sum(2).max(1)), 1e-30))
        lam = np.linalg.eigvalsh(M)
        g = np.linalg.solve(M + 1e-6 * np.eye(3), b[..., None])[..., 0]
        with np.errstate(divide="ignore", invalid="ignore"):
            t = 4e-6 * (lam[:, 2] * lam[:, 2] / (lam[:, 0] * lam[:, 1])) * np.maximum(np.abs(g).max(1), 1e-4) * mag + 1e-7
        t = np.where(np.isfinite(t) & (lam[:, 0] > 0), t, np.inf)
        ref[s:e], tol[s:e] = g, t
    ref[zero] = 0.0
    return ref, tol, zero


def gradient_cloud(n, max_nn, seed):
    """random fp32 points (distinct: the point itself is the unique nearest), unit normals and colours, and a radius
    at which a uniform cloud of n points holds about max_nn neighbours: counts run from under 5 to over max_nn"""
    rng = np.random.default_rng(seed)
    pts = np.unique(rng.random((n, 3), dtype=F32), axis=0)
    pts = pts[rng.permutation(len(pts))] - F32(0.5)
    pts[: len(pts) // 10] *= F32(3.0)                     # a sparse shell around the unit cube
    nrm = rng.standard_normal((len(pts), 3)).astype(F32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True).astype(F32)
    col = rng.random((len(pts), 3), dtype=F32)
    # the scale of test_gpu_outside_checks.py's lstsq check: a radius of 6 (tangent offsets and the normal's weight
    # (nn - 1) of one order, as in a colored-ICP scan in metres with a radius of centimetres... in units of it)
    scale = 6.0 / ((max_nn / (len(pts) * 4.19)) ** (1.0 / 3.0))
    return (pts * F32(scale)).astype(F32), nrm, col, 6.0


# ---- KDTreeFlann rows ---------------------------------------------------------------------------------------------
def rows_equal_up_to_ties(idx, d2, oi, od, tgt, qry):
    """search rows against the oracle's: distances bit-exact; indices equal except where equal distances allow a
    choice; every row's valid indices distinct and inside [0, nt), its padding exactly -1 / +inf"""
    nt = len(tgt)
    fin = np.isfinite(od)
    assert np.array_equal(np.isfinite(d2), fin)
    assert np.array_equal(d2[fin], od[fin])
    assert np.array_equal(idx < 0, oi < 0)
    got = idx >= 0
    assert np.array_equal(got, fin), "an index without a distance, or a distance without an index"
    assert (idx[~got] == -1).all() and (d2[~fin] == np.inf).all(), "padding is not -1 / +inf"
    assert (idx[got] < nt).all(), "index outside the target"
    # padding only at the end of a row, and no index twice in one row
    assert (np.diff(got.astype(np.int8), axis=1) <= 0).all(), "padding inside a row"
    srt = np.sort(np.where(got, idx, -1 - np.arange(idx.shape[1])[None, :]), axis=1)
    assert not (np.diff(srt, axis=1) == 0).any(), "an index twice in one row"
    bad = np.flatnonzero((idx != oi).any(axis=1))
    for r in bad:                                      # only ties may differ
        k = int(fin[r].sum())
        dd = tgt[idx[r, :k]] - qry[r]
        chk = (dd[:, 2] * dd[:, 2] + (dd[:, 1] * dd[:, 1] + dd[:, 0] * dd[:, 0])).astype(np.float32)
        np.testing.assert_allclose(chk, od[r, :k], rtol=5e-7, err_msg=str(r))   # (numpy has no fma: last-ulp slack)
        # (a tie inside the row, or between its last entry and the first point left out: the
        # distances are the oracle's bit for bit either way, so this is a valid answer)
    assert len(bad) <= max(2, len(idx) // 200)

