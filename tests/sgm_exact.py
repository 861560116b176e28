"""The stereo contract of include/mi_icp.h ("stereo") restated in numpy, stage by stage: a helper, not a test.
Semi-global matching is integer arithmetic up to the disparity image, so these are the bytes the kernels must produce;
points_from_disparity carries float32 one rounding at a time in the order the contract writes it (numpy never fuses a
multiply with an add).  The keyword arguments named `wrong_*` build deliberately wrong variants for test_sgm_cpu.py:
the contract is what every function computes without them."""
import numpy as np

F = np.float32
INVALID = 0xFFFF
MAX_P2 = 224
_BIG = 0x3FFF
_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.uint8)
PATHS4 = [(0, 1), (0, -1), (1, 0), (-1, 0)]
PATHS8 = PATHS4 + [(1, 1), (1, -1), (-1, 1), (-1, -1)]
OFFSETS = [(dy, dx) for dy in range(-3, 4) for dx in range(-4, 5)][:31]        # all offsets before the centre


def pair(w, h, seed, bg=5, fg=20):
    """(left, right, truth): a smoothed random texture seen with disparity bg, and fg in the middle box"""
    rng = np.random.default_rng(seed)
    tex = rng.integers(0, 256, (h, w + 64)).astype(F)
    tex = (tex + np.roll(tex, 1, 0) + np.roll(tex, 1, 1) + np.roll(np.roll(tex, 1, 0), 1, 1)) / F(4)
    left = tex[:, :w]
    truth = np.full((h, w), bg, np.int32)
    truth[h // 4:3 * h // 4, w // 3:2 * w // 3] = fg
    right = rng.integers(0, 256, (h, w)).astype(F)
    ys, xs = np.nonzero(np.ones((h, w), bool))
    for value in (bg, fg):
        sel = (truth[ys, xs] == value) & (xs - value >= 0)
        right[ys[sel], xs[sel] - value] = left[ys[sel], xs[sel]]
    return left.astype(np.uint8), right.astype(np.uint8), truth


def census(img, wrong_order=False):
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    out = np.zeros((h, w), np.uint32)
    if h < 7 or w < 9:
        return out
    core = np.zeros((h - 6, w - 8), np.uint32)
    for k, (dy, dx) in enumerate(OFFSETS):
        a = img[3 + dy:h - 3 + dy, 4 + dx:w - 4 + dx]
        b = img[3 - dy:h - 3 - dy, 4 - dx:w - 4 - dx]
        core |= ((b > a) if wrong_order else (a > b)).astype(np.uint32) << np.uint32(k)
    out[3:h - 3, 4:w - 4] = core
    return out


def cost_volume(cen_l, cen_r, disp_size, min_disp=0):
    """C[y][x][d] as uint8"""
    h, w = cen_l.shape
    C = np.empty((h, w, disp_size), np.uint8)
    for d in range(disp_size):
        s = d + min_disp
        shifted = np.zeros_like(cen_r)
        if s < w:
            shifted[:, s:] = cen_r[:, :w - s]
        x = cen_l ^ shifted
        C[:, :, d] = _POP16[x & 0xFFFF] + _POP16[x >> 16]
    return C


def _step(c, prev, p1, p2, reach):
    m = prev.min(axis=1, keepdims=True)
    best = np.minimum(prev, m + np.int16(p2))
    best[:, reach:] = np.minimum(best[:, reach:], prev[:, :-reach] + np.int16(p1))
    best[:, :-reach] = np.minimum(best[:, :-reach], prev[:, reach:] + np.int16(p1))
    return c + best - m


def aggregate(C, dy, dx, p1=10, p2=120, wrong_reach=1):
    """L_r for r = (dy, dx) as int16 [y][x][d]"""
    h, w, D = C.shape
    C = C.astype(np.int16)
    L = np.empty_like(C)
    if dy == 0:
        xs = range(w) if dx > 0 else range(w - 1, -1, -1)
        for i, x in enumerate(xs):
            L[:, x] = C[:, x] if i == 0 else _step(C[:, x], L[:, x - dx], p1, p2, wrong_reach)
        return L
    ys = range(h) if dy > 0 else range(h - 1, -1, -1)
    for i, y in enumerate(ys):
        if i == 0:
            L[y] = C[y]
            continue
        # the pixel before (y, x) is (y - dy, x - dx): columns whose x - dx lies in the image continue their path
        lo, hi = max(0, dx), w + min(0, dx)
        L[y] = C[y]
        if hi > lo:
            L[y, lo:hi] = _step(C[y, lo:hi], L[y - dy, lo - dx:hi - dx], p1, p2, wrong_reach)
    return L


def sums(C, path8=True, p1=10, p2=120, wrong_reach=1):
    S = np.zeros(C.shape, np.int16)
    for dy, dx in (PATHS8 if path8 else PATHS4):
        S += aggregate(C, dy, dx, p1, p2, wrong_reach)
    return S.astype(np.uint16)


def _argmin(S, wrong_last):
    if wrong_last:
        return S.shape[2] - 1 - np.argmin(S[:, :, ::-1], axis=2)
    return np.argmin(S, axis=2)


def left_map(S, uniqueness=0.95, wrong_last=False):
    S = S.astype(np.int32)
    D = S.shape[2]
    dl = _argmin(S, wrong_last)
    s1 = np.take_along_axis(S, dl[:, :, None], 2)[:, :, 0]
    far = np.abs(np.arange(D)[None, None, :] - dl[:, :, None]) > 1
    s2 = np.where(far, S, np.int32(1 << 30)).min(axis=2)
    invalid = F(uniqueness) * s2.astype(F) < s1.astype(F)
    return np.where(invalid, INVALID, dl).astype(np.uint16)


def right_map(S, min_disp=0, wrong_last=False):
    h, w, D = S.shape
    R = np.full((h, w, D), 1 << 30, np.int32)
    for d in range(D):
        s = d + min_disp
        if s < w:
            R[:, :w - s, d] = S[:, s:, d]
    dr = _argmin(R, wrong_last)
    dr[(R == (1 << 30)).all(axis=2)] = 0
    return dr.astype(np.uint16)


def median3(m):
    m = np.asarray(m, np.uint16)
    h, w = m.shape
    out = m.copy()
    if h < 3 or w < 3:
        return out
    win = np.stack([m[j:h - 2 + j, i:w - 2 + i] for j in range(3) for i in range(3)], axis=0)
    out[1:h - 1, 1:w - 1] = np.sort(win, axis=0)[4]
    return out


def check(lm, rm, min_disp=0, lr_max_diff=1):
    """left-right check of the two maps and the 8-bit output"""
    h, w = lm.shape
    d = lm.astype(np.int32)
    valid = d != INVALID
    if lr_max_diff >= 0:
        k = np.arange(w)[None, :] - (d + min_disp)
        inside = valid & (k >= 0)
        other = np.take_along_axis(rm.astype(np.int32), np.where(inside, k, 0), axis=1)
        valid = inside & (np.abs(other - d) <= lr_max_diff)
    return np.where(valid, d + min_disp, min_disp - 1).astype(np.uint8)


def valid_options(width, height, p1, p2, disp_size, min_disp):
    return bool(width > 0 and height > 0 and 0 <= p1 <= p2 <= MAX_P2 and disp_size in (64, 128, 256) and min_disp >= 0
                and min_disp + disp_size <= 256)


def sgm(left, right, p1=10, p2=120, uniqueness=0.95, disp_size=128, path8=True, min_disp=0, lr_max_diff=1, stages=None,
        wrong_order=False, wrong_reach=1, wrong_last=False, wrong_median_last=False):
    """the disparity image; `stages`, a dict, receives the census planes, S and the four maps"""
    cl, cr = census(left, wrong_order), census(right, wrong_order)
    S = sums(cost_volume(cl, cr, disp_size, min_disp), path8, p1, p2, wrong_reach)
    lm, rm = left_map(S, uniqueness, wrong_last), right_map(S, min_disp, wrong_last)
    if wrong_median_last:
        out = check(lm, rm, min_disp, lr_max_diff)
        return median3(out.astype(np.uint16)).astype(np.uint8)
    lmm, rmm = median3(lm), median3(rm)
    if stages is not None:
        stages.update(census_left=cl, census_right=cr, S=S, left=lm, right=rm, left_median=lmm, right_median=rmm)
    return check(lmm, rmm, min_disp, lr_max_diff)


def disparity_q(fx, fy, cx, cy, cx_right, baseline):
    """{q00, q03, q11, q13, q23, q32, q33} in float32, left to right"""
    fx, fy, cx, cy, cxr = F(fx), F(fy), F(cx), F(cy), F(cx_right)
    tx = -F(baseline)
    return np.array([fy * tx, -fy * cx * tx, fx * tx, -fx * cy * tx, fx * fy * tx, -fy, fy * (cx - cxr)], F)


def points_from_disparity(disp, color, fx, fy, cx, cy, cx_right, baseline):
    """-> (points [H * W, 3], colors [H * W, 3]) float32"""
    disp = np.asarray(disp, np.uint8)
    color = np.asarray(color)
    h, w = disp.shape
    q00, q03, q11, q13, q23, q32, q33 = disparity_q(fx, fy, cx, cy, cx_right, baseline)
    v, u = np.divmod(np.arange(h * w), w)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wv = q32 * disp.reshape(-1).astype(F) + q33
        r = (1.0 / wv.astype(np.float64)).astype(F)
        pts = np.stack([(q00 * u.astype(F) + q03) * r, (q11 * v.astype(F) + q13) * r, q23 * r], axis=1).astype(F)
    k = F(255.0) if color.dtype.itemsize == 1 else F(65535.0)
    return pts, (color.reshape(-1, 3).astype(F) / k).astype(F)


def same_words(a, b):
    """same shape, same NaN mask, same bits elsewhere"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())
