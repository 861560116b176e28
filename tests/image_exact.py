"""The image contract of include/mi_icp.h ("image") restated in numpy: a helper, not a test.  Every operation is carried
in float32 one rounding at a time in the order the contract writes it (numpy never fuses a multiply with an add; where
the contract writes fmaf, fma32 below rounds the exact product-plus-addend once), so the results are the words the
kernels must produce -- except the bilateral filter, whose restatement carries the exponential, the two sums and the
quotient in float64 and is compared under a bound (bilateral_bound).  The filters, the three-channel intensity and the
depth value are held to the reference's own byte vectors (tests/test_reference_vectors_cpu.py)."""
import numpy as np

F = np.float32
MAX_TAPS = 31
MAX_DIAMETER = 31

GAUSSIAN3, GAUSSIAN5, GAUSSIAN7, SOBEL3DX, SOBEL3DY = range(5)
EQUAL, WEIGHTED = 0, 1
_G3 = [.25, .5, .25]
_G5 = [.0625, .25, .375, .25, .0625]
_G7 = [.03125, .109375, .21875, .28125, .21875, .109375, .03125]
_S1, _S2 = [-1.0, 0.0, 1.0], [1.0, 2.0, 1.0]
NAMED = {GAUSSIAN3: (_G3, _G3), GAUSSIAN5: (_G5, _G5), GAUSSIAN7: (_G7, _G7), SOBEL3DX: (_S1, _S2), SOBEL3DY: (_S2, _S1)}
SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 5), (37, 23), (64, 16), (65, 17)]       # (width, height)


def same_words(a, b):
    """same shape and type, same NaN mask, same bits elsewhere"""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != F:
        return a.tobytes() == b.tobytes()
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and (a.view(np.uint32)[~na] == b.view(np.uint32)[~nb]).all())


def float_image(w, h, seed=0, specials=True):
    """a float image of noise on a ramp with (room permitting) a NaN, a +inf and a -inf pixel"""
    rng = np.random.default_rng(seed + 1000 * w + h)
    img = (rng.standard_normal((h, w)) + np.linspace(0.0, 3.0, w)[None, :]).astype(F)
    if specials and w * h >= 15:
        flat = img.reshape(-1)
        flat[(w * h) // 3] = np.nan
        flat[(w * h) // 2] = np.inf
        flat[(2 * w * h) // 3 + 1] = -np.inf
    return img


def fma32(a, b, c):
    """fmaf(a, b, c) element-wise: the exact a * b + c rounded to float32 once.  The product of two float32 is exact in
    float64 (48 bits), but float64(product + c) -> float32 rounds twice and is wrong on ties (math.fma on doubles would
    round the same two times).  So the float64 sum is made round-to-odd from its exact error term (Knuth's two-sum):
    with 53 >= 24 + 2 bits the final rounding to float32 is then the correct single rounding."""
    with np.errstate(all="ignore"):
        p = np.asarray(a, F).astype(np.float64) * np.asarray(b, F).astype(np.float64)
        c = np.asarray(c, F).astype(np.float64)
        p, c = np.broadcast_arrays(p, c)
        s = p + c
        bb = s - p
        e = (p - (s - bb)) + (c - bb)            # p + c = s + e exactly
        even = ((np.ascontiguousarray(s).reshape(-1).view(np.uint64) & np.uint64(1)) == 0).reshape(s.shape)
        fix = np.isfinite(s) & (e != 0) & even   # s is not exact and its last bit is even: step towards the true sum
        toward = np.where(e > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(F)[()]


def filter_horizontal(src, k):
    src, k = np.asarray(src, F), np.asarray(k, F)
    h, w = src.shape
    half = len(k) // 2
    x = np.arange(w)
    t = np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for i in range(-half, half + 1):
            t = fma32(src[:, np.clip(x + i, 0, w - 1)], k[i + half], t)
    return t


def filter_literal(src, dx, dy):
    """horizontal(dx), transpose, horizontal(dy), transpose: the reference's four steps"""
    return np.ascontiguousarray(filter_horizontal(np.ascontiguousarray(filter_horizontal(src, dx).T), dy).T)


def filter_taps(src, dx, dy):
    """the one-pass form: column sums of the row sums of the clamped rows"""
    src, dy = np.asarray(src, F), np.asarray(dy, F)
    h, w = src.shape
    rows = filter_horizontal(src, dx)
    half = len(dy) // 2
    y = np.arange(h)
    out = np.zeros((h, w), F)
    with np.errstate(all="ignore"):
        for j in range(-half, half + 1):
            out = fma32(rows[np.clip(y + j, 0, h - 1), :], dy[j + half], out)
    return out


def filter_named(src, kind):
    return filter_taps(src, *NAMED[kind])


def downsample(src):
    src = np.asarray(src)
    h, w = src.shape[:2]
    hh, hw = h // 2, w // 2
    p00, p01 = src[0:2 * hh:2, 0:2 * hw:2], src[0:2 * hh:2, 1:2 * hw:2]
    p10, p11 = src[1:2 * hh:2, 0:2 * hw:2], src[1:2 * hh:2, 1:2 * hw:2]
    if src.dtype == np.uint8:
        s = p00.astype(np.int32) + p01 + p10 + p11
        return (s // 4).astype(np.uint8)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray((((p00 + p01) + p10) + p11) / F(4.0)).astype(F)


def pyramid_level(src):
    return downsample(filter_named(src, GAUSSIAN3))


def create_pyramid(src, levels, with_gaussian):
    out = []
    for i in range(levels):
        if i == 0:
            out.append(np.array(src, copy=True))
        elif out[-1].size == 0 or out[-1].shape[0] // 2 == 0 or out[-1].shape[1] // 2 == 0:
            out.append(np.zeros((0, 0) + src.shape[2:], src.dtype))
        elif with_gaussian and src.ndim == 2:
            out.append(pyramid_level(out[-1]))
        else:
            out.append(downsample(out[-1]))
    return out


def bilateral_table(diameter, sigma_space, shift=0):
    s2 = F(sigma_space) * F(sigma_space)
    x = (np.arange(2 * diameter + 1) - diameter + shift).astype(F)
    arg = -(x * x) / (F(2) * s2)
    return np.exp(arg.astype(np.float64)).astype(F)


def _windows(src, d, past_end=False):
    """[2d+1, 2d+1, H, W]: the clamped taps of every pixel (past_end: the reference's clamp to h and w on the image
    zero-padded by one row and one column)"""
    h, w = src.shape
    if past_end:
        src = np.pad(src, ((0, 1), (0, 1)))
    ys, xs = np.arange(h), np.arange(w)
    hi_y, hi_x = (h, w) if past_end else (h - 1, w - 1)
    out = np.empty((2 * d + 1, 2 * d + 1, h, w), src.dtype)
    for dy in range(-d, d + 1):
        rows = src[np.clip(ys + dy, 0, hi_y)]
        for dx in range(-d, d + 1):
            out[dy + d, dx + d] = rows[:, np.clip(xs + dx, 0, hi_x)][:, :w]
    return out


def bilateral(src, diameter, sigma_color, sigma_space, past_end=False, table_shift=0):
    """the reference value of the bound: fp32 arguments and fp32 table products as the contract writes them, the
    exponential, the two sums and the quotient in float64"""
    src = np.asarray(src, F)
    d = int(diameter)
    g = bilateral_table(d, sigma_space, table_shift)
    win = _windows(src, d, past_end)
    with np.errstate(all="ignore"):
        c = src[None, None] - win
        arg = -(c * c) / ((F(2.0) * F(sigma_color)) * F(sigma_color))
        gg = (g[:, None] * g[None, :]).astype(F)
        w = gg[:, :, None, None].astype(np.float64) * np.exp(arg.astype(np.float64))
        wc = w * win.astype(np.float64)
        n = (2 * d + 1) ** 2
        filtered = wc.reshape(n, *src.shape).sum(0)
        total = w.reshape(n, *src.shape).sum(0)
        return filtered / total


def bilateral_bound(src, diameter):
    """(4 T + 64) 2^-24 M per pixel, T = (2 d + 1)^2, M the largest |value| in the pixel's clamped window"""
    d = int(diameter)
    with np.errstate(all="ignore"):
        m = np.abs(_windows(np.asarray(src, F), d)).reshape((2 * d + 1) ** 2, *src.shape).max(0)
    return (4.0 * (2 * d + 1) ** 2 + 64.0) * 2.0 ** -24 * m.astype(np.float64)


def bilateral_image(w, h, seed, special=None):
    """a step edge, a ramp and noise; special: None, "nan" or "inf" (one pixel)"""
    rng = np.random.default_rng(seed)
    x = np.arange(w)[None, :]
    img = np.where(x < w // 2, 1.0, 2.5) + 0.01 * np.arange(h)[:, None] + 0.05 * rng.standard_normal((h, w))
    img = img.astype(F)
    if special:
        img[h // 3, w // 4] = np.nan if special == "nan" else np.inf
    return img


def sat(v, top):
    """float -> unsigned by truncation, saturating, NaN -> 0"""
    v = np.asarray(v)
    with np.errstate(all="ignore"):
        out = np.where(v > 0, np.minimum(v, top), 0)
        return np.trunc(np.where(np.isnan(out), 0, out))


def _values(img):
    """(float32 values [H, W, C], channels, bytes per channel)"""
    img = np.asarray(img)
    a = img if img.ndim == 3 else img[:, :, None]
    return a.astype(F), a.shape[2], img.dtype.itemsize


def _weights(kind):
    return (F(1.0 / 3.0),) * 3 if kind == EQUAL else (F(0.2990), F(0.5870), F(0.1140))


def _intensity(img, kind, denom):
    v, ch, _ = _values(img)
    with np.errstate(all="ignore"):
        if ch == 1:
            return v[:, :, 0] * denom
        if ch == 3:
            w = _weights(kind)
            return fma32(w[2], v[:, :, 2], fma32(w[0], v[:, :, 0], w[1] * v[:, :, 1])) * denom
    return np.zeros(v.shape[:2], F)


def create_float(img, kind=WEIGHTED):
    denom = F(1.0 / 255.0) if np.asarray(img).dtype.itemsize == 1 else F(1.0)
    return _intensity(img, kind, denom).astype(F)


def create_gray(img, kind=WEIGHTED):
    size = np.asarray(img).dtype.itemsize
    denom = F(1.0) if size == 1 else (F(255.0 / 65535.0) if size == 2 else F(255.0))
    return sat(_intensity(img, kind, denom), 255).astype(np.uint8)


def depth_to_float(img, scale=1000.0, trunc=3.0):
    with np.errstate(all="ignore"):
        f = create_float(img) * F(np.float64(1.0) / np.float64(F(int(scale))))
    return np.where(f >= F(int(trunc)), F(0), f).astype(F)


def from_float(img, size):
    img = np.asarray(img, F)
    with np.errstate(all="ignore"):
        return sat(img * F(255.0), 255).astype(np.uint8) if size == 1 else sat(img, 65535).astype(np.uint16)


def linear_transform(img, scale, offset):
    img = np.asarray(img)
    with np.errstate(all="ignore"):
        v = F(scale) * img.astype(F) + F(offset)
    return sat(v, 255).astype(np.uint8) if img.dtype == np.uint8 else v.astype(F)


def clip(img, lo, hi):
    return np.fmax(np.fmin(F(hi), np.asarray(img, F)), F(lo)).astype(F)


def sun(depth):
    d = np.asarray(depth, np.uint16).astype(np.uint32)
    return (((d >> 3) | (d << 13)) & 0xffff).astype(np.uint16)


def nyu(depth):
    d = np.asarray(depth, np.uint16).byteswap().astype(np.float64)
    xx = (351.3 / (1092.5 - d)).astype(F)
    r = np.floor(xx.astype(np.float64) * 1000 + 0.5)
    return np.where(xx <= 0, 0, np.minimum(r, 65535)).astype(np.uint16)


FORMATS = {"redwood": (1000.0, 4.0), "tum": (5000.0, 4.0), "sun": (1000.0, 7.0), "nyu": (1000.0, 7.0)}


def rgbd(color, depth, scale=1000.0, trunc=3.0, convert_rgb_to_intensity=True, fmt=None):
    """(colour, depth) of RGBDImage::CreateFromColorAndDepth and the four format factories"""
    if fmt is not None:
        scale, trunc = FORMATS[fmt]
        depth = sun(depth) if fmt == "sun" else (nyu(depth) if fmt == "nyu" else depth)
    return (create_float(color) if convert_rgb_to_intensity else np.array(color, copy=True)), depth_to_float(depth, scale, trunc)
