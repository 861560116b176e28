"""GPU: geometry.Image / geometry.RGBDImage against the numpy restatement of the image contract (tests/image_exact.py).

Everything but the bilateral filter is compared on the words: same NaN mask, same uint32 view elsewhere
(image_exact.same_words), at the smallest sizes at which tiling, halos and clamps can go wrong and once at 640x480, from a
numpy input and from a CUDA tensor.  The three 3-tap filters are also held to the odometry oracle.

The bilateral filter is held by a derived bound: |got - ref| <= (4 T + 64) 2^-24 M, T = (2 d + 1)^2 taps, M the largest
|value| in the pixel's clamped window; ref carries the fp32 arguments and fp32 table products of the contract and the
exponential, the two sums and the quotient in float64.  Where it comes from: each of the two sums rounds once per tap
(2 T roundings of terms bounded by the running sums, which are at most `total` M and `total`), each product w cur and
each w rounds (folded into the same count: 4 T in all, relative to `total` >= the centre's weight 1), the quotient rounds
once, the device exponential is within 2 ulp, and the exp2 path's argument scaling costs |arg| 2^-24 relative on a weight
w, where w |arg| <= 1/e -- the 64 covers those constants.  tests/test_image_cpu.py shows that a wrong clamp or table index
lies more than 100 bounds away on these images.  MEASURED on an MI355X over every case below, both exponentials: the
largest |got - ref| / bound is 0.0485 (hardware exponential) and 0.0474 (expf)."""
import functools

import numpy as np
import pytest

import image_exact as ix
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

F = np.float32
SIDES = ["numpy", "cuda"]
SIZES = ix.SIZES + [(640, 480)]
SIZE_IDS = ["%dx%d" % s for s in SIZES]
BILATERAL_CASES = [(40, 30, 11, "nan"), (37, 23, 12, "inf"), (37, 23, 13, None)]      # as tests/test_image_cpu.py
BILATERAL_SIGMAS = [(2.0, 2.0), (0.5, 3.0), (0.1, 4.5)]      # the controls' pair, an edge-preserving one, KinFu's depth pair


def put(a, side):
    import torch
    return a if side == "numpy" else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def img(a, side="numpy"):
    from cupoch_amd import geometry as g
    return g.Image(put(a, side))


def host(image):
    a = np.asarray(image)
    return np.ascontiguousarray(a)


@functools.lru_cache(maxsize=None)
def source(w, h):
    return ix.float_image(w, h)


@functools.lru_cache(maxsize=None)
def filtered(w, h, kind):
    return ix.filter_named(source(w, h), kind)


def kinds():
    from cupoch_amd import geometry as g
    T = g.ImageFilterType
    return {ix.GAUSSIAN3: T.Gaussian3, ix.GAUSSIAN5: T.Gaussian5, ix.GAUSSIAN7: T.Gaussian7, ix.SOBEL3DX: T.Sobel3dx, ix.SOBEL3DY: T.Sobel3dy}


# ---------------------------------------------------------------- filters
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("size", SIZES, ids=SIZE_IDS)
def test_named_filters(size, side):
    w, h = size
    src = img(source(w, h), side)
    for kind, name in kinds().items():
        got = src.filter(name)
        assert (got.width, got.height, got.num_of_channels, got.bytes_per_channel) == (w, h, 1, 4)
        assert ix.same_words(host(got), filtered(w, h, kind)), (kind, size)
    for oracle_kind, kind in enumerate((ix.GAUSSIAN3, ix.SOBEL3DX, ix.SOBEL3DY)):
        assert ix.same_words(host(src.filter(kinds()[kind])), orc.od_filter(source(w, h), oracle_kind))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("size", [(5, 3), (37, 23), (65, 17)], ids=["5x3", "37x23", "65x17"])
def test_caller_taps_and_the_horizontal_pass(size, side):
    rng = np.random.default_rng(5)
    src = source(*size)
    for nx, ny in [(1, 1), (9, 9), (31, 31), (1, 31), (31, 3), (9, 1)]:
        dx, dy = rng.standard_normal(nx).astype(F), rng.standard_normal(ny).astype(F)
        got = img(src, side).filter_taps(dx, dy)
        want = ix.filter_taps(src, dx, dy)
        assert ix.same_words(host(got), want), (nx, ny)
        assert ix.same_words(want, ix.filter_literal(src, dx, dy))
        assert ix.same_words(host(img(src, side).filter_horizontal(dx)), ix.filter_horizontal(src, dx)), nx


def test_filter_makes_a_float_image_first():
    rng = np.random.default_rng(6)
    rgb = rng.integers(0, 256, (23, 37, 3), dtype=np.uint8)
    got = img(rgb).filter(kinds()[ix.GAUSSIAN5])
    assert ix.same_words(host(got), ix.filter_named(ix.create_float(rgb), ix.GAUSSIAN5))


# ---------------------------------------------------------------- downsample and pyramids
@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("size", [(2, 2), (3, 5), (37, 23), (65, 17), (640, 480)], ids=["2x2", "3x5", "37x23", "65x17", "640x480"])
def test_downsample(size, side):
    w, h = size
    got = img(source(w, h), side).downsample()
    assert ix.same_words(host(got), ix.downsample(source(w, h))) and ix.same_words(host(got), orc.od_downsample(source(w, h)))
    rgb = np.random.default_rng(w).integers(0, 256, (h, w, 3), dtype=np.uint8)
    rgb[: h // 2, : w // 2] = 255             # sums above 255 * 3
    got = img(rgb, side).downsample()
    assert (got.width, got.height, got.num_of_channels, got.bytes_per_channel) == (w // 2, h // 2, 3, 1)
    assert host(got).tobytes() == ix.downsample(rgb).tobytes()
    assert img(source(1, 9), side).downsample().is_empty()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("gaussian", [True, False])
def test_create_pyramid(gaussian, side):
    import torch
    src = source(37, 23)
    given = put(src, side)
    levels = img(given).create_pyramid(7, gaussian)
    want = ix.create_pyramid(src, 7, gaussian)
    assert [(p.width, p.height) for p in levels] == [(37, 23), (18, 11), (9, 5), (4, 2), (2, 1), (0, 0), (0, 0)]
    for got, ref in zip(levels[:5], want[:5]):
        assert ix.same_words(host(got), ref)
    assert levels[5].is_empty() and levels[6].is_empty()
    if side == "cuda":                                       # level 0 is a copy, not the input
        assert levels[0].data.data_ptr() != given.data_ptr()
        levels[0].data.zero_()
        assert ix.same_words(given.cpu().numpy(), src)
    if gaussian:                                             # the fused level is the two steps
        two = img(src, side).filter(kinds()[ix.GAUSSIAN3]).downsample()
        assert ix.same_words(host(levels[1]), host(two))
    assert isinstance(levels[1].data, torch.Tensor) and levels[1].data.is_cuda


@pytest.mark.parametrize("size", [(64, 16), (65, 17), (640, 480), (2, 2), (3, 5)], ids=["64x16", "65x17", "640x480", "2x2", "3x5"])
def test_fused_pyramid_level(size):
    from cupoch_amd import geometry as g
    src = source(*size)
    got = g.get_engine().image_pyramid_level(put(src, "cuda"))
    assert ix.same_words(got.cpu().numpy(), ix.pyramid_level(src))
    assert ix.same_words(got.cpu().numpy(), orc.od_downsample(orc.od_filter(src, 0)))


def test_rgb_pyramid_and_the_pyramid_filters():
    from cupoch_amd import geometry as g
    rgb = np.random.default_rng(8).integers(0, 256, (23, 37, 3), dtype=np.uint8)
    levels = g.Image(rgb)._pyramid(3, True)                  # the C++ rule: 3 x uint8 stays 3 x uint8, no Gaussian
    want = ix.create_pyramid(rgb, 3, False)
    assert all(host(a).tobytes() == b.tobytes() and a.num_of_channels == 3 for a, b in zip(levels, want))
    levels = g.Image(rgb).create_pyramid(3, True)            # the Python rule: a float image first
    want = ix.create_pyramid(ix.create_float(rgb), 3, True)
    assert all(ix.same_words(host(a), b) for a, b in zip(levels, want))
    for kind, name in kinds().items():
        out = g.Image.filter_pyramid(levels, name)
        assert all(ix.same_words(host(a), ix.filter_named(b, kind)) for a, b in zip(out, want))
    out = g.Image.bilateral_filter_pyramid(levels, 2, 0.2, 1.5)
    for a, b in zip(out, want):
        ref, bound = ix.bilateral(b, 2, 0.2, 1.5), ix.bilateral_bound(b, 2)
        assert (np.abs(host(a) - ref) <= bound).all()


# ---------------------------------------------------------------- bilateral
RATIOS = {}


@functools.lru_cache(maxsize=None)
def bilateral_case(case, d, sigma_color, sigma_space):
    """(the image, the float64 reference, the bound) of one of BILATERAL_CASES: computed once, shared, never written"""
    src = ix.bilateral_image(*case)
    return src, ix.bilateral(src, d, sigma_color, sigma_space), ix.bilateral_bound(src, d)


def check_bilateral(got, src, d, sigma_color, sigma_space, key, ref=None, bound=None):
    if ref is None:
        ref, bound = ix.bilateral(src, d, sigma_color, sigma_space), ix.bilateral_bound(src, d)
    assert got.dtype == F and got.shape == src.shape
    assert (np.isnan(got) == np.isnan(ref)).all()
    ok = np.isfinite(ref) & np.isfinite(bound)
    if ok.any():
        ratio = float((np.abs(got.astype(np.float64) - ref)[ok] / bound[ok]).max())
        RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
        print("bilateral |got - ref| / bound: %.4f (%s; largest so far %.4f)" % (ratio, key, RATIOS[key]))
        assert ratio <= 1.0
    return int(ok.sum())


@pytest.mark.parametrize("side", SIDES)
def test_bilateral_diameter_zero_is_the_input(side):
    for w, h, seed, special in BILATERAL_CASES:
        src = ix.bilateral_image(w, h, seed, special)
        got = host(img(src, side).bilateral_filter(0, 0.5, 3.0))     # one tap of weight (1 * 1) * exp(-0): cur / 1
        want = src.copy()
        want[np.isinf(src)] = np.nan                                   # the contract's c = inf - inf
        assert ix.same_words(got, want), special


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("d", [1, 5, 31])
@pytest.mark.parametrize("case", BILATERAL_CASES, ids=["40x30-nan", "37x23-inf", "37x23"])
def test_bilateral(case, d, side):
    from cupoch_amd import geometry as g
    special = case[3]
    compared = 0
    for sigma_color, sigma_space in BILATERAL_SIGMAS:
        src, ref, bound = bilateral_case(case, d, sigma_color, sigma_space)
        got = host(img(src, side).bilateral_filter(d, sigma_color, sigma_space))
        compared += check_bilateral(got, src, d, sigma_color, sigma_space, "hardware", ref, bound)
        if side == "cuda":                                     # the exponential that was not kept, same bound
            other = g.get_engine().image_bilateral(put(src, "cuda"), d, sigma_color, sigma_space, exp_kind=0)
            check_bilateral(other.cpu().numpy(), src, d, sigma_color, sigma_space, "expf", ref, bound)
            same = g.get_engine().image_bilateral(put(src, "cuda"), d, sigma_color, sigma_space, exp_kind=1)
            assert ix.same_words(same.cpu().numpy(), got)
    assert compared > 0 or (special and d == 31)


def test_bilateral_many_workgroups():
    src = ix.bilateral_image(640, 480, 14)
    got = host(img(src, "cuda").bilateral_filter(2, 0.5, 3.0))
    assert check_bilateral(got, src, 2, 0.5, 3.0, "hardware") == 640 * 480


# ---------------------------------------------------------------- conversions
def conversion_sources():
    rng = np.random.default_rng(21)
    h, w = 23, 37
    f1 = (rng.random((h, w)) * 1.5 - 0.2).astype(F)          # below 0 and above 1: gray saturates both ways
    f1.reshape(-1)[[3, 50, 90]] = (np.nan, np.inf, -np.inf)
    f3 = (rng.random((h, w, 3)) * 1.5 - 0.2).astype(F)
    f3[2, 2] = (np.nan, 0.5, 0.5)
    f3[3, 3] = (np.inf, 0.5, 0.5)
    u16 = rng.integers(0, 65536, (h, w), dtype=np.uint16)
    u16.reshape(-1)[:3] = (0, 65535, 257)
    return {"u8x1": rng.integers(0, 256, (h, w), dtype=np.uint8), "u8x3": rng.integers(0, 256, (h, w, 3), dtype=np.uint8),
            "u16x1": u16, "u16x3": rng.integers(0, 65536, (h, w, 3), dtype=np.uint16), "f32x1": f1, "f32x3": f3}


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("name", ["u8x1", "u8x3", "u16x1", "u16x3", "f32x1", "f32x3"])
def test_create_float_and_gray(name, side):
    from cupoch_amd import geometry as g
    src = conversion_sources()[name]
    C = g.ImageColorToIntensityConversionType
    for kind, t in ((ix.EQUAL, C.Equal), (ix.WEIGHTED, C.Weighted)):
        f = img(src, side).create_float_image(t)
        assert (f.num_of_channels, f.bytes_per_channel) == (1, 4) and ix.same_words(host(f), ix.create_float(src, kind)), kind
        gray = img(src, side).create_gray_image(t)
        want = ix.create_gray(src, kind)
        assert (gray.num_of_channels, gray.bytes_per_channel) == (1, 1) and host(gray).tobytes() == want.tobytes(), kind
        if name.startswith("f32"):
            assert (want == 255).any() and (want == 0).any()
    assert ix.same_words(host(img(src, side).create_float_image()), ix.create_float(src, ix.WEIGHTED))      # the default


def test_two_and_four_channels_convert_to_zeros():
    two = np.ones((5, 7, 2), np.uint8)
    assert not host(img(two).create_float_image()).any() and host(img(two).create_float_image()).shape == (5, 7)
    assert not host(img(np.ones((5, 7, 4), F)).create_gray_image()).any()


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("scale,trunc", [(1000.0, 3.0), (999.7, 2.9), (5000.0, 4.0)])
def test_convert_depth_to_float_image(scale, trunc, side):
    s = conversion_sources()
    for name in ("u16x1", "f32x1", "u8x1"):
        src = s[name] if name != "f32x1" else (s[name] * F(4000.0)).astype(F)
        got = img(src, side).convert_depth_to_float_image(scale, trunc)
        want = ix.depth_to_float(src, scale, trunc)
        assert ix.same_words(host(got), want), name
    want = ix.depth_to_float(s["u16x1"], scale, trunc)
    assert (want == 0).sum() > 100 and (want > 0).sum() > 10


@pytest.mark.parametrize("side", SIDES)
def test_linear_transform_and_clip(side):
    s = conversion_sources()
    for name in ("u8x1", "u8x3"):
        for scale, offset in [(2.5, -200.0), (-1.0, 300.0), (float("inf"), 0.0), (1.0, 0.0)]:
            src = s[name].copy()
            src.reshape(-1)[:4] = (0, 1, 200, 255)
            image = img(src, side)
            assert image.linear_transform(scale, offset) is image
            want = ix.linear_transform(src, scale, offset)
            assert host(image).tobytes() == want.tobytes(), (name, scale, offset)
    assert ix.linear_transform(np.array([[0, 1]], np.uint8), float("inf"), 0.0).tolist() == [[0, 255]]      # 0 * inf is NaN: 0
    image = img(s["f32x1"], side)
    assert ix.same_words(host(image.linear_transform(-1.5, 0.25)), ix.linear_transform(s["f32x1"], -1.5, 0.25))
    image = img(s["f32x1"], side)
    assert image.clip_intensity(0.1, 0.9) is image and ix.same_words(host(image), ix.clip(s["f32x1"], 0.1, 0.9))
    assert ix.same_words(host(img(s["f32x1"], side).clip_intensity()), ix.clip(s["f32x1"], 0.0, 1.0))
    if side == "numpy":                                       # the in-place calls leave a host input as it was
        assert ix.same_words(s["f32x1"], conversion_sources()["f32x1"])


def test_create_image_from_float_image():
    from cupoch_amd import geometry as g
    src = conversion_sources()["f32x1"].copy()
    src.reshape(-1)[200:204] = (70000.0, 65535.0, 1234.9, -1.0)
    eng = g.get_engine()
    for size in (1, 2):
        got = eng.image_from_float(put(src, "cuda"), size).cpu().numpy()
        want = ix.from_float(src, size)
        assert got.dtype == want.dtype and got.tobytes() == want.tobytes()
        assert host(g.Image(src).create_image_from_float_image(size)).tobytes() == want.tobytes()
    assert ix.from_float(src, 2).reshape(-1)[200:204].tolist() == [65535, 65535, 1234, 0]


@pytest.mark.parametrize("fmt", [0, 1], ids=["sun", "nyu"])
def test_depth_formats_on_every_value(fmt):
    from cupoch_amd import geometry as g
    every = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    got = g.get_engine().image_depth_format(put(every, "cuda"), fmt).cpu().numpy()
    want = ix.sun(every) if fmt == 0 else ix.nyu(every)
    assert got.dtype == np.uint16 and got.tobytes() == want.tobytes()


# ---------------------------------------------------------------- byte moves
def pixels(w, h, bpp):
    rng = np.random.default_rng(bpp)
    dtype, ch = {1: (np.uint8, 1), 2: (np.uint16, 1), 3: (np.uint8, 3), 4: (F, 1), 6: (np.uint16, 3), 12: (F, 3)}[bpp]
    shape = (h, w) if ch == 1 else (h, w, ch)
    return rng.integers(0, 256, shape + (np.dtype(dtype).itemsize,), dtype=np.uint8).view(dtype).reshape(shape)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("bpp", [1, 2, 3, 4, 6, 12])
@pytest.mark.parametrize("size", [(37, 23), (65, 17)], ids=["37x23", "65x17"])
def test_transpose_and_flips(size, bpp, side):
    w, h = size
    a = pixels(w, h, bpp)
    t = img(a, side).transpose()
    assert (t.width, t.height, t.num_of_channels, t.bytes_per_channel) == (h, w, 1 if a.ndim == 2 else 3, a.dtype.itemsize)
    assert host(t).tobytes() == np.ascontiguousarray(np.swapaxes(a, 0, 1)).tobytes()
    assert host(img(a, side).flip_vertical()).tobytes() == np.ascontiguousarray(a[::-1]).tobytes()
    assert host(img(a, side).flip_horizontal()).tobytes() == np.ascontiguousarray(a[:, ::-1]).tobytes()


def test_moves_many_workgroups():
    for bpp in (4, 3):
        a = pixels(640, 480, bpp)
        assert host(img(a, "cuda").transpose()).tobytes() == np.ascontiguousarray(np.swapaxes(a, 0, 1)).tobytes()
        assert host(img(a, "cuda").flip_vertical()).tobytes() == np.ascontiguousarray(a[::-1]).tobytes()
        assert host(img(a, "cuda").flip_horizontal()).tobytes() == np.ascontiguousarray(a[:, ::-1]).tobytes()
    rgb = pixels(640, 480, 3)
    assert ix.same_words(host(img(rgb, "cuda").create_float_image()), ix.create_float(rgb))


# ---------------------------------------------------------------- RGBDImage
def frames(w=64, h=48, seed=3):
    rng = np.random.default_rng(seed)
    color = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    depth = (1200 + 6 * x + 4 * y + rng.integers(0, 8, (h, w))).astype(np.uint16)
    depth[5:9, 5:9] = 0
    depth[20:24, 30:40] = 60000
    return color, depth


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("convert", [True, False])
def test_rgbd_factories(convert, side):
    from cupoch_amd import geometry as g
    color, depth = frames()
    R = g.RGBDImage
    cases = [(lambda c, d: R.create_from_color_and_depth(c, d, convert_rgb_to_intensity=convert), dict()),
             (lambda c, d: R.create_from_color_and_depth(c, d, 999.7, 2.9, convert), dict(scale=999.7, trunc=2.9)),
             (lambda c, d: R.create_from_redwood_format(c, d, convert), dict(fmt="redwood")),
             (lambda c, d: R.create_from_tum_format(c, d, convert), dict(fmt="tum")),
             (lambda c, d: R.create_from_sun_format(c, d, convert), dict(fmt="sun")),
             (lambda c, d: R.create_from_nyu_format(c, d, convert), dict(fmt="nyu"))]
    for make, kw in cases:
        src_depth = depth
        if kw.get("fmt") == "sun":
            src_depth = ((depth << 3) | (depth >> 13)).astype(np.uint16)          # encoded so that decoding gives `depth`
            assert ix.sun(src_depth).tobytes() == depth.tobytes()
        got = make(put(color, side), put(src_depth, side))
        want_c, want_d = ix.rgbd(color, src_depth, convert_rgb_to_intensity=convert, **kw)
        assert ix.same_words(host(g.Image(got.depth)), want_d), kw
        assert ix.same_words(host(g.Image(got.color)), want_c), kw
        assert (want_d > 0).sum() > 50 or kw.get("fmt") == "nyu"
        assert got.depth.is_cuda and got.color.is_cuda and not got.is_empty()


def test_rgbd_mismatch_prints_the_references_message(capsys):
    from cupoch_amd import geometry as g
    color, depth = frames()
    assert g.RGBDImage.create_from_color_and_depth(color[:40], depth).is_empty()
    assert capsys.readouterr().out == "[cupoch_amd] Error: [CreateFromColorAndDepth] Unsupported image format.\n"
    assert g.RGBDImage.create_from_sun_format(color[:, :60], depth).is_empty()
    assert capsys.readouterr().out == "[cupoch_amd] Error: [CreateRGBDImageFromSUNFormat] Unsupported image format.\n"
    assert g.RGBDImage.create_from_nyu_format(color[:40], depth).is_empty()
    assert capsys.readouterr().out == "[cupoch_amd] Error: [CreateRGBDImageFromNYUFormat] Unsupported image format.\n"


def test_rgbd_pyramids_and_the_kinfu_chain():
    from cupoch_amd import geometry as g
    from cupoch_amd.camera import PinholeCameraIntrinsic
    color, depth = frames()
    rgbd = g.RGBDImage.create_from_color_and_depth(color, depth, 1000.0, 3.0)
    want_c, want_d = ix.rgbd(color, depth, 1000.0, 3.0)
    pyramid = rgbd.create_pyramid(3)
    cs, ds = ix.create_pyramid(want_c, 3, True), ix.create_pyramid(want_d, 3, False)
    assert len(pyramid) == 3
    for level, c, d in zip(pyramid, cs, ds):
        assert ix.same_words(host(g.Image(level.color)), c) and ix.same_words(host(g.Image(level.depth)), d)
    both = rgbd.create_pyramid(3, False, True)
    assert ix.same_words(host(g.Image(both[2].depth)), ix.create_pyramid(want_d, 3, True)[2])
    assert ix.same_words(host(g.Image(both[2].color)), ix.create_pyramid(want_c, 3, False)[2])
    for kind, name in kinds().items():
        out = g.RGBDImage.filter_pyramid(pyramid, name)
        for level, c, d in zip(out, cs, ds):
            assert ix.same_words(host(g.Image(level.color)), ix.filter_named(c, kind))
            assert ix.same_words(host(g.Image(level.depth)), ix.filter_named(d, kind))

    # KinFu's SurfaceMeasurement: pyramid, bilateral filter of the depth, a cloud per level
    smooth = g.RGBDImage.bilateral_filter_pyramid_depth(pyramid, 5, 0.1, 4.5)
    intrinsic = PinholeCameraIntrinsic(64, 48, 60.0, 60.0, 31.5, 23.5)
    for i, (level, before, d) in enumerate(zip(smooth, pyramid, ds)):
        got = host(g.Image(level.depth))
        check_bilateral(got, d, 5, 0.1, 4.5, "hardware")
        assert level.color.data_ptr() == before.color.data_ptr() or ix.same_words(host(g.Image(level.color)), cs[i])
        cloud = g.PointCloud.create_from_rgbd_image(level, intrinsic.create_pyramid_level(i))
        n = len(cloud.points)
        assert n == int((got > 0).sum()) and n > (64 >> i) * (48 >> i) // 2
