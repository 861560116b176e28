"""geometry.Image / geometry.RGBDImage without a GPU: the numpy restatement of the image contract (tests/image_exact.py)
against independent yardsticks (the odometry oracle's filter and downsample, the literal four-step filter), the Python
surface's names and defaults, the errors that are turned away before any device is touched, and the negative controls of
the bilateral bound: the two mistakes the bound exists for lie far outside it on the very images the GPU test uses."""
import inspect

import numpy as np
import pytest

import image_exact as ix
from oracle import oracle as orc

F = np.float32
BILATERAL_CASES = [(40, 30, 11, "nan"), (37, 23, 12, "inf"), (37, 23, 13, None)]   # (width, height, seed, special): tests/test_gpu_image.py
BILATERAL_SIGMAS = (2.0, 2.0)       # sigma_color, sigma_space of the controls; the GPU test runs these and two more pairs


@pytest.fixture(scope="module")
def img():
    a = ix.float_image(37, 23)
    assert np.isnan(a).sum() == 1 and np.isinf(a).sum() == 2
    return a


def test_three_tap_filters_are_the_oracles(img):
    for oracle_kind, kind in enumerate((ix.GAUSSIAN3, ix.SOBEL3DX, ix.SOBEL3DY)):
        got = ix.filter_named(img, kind)
        assert ix.same_words(got, orc.od_filter(img, oracle_kind)), kind
        assert np.isnan(got).sum() >= 9             # the special pixels spread over their 3 x 3 neighbourhoods


def test_float_downsample_is_the_oracles(img):
    got = ix.downsample(img)
    assert got.shape == (11, 18) and ix.same_words(got, orc.od_downsample(img))


@pytest.mark.parametrize("kind", sorted(ix.NAMED))
def test_one_pass_filter_equals_the_four_steps(img, kind):
    dx, dy = ix.NAMED[kind]
    assert ix.same_words(ix.filter_taps(img, dx, dy), ix.filter_literal(img, dx, dy))
    clean = ix.float_image(65, 17, specials=False)
    assert ix.same_words(ix.filter_taps(clean, dx, dy), ix.filter_literal(clean, dx, dy))


def test_fused_level_is_downsample_of_filter(img):
    assert ix.same_words(ix.pyramid_level(img), orc.od_downsample(orc.od_filter(img, 0)))
    sizes = [(p.shape[1], p.shape[0]) if p.size else (0, 0) for p in ix.create_pyramid(img, 7, True)]
    assert sizes == [(37, 23), (18, 11), (9, 5), (4, 2), (2, 1), (0, 0), (0, 0)]


def test_conversions_saturate_and_truncate():
    assert ix.sat(np.array([-3.5, np.nan, 0.99, 254.99, 255.0, 1e9, np.inf, -np.inf], F), 255).tolist() == [0, 0, 0, 254, 255, 255, 255, 0]
    assert ix.sun(np.array([0x0008, 0x0007, 0xffff], np.uint16)).tolist() == [0x0001, 0xe000, 0xffff]
    n = ix.nyu(np.array([0, 0x4404, 0xffff], np.uint16))        # bytes swapped: 0, 0x0444 = 1092, 0xffff
    assert n.tolist() == [int(np.floor(float(F(351.3 / 1092.5)) * 1000 + 0.5)), 65535, 0]
    assert ix.clip(np.array([np.nan, -1, 0.5, 2], F), 0, 1).tolist() == [1.0, 0.0, 0.5, 1.0]


def test_python_surface_names_and_defaults():
    from cupoch_amd import geometry as g
    T, C = g.ImageFilterType, g.ImageColorToIntensityConversionType
    assert [int(T.Gaussian3), int(T.Gaussian5), int(T.Gaussian7), int(T.Sobel3dx), int(T.Sobel3dy)] == [0, 1, 2, 3, 4]
    assert (int(C.Equal), int(C.Weighted)) == (0, 1) and C.Gaussian3 is C.Equal and C.Gaussian5 is C.Weighted

    def defaults(fn):
        return {k: v.default for k, v in inspect.signature(fn).parameters.items() if v.default is not inspect.Parameter.empty}
    I, R = g.Image, g.RGBDImage
    assert defaults(I.clip_intensity) == {"min": 0.0, "max": 1.0}
    assert defaults(I.linear_transform) == {"scale": 1.0, "offset": 0.0}
    assert defaults(I.create_gray_image) == {"type": C.Weighted} and defaults(I.create_float_image) == {"type": C.Weighted}
    assert defaults(I.convert_depth_to_float_image) == {"depth_scale": 1000.0, "depth_trunc": 3.0}
    assert list(inspect.signature(I.create_pyramid).parameters) == ["self", "num_of_levels", "with_gaussian_filter"]
    assert list(inspect.signature(I.bilateral_filter).parameters) == ["self", "diameter", "sigma_color", "sigma_space"]
    assert list(inspect.signature(I.filter_pyramid).parameters) == ["image_pyramid", "filter_type"]
    assert list(inspect.signature(I.bilateral_filter_pyramid).parameters) == ["image_pyramid", "diameter", "sigma_color", "sigma_space"]
    for name in ("downsample", "filter", "flip_vertical", "flip_horizontal", "transpose", "is_empty"):
        assert callable(getattr(I, name)), name
    d = defaults(R.create_from_color_and_depth)
    assert (d["depth_scale"], d["depth_trunc"], d["convert_rgb_to_intensity"]) == (1000.0, 3.0, True)
    for name in ("create_from_redwood_format", "create_from_tum_format", "create_from_sun_format", "create_from_nyu_format"):
        assert defaults(getattr(R, name)) == {"convert_rgb_to_intensity": True}, name
    assert defaults(R.create_pyramid) == {"with_gaussian_filter_for_color": True, "with_gaussian_filter_for_depth": False}
    assert list(inspect.signature(R.bilateral_filter_pyramid_depth).parameters) == ["rgbd_image_pyramid", "diameter", "sigma_depth", "sigma_space"]
    assert list(inspect.signature(R.filter_pyramid).parameters) == ["rgbd_image_pyramid", "filter_type"]

    a = I(np.zeros((5, 7, 3), np.uint8))
    assert (a.width, a.height, a.num_of_channels, a.bytes_per_channel, a.is_empty()) == (7, 5, 3, 1, False)
    assert repr(a) == "Image of size 7x5, with 3 channels." and np.asarray(a).shape == (5, 7, 3)
    e = I()
    assert (e.width, e.height, e.num_of_channels, e.bytes_per_channel, e.is_empty()) == (0, 0, 0, 0, True)
    assert I(np.zeros((4, 6), np.uint16)).bytes_per_channel == 2 and I(np.zeros((4, 6), F)).test_image_boundary(5.5, 3.5)
    assert not I(np.zeros((4, 6), F)).test_image_boundary(5.5, 3.5, 1.0)
    assert "Color image : 7x5, with 3 channels." in repr(R(a, np.zeros((5, 7), F)))


def test_errors_that_need_no_device(capsys):
    from cupoch_amd import geometry as g
    f = g.Image(np.ones((6, 8), F))
    rgb = g.Image(np.ones((6, 8, 3), np.uint8))
    assert f.filter_taps([1, 2], [1, 2, 1]).is_empty() and f.filter_horizontal([0.5, 0.5]).is_empty()
    assert f.filter_taps([1.0] * 33, [1.0]).is_empty()
    assert capsys.readouterr().out.count("[cupoch_amd] Error: [FilterHorizontal] Unsupported image format or kernel size.") == 3
    assert f.bilateral_filter(32, 0.1, 2.0).is_empty() and f.bilateral_filter(-1, 0.1, 2.0).is_empty()
    assert capsys.readouterr().out.count("[cupoch_amd] Error: [BilateralFilter] Diameter should be in [0, 31].") == 2
    assert rgb.filter_taps([.25, .5, .25], [.25, .5, .25]).is_empty()
    assert capsys.readouterr().out == "[cupoch_amd] Error: [Filter] Unsupported image format.\n"
    u16 = g.Image(np.ones((6, 8), np.uint16))
    assert rgb.clip_intensity() is rgb and u16.linear_transform(2.0) is u16
    out = capsys.readouterr().out
    assert "[cupoch_amd] Error: [ClipIntensity] Unsupported image format." in out
    assert "[cupoch_amd] Error: [LinearTransform] Unsupported image format." in out
    assert g.Image(np.ones((6, 8), np.uint16)).downsample().is_empty()
    assert "[cupoch_amd] Error: [Downsample] Unsupported image format." in capsys.readouterr().out
    assert g.RGBDImage.create_from_color_and_depth(rgb, np.ones((5, 8), np.uint16)).is_empty()
    assert capsys.readouterr().out == "[cupoch_amd] Error: [CreateFromColorAndDepth] Unsupported image format.\n"
    assert g.Image().create_float_image().is_empty() and g.Image().flip_vertical().is_empty() and capsys.readouterr().out == ""


@pytest.mark.parametrize("w,h,seed,special", BILATERAL_CASES)
@pytest.mark.parametrize("d", [1, 5, 31])
def test_bilateral_bound_sees_a_wrong_clamp_and_a_wrong_table_index(w, h, seed, special, d):
    """The reference's clamp to h and w (one past the end; here on the image padded with a zero row and column) and a
    spatial table shifted by one entry each move some pixel by more than 100 bounds.  The bound grows with the window
    (T = 3969 taps at diameter 31: 9.5e-4 M), so what it can see there depends on the sigmas: with (2.0, 2.0) the two
    mistakes reach 415 and 114 bounds at diameter 31 and thousands below; with (0.5, 3.0), which the GPU test also
    runs, they reach 33 and 7 at diameter 31 (1700 and 220 at diameter 5) -- that pair is no control for diameter 31."""
    src = ix.bilateral_image(w, h, seed, special)
    ref = ix.bilateral(src, d, *BILATERAL_SIGMAS)
    bound = ix.bilateral_bound(src, d)
    ok = np.isfinite(ref) & np.isfinite(bound)
    if special and d == 31:             # the special pixel is in every window: nothing but the NaN mask to compare
        assert ok.sum() == 0
        return
    assert ok.sum() > w * h // 3
    for wrong in (ix.bilateral(src, d, *BILATERAL_SIGMAS, past_end=True), ix.bilateral(src, d, *BILATERAL_SIGMAS, table_shift=1)):
        both = ok & np.isfinite(wrong)
        assert (np.abs(wrong - ref)[both] / bound[both]).max() > 100.0
