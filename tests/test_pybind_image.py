"""geometry.Image / geometry.RGBDImage of the reference's pybind11 module (cupoch_amd/cpp/src/pybind_module.cpp) with the
reference's Python names and defaults: names on the CPU, and on the GPU the same bytes as the ctypes mirror for a filter,
the bilateral filter, a pyramid and one factory, and the reference's own bytes for three of its 5 x 5 cases
(tests/golden/reference_tests.json).  Skips only where there is nothing to build the module with."""
import re

import numpy as np
import pytest

import image_exact as ix

F = np.float32


def module():
    import importlib.util
    import shutil
    missing = [n for n in ("make", "g++") if shutil.which(n) is None] + ([] if importlib.util.find_spec("pybind11") else ["pybind11"])
    if missing:                 # nothing to build the module with: the only reason to skip
        pytest.skip("cupoch_pybind cannot be built here: no %s" % ", ".join(missing))
    from cupoch_amd import pybind as cph        # (a build or an import that breaks is a failure)
    return cph


def test_image_rows_have_the_references_names():
    cph = module()
    I, R, G = cph.geometry.Image, cph.geometry.RGBDImage, cph.geometry
    for name in ("clip_intensity", "linear_transform", "downsample", "filter", "flip_vertical", "flip_horizontal",
                 "bilateral_filter", "create_gray_image", "create_float_image", "create_pyramid", "filter_pyramid",
                 "bilateral_filter_pyramid", "width", "height", "num_of_channels", "bytes_per_channel", "is_empty", "transpose",
                 "convert_depth_to_float_image", "__array__"):
        assert hasattr(I, name), name
    for name in ("create_from_color_and_depth", "create_from_redwood_format", "create_from_tum_format", "create_from_sun_format",
                 "create_from_nyu_format", "create_pyramid", "filter_pyramid", "bilateral_filter_pyramid_depth", "color", "depth"):
        assert hasattr(R, name), name
    T, C = G.ImageFilterType, G.ImageColorToIntensityConversionType
    assert [int(T.Gaussian3), int(T.Gaussian5), int(T.Gaussian7), int(T.Sobel3dx), int(T.Sobel3dy)] == [0, 1, 2, 3, 4]
    assert (int(C.Equal), int(C.Weighted)) == (0, 1) and C.Gaussian3 == C.Equal and C.Gaussian5 == C.Weighted
    assert G.Gaussian7 == T.Gaussian7               # exported into the module, as in the reference

    def default(fn, name, value):            # "name: <the type, as this pybind11 spells it> = value"
        return re.search(r"\b%s: [^,)]*= %s[,)]" % (name, re.escape(value)), fn.__doc__) is not None
    assert default(I.clip_intensity, "min", "0.0") and default(I.clip_intensity, "max", "1.0")
    assert default(I.linear_transform, "scale", "1.0") and default(I.linear_transform, "offset", "0.0")
    assert re.search(r"\btype: [^,)]*Weighted", I.create_gray_image.__doc__) and re.search(r"\btype: [^,)]*Weighted", I.create_float_image.__doc__)
    assert default(R.create_from_color_and_depth, "depth_scale", "1000.0") and default(R.create_from_color_and_depth, "depth_trunc", "3.0")
    for fn in (R.create_from_color_and_depth, R.create_from_redwood_format, R.create_from_tum_format, R.create_from_sun_format,
               R.create_from_nyu_format):
        assert default(fn, "convert_rgb_to_intensity", "True")
    assert default(R.create_pyramid, "with_gaussian_filter_for_color", "True") and default(R.create_pyramid, "with_gaussian_filter_for_depth", "False")
    assert "with_gaussian_filter" in I.create_pyramid.__doc__ and "sigma_space" in I.bilateral_filter.__doc__
    assert repr(I()) == "Image of size 0x0, with 0 channels." and I().is_empty()


@pytest.mark.gpu
def test_same_bytes_as_the_ctypes_mirror():
    cph = module()
    from cupoch_amd import geometry as g
    rng = np.random.default_rng(17)
    gray = ix.float_image(37, 23)
    a, b = cph.geometry.Image(gray), g.Image(gray)
    assert repr(a) == repr(b) == "Image of size 37x23, with 1 channels."
    assert ix.same_words(np.asarray(a), gray)
    for ta, tb in ((cph.geometry.ImageFilterType.Gaussian7, g.ImageFilterType.Gaussian7),
                   (cph.geometry.ImageFilterType.Sobel3dy, g.ImageFilterType.Sobel3dy)):
        assert ix.same_words(np.asarray(a.filter(ta)), np.asarray(b.filter(tb)))
    clean = ix.bilateral_image(40, 30, 11)
    fa, fb = cph.geometry.Image(clean).bilateral_filter(5, 0.5, 3.0), g.Image(clean).bilateral_filter(5, 0.5, 3.0)
    assert ix.same_words(np.asarray(fa), np.asarray(fb)) and not ix.same_words(np.asarray(fb), clean)
    pa, pb = a.create_pyramid(6, True), b.create_pyramid(6, True)
    assert [(p.width, p.height) for p in pa] == [(p.width, p.height) for p in pb] == [(37, 23), (18, 11), (9, 5), (4, 2), (2, 1), (0, 0)]
    assert all(ix.same_words(np.asarray(x), np.asarray(y)) for x, y in zip(pa[:5], pb[:5])) and pa[5].is_empty()
    sa = cph.geometry.Image.filter_pyramid(pa[:3], cph.geometry.ImageFilterType.Sobel3dx)
    assert ix.same_words(np.asarray(sa[2]), ix.filter_named(ix.create_pyramid(gray, 3, True)[2], ix.SOBEL3DX))

    color = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    depth = rng.integers(0, 9000, (48, 64)).astype(np.uint16)
    assert ix.same_words(np.asarray(cph.geometry.Image(color).filter(cph.geometry.ImageFilterType.Gaussian3)),
                         ix.filter_named(ix.create_float(color), ix.GAUSSIAN3))          # a float image first
    ra = cph.geometry.RGBDImage.create_from_tum_format(cph.geometry.Image(color), cph.geometry.Image(depth))
    rb = g.RGBDImage.create_from_tum_format(color, depth)
    want_c, want_d = ix.rgbd(color, depth, fmt="tum")
    assert ix.same_words(np.asarray(ra.depth), want_d) and ix.same_words(np.asarray(g.Image(rb.depth)), want_d)
    assert ix.same_words(np.asarray(ra.color), want_c) and ix.same_words(np.asarray(g.Image(rb.color)), want_c)
    levels = ra.create_pyramid(3)
    assert ix.same_words(np.asarray(levels[2].color), ix.create_pyramid(want_c, 3, True)[2])
    smooth = cph.geometry.RGBDImage.bilateral_filter_pyramid_depth(levels, 2, 0.1, 1.5)
    mirror = g.RGBDImage.bilateral_filter_pyramid_depth(rb.create_pyramid(3), 2, 0.1, 1.5)
    assert all(ix.same_words(np.asarray(x.depth), np.asarray(g.Image(y.depth))) for x, y in zip(smooth, mirror))
    u8 = cph.geometry.Image(color)
    assert u8.linear_transform(1.5, -40.0) is u8 and np.asarray(u8).tobytes() == ix.linear_transform(color, 1.5, -40.0).tobytes()


@pytest.mark.gpu
def test_reference_vectors_through_the_pybind_surface(golden):
    """src/tests/geometry/image.cpp: Filter_Gaussian7, CreateFloatImage_3_1_Weighted, ConvertDepthToFloatImage"""
    cph = module()
    import test_reference_vectors_cpu as rv
    I = cph.geometry.Image
    e = golden["image_Filter_Gaussian7"]
    rv.image_compare(e, np.asarray(I(rv.image_input(e)).create_float_image().filter(cph.geometry.ImageFilterType.Gaussian7)))
    e = golden["image_CreateFloatImage_3_1_Weighted"]
    rv.image_compare(e, np.asarray(I(rv.image_input(e)).create_float_image()))
    e = golden["image_ConvertDepthToFloatImage"]
    rv.image_compare(e, np.asarray(I(rv.image_input(e)).convert_depth_to_float_image()))
