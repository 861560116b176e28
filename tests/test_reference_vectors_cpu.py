"""The numpy restatements held to the reference's own test vectors, without a GPU.

tests/golden/reference_tests.json (oracle/make_golden.py) records, for every case of the reference's
src/tests/geometry/image.cpp, pointcloud.cpp and lineset.cpp whose operation is built here, the input the test builds and
the literal values it expects.  image.cpp compares BYTES (ExpectEQ(host_vector<uint8_t>), unit_test.cpp:47-58: EXPECT_EQ
per byte), so tests/image_exact.py must give those bytes: that is what pins the fused multiply-adds of the filters and of
the three-channel intensity and the reciprocal of the depth scale (include/mi_icp.h "image").  The GPU side of the same
vectors is tests/test_gpu_reference_vectors.py; the kernels are compared with image_exact everywhere else.

`reference_cases` in the same file is the ledger: one status for every TEST(suite, case) of the reference."""
import fractions
import glob
import math
import os
import re

import numpy as np
import pytest

import image_exact as ie
from conftest import ROOT

F = np.float32

IMAGE_VALUE_KEYS = tuple("image_" + c for c in (
    "CreateFloatImage_1_1", "CreateFloatImage_1_2", "CreateFloatImage_1_4", "CreateFloatImage_3_1_Weighted",
    "CreateFloatImage_3_1_Equal", "CreateFloatImage_3_2_Weighted", "CreateFloatImage_3_2_Equal", "CreateFloatImage_3_4_Weighted",
    "CreateFloatImage_3_4_Equal", "ConvertDepthToFloatImage", "TransposeUint8", "TransposeFloat", "FlipVerticalImage",
    "FlipHorizontalImage", "Filter_Gaussian3", "Filter_Gaussian5", "Filter_Gaussian7", "Filter_Sobel3Dx", "Filter_Sobel3Dy",
    "FilterHorizontal", "Downsample"))
IMAGE_SHAPE_KEYS = ("image_DefaultConstructor", "image_CreateImage", "image_Clear")
CLOUD_KEYS = ("pointcloud_get_min_bound", "pointcloud_get_max_bound", "pointcloud_select_by_index", "pointcloud_select_by_mask",
              "pointcloud_uniform_down_sample", "pointcloud_crop", "pointcloud_constuctor", "pointcloud_clear", "pointcloud_is_empty",
              "pointcloud_has_points", "pointcloud_has_normals", "pointcloud_has_colors", "lineset_constructor", "lineset_clear")
GOLDEN_KEYS = IMAGE_VALUE_KEYS + IMAGE_SHAPE_KEYS + CLOUD_KEYS      # the keys this module consumes

_DTYPES = {1: np.uint8, 2: np.uint16, 4: np.float32}
_FILTERS = {"Gaussian3": ie.GAUSSIAN3, "Gaussian5": ie.GAUSSIAN5, "Gaussian7": ie.GAUSSIAN7, "Sobel3Dx": ie.SOBEL3DX,
            "Sobel3Dy": ie.SOBEL3DY}


def image_input(e):
    """the recorded input bytes as the [H, W] or [H, W, C] array the test's Prepare + SetData hold"""
    a = np.frombuffer(bytes(e["input"]), _DTYPES[e["bytes_per_channel"]])
    shape = (e["height"], e["width"]) + ((e["channels"],) if e["channels"] > 1 else ())
    return np.ascontiguousarray(a.reshape(shape))


def image_restated(e):
    """the recorded call through tests/image_exact.py (the moves: the numpy one-liner test_gpu_image.py compares with)"""
    a = image_input(e)
    if e.get("pre") == "create_float_image":
        a = ie.create_float(a)
    call = e["call"]
    if call == "create_float_image":
        return ie.create_float(a)                  # the helper calls CreateFloatImage() with the default type
    if call == "convert_depth_to_float_image":
        return ie.depth_to_float(a, e["args"]["depth_scale"], e["args"]["depth_trunc"])
    if call == "filter":
        return ie.filter_named(a, _FILTERS[e["args"]["filter_type"]])
    if call == "filter_horizontal":
        return ie.filter_horizontal(a, e["args"]["kernel"])
    if call == "downsample":
        return ie.downsample(a)
    return {"transpose": lambda: np.ascontiguousarray(np.swapaxes(a, 0, 1)), "flip_vertical": lambda: np.ascontiguousarray(a[::-1]),
            "flip_horizontal": lambda: np.ascontiguousarray(a[:, ::-1])}[call]()


def image_compare(e, out):
    """as the reference's test compares: the four dimensions, then the bytes (or, TransposeFloat, floats under 1e-4)"""
    out = np.asarray(out)
    channels = out.shape[2] if out.ndim == 3 else 1
    assert (out.shape[1], out.shape[0], channels, out.dtype.itemsize) == \
        (e["ref_width"], e["ref_height"], e["ref_channels"], e["ref_bytes_per_channel"])
    if "ref_bytes" in e:
        got, ref = np.frombuffer(out.tobytes(), np.uint8), np.array(e["ref_bytes"], np.uint8)
        assert got.size == ref.size
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, "%d bytes (%d words) differ from %s" % (bad.size, np.unique(bad // 4).size, e["cite"])
    else:
        assert out.dtype == F and np.abs(out.reshape(-1).astype(np.float64) - np.array(e["ref_floats"])).max() <= e["tol"]


@pytest.mark.parametrize("key", IMAGE_VALUE_KEYS)
def test_image_restatement_gives_the_reference_bytes(golden, key):
    e = golden[key]
    assert e["cite"].startswith("src/tests/geometry/image.cpp:")
    image_compare(e, image_restated(e))


def test_equal_cases_hold_the_weighted_vectors(golden):
    """TEST_CreateFloatImage ignores its `type`: the _Equal vectors are the Weighted ones, recorded as written"""
    for c in ("3_1", "3_2", "3_4"):
        w, q = golden["image_CreateFloatImage_%s_Weighted" % c], golden["image_CreateFloatImage_%s_Equal" % c]
        assert w["ref_bytes"] == q["ref_bytes"] and w["input"] == q["input"]
        assert ie.create_float(image_input(q), ie.EQUAL).tobytes() != bytes(q["ref_bytes"])    # (the Equal weights differ)


def shape_state(width, height, channels, bpc):
    """what the reference's test reads from an Image of these dimensions (image.h)"""
    return {"width": width, "height": height, "num_of_channels": channels, "bytes_per_channel": bpc,
            "data_size": width * height * channels * bpc, "is_empty": width * height * channels * bpc == 0,
            "min_bound": [0.0, 0.0], "max_bound": [float(width), float(height)],
            "test_image_boundary_0_0": 0 < width and 0 < height, "bytes_per_line": width * channels * bpc}


@pytest.mark.parametrize("key", IMAGE_SHAPE_KEYS)
def test_image_shape_cases(golden, key):
    e = golden[key]
    dims = (0, 0, 0, 0) if e["prepare"] is None or e["clear"] else tuple(e["prepare"])
    assert shape_state(*dims) == e["expect"]


# ---- the point cloud and line set cases: the numpy one-liners the GPU tests of these operations compare with
def _near(a, b, tol):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and (a.size == 0 or np.abs(a - b).max() <= tol)


def _lex(p):
    p = np.asarray(p, F).reshape(-1, 3)
    return p[np.lexsort((p[:, 2], p[:, 1], p[:, 0]))]


def bounds_of(points):
    """GetMinBound / GetMaxBound: the coordinate-wise extremes, zeros for an empty set"""
    p = np.asarray(points, F).reshape(-1, 3)
    return (np.zeros(3, F), np.zeros(3, F)) if len(p) == 0 else (p.min(0), p.max(0))


def test_pointcloud_bounds(golden):
    for key, which in (("pointcloud_get_min_bound", 0), ("pointcloud_get_max_bound", 1)):
        g = golden[key]
        assert _near(bounds_of(g["points"])[which], g["ref"], g["tol"]), key      # ExpectEQ, THRESHOLD_1E_4 (unit_test.h:40)


def test_pointcloud_selections(golden):
    g = golden["pointcloud_select_by_index"]
    pts = np.array(g["points"], F)
    assert _near(_lex(pts[g["indices"]]), _lex(g["ref_points"]), g["tol"])
    g = golden["pointcloud_select_by_mask"]
    mask = np.zeros(len(pts), bool)
    mask[g["indices"]] = True
    assert _near(_lex(np.array(g["points"], F)[mask]), _lex(g["ref_points"]), g["tol"])
    g = golden["pointcloud_uniform_down_sample"]
    assert _near(np.array(g["points"], F)[::g["every_k_points"]], g["ref_points"], g["tol"])
    g = golden["pointcloud_crop"]
    pts, lo, hi = np.array(g["points"], F), np.array(g["min_bound"], F), np.array(g["max_bound"], F)
    kept = pts[((pts >= lo) & (pts <= hi)).all(1)]
    assert 0 < len(kept) < len(pts) and (kept >= lo).all() and (kept <= hi).all()     # ExpectLE / ExpectGE


def test_container_cases(golden):
    for key in ("pointcloud_constuctor", "lineset_constructor"):
        g = golden[key]
        assert g["dimension"] == 3 and g["expect"]["is_empty"] and not g["expect"]["has_points"]
        assert _near(bounds_of([])[0], g["expect"]["min_bound"], g["tol"]) and _near(bounds_of([])[1], g["expect"]["max_bound"], g["tol"])
    for key in ("pointcloud_clear", "lineset_clear"):
        g = golden[key]
        lo, hi = bounds_of(g["points"])
        assert _near(lo, g["expect_set"]["min_bound"], g["tol"]) and _near(hi, g["expect_set"]["max_bound"], g["tol"])
        assert not g["expect_set"]["is_empty"] and g["expect_cleared"]["is_empty"]
        assert g["expect_cleared"]["min_bound"] == [0, 0, 0] and g["expect_cleared"]["max_bound"] == [0, 0, 0]
    lines = np.array(golden["lineset_clear"]["lines"])
    assert lines.shape == (100, 2) and lines.min() >= 0 and lines.max() <= 1000
    g = golden["pointcloud_is_empty"]
    assert g["expect_before"] is True and g["expect_after"] is False and len(g["points"]) == 100
    for what in ("points", "normals", "colors"):
        g = golden["pointcloud_has_" + what]
        assert g["flag"] == "has_" + what and what in g["set"] and g["expect_before"] is False and g["expect_after"] is True


# ---- fma32: the exact fused multiply-add the restatement stands on
def _round_f32(q):
    """a Fraction rounded to the nearest float32, ties to even (no overflow handling: the operands stay far from it)"""
    if q == 0:
        return F(0.0)
    sign, q = (-1.0 if q < 0 else 1.0), abs(q)
    e = max(math.floor(math.log2(q)) - 23, -149)
    while q / fractions.Fraction(2) ** e >= 2 ** 24:
        e += 1
    while e > -149 and q / fractions.Fraction(2) ** e < 2 ** 23:
        e -= 1
    n = round(q / fractions.Fraction(2) ** e)        # Fraction.__round__: exact, ties to even
    return F(sign * math.ldexp(float(n), e))


def _fma_exact(a, b, c):
    return _round_f32(fractions.Fraction(float(a)) * fractions.Fraction(float(b)) + fractions.Fraction(float(c)))


def test_fma32_is_the_exact_fused_multiply_add():
    rng = np.random.default_rng(5)
    n = 4000
    a = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F)
    b = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F)
    c = (rng.standard_normal(n) * 2.0 ** rng.integers(-20, 20, n)).astype(F)
    c[::3] = (-(a[::3].astype(np.float64) * b[::3]) * (1 + rng.integers(-3, 4, len(a[::3])) * 2.0 ** -24)).astype(F)   # cancellation
    c[1::7] = 0.0
    a[5::11] = (a[5::11] * F(2.0 ** -100)).astype(F)                                                        # subnormal results
    c[5::11] = (c[5::11] * F(2.0 ** -120)).astype(F)
    got = ie.fma32(a, b, c)
    want = np.array([_fma_exact(x, y, z) for x, y, z in zip(a, b, c)], F)
    assert got.dtype == F and got.tobytes() == want.tobytes()
    # constructed ties.  (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 lies halfway between two float32: ties to even
    t = F(1.0) + F(2.0 ** -12)
    assert ie.fma32(t, t, F(0.0)) == _fma_exact(t, t, 0.0) == F(1.0) + F(2.0 ** -11)
    # 64 - 2^-40 added to 2^30 + 128 lies just below a float32 tie; rounding the sum to float64 first lands on the tie and
    # then goes the other way, which is why fma32 does not do that
    x, y, z = F(8.0) * (F(1.0) + F(2.0 ** -23)), F(8.0) * (F(1.0) - F(2.0 ** -23)), F(2.0 ** 30 + 128)
    for s in (1.0, -1.0):
        exact = _fma_exact(F(s) * x, y, F(s) * z)
        assert exact == F(s * (2.0 ** 30 + 128)) and ie.fma32(F(s) * x, y, F(s) * z) == exact
        assert F(np.float64(F(s) * x) * np.float64(y) + np.float64(F(s) * z)) != exact
    # the special values pass through as fmaf's
    assert np.isnan(ie.fma32(F(np.inf), F(0.0), F(1.0))) and ie.fma32(F(np.inf), F(1.0), F(1.0)) == F(np.inf)
    assert np.isnan(ie.fma32(F(np.nan), F(1.0), F(1.0))) and ie.fma32(F(3.0), F(0.5), F(-np.inf)) == F(-np.inf)
    assert ie.fma32(np.array([[1, 2], [3, 4]], F), F(0.5), np.array([1, 1], F)).tolist() == [[1.5, 2.0], [2.5, 3.0]]


# ---- the ledger
def _modules():
    return sorted(glob.glob(os.path.join(ROOT, "tests", "*.py")))


def test_ledger_gives_every_reference_case_one_status(golden):
    cases = golden["reference_cases"]
    assert len(cases) == 103 and all(re.fullmatch(r"\w+\.\w+", n) for n in cases)
    keys = set(golden) - {"reference_cases"}
    for name, status in cases.items():
        kinds = [status.startswith(p) for p in ("golden:", "ported:", "not built: ")]
        assert sum(kinds) == 1, (name, status)
        if kinds[0]:
            assert status[len("golden:"):] in keys, (name, status)
        elif kinds[1]:
            path = os.path.join(ROOT, status[len("ported:"):])
            assert os.path.isfile(path), (name, status)
            src_file = _REFERENCE_FILE[name.split(".")[0]] if name.split(".")[0] in _REFERENCE_FILE else _REFERENCE_FILE[name]
            assert src_file in open(path).read(), "%s does not cite %s" % (status, src_file)
        else:
            assert len(status) > len("not built: ")
    for name in ("TriangleMesh.Constructor", "Feature.ComputeFPFHFeature", "PointCloud.GetOrientedBoundingBox"):
        assert cases[name].startswith("not built: ")
    assert {n for n, s in cases.items() if n.startswith("Image.") and not s.startswith("golden:")} == \
        {"Image.FloatValueAt", "Image.CreateDepthToCameraDistanceMultiplierFloatImage"}


# the reference file a ported suite (or case) comes from: what the porting file must cite
_REFERENCE_FILE = {
    "Collision": "tests/collision/collision.cpp", "Graph": "tests/geometry/graph.cpp", "SimplePlanner": "tests/planning/planner.cpp",
    "VoxelGrid": "tests/geometry/voxelgrid.cpp", "OccupancyGrid": "tests/geometry/occupancygrid.cpp",
    "DistanceTransform": "tests/geometry/distancetransform.cpp", "LaserScanBuffer": "tests/geometry/laserscanbuffer.cpp",
    "UniformTSDFVolume": "tests/integration/uniform_fsdfvolume.cpp", "PointCloud.SegmentPlaneKnownPlane": "tests/geometry/pointcloud.cpp",
    "PointCloud.RemoveRadiusOutliers": "tests/geometry/pointcloud.cpp",
    "PointCloud.CreatePointCloudFromFile": "tests/io/class_io/pointcloud_io.cpp",
}


def test_every_golden_key_is_consumed_by_a_test_module(golden):
    """a module consumes a key by naming it: in its GOLDEN_KEYS, or as golden["key"] / a parametrised name"""
    import test_gpu_reference_vectors as gpu_side
    assert set(gpu_side.GOLDEN_KEYS) == set(GOLDEN_KEYS)                 # the GPU file replays every case this one holds
    named = set(GOLDEN_KEYS)
    for path in _modules():
        if os.path.basename(path) not in ("test_reference_vectors_cpu.py", "test_gpu_reference_vectors.py"):
            named |= set(re.findall(r"\"(\w+)\"", open(path).read()))
    keys = set(golden) - {"reference_cases"}
    assert keys <= named, sorted(keys - named)
    assert set(GOLDEN_KEYS) <= keys
    used = {s[len("golden:"):] for s in golden["reference_cases"].values() if s.startswith("golden:")}
    assert used == keys, sorted(used ^ keys)                             # no vector without a reference case, and none unused
