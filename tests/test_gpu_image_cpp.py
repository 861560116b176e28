"""GPU: geometry::Image / geometry::RGBDImage through the C++ surface (tests/cpp/test_image.cpp: every method, Transpose,
FilterHorizontal, Filter(dx, dy), CreateImageFromFloatImage and the RGBDImage statics included), built as the other
tests/cpp programs are.  The program writes every result's bytes; they are held to the numpy restatement of the
contract (tests/image_exact.py): bit for bit, the bilateral results under the bound of tests/test_gpu_image.py.  Three of
the reference's own 5 x 5 cases (tests/golden/reference_tests.json) go through the same run and are held to its bytes."""
import json
import os
import subprocess

import numpy as np
import pytest

import image_exact as ix

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = {1: np.uint8, 2: np.uint16, 4: F}


def test_cpp_surface(tmp_path, golden):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_image")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_image.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(41)
    gray = ix.float_image(37, 23)
    color = rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)
    y, x = np.mgrid[0:48, 0:64]
    depth = (900 + 40 * x + 25 * y + rng.integers(0, 8, (48, 64))).astype(np.uint16)
    depth[4:8, 4:8] = 0
    gray.tofile(str(tmp_path / "gray.f32"))
    color.tofile(str(tmp_path / "color.u8"))
    depth.tofile(str(tmp_path / "depth.u16"))
    reference = {"ref_gaussian7": ("ref_f32.u8", golden["image_Filter_Gaussian7"]),
                 "ref_float_3_1": ("ref_rgb.u8", golden["image_CreateFloatImage_3_1_Weighted"]),
                 "ref_depth_float": ("ref_depth.u8", golden["image_ConvertDepthToFloatImage"])}
    for file, e in reference.values():
        np.array(e["input"], np.uint8).tofile(str(tmp_path / file))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["failed"] == 0
    for msg in ("[Filter] Unsupported image format.", "[FilterHorizontal] Unsupported image format or kernel size.",
                "[BilateralFilter] Diameter should be in [0, 31].", "[BilateralFilter] Unsupported image format.",
                "[Downsample] Unsupported image format.", "[CreateImageFromFloatImage] Unsupported image format.",
                "[CreateImagePyramid] Unsupported image format.", "[CreateFromColorAndDepth] Unsupported image format.",
                "[CreateRGBDImageFromSUNFormat] Unsupported image format.", "[ClipIntensity] Unsupported image format."):
        assert "[cupoch_amd] Error: " + msg in out.stderr, msg

    def got(name):
        w, h, ch, size = r["images"][name]
        a = np.fromfile(str(tmp_path / (name + ".bin")), DTYPES[size])
        return a.reshape((h, w) if ch == 1 else (h, w, ch))

    def same(name, want):
        assert ix.same_words(got(name), np.ascontiguousarray(want)), name

    def within(name, src, d, sigma_color, sigma_space):
        ref, bound = ix.bilateral(src, d, sigma_color, sigma_space), ix.bilateral_bound(src, d)
        a = got(name)
        assert a.shape == ref.shape and (np.isnan(a) == np.isnan(ref)).all(), name
        ok = np.isfinite(ref) & np.isfinite(bound)
        assert ok.any() and (np.abs(a.astype(np.float64) - ref)[ok] <= bound[ok]).all(), name

    for name, (_, e) in reference.items():              # as the reference compares: the dimensions, then every byte
        assert r["images"][name] == [e["ref_width"], e["ref_height"], e["ref_channels"], e["ref_bytes_per_channel"]], name
        assert got(name).tobytes() == bytes(e["ref_bytes"]), (name, e["cite"])
    k5, k3 = [0.5, -1.25, 2.0, 0.75, -0.5], [1.0, -2.0, 0.5]
    same("transpose", gray.T)
    same("transpose_rgb", np.swapaxes(color, 0, 1))
    same("flip_v", color[::-1])
    same("flip_h", depth[:, ::-1])
    same("horizontal", ix.filter_horizontal(gray, k5))
    same("taps", ix.filter_taps(gray, k5, k3))
    for name, kind in (("gaussian3", ix.GAUSSIAN3), ("gaussian5", ix.GAUSSIAN5), ("gaussian7", ix.GAUSSIAN7),
                       ("sobel_dx", ix.SOBEL3DX), ("sobel_dy", ix.SOBEL3DY)):
        same(name, ix.filter_named(gray, kind))
    same("downsample", ix.downsample(gray))
    same("downsample_rgb", ix.downsample(color))
    within("bilateral", gray, 3, 0.5, 2.0)
    same("float_weighted", ix.create_float(color))
    same("float_equal", ix.create_float(color, ix.EQUAL))
    same("gray_weighted", ix.create_gray(color))
    same("gray_from_float", ix.create_gray(gray))
    same("depth_float", ix.depth_to_float(depth))
    same("depth_float_tum", ix.depth_to_float(depth, 5000.0, 4.0))
    same("from_float_u8", ix.from_float(gray, 1))
    same("from_float_u16", ix.from_float(ix.create_float(depth), 2))
    assert got("from_float_u16").dtype == np.uint16 and got("from_float_u16").tobytes() == depth.tobytes()
    same("clip", ix.clip(gray, 0.25, 1.5))
    same("linear_u8", ix.linear_transform(color, 1.5, -40.0))
    same("linear_f32", ix.linear_transform(gray, -2.0, 0.125))
    for i, want in enumerate(ix.create_pyramid(gray, 5, True)):
        same("pyramid%d" % i, want)
    plain = ix.create_pyramid(gray, 3, False)
    for i, want in enumerate(plain):
        same("plain%d" % i, want)
        same("plain_sobel%d" % i, ix.filter_named(want, ix.SOBEL3DX))
        within("plain_bilateral%d" % i, want, 2, 0.5, 1.5)
    want_c, want_d = ix.rgbd(color, depth)
    same("rgbd_color", want_c)
    same("rgbd_depth", want_d)
    same("rgbd_raw_color", color)
    for fmt in ("redwood", "tum", "sun", "nyu"):
        same(fmt + "_depth", ix.rgbd(color, depth, fmt=fmt)[1])
    cs, ds = ix.create_pyramid(want_c, 3, True), ix.create_pyramid(want_d, 3, False)
    for i in range(3):
        same("level_color%d" % i, cs[i])
        same("level_depth%d" % i, ds[i])
        same("level_gauss_depth%d" % i, ix.filter_named(ds[i], ix.GAUSSIAN3))
        within("level_bilateral_depth%d" % i, ds[i], 2, 0.1, 1.5)
