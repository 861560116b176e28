"""GPU: the five cloud-conditioning members of the C++ PointCloud (tests/cpp/test_cloud_filters.cpp), built as the other
tests/cpp programs are and held to the C ABI's results."""
import json
import os
import subprocess

import numpy as np
import pytest

import filters_exact as fx

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    from cupoch_amd.engine import Engine
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_cloud_filters")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_cloud_filters.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    pts = np.load(os.path.join(ROOT, "tests", "golden", "fragment_every3rd.npz"))["points"].astype(F32)
    n = len(pts)
    src = str(tmp_path / "points.f32")
    pts.tofile(src)
    out = subprocess.run([exe, src, str(tmp_path)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])

    def got(name):
        return np.fromfile(str(tmp_path / name), F32).reshape(-1, 3)

    eng = Engine(0)
    try:
        assert r["points"] == n and r["written"]
        assert np.array_equal(got("fps.f32"), pts[fx.fps(pts, 200)])
        assert (r["fps"], r["fps_none"], r["fps_all"], r["fps_too_many"]) == (200, 0, n, 0)
        gp, _, gc = eng.gaussian_filter(pts, 0.05, 4e-4, 50, colors=pts)
        assert got("gauss.f32").tobytes() == gp.tobytes() and got("gauss_colors.f32").tobytes() == gc.tobytes()
        assert r["gauss"] == n and r["gauss_bad"] == 0
        keep = fx.pass_through(pts, 2, 1.0, 2.0)
        assert 0 < keep.sum() < n and np.array_equal(got("pass.f32"), pts[keep]) and r["pass"] == int(keep.sum())
        assert r["pass_bad_axis"] == 0
        keep = fx.crop(pts, [0.5, 0.5, 1.0], [2.0, 2.0, 2.5])
        assert 0 < keep.sum() < n and np.array_equal(got("crop.f32"), pts[keep]) and r["crop"] == int(keep.sum())
        assert r["crop_empty_box"] == 0 and r["crop_own_box"] == n
        keep = np.ones(n, bool)
        keep[[1, n // 2, n - 1]] = False
        assert r["in_place"] and np.array_equal(got("finite.f32"), pts[keep])
        assert r["nan_only"] == n - 1 and r["neither"] == n - 1
    finally:
        eng.close()
    for msg in ("[FarthestPointDownSample] Illegal number of samples", "[GaussianFilter] Illegal input parameters",
                "[PassThroughFilter] Illegal input parameters", "[CropPointCloud] AxisAlignedBoundingBox either has zeros size"):
        assert msg in out.stderr, msg
