"""GPU: imageproc::SemiGlobalMatching and PointCloud::CreateFromDisparity through the C++ surface
(tests/cpp/test_sgm.cpp), built as the other tests/cpp programs are.  This test writes the images and the bytes the
numpy restatement (tests/sgm_exact.py) gives for them; the program compares its results with those on the bytes, checks
the option's enums and defaults and the error paths, and writes its results back, which are compared here once more."""
import json
import os
import subprocess

import numpy as np
import pytest

import sgm_exact as sx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 130, 40
CAMERA = (517.3, 531.9, 64.6, 19.3, 61.25, 0.0754)      # fx, fy, cx, cy, cx_right, baseline: as tests/cpp/test_sgm.cpp


def frame(tmp_path):
    """writes the inputs and the expected bytes; -> (disparity, points, colours) as the restatement has them"""
    left, right, _ = sx.pair(W, H, 3)
    color = np.random.default_rng(9).integers(0, 65536, (H, W, 3)).astype(np.uint16)
    disp = sx.sgm(left, right)
    points, colors = sx.points_from_disparity(disp, color, *CAMERA)
    for name, a in (("left.u8", left), ("right.u8", right), ("color.u16", color), ("want_disp.u8", disp),
                    ("want_points.f32", points), ("want_colors.f32", colors)):
        np.ascontiguousarray(a).tofile(str(tmp_path / name))
    return left, right, color, disp, points, colors


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_sgm")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_sgm.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    _, _, _, disp, points, colors = frame(tmp_path)
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["failed"] == 0
    for msg in ("[SemiGlobalMatching::ProcessFrame] Invalid SGM parameters.", "[SemiGlobalMatching::ProcessFrame] Unsupport image type.",
                "[PointCloud::CreateFromDisparity] Unsupported image format."):
        assert "[cupoch_amd] Error: " + msg in out.stderr, msg
    assert np.fromfile(str(tmp_path / "disp.bin"), np.uint8).tobytes() == disp.tobytes()
    assert (disp != 255).mean() > 0.8                                       # a matched frame, not a blank one
    assert sx.same_words(np.fromfile(str(tmp_path / "points.bin"), np.float32).reshape(-1, 3), points)
    assert sx.same_words(np.fromfile(str(tmp_path / "colors.bin"), np.float32).reshape(-1, 3), colors)
