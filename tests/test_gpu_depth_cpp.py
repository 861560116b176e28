"""GPU: PointCloud::CreateFromDepthImage and CreateFromRGBDImage through the C++ surface (tests/cpp/test_depth_cloud.cpp),
built as the other tests/cpp programs are.  The program makes its images from integer formulas, repeated here, and
prints the count and a 64-bit FNV-1a of every output array; both are held to the restatement (tests/depth_exact.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import depth_exact as dx

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = 70, 50
K4 = [59.5, 57.25, 34.75, 24.5]
CUTOFF = F(1.4)


def images():
    y, x = np.mgrid[0:H, 0:W]
    pix = y * W + x
    d = (900 + (7 * x + 13 * y) % 700).astype(F) / F(1000.0)
    d[pix % 11 == 0] = 0.0
    d[pix % 97 == 5] = np.inf
    d[pix % 89 == 3] = -1.0
    c = np.stack([(31 * x + 17 * y + 101 * k) % 256 for k in range(3)], -1).astype(np.uint8)
    E = np.eye(4, dtype=F)
    E[1, 1], E[1, 2], E[2, 1], E[2, 2] = 0.8, -0.6, 0.6, 0.8
    E[:3, 3] = (0.1, -0.2, 0.3)
    return d.astype(F), c, E


def fnv(a):
    """64-bit FNV-1a over the little-endian bytes of the float32 words, every NaN as 0x7fc00000"""
    if a is None:
        a = np.zeros((0, 3), F)
    w = np.ascontiguousarray(a, F).view(np.uint32).copy()
    w[np.isnan(np.ascontiguousarray(a, F))] = 0x7fc00000
    h = 0xcbf29ce484222325
    for b in w.astype("<u4").tobytes():
        h = ((h ^ b) * 0x100000001b3) & 0xffffffffffffffff
    return "%016x" % h


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_depth_cloud")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_depth_cloud.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    got = json.loads(out.stdout.strip().splitlines()[-1])

    d, c, E = images()
    assert (d == 0).sum() > 0 and np.isposinf(d).sum() > 0 and (d < 0).sum() > 0
    assert ((d > 0) & (d < CUTOFF)).sum() > 1000 and (np.isfinite(d) & (d >= CUTOFF)).sum() > 500
    rgbd = dict(color=c, rgbd=True, depth_cutoff=CUTOFF, compute_normals=True)
    want = {"depth_stride3": dx.cloud(d, K4, E, stride=3),
            "rgbd_valid": dx.cloud(d, K4, E, valid_only=True, **rgbd),
            "rgbd_all": dx.cloud(d, K4, E, valid_only=False, **rgbd)}
    assert 0 < len(want["depth_stride3"][0]) < 23 * 16 and 0 < len(want["rgbd_valid"][0]) < len(want["rgbd_all"][0]) == W * H
    for name, (p, n, col, _) in want.items():
        g = got[name]
        assert g["n"] == len(p), name
        assert g["normals"] == (0 if n is None else len(n)) and g["colors"] == (0 if col is None else len(col)), name
        assert (g["h_points"], g["h_normals"], g["h_colors"]) == (fnv(p), fnv(n), fnv(col)), name
