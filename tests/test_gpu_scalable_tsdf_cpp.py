"""GPU: integration::ScalableTSDFVolume through the C++ surface (tests/cpp/test_scalable_tsdfvolume.cpp: the
constructor's fields and a wall scene), built as the other tests/cpp programs are and held bit for bit to the numpy
restatement of the contract (tests/scalable_tsdf_exact.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import scalable_tsdf_exact as sx
import tsdf_exact as tx

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_scalable_tsdfvolume")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_scalable_tsdfvolume.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    W, H, fx, fy, cx, cy = 64, 48, 60.0, 60.0, 31.5, 23.5
    E = np.eye(4, dtype=F)
    E[:3, 3] = (-0.6, -0.6, 2.0)
    d, c = tx.render_scene(W, H, fx, fy, cx, cy, E, [((0, 0, 1), 0.22)], holes=True)
    d.tofile(str(tmp_path / "depth.f32"))
    c.tofile(str(tmp_path / "color.u8"))
    out = subprocess.run([exe, str(tmp_path / "depth.f32"), str(tmp_path / "color.u8"), str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["constructor"] and r["bad_arguments_throw"] and r["written"]

    ref = sx.Volume(0.05, 0.1, sx.RGB8, 2)
    for _ in range(2):
        assert sx.integrate(ref, d, c, W, H, fx, fy, cx, cy, E)[1] > 0

    def got(name, cols=3):
        return np.fromfile(str(tmp_path / name), F).reshape(-1, cols)

    def same(a, b):
        a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
        return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())

    rk, rt, rw, rc = ref.arrays()
    keys = np.fromfile(str(tmp_path / "unit_keys.i32"), np.int32).reshape(-1, 3)
    assert len(rk) > 8 and r["units"] == len(rk) and np.array_equal(keys, rk)     # (more than the map_size of 8)
    units = got("units.f32", 5).reshape(len(rk), 4096, 5)        # the two turned-away frames left no trace
    assert same(units[..., 0], rt) and same(units[..., 1], rw) and same(units[..., 2:], rc)
    assert out.stderr.count("[ScalableTSDFVolume::Integrate] Unsupported image format.") == 2
    p, n, col = sx.extract_point_cloud(ref)
    assert len(p) > 0 and r["cloud"] == len(p) and r["has_normals"]
    assert same(got("cloud_points.f32"), p) and same(got("cloud_normals.f32"), n) and same(got("cloud_colors.f32"), col)
    vp, vc = sx.extract_voxel_point_cloud(ref)
    assert len(vp) > 0 and r["voxels"] == len(vp) and not r["voxel_cloud_has_normals"]
    assert same(got("voxel_points.f32"), vp) and same(got("voxel_colors.f32"), vc)
    # the wall: every point within a voxel of the plane z = 0.22, most normals towards the camera at -z
    assert np.abs(p[:, 2] - 0.22).max() <= float(ref.vl) and (n[:, 2] < -0.9).mean() > 0.9
    assert r["after_reset"] == 0
