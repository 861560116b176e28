"""GPU: geometry::DistanceTransform through the C++ surface (tests/cpp/test_distancetransform.cpp: the reference's unit
test, a scene at 65^3 through the VoxelGrid form, the no-sites case and the two log messages), built as the other tests/cpp
programs are and held bit for bit to the numpy restatement of the contract (tests/edt_exact.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import edt_exact as ex

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_distancetransform")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_distancetransform.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    pts = ex.scene_points()
    pts.tofile(str(tmp_path / "points.f32"))
    with open(str(tmp_path / "scene.txt"), "w") as f:
        f.write(" ".join("%.9g" % v for v in [ex.SCENE_VS] + list(ex.SCENE_LO) + list(ex.SCENE_ORIGIN)) + " %d" % ex.SCENE_RES)
    out = subprocess.run([exe, str(tmp_path / "points.f32"), str(tmp_path / "scene.txt"), str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["unit"] and r["defaults"] and r["no_sites"] and r["unchanged"] and r["cells"] and r["written"]
    assert "DenseGrid::Transform is not supported" in out.stderr and "DenseGrid::Rotate is not supported" in out.stderr
    assert "Unsupport computing Voronoi diagrams from different voxel size." in out.stderr

    keys = np.fromfile(str(tmp_path / "keys.i32"), np.int32).reshape(-1, 3)
    near = np.fromfile(str(tmp_path / "nearest.i32"), np.int32).reshape(-1, 3)
    dist = np.fromfile(str(tmp_path / "distance.f32"), F)
    assert r["keys"] == len(keys) > 1000 and len(dist) == ex.SCENE_RES ** 3
    ex.scene_check(keys, near, dist)
    q = np.fromfile(str(tmp_path / "queried.f32"), F)
    c = ex.cells_of_points(pts, ex.SCENE_VS, ex.SCENE_ORIGIN, ex.SCENE_RES)
    ins = ex.inside(c, ex.SCENE_RES)
    assert r["queries"] == len(pts) == len(q) and 0 < ins.sum() < len(pts)
    lin = (c[ins, 0] * ex.SCENE_RES + c[ins, 1]) * ex.SCENE_RES + c[ins, 2]
    assert (q[ins].view(np.uint32) == dist[lin].view(np.uint32)).all() and np.isnan(q[~ins]).all()
