"""GPU: collision through the C++ surface (tests/cpp/test_collision.cpp: the reference's two unit tests, one scene per
side kind, Intersection<VoxelGrid> on an unsorted target, CreateVoxelGrid), built as the other tests/cpp programs are
and held exactly to the numpy restatement of the contract (tests/collision_exact.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import collision_exact as ex

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_collision")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_collision.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    a_keys, b_keys, pts, lines, prims, cloud, cap = ex.scene_inputs()
    for name, arr in (("a_keys.i32", a_keys), ("b_keys.i32", b_keys), ("points.f32", pts), ("lines.i32", lines), ("cloud.f32", cloud)):
        np.ascontiguousarray(arr).tofile(str(tmp_path / name))
    ex.prim_records(prims).tofile(str(tmp_path / "prims.bin"))
    ex.prim_records([cap]).tofile(str(tmp_path / "capsule.bin"))
    ob = ex.SCENE_ORIGIN + F(0.037)
    with open(str(tmp_path / "scene.txt"), "w") as f:
        f.write(" ".join("%.9g" % v for v in [F(ex.SCENE_VS), F(ex.SCENE_VS_B)] + list(ex.SCENE_ORIGIN) + list(ob)) +
                " %d %.9g" % (ex.SCENE_RES, F(ex.SCENE_MARGIN)))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    for flag in ("voxel_voxel", "voxel_lineset", "written", "kept_sorted", "same_again", "refused", "lineset"):
        assert r[flag], flag
    assert "voxel_size <= 0" in out.stderr and "Unsupported primitive type" in out.stderr and "margin" in out.stderr
    occ = np.fromfile(str(tmp_path / "occ.i32"), np.int32).reshape(-1, 3)
    assert len(occ) == r["occupied"] > 50
    want = ex.scene_expected(occ)
    for name, pairs in want.items():
        got = np.fromfile(str(tmp_path / (name + ".i32")), np.int32).reshape(-1, pairs.shape[1])
        assert np.array_equal(got, pairs), name
        assert len(pairs) > 0, name
    assert r["capsule"] == len(want["capsule"])
    mn, mx = ex.primitive_aabb(cap)
    assert np.array_equal(np.array(r["box"], F), np.concatenate([mn, mx])) and np.array_equal(np.array(r["origin"], F), cap.transform[:3, 3])
