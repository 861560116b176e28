"""GPU: geometry::VoxelGrid through the C++ surface (tests/cpp/test_voxelgrid.cpp: the reference's three unit tests and a
voxelise -> merge -> carve -> query scene), built as the other tests/cpp programs are and held bit for bit to the numpy
restatement of the contract (tests/voxelgrid_exact.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import voxelgrid_exact as vx

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_voxelgrid")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_voxelgrid.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    pts, col, intr, E, img, q = vx.scene_inputs()
    pts.tofile(str(tmp_path / "points.f32"))
    col.tofile(str(tmp_path / "colors.f32"))
    img.tofile(str(tmp_path / "depth.f32"))
    q.tofile(str(tmp_path / "queries.f32"))
    with open(str(tmp_path / "scene.txt"), "w") as f:
        f.write(" ".join("%.9g" % v for v in [vx.DENSE_VS] + list(intr) + list(E.reshape(-1)) + [vx.IMG_W, vx.IMG_H]))
    out = subprocess.run([exe, str(tmp_path / "points.f32"), str(tmp_path / "colors.f32"), str(tmp_path / "scene.txt"),
                          str(tmp_path / "depth.f32"), str(tmp_path / "queries.f32"), str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["bounds"] and r["get_voxel"] and r["one_voxel"] and r["written"] and r["paint"]
    assert "VoxelGrid::Transform is not supported" in out.stderr and "voxel_size <= 0" in out.stderr

    (ka, kb), (mk, mc), (ck, cc), inc = vx.scene_expected(pts, col, intr, E, img, q)

    def got(name, dtype=F):
        return np.fromfile(str(tmp_path / name), dtype)

    assert (r["na"], r["nb"], r["merged"], r["carved"]) == (len(ka), len(kb), len(mk), len(ck))
    assert len(mk) < len(ka) + len(kb) and 0.05 * len(mk) < len(ck) < 0.95 * len(mk)
    assert np.array_equal(got("merged_keys.i32", np.int32).reshape(-1, 3), mk) and vx.same_bits(got("merged_colors.f32").reshape(-1, 3), mc)
    assert np.array_equal(got("carved_keys.i32", np.int32).reshape(-1, 3), ck) and vx.same_bits(got("carved_colors.f32").reshape(-1, 3), cc)
    assert np.array_equal(got("included.u8", np.uint8).astype(bool), inc) and 0 < inc.sum() < len(inc)
    pick = np.array([i for i in range(len(ck) - 1, -1, -1) if i % 3 == 0])
    assert r["selected"] == len(pick) and np.array_equal(got("selected_keys.i32", np.int32).reshape(-1, 3), ck[pick])
    assert vx.same_bits(got("selected_colors.f32").reshape(-1, 3), cc[pick])
    assert r["split_agrees"] == len(q)                      # the unsorted selection and its complement split the answers
    lo, hi, ce = vx.bounds(mk, vx.DENSE_VS, (0, 0, 0))
    assert vx.same_bits(np.array(r["min"], F), lo) and vx.same_bits(np.array(r["max"], F), hi)
    assert vx.ulp_distance(np.array(r["center"], F), ce).max() <= 1
