"""GPU: geometry::OccupancyGrid through the C++ surface (tests/cpp/test_occupancygrid.cpp: the reference's four unit
tests and a scene on a grid of 33^3), built as the other tests/cpp programs are and held bit for bit to the numpy
restatement of the contract (tests/occgrid_exact.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import occgrid_exact as ox

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_occupancygrid")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_occupancygrid.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    res = 33
    free, ins = ox.scene("g", res, 5000)
    pts, vp = ins[1], ins[2]
    max_range = F(0.9)
    pts.tofile(str(tmp_path / "points.f32"))
    with open(str(tmp_path / "scene.txt"), "w") as f:
        f.write(" ".join("%.9g" % v for v in list(vp) + list(free[1]) + list(free[2]) + [max_range]))
    out = subprocess.run([exe, str(tmp_path / "points.f32"), str(tmp_path / "scene.txt"), str(tmp_path)],
                         capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["bounds"] and r["get_voxel"] and r["insert"] and r["set_free_area"] and r["written"]
    assert "not in the occupancy grid range" in out.stderr            # the AddVoxel outside the grid was logged

    ref = ox.new_grid(res)
    ox.set_free_area(ref, free[1], free[2])
    ox.insert(ref, pts, vp)
    ox.insert(ref, pts, vp, max_range)
    ox.insert(ref, pts, vp)
    dup = [((k * 7) % 33, (k * 5) % 11, (k * 3) % 33) for k in range(40)]
    dup += [dup[(k * 13) % 40] for k in range(40)]
    ox.add_voxels(ref, dup, True)
    ref.origin = (ref.origin + np.array([0.05, 0.0, -0.05], F)).astype(F)
    ref.voxel_size = F(ref.voxel_size * F(1.5))
    ox.insert(ref, pts, vp)

    def same(a, b):
        a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
        return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())

    def got(name, dtype=F):
        return np.fromfile(str(tmp_path / name), dtype)

    assert same(got("plane.f32"), ref.prob)
    ijk, p, _ = ox.extract(ref, ox.KNOWN)
    assert len(p) > 1000 and r["known"] == len(p)
    assert np.array_equal(got("known_index.i32", np.int32).reshape(-1, 3), ijk) and same(got("known_prob.f32"), p)
    assert same(got("free_prob.f32"), ox.extract(ref, ox.FREE)[1])
    _, po, pts_o = ox.extract(ref, ox.OCCUPIED)
    assert len(po) > 100 and same(got("occupied_prob.f32"), po)
    assert r["cloud"] == len(po) and r["has_colors"] and same(got("cloud_points.f32").reshape(-1, 3), pts_o)
    assert (got("cloud_colors.f32").reshape(-1, 3) == np.array([0, 0, 1], F)).all()
    assert r["min_bound"] == list(ref.min_bound) and r["max_bound"] == list(ref.max_bound)
    assert same(np.array(r["min"], F), ox.get_min_bound(ref)) and same(np.array(r["max"], F), ox.get_max_bound(ref))
