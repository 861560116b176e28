"""GPU: geometry::LaserScanBuffer through the C++ surface (tests/cpp/test_laserscanbuffer.cpp: the reference's three unit
tests and one conversion each way), built as the other tests/cpp programs are and held bit for bit to the numpy
restatement of the contract (tests/laserscan_exact.py)."""
import json
import os
import subprocess

import numpy as np
import pytest

import laserscan_exact as lx

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_laserscanbuffer")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_laserscanbuffer.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    rng = np.random.default_rng(31)
    steps = 181
    scans = rng.uniform(0.8, 15.0, (3, steps)).astype(F)
    scans[:, 7] = np.nan
    scans[1, 20:24] = (np.inf, 0.1, 25.0, 0.5)
    values = rng.random((3, steps)).astype(F)
    origins = np.stack([lx.pose_matrix(0.5 * k, -k, 0.3 * k, z=0.1 * k) for k in range(3)])
    bins_args = dict(angle_inc=0.02, min_h=0.0, max_h=2.0, divisions=3, min_range=0.2, max_range=9.0, min_angle=-1.5, max_angle=1.5)
    cloud = lx.points_in_bins(rng, 3000, **bins_args)
    scans.tofile(str(tmp_path / "scans.f32"))
    values.tofile(str(tmp_path / "values.f32"))
    np.ascontiguousarray(origins.transpose(0, 2, 1)).tofile(str(tmp_path / "origins.f32"))       # column-major
    cloud.tofile(str(tmp_path / "cloud.f32"))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["constructor"] and r["add_ranges"] and r["range_filter"] and r["written"]
    for msg in ("[AddRanges] Invalid size of input ranges.", "[Merge] Buffer is full.", "LaserScanBuffer::GetMinBound is not supported",
                "[PointCloud::CreateFromLaserScanBuffer] min_range must be smaller than max_range.",
                "[LaserScanBuffer::CreateFromPointCloud] angle_increment must be positive."):
        assert msg in out.stderr, msg

    # two slots, three adds: slot 0 holds scan 2, slot 1 scan 1; the live scans are 1 then 2
    store, org, val = scans[[2, 1]], origins[[2, 1]], values[[2, 1]]
    pts, cols = lx.to_points(store, val, org, 1, 2, -2.1, 2.3, 0.5, 20.0)
    got = np.fromfile(str(tmp_path / "points.f32"), F).reshape(-1, 3)
    assert len(pts) > steps and r["points"] == r["colors"] == len(pts) and r["empty"] == 0 and r["bad_is_null"]
    assert got.tobytes() == pts.tobytes()
    assert np.fromfile(str(tmp_path / "colors.f32"), F).tobytes() == cols.tobytes()
    want = lx.from_points(cloud, 0.02, 0.0, 2.0, 3, 0.2, 9.0, -1.5, 1.5)
    assert (r["virt_steps"], r["virt_scans"], r["virt_slots"]) == (want.shape[1], 3, 50)
    assert np.fromfile(str(tmp_path / "bins.f32"), F).tobytes() == want.tobytes() and (~np.isnan(want)).sum() > 300
    assert F(r["origin_z1"]) == lx.factory_origins(0.0, 2.0, 3, 50)[1, 2, 3]
