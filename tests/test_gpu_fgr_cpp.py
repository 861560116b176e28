"""GPU: registration::Feature, knn::BruteForceNN, CorrespondencesFromFeatures and FastGlobalRegistration through the C++
surface (tests/cpp/test_fgr.cpp), built as the other tests/cpp programs are.  This test writes the scene; the program
checks the defaults, the empty-input rule and its own consistency, and writes its results back, which are compared here
with the restatement and with the same call through the C ABI's ctypes mirror and the pybind11 module: one T, bit for
bit, on all three surfaces."""
import json
import os
import subprocess

import numpy as np
import pytest

import fgr_exact as fx

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_surface_and_the_three_surfaces_agree(tmp_path):
    from cupoch_amd import _lib
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_fgr")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_fgr.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    scenes = {33: fx.scene(33, seed=1), 352: fx.scene(352, seed=1)}
    for dim, sc in scenes.items():
        sc["src"].tofile(str(tmp_path / ("src%d.f32" % dim)))
        sc["tgt"].tofile(str(tmp_path / ("tgt%d.f32" % dim)))
        sc["sfeat"].tofile(str(tmp_path / ("sfeat%d.f32" % dim)))
        sc["tfeat"].tofile(str(tmp_path / ("tfeat%d.f32" % dim)))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["failed"] == 0
    assert out.stderr.count("[cupoch_amd] Error: Invalid source or target pointcloud.") == 4

    from cupoch_amd import pybind as cph
    from cupoch_amd import registration as reg
    from cupoch_amd.geometry import PointCloud
    for dim, sc in scenes.items():
        T_cpp = np.fromfile(str(tmp_path / ("T%d.bin" % dim)), np.float32).reshape(4, 4).T
        corr_cpp = np.fromfile(str(tmp_path / ("corr%d.bin" % dim)), np.int32).reshape(-1, 2)
        want = fx.fgr(sc["src"], sc["tgt"], sc["sfeat"], sc["tfeat"], fx.Option(), 0, fp32=True)
        assert np.linalg.norm(T_cpp - want.T) < 1e-5 and np.linalg.norm(T_cpp - sc["T_gt"]) < 1e-5
        # the ctypes mirror
        m = reg.registration_fast_based_on_feature_matching(PointCloud(sc["src"]), PointCloud(sc["tgt"]), reg.Feature(dim, sc["sfeat"]),
                                                            reg.Feature(dim, sc["tfeat"]))
        assert np.ascontiguousarray(m.transformation).tobytes() == np.ascontiguousarray(T_cpp).tobytes()
        assert np.array_equal(m.correspondence_set, corr_cpp)
        # the pybind11 module
        F = cph.registration.FeatureFPFH if dim == 33 else cph.registration.FeatureSHOT
        fs, ft = F(), F()
        fs.data, ft.data = sc["sfeat"], sc["tfeat"]
        ps, pt = cph.geometry.PointCloud(), cph.geometry.PointCloud()
        ps.points, pt.points = cph.utility.Vector3fVector(sc["src"]), cph.utility.Vector3fVector(sc["tgt"])
        p = cph.registration.registration_fast_based_on_feature_matching(ps, pt, fs, ft)
        assert np.asarray(p.transformation, np.float32).tobytes() == np.ascontiguousarray(T_cpp).tobytes()
        assert np.array_equal(np.asarray(p.correspondence_set), corr_cpp) and p.fitness == pytest.approx(m.fitness, abs=0)
    sc = scenes[33]
    D = fx.dist64(sc["sfeat"], sc["tfeat"])
    nn = np.fromfile(str(tmp_path / "nn33.bin"), np.int32)
    assert np.array_equal(nn, fx.neighbours(D))
    assert np.array_equal(np.fromfile(str(tmp_path / "cffm33.bin"), np.int32).reshape(-1, 2), fx.reciprocal_pairs(nn, fx.neighbours(D.T)))
    fs, ft = cph.registration.FeatureFPFH(), cph.registration.FeatureFPFH()
    fs.data, ft.data = sc["sfeat"], sc["tfeat"]
    assert np.array_equal(cph.registration.correspondences_from_features(fs, ft, mutual_filter=True), fx.reciprocal_pairs(nn, fx.neighbours(D.T)))
