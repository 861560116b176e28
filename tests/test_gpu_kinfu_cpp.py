"""GPU: kinfu::KinfuPipeline through the C++ surface (tests/cpp/test_kinfu.cpp), built as the other tests/cpp programs
are.  This test writes the frames of tests/kinfu_scene.py; the program runs the pipeline over them and writes its poses,
the voxels and the model pyramid of frame 0 back.  Frame 0 involves no registration: its bytes equal the Python mirror's.
The poses are held to the mirror's within 1e-5 Frobenius, the bound the project holds final transforms to.  The
refusals' lines appear on stderr."""
import json
import os
import subprocess

import numpy as np
import pytest

import kinfu_scene as ks

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 3


def test_cpp_surface(tmp_path):
    from cupoch_amd import _lib, kinfu
    _lib.build()
    cpp = os.path.join(ROOT, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_kinfu")
    libdir = os.path.join(ROOT, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(ROOT, "include"),
                           "-I/opt/rocm/include", os.path.join(ROOT, "tests", "cpp", "test_kinfu.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    images = [ks.render(k) for k in range(FRAMES)]
    for k, (d, c) in enumerate(images):
        np.ascontiguousarray(d, F).tofile(str(tmp_path / ("depth_%d.f32" % k)))
        np.ascontiguousarray(c, np.uint8).tofile(str(tmp_path / ("color_%d.u8" % k)))
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1])["failed"] == 0
    for why in ("The frame has no colour or no depth data.", "num_pyramid_levels must be in [1, 16].",
                "icp_iterations has fewer entries than num_pyramid_levels.", "The frame's size is not the intrinsic's.",
                "Unsupported image format."):
        assert "[cupoch_amd] Error: [KinfuPipeline::ProcessFrame] " + why in out.stderr, why
    assert out.stderr.count("[KinfuPipeline::ProcessFrame] Unsupported image format.") == 2
    assert "[cupoch_amd] Error: [UniformTSDFVolume::Integrate] Unsupported image format." in out.stderr

    def read(name, shape):
        return np.fromfile(str(tmp_path / name), F).reshape(shape)

    pipe = kinfu.KinfuPipeline(ks.intrinsic(), ks.option())
    for k, (d, c) in enumerate(images):
        assert pipe.process_frame(ks.rgbd(d, c)) is True
        pose = read("pose_%d.bin" % k, (4, 4))
        err = float(np.linalg.norm(pose.astype(np.float64) - np.asarray(pipe.cur_pose, np.float64)))
        print("frame %d: |C++ pose - mirror pose|_F = %.3g" % (k, err))
        assert err <= 1e-5
        if k == 0:
            t, w, col = pipe.volume.get_voxels()
            assert w.any() and ks.same(read("tsdf.bin", (-1,)), t) and ks.same(read("weight.bin", (-1,)), w)
            assert ks.same(read("color.bin", (-1, 3)), col)
            for i, m in enumerate(pipe.model_pyramid):
                assert len(m.points) > 50
                for part, want in (("points", m.points), ("normals", m.normals), ("colors", m.colors)):
                    assert ks.same(read("model_%d_%s.bin" % (i, part), (-1, 3)), want), (i, part)
    assert ks.pose_error(read("pose_%d.bin" % (FRAMES - 1), (4, 4)), ks.true_pose(FRAMES - 1)[0]) < \
        0.5 * ks.pose_error(np.eye(4), ks.true_pose(FRAMES - 1)[0])      # it tracked
