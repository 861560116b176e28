"""The `kinfu` rows of the reference's pybind11 module (cupoch_amd/cpp/src/pybind_module.cpp) on the GPU: the call
sequence of the reference's example (examples/python/advanced/kinfu.py) on two small frames -- option with fields set,
pipeline, create_from_color_and_depth(..., depth_trunc=4.0, convert_rgb_to_intensity=False), process_frame, cur_pose,
extract_point_cloud -- with the results of the ctypes mirror.  Skips only where the module cannot be imported.  (The
surface itself is checked without a GPU in tests/test_kinfu_cpu.py.)"""
import numpy as np
import pytest

import kinfu_scene as ks

F = np.float32


def module():
    try:
        from cupoch_amd import pybind as cph
    except Exception as e:      # not built and not buildable here
        pytest.skip("cupoch_pybind cannot be imported: %s" % e)
    return cph


@pytest.mark.gpu
def test_example_sequence_equals_the_mirror():
    cph = module()
    from cupoch_amd import geometry, kinfu
    mirror_opt = ks.option()
    kop = cph.kinfu.KinfuOption()
    kop.num_pyramid_levels, kop.icp_iterations = mirror_opt.num_pyramid_levels, list(mirror_opt.icp_iterations)
    kop.depth_cutoff, kop.distance_threshold = mirror_opt.depth_cutoff, mirror_opt.distance_threshold
    kop.tsdf_length, kop.tsdf_resolution, kop.sdf_trunc = mirror_opt.tsdf_length, mirror_opt.tsdf_resolution, mirror_opt.sdf_trunc
    kop.tsdf_origin = mirror_opt.tsdf_origin
    K = cph.camera.PinholeCameraIntrinsic(ks.W, ks.H, ks.FX, ks.FY, ks.CX, ks.CY)
    pipe = cph.kinfu.KinfuPipeline(K, kop)
    mirror = kinfu.KinfuPipeline(ks.intrinsic(), mirror_opt)
    assert np.array_equal(pipe.cur_pose, np.eye(4, dtype=F)) and pipe.model_pyramid == []
    for k in range(2):
        d, c = ks.render(k)
        d16 = np.round(d * 1000.0).astype(np.uint16)                    # a depth image in millimetres, as the files are
        rgbd = cph.geometry.RGBDImage.create_from_color_and_depth(cph.geometry.Image(c), cph.geometry.Image(d16),
                                                                  depth_trunc=4.0, convert_rgb_to_intensity=False)
        assert pipe.process_frame(rgbd) is True
        assert mirror.process_frame(geometry.RGBDImage.create_from_color_and_depth(
            c, d16, depth_trunc=4.0, convert_rgb_to_intensity=False)) is True
        err = float(np.linalg.norm(np.asarray(pipe.cur_pose, np.float64) - np.asarray(mirror.cur_pose, np.float64)))
        print("frame %d: |pybind pose - mirror pose|_F = %.3g" % (k, err))
        assert err <= 1e-5                                               # the bound the project holds final transforms to
        assert len(pipe.model_pyramid) == ks.LEVELS
        if k == 0:                                                       # no registration yet: the same bytes
            for a, b in zip(pipe.model_pyramid, mirror.model_pyramid):
                assert len(b.points) > 50 and ks.same(a.points, b.points) and ks.same(a.normals, b.normals) and ks.same(a.colors, b.colors)
    assert not np.array_equal(pipe.cur_pose, np.eye(4, dtype=F))
    got, want = pipe.extract_point_cloud(), mirror.extract_point_cloud()
    assert len(want.points) > 1000 and abs(len(got.points) - len(want.points)) <= 0.02 * len(want.points)
    assert pipe.process_frame(cph.geometry.RGBDImage()) is False         # the reference's own refusal
    pipe.reset()
    assert np.array_equal(pipe.cur_pose, np.eye(4, dtype=F)) and pipe.model_pyramid == []
