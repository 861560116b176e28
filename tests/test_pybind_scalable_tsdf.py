"""integration_scalable.ScalableTSDFVolume of the reference's pybind11 module (cupoch_amd/cpp/src/pybind_module.cpp) with the
reference's Python names (src/python/cupoch_pybind/integration/integration.cpp:153-195): the surface on the CPU, and on
the GPU the same bytes as the ctypes mirror and the numpy restatement (tests/scalable_tsdf_exact.py).  Skips only where
the module cannot be imported."""
import numpy as np
import pytest

import scalable_tsdf_exact as sx
import tsdf_exact as tx

F = np.float32


def module():
    try:
        from cupoch_amd import pybind as cph
    except Exception as e:      # not built and not buildable here
        pytest.skip("cupoch_pybind cannot be imported: %s" % e)
    return cph


def test_scalable_volume_has_the_references_names():
    cph = module()
    S = cph.integration_scalable.ScalableTSDFVolume
    for name in ("integrate", "extract_point_cloud", "extract_voxel_point_cloud", "reset", "voxel_length", "sdf_trunc",
                 "color_type", "volume_unit_length", "resolution", "volume_unit_voxel_num", "depth_sampling_stride"):
        assert hasattr(S, name), name
    for name in ("extract_triangle_mesh", "raycast"):
        assert not hasattr(S, name)                                   # not built, and not pretended
    with pytest.raises(TypeError):
        S(0.01, 0.04)                                                 # no default colour type in the reference either


@pytest.mark.gpu
def test_volume_through_the_pybind_module_equals_the_restatement():
    cph = module()
    from cupoch_amd import camera, geometry, integration, integration_scalable
    W, H, fx, fy, cx, cy = 64, 48, 60.0, 60.0, 31.5, 23.5
    E = np.eye(4, dtype=F)
    E[:3, 3] = (-0.6, -0.6, 2.0)
    d, c = tx.render_scene(W, H, fx, fy, cx, cy, E, [((0, 0, 1), 0.22)], holes=True)
    T = cph.integration.TSDFVolumeColorType
    vol = cph.integration_scalable.ScalableTSDFVolume(0.05, 0.1, T.RGB8, depth_sampling_stride=2)
    assert repr(vol) == "pipelines::integration::ScalableTSDFVolume with color."
    assert repr(cph.integration_scalable.ScalableTSDFVolume(0.05, 0.1, T.NoColor)).endswith("without color.")
    assert (vol.resolution, vol.volume_unit_voxel_num, vol.depth_sampling_stride, vol.color_type) == (16, 4096, 2, T.RGB8)
    assert vol.voxel_length == F(0.05) and vol.sdf_trunc == F(0.1) and vol.volume_unit_length == F(0.05) * F(16)
    assert cph.integration_scalable.ScalableTSDFVolume(0.05, 0.1, T.RGB8).depth_sampling_stride == 4
    with pytest.raises(Exception):
        cph.integration_scalable.ScalableTSDFVolume(0.01, 0.2, T.RGB8)         # sdf_trunc > 16 voxels
    K = cph.camera.PinholeCameraIntrinsic(W, H, fx, fy, cx, cy)
    rgbd = cph.geometry.RGBDImage(cph.geometry.Image(c), cph.geometry.Image(d))
    ref = sx.Volume(0.05, 0.1, sx.RGB8, 2)
    mirror = integration_scalable.ScalableTSDFVolume(0.05, 0.1, integration.TSDFVolumeColorType.RGB8, 2)
    for _ in range(2):
        vol.integrate(rgbd, K, E)
        sx.integrate(ref, d, c, W, H, fx, fy, cx, cy, E)
        assert mirror.integrate(geometry.RGBDImage(c, d), camera.PinholeCameraIntrinsic(W, H, fx, fy, cx, cy), E)
    assert vol.num_volume_units() == len(ref.units) > 8

    def same(v, b):
        a = np.ascontiguousarray(np.asarray(v.cpu()), F)
        b = np.ascontiguousarray(np.asarray(b.cpu() if hasattr(b, "cpu") else b), F)
        return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())

    p, n, col = sx.extract_point_cloud(ref)
    g, mg = vol.extract_point_cloud(), mirror.extract_point_cloud()
    assert len(p) > 0 and same(g.points, p) and same(g.normals, n) and same(g.colors, col)
    assert same(g.points, mg.points) and same(g.normals, mg.normals) and same(g.colors, mg.colors)
    vp, vc = sx.extract_voxel_point_cloud(ref)
    g = vol.extract_voxel_point_cloud()
    assert len(vp) > 0 and same(g.points, vp) and same(g.colors, vc) and not g.has_normals()
    vol.reset()
    assert len(vol.extract_voxel_point_cloud().points) == 0 and vol.num_volume_units() == 0
