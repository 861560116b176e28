"""The `integration` rows of the reference's pybind11 module (cupoch_amd/cpp/src/pybind_module.cpp) with the reference's
Python names (src/python/cupoch_pybind/integration/integration.cpp): the surface on the CPU, and on the GPU the same
bytes as the ctypes mirror and the numpy restatement (tests/tsdf_exact.py).  Skips only where the module cannot be
imported."""
import numpy as np
import pytest

import tsdf_exact as tx

F = np.float32


def module():
    try:
        from cupoch_amd import pybind as cph
    except Exception as e:      # not built and not buildable here
        pytest.skip("cupoch_pybind cannot be imported: %s" % e)
    return cph


def test_integration_rows_have_the_references_names():
    cph = module()
    i = cph.integration
    T = i.TSDFVolumeColorType
    assert [int(T.NoColor), int(T.RGB8), int(T.Gray32)] == [0, 1, 2]
    for name in ("integrate", "extract_point_cloud", "extract_voxel_point_cloud", "raycast", "reset",
                 "voxel_length", "sdf_trunc", "color_type", "length", "resolution", "origin"):
        assert hasattr(i.UniformTSDFVolume, name), name
    for name in ("extract_triangle_mesh", "extract_voxel_grid"):
        assert not hasattr(i.UniformTSDFVolume, name)                # not built, and not pretended
    assert not hasattr(i, "ScalableTSDFVolume")
    K = cph.camera.PinholeCameraIntrinsic(640, 480, 525.0, 525.0, 319.5, 239.5)
    K1 = K.create_pyramid_level(1)
    assert (K1.width, K1.height) == (320, 240) and K1.get_focal_length() == (262.5, 262.5)
    assert K1.get_principal_point() == (159.5, 119.5) and K.is_valid()
    assert cph.geometry.Image().is_empty()                            # (pixels live on the device: the GPU test fills one)
    assert cph.geometry.RGBDImage().depth.width == 0
    with pytest.raises(TypeError):
        i.UniformTSDFVolume(1.0, 16, 0.1)                             # no default colour type in the reference either


@pytest.mark.gpu
def test_volume_through_the_pybind_module_equals_the_restatement():
    cph = module()
    W, H, fx, fy, cx, cy = 64, 48, 60.0, 60.0, 31.5, 23.5
    E = np.eye(4, dtype=F)
    E[:3, 3] = (-0.6, -0.6, 2.0)
    d, c = tx.render_scene(W, H, fx, fy, cx, cy, E, [((0, 0, 1), 0.21)], holes=True)
    T = cph.integration.TSDFVolumeColorType
    vol = cph.integration.UniformTSDFVolume(1.6, 32, 0.1, T.RGB8, np.array([0.8, 0.8, 0.0], F))
    assert (vol.resolution, vol.color_type) == (32, T.RGB8) and vol.length == F(1.6) and vol.sdf_trunc == F(0.1)
    assert vol.voxel_length == F(1.6) / F(32) and np.array_equal(vol.origin, np.array([0.8, 0.8, 0.0], F))
    K = cph.camera.PinholeCameraIntrinsic(W, H, fx, fy, cx, cy)
    img, dep = cph.geometry.Image(c), cph.geometry.Image(d)
    assert (img.width, img.height, img.num_of_channels, img.bytes_per_channel) == (W, H, 3, 1)
    assert (dep.width, dep.height, dep.num_of_channels, dep.bytes_per_channel) == (W, H, 1, 4)
    rgbd = cph.geometry.RGBDImage(img, dep)
    assert rgbd.color.width == W and rgbd.depth.bytes_per_channel == 4
    ref = tx.Volume(1.6, 32, 0.1, tx.RGB8, (0.8, 0.8, 0.0))
    for _ in range(2):
        vol.integrate(rgbd, K, E)
        tx.integrate(ref, d, c, W, H, fx, fy, cx, cy, E)

    def same(v, b):
        a = np.ascontiguousarray(np.asarray(v.cpu()), F)
        b = np.ascontiguousarray(b, F)
        return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())

    p, n, col = tx.extract_point_cloud(ref)
    g = vol.extract_point_cloud()
    assert len(p) > 0 and same(g.points, p) and same(g.normals, n) and same(g.colors, col)
    vp, vc = tx.extract_voxel_point_cloud(ref)
    g = vol.extract_voxel_point_cloud()
    assert len(vp) > 0 and same(g.points, vp) and same(g.colors, vc) and not g.has_normals()
    P, N, C, _ = tx.raycast(ref, W, H, fx, fy, cx, cy, E, 0.1)
    ok = np.isfinite(P).all(1)
    g = vol.raycast(K, E, 0.1)                                        # project_valid_depth_only = True
    assert ok.sum() > 50 and same(g.points, P[ok]) and same(g.normals, N[ok]) and same(g.colors, C[ok])
    g = vol.raycast(K, E, 0.1, project_valid_depth_only=False)
    assert same(g.points, P) and same(g.normals, N)
    vol.reset()
    assert len(vol.extract_voxel_point_cloud().points) == 0
