"""integration::UniformTSDFVolume without a GPU: the numpy fp32 restatement of the contract (tests/tsdf_exact.py) is
held to the reference's own RealData test (src/tests/integration/uniform_fsdfvolume.cpp) on the reference's five
RGB-D frames, and to a synthetic wall; the Python type's surface."""
import os

import numpy as np
import pytest

import tsdf_exact as tx
from conftest import ROOT

F = np.float32
RGBD = os.path.join(ROOT, "tests", "golden", "rgbd")

# the values the reference's RealData test pins (uniform_fsdfvolume.cpp:158-183)
REF_POINTS, REF_VOXELS = 2227, 4488
REF_COLOR_SUM = (1877.673116, 1862.126057, 1862.190616)
REF_NORMAL_SUM = (-161.569098, -95.969433, -1783.167177)
REF_VOXEL_COLOR_SUM = 2096.428416


def test_restatement_reproduces_the_references_real_data_values():
    """Counts exactly; colour sums within the reference's own 0.1; the normal sum within 0.2 of the reference's pinned
    values (its 0.1 is for a build that contracts multiply-adds; a unit normal over a near-zero gradient amplifies the
    difference).  Measured here: |normal sum - pinned| = 0.098 / 0.062 / 0.020, colour sums within 0.03."""
    frames = tx.load_rgbd_frames(RGBD)
    assert len(frames) == 5
    vol = tx.Volume(8.0, 200, 0.04, tx.RGB8)
    for d, c, E in frames:
        tx.integrate(vol, d, c, *tx.PRIMESENSE, E)
    vp, vc = tx.extract_voxel_point_cloud(vol)
    assert len(vp) == REF_VOXELS and len(vc) == REF_VOXELS
    vsum = vc.astype(np.float64).sum(0)
    print("voxel colour sum", vsum)
    assert np.abs(vsum - REF_VOXEL_COLOR_SUM).max() <= 0.1
    p, n, c = tx.extract_point_cloud(vol)
    assert len(p) == REF_POINTS and len(c) == REF_POINTS and len(n) == REF_POINTS
    csum, nsum = c.astype(np.float64).sum(0), n.astype(np.float64).sum(0)
    print("colour sum", csum, "normal sum", nsum, "normal sum - pinned", nsum - np.array(REF_NORMAL_SUM))
    assert np.abs(csum - np.array(REF_COLOR_SUM)).max() <= 0.1
    assert np.abs(nsum - np.array(REF_NORMAL_SUM)).max() <= 0.2


def test_wall_scene_is_self_consistent():
    """A fronto-parallel plane at depth d seen by a camera outside the volume.  A sign change can occur only inside
    the truncation band and the tsdf is sampled at the nearest voxel centre, so every raycast vertex and every extracted
    point lies within sdf_trunc + voxel_length of the plane; normals point at the camera; weights count the frames."""
    W, H, fx, fy, cx, cy = 64, 48, 60.0, 60.0, 31.5, 23.5
    vol = tx.Volume(1.6, 32, 0.1, tx.RGB8)
    cam_z, wall_z = -2.0, 0.21
    E = np.eye(4, dtype=F)
    E[2, 3] = -cam_z                                    # the camera at (0, 0, cam_z), looking along +z
    d, c = tx.render_scene(W, H, fx, fy, cx, cy, E, [((0, 0, 1), wall_z)], holes=False)
    assert np.allclose(d, wall_z - cam_z, atol=1e-6)
    frames = 3
    for _ in range(frames):
        assert tx.integrate(vol, d, c, W, H, fx, fy, cx, cy, E) > 0
    w = vol.weight
    assert set(np.unique(w).tolist()) == {0.0, float(frames)}
    band = float(vol.trunc + vol.vl)
    p, n, col = tx.extract_point_cloud(vol)
    assert len(p) > 0
    assert np.abs(p[:, 2] - wall_z).max() <= band
    assert (n[:, 2] < -0.9).all()                       # towards the camera, which sits at -z
    assert col.min() >= 0.0 and col.max() <= 1.0 + 1e-6     # a convex combination of bytes / 255, three roundings
    # The reference's entry test takes the cube [0, length]^3 in the frame of (camera - origin): a camera on the
    # volume's axis sits on that cube's edge.  One at (0.8, 0.8, cam_z) looks down the cube's middle, and the wall
    # continues there (it is a plane), the voxels only up to +0.8: shift the volume instead.
    vol2 = tx.Volume(1.6, 32, 0.1, tx.RGB8, origin=(0.8, 0.8, 0.0))
    E2 = E.copy()
    E2[0, 3], E2[1, 3] = -0.6, -0.6                     # camera at (0.6, 0.6, cam_z)
    d2, c2 = tx.render_scene(W, H, fx, fy, cx, cy, E2, [((0, 0, 1), wall_z)], holes=False)
    tx.integrate(vol2, d2, c2, W, H, fx, fy, cx, cy, E2)
    P, N, C, gathers = tx.raycast(vol2, W, H, fx, fy, cx, cy, E2, 0.1)
    ok = np.isfinite(P).all(1)
    assert ok.sum() > 50 and gathers >= ok.sum()
    assert np.abs(P[ok, 2] - wall_z).max() <= band
    assert (N[ok, 2] < -0.9).all()
    assert np.isfinite(N[ok]).all() and np.isfinite(C[ok]).all()
    assert np.isnan(N[~ok]).all() and np.isnan(C[~ok]).all()


def test_python_type_surface():
    """what the Python type offers without touching a GPU: the enum's values and the module's names"""
    from cupoch_amd import integration, kinfu
    T = integration.TSDFVolumeColorType
    assert [int(T.NoColor), int(T.RGB8), int(T.Gray32)] == [0, 1, 2]
    for name in ("integrate", "extract_point_cloud", "extract_voxel_point_cloud", "raycast", "reset", "get_voxels"):
        assert callable(getattr(integration.UniformTSDFVolume, name))
    for name in ("extract_triangle_mesh", "extract_voxel_grid"):
        assert not hasattr(integration.UniformTSDFVolume, name)          # out of scope, and said so
    assert "ScalableTSDFVolume" in integration.__doc__ and not hasattr(integration, "ScalableTSDFVolume")
    o = kinfu.KinfuOption()
    assert (o.tsdf_length, o.tsdf_resolution, o.sdf_trunc) == (8.0, 512, pytest.approx(0.05))
    assert o.tsdf_color_type == T.RGB8 and np.array_equal(o.tsdf_origin, np.zeros(3, F))
    assert callable(kinfu.integrate_and_raycast) and callable(kinfu.create_volume)
    b = integration.TSDFVolume(0.03125, 0.04, T.Gray32)
    assert b.voxel_length == 0.03125 and b.sdf_trunc == float(F(0.04)) and b.color_type == T.Gray32
