"""mi_icp_tsdf_raycast_levels (UniformTSDFVolume.raycast_levels): the model pyramid of KinectFusion in one pass equals
one raycast per level, taken with create_pyramid_level, bit for bit and count for count -- at odd sizes with partial
16 x 16 tiles, with an empty last level, with one level, for every colour type and both values of valid_only, for a
camera that sees nothing; the capacity rule; the limits on `levels`."""
import ctypes as C

import numpy as np
import pytest

import tsdf_exact as tx

pytestmark = pytest.mark.gpu
F = np.float32
LENGTH, RES, TRUNC, ORIGIN = 1.6, 32, 0.1, (0.8, 0.8, 0.0)
# Raycast enters the volume through the box [0, length]^3 of the camera's frame minus the origin (include/mi_icp.h): the
# scene lies in the volume's upper octant, x and y in [0.8, 1.6), z in [0, 0.8)
PLANES, SPHERE = [((0.0, 0.0, 1.0), 0.5), ((0.0, 0.6, 0.8), 1.24)], ((1.1, 1.1, 0.4), 0.15)
CAMERAS = {"70x50": (70, 50, 66.0, 64.0, 34.3, 25.1), "3x3": (3, 3, 6.0, 6.0, 1.0, 1.0)}


def extrinsic():
    E = np.eye(4, dtype=F)
    E[:3, 3] = (-1.2, -1.2, 0.7)                    # the camera at (1.2, 1.2, -0.7), in front of that octant
    return E


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def same(a, b):
    a, b = np.ascontiguousarray(to_np(a), F), np.ascontiguousarray(to_np(b), F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


@pytest.fixture(scope="module")
def volumes():
    """one volume per colour type with two frames of the scene in it"""
    from cupoch_amd import camera, geometry, integration
    w, h, fx, fy, cx, cy = 64, 48, 60.0, 60.0, 31.5, 23.5
    K = camera.PinholeCameraIntrinsic(w, h, fx, fy, cx, cy)
    out = {}
    for ct in (tx.NO_COLOR, tx.RGB8, tx.GRAY32):
        vol = integration.UniformTSDFVolume(LENGTH, RES, TRUNC, integration.TSDFVolumeColorType(ct), ORIGIN)
        for k in range(2):
            E = extrinsic()
            E[0, 3] -= F(0.02 * k)
            d, c = tx.render_scene(w, h, fx, fy, cx, cy, E, PLANES, SPHERE)
            col = {tx.NO_COLOR: None, tx.RGB8: c, tx.GRAY32: np.ascontiguousarray(c[..., 0].astype(F) / F(255))}[ct]
            assert vol.integrate(geometry.RGBDImage(col, d), K, E)
        out[ct] = vol
    return out


def intrinsic(name):
    from cupoch_amd import camera
    return camera.PinholeCameraIntrinsic(*CAMERAS[name])


def check(vol, K, E, levels, valid_only):
    """-> the levels' sizes, after comparing every level with its own raycast"""
    got = vol.raycast_levels(K, E, TRUNC, levels, valid_only)
    assert len(got) == levels
    for i, g in enumerate(got):
        want = vol.raycast(K.create_pyramid_level(i), E, TRUNC, valid_only)
        assert len(g.points) == len(want.points), "level %d: %d points, the raycast gives %d" % (i, len(g.points), len(want.points))
        assert same(g.points, want.points) and same(g.normals, want.normals) and same(g.colors, want.colors), "level %d" % i
    return [len(g.points) for g in got]


@pytest.mark.parametrize("valid_only", [True, False])
@pytest.mark.parametrize("color_type", [tx.NO_COLOR, tx.RGB8, tx.GRAY32])
def test_levels_equal_the_raycasts_at_odd_sizes(volumes, color_type, valid_only):
    """70 x 50, 35 x 25 and 17 x 12: partial tiles in both directions, a level's first tile at 20 and 26"""
    sizes = check(volumes[color_type], intrinsic("70x50"), extrinsic(), 3, valid_only)
    if valid_only:
        assert sizes[0] > 800 and sizes[1] > 200 and sizes[2] > 50       # a scene, not a blank
        assert sizes[0] < 70 * 50
    else:
        assert sizes == [70 * 50, 35 * 25, 17 * 12]


@pytest.mark.parametrize("valid_only", [True, False])
def test_empty_last_level_and_one_level(volumes, valid_only):
    vol = volumes[tx.RGB8]
    sizes = check(vol, intrinsic("3x3"), extrinsic(), 3, valid_only)    # 3 x 3, 1 x 1, 0 x 0
    assert sizes[2] == 0 and (valid_only or sizes == [9, 1, 0])
    assert valid_only is False or sizes[0] > 0
    sizes = check(vol, intrinsic("70x50"), extrinsic(), 1, valid_only)
    assert len(sizes) == 1 and sizes[0] > 800
    sizes = check(vol, intrinsic("70x50"), extrinsic(), 16, valid_only)  # level 5 is 2 x 1, every later one is empty
    assert sizes[6:] == [0] * 10 and (valid_only or sizes[5] == 2)


def test_a_camera_that_sees_nothing(volumes):
    E = tx.look_at((1.2, 1.2, -0.7), (1.2, 1.2, -5.0))
    assert check(volumes[tx.RGB8], intrinsic("70x50"), E, 3, True) == [0, 0, 0]
    got = volumes[tx.RGB8].raycast_levels(intrinsic("70x50"), E, TRUNC, 3, False)
    assert [len(g.points) for g in got] == [3500, 875, 204] and all(np.isnan(to_np(g.points)).all() for g in got)


def call(vol, levels, K, E, valid_only, bufs, capacity):
    """the C ABI itself -> (status, m[16])"""
    eng = vol._eng
    k4 = (C.c_float * 4)(*K.as4())
    Et = np.ascontiguousarray(np.asarray(E, F).T)
    m = (C.c_int64 * 16)(*([-1] * 16))
    rc = eng._L.mi_icp_tsdf_raycast_levels(eng._ctx, vol._vol, levels, K.width, K.height, k4, Et.ctypes.data_as(C.c_void_p),
                                           TRUNC, int(valid_only), *[C.c_void_p(b.data_ptr()) for b in bufs], capacity, m)
    eng.synchronize()
    return rc, list(m)


@pytest.mark.parametrize("valid_only", [True, False])
def test_capacity_rule(volumes, valid_only):
    import torch
    vol, K, E = volumes[tx.GRAY32], intrinsic("70x50"), extrinsic()
    want = vol.raycast_levels(K, E, TRUNC, 3, valid_only)
    sizes = [len(g.points) for g in want]
    total = sum(sizes)
    bufs = [torch.full((total + 1, 3), -7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    rc, m = call(vol, 3, K, E, valid_only, bufs, total - 1)              # one too few: nothing written, counts filled
    assert rc == 0 and m[:3] == sizes and m[3:] == [-1] * 13
    assert all(bool((b == -7.0).all()) for b in bufs)
    rc, m = call(vol, 3, K, E, valid_only, bufs, total)                  # exactly enough
    assert rc == 0 and m[:3] == sizes
    first = 0
    for g, n in zip(want, sizes):
        for b, w in zip(bufs, (g.points, g.normals, g.colors)):
            assert same(b[first:first + n], w)
        first += n
    assert all(bool((b[total:] == -7.0).all()) for b in bufs)            # and nothing behind the last point


def test_levels_outside_the_limits_are_refused(volumes):
    import torch
    from cupoch_amd._lib import MiIcpError
    vol, K, E = volumes[tx.RGB8], intrinsic("70x50"), extrinsic()
    bufs = [torch.full((8000, 3), -7.0, dtype=torch.float32, device="cuda") for _ in range(3)]
    for levels in (0, 17, -1):
        rc, m = call(vol, levels, K, E, True, bufs, 8000)
        assert rc == -1 and m[1:] == [-1] * 15, levels                  # MI_ICP_ERR_INVALID; nothing past m[0] touched
        assert "levels" in vol._eng._L.mi_icp_last_error(vol._eng._ctx).decode()
        with pytest.raises(MiIcpError):
            vol.raycast_levels(K, E, TRUNC, levels)
    assert all(bool((b == -7.0).all()) for b in bufs)
    with pytest.raises(MiIcpError):
        vol.raycast_levels(K, E, 1e-9, 3)                                 # the march's limit, as for raycast
    rc, m = call(vol, 16, K, E, True, bufs, 8000)
    assert rc == 0 and sum(m) == sum(len(g.points) for g in vol.raycast_levels(K, E, TRUNC, 16))
