"""The numpy restatement of integration::ScalableTSDFVolume (tests/scalable_tsdf_exact.py) checked on the CPU: against
the uniform volume's restatement, with which it shares only the per-voxel update, and for the properties of its open
rule and of its extraction across unit borders; and the Python type's surface."""
import numpy as np
import pytest

import scalable_tsdf_exact as sx
import tsdf_exact as tx

F = np.float32

# all coordinate arithmetic of this scene is exact in fp32: the voxel length and the camera's translation are dyadic
W, H, FX, FY, CX, CY = 64, 48, 60.0, 60.0, 31.5, 23.5
VL, TRUNC = 2.0 ** -6, 0.05
PLANES = [((0.0, 0.0, 1.0), 0.4), ((1.0, 0.0, 0.0), 0.6)]
SPHERE = ((-0.2, 0.1, 0.1), 0.25)


def exact_extrinsic():
    E = np.eye(4, dtype=F)
    E[:3, 3] = (0.125, -0.0625, 1.25)
    return E


@pytest.fixture(scope="module")
def pair():
    """the scene integrated twice (RGB8) into the sparse restatement and into a uniform one of 128^3"""
    E = exact_extrinsic()
    d, c = tx.render_scene(W, H, FX, FY, CX, CY, E, PLANES, SPHERE)
    sv = sx.Volume(VL, TRUNC, sx.RGB8, 4)
    uv = tx.Volume(2.0, 128, TRUNC, tx.RGB8, (0, 0, 0))
    opened = []
    for _ in range(2):
        opened.append(sx.integrate(sv, d, c, W, H, FX, FY, CX, CY, E)[0])
        tx.integrate(uv, d, c, W, H, FX, FY, CX, CY, E)
    return sv, uv, opened


def test_units_equal_the_uniform_restatement(pair):
    """stride 4 opens 69 units, all in the first frame; 63 lie inside the uniform volume, and every voxel of those is
    bit-equal (tsdf, weight, colour) to the uniform voxel at 16*key + 64"""
    sv, uv, opened = pair
    assert opened == [69, 0] and len(sv.units) == 69
    T, Wt, C = uv.grid(uv.tsdf), uv.grid(uv.weight), uv.color.reshape(128, 128, 128, 3)
    inside = touched = 0
    for k, u in sv.units.items():
        lo = [16 * k[a] + 64 for a in range(3)]
        if min(lo) < 0 or max(lo) + 16 > 128:
            continue
        inside += 1
        s = tuple(slice(l, l + 16) for l in lo)
        for a, b in ((u.grid(u.tsdf), T[s]), (u.grid(u.weight), Wt[s]), (u.color.reshape(16, 16, 16, 3), C[s])):
            assert (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all(), k
        touched += int((u.weight > 0).sum())
    assert inside == 63 and touched > 10000


def test_open_set_holds_every_unit_within_trunc_of_a_point():
    p = np.array([[0.01, 0.26, -0.01], [0.375, 0.375, 0.375]], F)
    keys = sx.keys_of_points(p, 0.05, 0.25)
    assert keys == sorted({(x, y, z) for x in (-1, 0) for y in (0, 1) for z in (-1, 0)} | {(1, 1, 1)})
    assert sx.keys_of_points(np.array([[3.0e5, 0, 0]], F), 0.05, 0.25) == []      # 1.2e6 > 2^20 - 1: not opened
    assert sx.keys_of_points(np.zeros((0, 3), F), 0.05, 0.25) == []


def test_wall_gives_points_on_the_plane_and_normals_towards_the_camera():
    E = np.eye(4, dtype=F)
    E[:3, 3] = (0.0, 0.0, 1.0)                    # camera at z = -1 looking along +z at the wall z = 0.2
    d, c = tx.render_scene(W, H, FX, FY, CX, CY, E, [((0.0, 0.0, 1.0), 0.2)], holes=False)
    sv = sx.Volume(0.02, 0.06, sx.RGB8, 2)
    for _ in range(2):
        sx.integrate(sv, d, c, W, H, FX, FY, CX, CY, E)
    keys = np.array(sv.keys())
    assert (keys[:, 0] < 0).any() and (keys[:, 0] >= 0).any()        # the units straddle 0
    p, n, col = sx.extract_point_cloud(sv)
    assert len(p) > 500 and np.abs(p[:, 2] - 0.2).max() <= 0.02
    assert (n[:, 2] < -0.9).mean() > 0.9 and np.isfinite(n).all()
    assert col.min() >= 0.0 and col.max() <= 1.0 + 4 * 2.0 ** -24      # (four roundings of a blend of bytes / 255)
    vp, vc = sx.extract_voxel_point_cloud(sv)
    assert len(vp) > len(p) and np.abs(vp[:, 2] - 0.2).max() <= 0.06 + 0.02


def two_units(second=True):
    """unit (0,0,0) with +0.5 in its last x layer and, when `second`, unit (1,0,0) with -0.5 in its first"""
    sv = sx.Volume(0.25, 1.0, sx.GRAY32, 4)
    for k, layer, val in (((0, 0, 0), 15, 0.5), ((1, 0, 0), 0, -0.5)):
        if k == (1, 0, 0) and not second:
            continue
        u = tx.Volume(sv.L, 16, sv.trunc, sx.GRAY32, [F(a) * sv.L for a in k])
        u.h = 0
        t, w = u.grid(u.tsdf), u.grid(u.weight)
        t[layer], w[layer] = F(val), F(1)
        u.color[:] = F(0.25) if val > 0 else F(0.75)
        sv.units[k] = u
    return sv


def test_an_edge_across_a_unit_border_is_found_once():
    sv = two_units()
    p, n, c = sx.extract_point_cloud(sv)
    assert len(p) == 256                                              # one per (y, z), along x only
    assert np.array_equal(p[:, 0], np.full(256, F(4.0)))              # halfway between 3.875 and 4.125
    yz = (F(0.125) + F(0.25) * np.arange(16).astype(F))
    assert np.array_equal(p[:, 1], np.repeat(yz, 16)) and np.array_equal(p[:, 2], np.tile(yz, 16))
    assert np.array_equal(c, np.full((256, 3), F(0.5)))
    inner = (p[:, 1] > 0.2) & (p[:, 1] < 3.8) & (p[:, 2] > 0.2) & (p[:, 2] < 3.8)
    assert np.array_equal(n[inner], np.tile(np.array([-1, 0, 0], F), (int(inner.sum()), 1)))
    assert len(sx.extract_voxel_point_cloud(sv)[0]) == 512


def test_a_face_whose_neighbour_is_absent_emits_nothing():
    sv = two_units(second=False)
    p, n, c = sx.extract_point_cloud(sv)
    assert len(p) == 0 and len(n) == 0 and len(c) == 0
    assert len(sx.extract_voxel_point_cloud(sv)[0]) == 256
    g = sx._Grid(sv)
    assert sx.tsdf_at(sv, g, np.array([[5.0, 1.0, 1.0]], F))[0] == 0.0           # a unit that is not open reads 0
    # between the last layer (0.5) and the absent unit (0): halfway is 0.25
    assert sx.tsdf_at(sv, g, np.array([[4.0, 1.0, 1.0]], F))[0] == F(0.25)


def test_python_type_surface():
    from cupoch_amd import integration, integration_scalable
    S = integration_scalable.ScalableTSDFVolume
    assert issubclass(S, integration.TSDFVolume)
    for name in ("reset", "integrate", "extract_point_cloud", "extract_voxel_point_cloud", "get_volume_units"):
        assert callable(getattr(S, name))
    for name in ("extract_triangle_mesh", "raycast", "integrate_with_depth_to_camera_distance_multiplier"):
        assert not hasattr(S, name)                                    # not built, and said so
    assert "integration_scalable" in integration.__doc__               # where the uniform volume's module points
