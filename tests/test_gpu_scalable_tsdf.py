"""integration::ScalableTSDFVolume on the GPU against the numpy fp32 restatement of its contract
(tests/scalable_tsdf_exact.py): the open units' keys and every voxel of every unit after every frame, both extractions
bit for bit in the canonical order; the open set against the GPU's own depth cloud; growth, determinism, reset, memory
kinds, error returns, the uniform volume as a second witness, and one real frame."""
import functools
import os

import numpy as np
import pytest

import scalable_tsdf_exact as sx
import tsdf_exact as tx
from conftest import ROOT

pytestmark = pytest.mark.gpu
F = np.float32
RGBD = os.path.join(ROOT, "tests", "golden", "rgbd")

# the scene of test_gpu_tsdf.py: two walls and a sphere; the walls meet at (0.9, y, 1.0)
PLANES = [((0.0, 0.0, 1.0), 1.0), ((1.0, 0.0, 0.0), 0.9)]
SPHERE = ((-0.2, 0.1, 0.7), 0.25)
IMAGES = {"70x50": (70, 50, 66.0, 64.0, 34.3, 25.1), "64x48": (64, 48, 60.0, 60.0, 31.5, 23.5)}
VOXEL = {"dyadic": (2.0 ** -6, 0.05), "0.02": (0.02, 0.06)}        # voxel_length, sdf_trunc (<= 16 * voxel_length)


def extrinsic(kind, k=0):
    """(a) identity: the wall z = 1 seen from the origin, the units straddling 0 in x and y; (b) rotated; (c) amid: the
    first frame as (b), the later ones from a camera 0.1 from both walls, inside units that frame opened, with voxels
    behind it.  Frame k of a sequence is shifted a little."""
    s = 0.03 * k
    if kind == "identity":
        E = np.eye(4, dtype=F)
        E[0, 3] = F(-s)
        return E
    if kind == "rotated" or k == 0:
        return tx.look_at((-1.0 + s, -0.4, -0.8), (0.3, 0.1, 0.6))
    return tx.look_at((0.8, 0.1 + s, 0.9), (-0.5, 0.0, 0.95))


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def same(a, b):
    """bit-equal arrays of float32, NaN positions included"""
    a, b = np.ascontiguousarray(to_np(a), F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


@functools.lru_cache(maxsize=None)
def frame(image, kind, k, color_type):
    w, h, fx, fy, cx, cy = IMAGES[image]
    E = extrinsic(kind, k)
    d, c = tx.render_scene(w, h, fx, fy, cx, cy, E, PLANES, SPHERE)
    if color_type == tx.GRAY32:
        c = np.ascontiguousarray(c[..., 0].astype(F) / F(255))
    elif color_type == tx.NO_COLOR:
        c = None
    return d, c, E


def intrinsic_of(image):
    from cupoch_amd import camera
    return camera.PinholeCameraIntrinsic(*IMAGES[image])


def gpu_volume(voxel, color_type, stride=4, map_size=1000):
    from cupoch_amd import integration, integration_scalable
    vl, trunc = VOXEL[voxel]
    return integration_scalable.ScalableTSDFVolume(vl, trunc, integration.TSDFVolumeColorType(color_type), stride, map_size)


def ref_volume(voxel, color_type, stride=4):
    vl, trunc = VOXEL[voxel]
    return sx.Volume(vl, trunc, color_type, stride)


def both(vol, ref, image, d, c, E):
    from cupoch_amd import geometry
    w, h, fx, fy, cx, cy = IMAGES[image]
    out = sx.integrate(ref, d, c, w, h, fx, fy, cx, cy, E)
    assert vol.integrate(geometry.RGBDImage(c, d), intrinsic_of(image), E) is True
    return out


def check_units(vol, ref):
    k, t, w, c = vol.get_volume_units()
    rk, rt, rw, rc = ref.arrays()
    assert k.dtype == np.int32 and np.array_equal(k, rk), "keys differ: %d against %d units" % (len(k), len(rk))
    assert vol.num_volume_units()[0] == len(rk)
    assert same(t, rt), "tsdf differs at %d voxels" % int((to_np(t) != rt).sum())
    assert same(w, rw)
    assert same(c, rc)


def check_clouds(vol, ref):
    vp, vc = sx.extract_voxel_point_cloud(ref)
    g = vol.extract_voxel_point_cloud()
    assert len(g.points) == len(vp) and not g.has_normals()
    if len(vp):
        assert same(g.points, vp) and same(g.colors, vc)
    p, n, c, idx = sx.extract_point_cloud(ref, with_index=True)
    g = vol.extract_point_cloud()
    assert len(g.points) == len(p)
    if len(p):
        assert same(g.points, p) and same(g.normals, n)
    if ref.color_type == tx.NO_COLOR:
        assert not g.has_colors()
    elif len(p):
        assert same(g.colors, c)
    return len(vp), idx


def border_facts(ref, idx):
    """per axis: surface points whose edge leaves its unit, and valid voxels on a face whose neighbour unit is not open"""
    g = sx._Grid(ref)
    crossing = [int(((idx[:, 4] == ax) & (idx[:, 1 + ax] == 15)).sum()) for ax in range(3)]
    valid = sx._valid(g.W, g.T)
    orphan = []
    for ax in range(3):
        step = np.zeros(3, np.int64)
        step[ax] = 1
        absent = g.find(g.keys.astype(np.int64) + step) < 0
        face = [slice(None)] * 4
        face[ax + 1] = 15
        orphan.append(int(valid[tuple(face)][absent].sum()))
    return crossing, orphan


CASES = [  # voxel, stride, image, camera, colour type
    ("dyadic", 4, "64x48", "identity", tx.RGB8),
    ("0.02", 3, "70x50", "rotated", tx.GRAY32),
    ("0.02", 1, "70x50", "amid", tx.NO_COLOR),
    ("dyadic", 1, "64x48", "rotated", tx.NO_COLOR),
    ("0.02", 4, "64x48", "amid", tx.RGB8),
    ("dyadic", 3, "70x50", "identity", tx.GRAY32),
]


@pytest.mark.parametrize("voxel,stride,image,kind,color_type", CASES)
def test_units_and_clouds_bit_equal(voxel, stride, image, kind, color_type):
    """After each of 3 frames the keys (ascending) and the tsdf, weight and colour of every voxel of every open unit
    equal the restatement; then both extractions in count, order and every value.  Every case has keys below and above
    0 and surface points on unit faces along every axis."""
    ref, vol = ref_volume(voxel, color_type, stride), gpu_volume(voxel, color_type, stride)
    assert vol.volume_unit_length == ref.L and vol.resolution == 16 and vol.volume_unit_voxel_num == 4096
    assert vol.depth_sampling_stride == stride
    opened, updated = [], 0
    for k in range(3):
        d, c, E = frame(image, kind, k, color_type)
        n_new, n_upd = both(vol, ref, image, d, c, E)
        opened.append(n_new)
        updated += n_upd
        check_units(vol, ref)
    keys = np.array(ref.keys())
    assert (keys.min(0) < 0).any() and (keys.min(0) < 0).sum() >= 1 and (keys.max(0) >= 0).all()
    nv, idx = check_clouds(vol, ref)
    crossing, orphan = border_facts(ref, idx)
    print("%s stride %d %s %s: units opened %s, %d voxels updated, %d valid, %d surface points, on unit faces %s, "
          "valid voxels on open faces %s" % (voxel, stride, image, kind, opened, updated, nv, len(idx), crossing, orphan))
    assert opened[0] >= 10 and updated > 0 and nv > 0 and len(idx) > 0
    assert min(crossing) > 0
    if kind == "amid":      # the later cameras sit inside open units: some of their voxels are behind the camera
        E = extrinsic(kind, 2)
        centre = (keys.astype(F) + F(0.5)) * ref.L
        z = centre @ E[2, :3] + E[2, 3]
        assert (z < 0).any() and (z > 0).any()


def test_open_set_equals_the_units_of_the_depth_cloud():
    """the keys a first frame opens are those within sdf_trunc of the points that create_from_depth_image makes on the
    GPU from the same frame with the same stride"""
    from cupoch_amd import geometry
    for voxel, stride, image, kind in (("dyadic", 4, "64x48", "rotated"), ("0.02", 3, "70x50", "identity"),
                                       ("0.02", 1, "64x48", "amid")):
        d, _, E = frame(image, kind, 1, tx.NO_COLOR)
        vol = gpu_volume(voxel, tx.NO_COLOR, stride)
        assert vol.integrate(geometry.RGBDImage(None, d), intrinsic_of(image), E)
        cloud = geometry.PointCloud.create_from_depth_image(d, intrinsic_of(image), E, 1000.0, 1000.0, stride)
        pts = to_np(cloud.points)
        w, h = IMAGES[image][:2]
        assert 0 < len(pts) <= (w // stride) * (h // stride)
        vl, trunc = VOXEL[voxel]
        want = sx.keys_of_points(pts, trunc, F(F(vl) * F(16)))
        got = vol.get_volume_units()[0]
        assert len(want) >= 10 and np.array_equal(got, np.array(want, np.int32))
        # ... and the restatement's own points are those points
        assert same(sx.depth_points(d, *IMAGES[image], E, stride), pts)


def test_later_frames_open_units_that_sort_first():
    """a second camera further along -x opens units whose keys sort before every earlier one: the read-back is still
    ascending, the earlier units keep their contents, the extractions follow the canonical order"""
    ref, vol = ref_volume("dyadic", tx.RGB8, 4), gpu_volume("dyadic", tx.RGB8, 4)
    w, h, fx, fy, cx, cy = IMAGES["64x48"]
    first = None
    for shift in (0.0, 0.7, 0.35):
        E = np.eye(4, dtype=F)
        E[0, 3] = F(shift)                                   # the camera at x = -shift
        d, c = tx.render_scene(w, h, fx, fy, cx, cy, E, PLANES, SPHERE)
        n_new, _ = both(vol, ref, "64x48", d, c, E)
        check_units(vol, ref)
        if first is None:
            first = ref.keys()
        else:
            new = [k for k in ref.keys() if k not in first]
            assert n_new == 0 or min(new) < min(first)
    assert len(ref.keys()) > len(first) and min(ref.keys()) < min(first)
    k = vol.get_volume_units()[0].astype(np.int64)
    packed = sx._pack(k)
    assert (np.diff(packed) > 0).all()
    check_clouds(vol, ref)


def test_a_face_whose_neighbour_is_not_open_emits_nothing():
    """A second frame from a camera moved along +x whose sampled pixels carry no depth opens nothing, yet updates the
    open units from the new view: valid voxels then lie on unit faces whose +axis neighbour is not open.  Those edges
    count as crossing into weight 0; units, contents and both clouds equal the restatement."""
    ref, vol = ref_volume("dyadic", tx.RGB8, 4), gpu_volume("dyadic", tx.RGB8, 4)
    w, h, fx, fy, cx, cy = IMAGES["64x48"]
    d, c, E = frame("64x48", "identity", 0, tx.RGB8)
    n0, _ = both(vol, ref, "64x48", d, c, E)
    E1 = np.eye(4, dtype=F)
    E1[0, 3] = F(-0.3)
    d1, c1 = tx.render_scene(w, h, fx, fy, cx, cy, E1, PLANES, SPHERE)
    d1[::4, ::4] = 0
    n1, upd = both(vol, ref, "64x48", d1, c1, E1)
    assert n0 >= 10 and n1 == 0 and upd > 0
    check_units(vol, ref)
    nv, idx = check_clouds(vol, ref)
    crossing, orphan = border_facts(ref, idx)
    print("valid voxels on faces whose neighbour is not open, per axis:", orphan, "surface points:", len(idx))
    assert orphan[0] > 0 and len(idx) > 0


def exact_scene():
    """the scene whose coordinate arithmetic is exact (tests/test_scalable_tsdf_cpu.py): 69 units at stride 4"""
    E = np.eye(4, dtype=F)
    E[:3, 3] = (0.125, -0.0625, 1.25)
    d, c = tx.render_scene(64, 48, 60.0, 60.0, 31.5, 23.5, E, [((0.0, 0.0, 1.0), 0.4), ((1.0, 0.0, 0.0), 0.6)],
                           ((-0.2, 0.1, 0.1), 0.25))
    return d, c, E


def test_growth_gives_what_a_large_map_gives():
    """map_size 3 against a frame of 69 units (3 -> 96 slots), then a frame that outgrows the doubled pool again (126
    units -> 192 slots): units, contents and clouds equal those of a volume made with map_size 1000, and the
    restatement"""
    from cupoch_amd import geometry
    d0, c0, E0 = exact_scene()
    E1 = tx.look_at((-1.3, -0.5, -1.6), (0.2, 0.0, 0.3))
    d1, c1 = tx.render_scene(64, 48, 60.0, 60.0, 31.5, 23.5, E1, [((0.0, 0.0, 1.0), 0.4), ((1.0, 0.0, 0.0), 0.6)],
                             ((-0.2, 0.1, 0.1), 0.25))
    K = intrinsic_of("64x48")
    small, large = gpu_volume("dyadic", tx.RGB8, 4, map_size=3), gpu_volume("dyadic", tx.RGB8, 4, map_size=1000)
    ref = ref_volume("dyadic", tx.RGB8, 4)
    assert small.num_volume_units() == (0, 3) and large.num_volume_units() == (0, 1000)
    caps = []
    for d, c, E in ((d0, c0, E0), (d1, c1, E1), (d0, c0, E0)):
        sx.integrate(ref, d, c, 64, 48, 60.0, 60.0, 31.5, 23.5, E)
        for v in (small, large):
            assert v.integrate(geometry.RGBDImage(c, d), K, E)
        check_units(small, ref)
        caps.append(small.num_volume_units())
    print("units, capacity after each frame:", caps)
    assert caps == [(69, 96), (126, 192), (126, 192)] and large.num_volume_units() == (126, 1000)
    for a, b in zip(small.get_volume_units(), large.get_volume_units()):
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
    check_clouds(small, ref)
    ps, pl = small.extract_point_cloud(), large.extract_point_cloud()
    assert same(ps.points, to_np(pl.points)) and same(ps.normals, to_np(pl.normals)) and same(ps.colors, to_np(pl.colors))


def test_empty_volumes_give_empty_clouds():
    from cupoch_amd import geometry
    vol = gpu_volume("0.02", tx.RGB8)
    for _ in range(2):
        assert len(vol.extract_point_cloud().points) == 0 and len(vol.extract_voxel_point_cloud().points) == 0
        k, t, w, c = vol.get_volume_units()
        assert k.shape == (0, 3) and t.shape == (0, 4096) and c.shape == (0, 4096, 3)
        # a frame without depth opens nothing
        d, c, E = frame("64x48", "identity", 0, tx.RGB8)
        assert vol.integrate(geometry.RGBDImage(c, np.zeros_like(d)), intrinsic_of("64x48"), E)
        assert vol.num_volume_units()[0] == 0


def test_units_without_a_crossing_give_an_empty_surface_cloud():
    """a wall through voxel centres (z = 64.5 voxels, an unrotated camera, dyadic lengths: the arithmetic is exact) gives
    tsdf 0 there and no product f0*f1 below 0: units are open and hold valid voxels, the surface cloud is empty"""
    w, h, fx, fy, cx, cy = IMAGES["64x48"]
    E = np.eye(4, dtype=F)
    d, _ = tx.render_scene(w, h, fx, fy, cx, cy, E, [((0.0, 0.0, 1.0), 64.5 / 64.0)], holes=False)
    ref, vol = ref_volume("dyadic", tx.NO_COLOR, 4), gpu_volume("dyadic", tx.NO_COLOR, 4)
    n_new, upd = both(vol, ref, "64x48", d, None, E)
    check_units(vol, ref)
    p, n, c = sx.extract_point_cloud(ref)
    g = vol.extract_point_cloud()
    assert n_new > 0 and upd > 0 and len(p) == 0 and len(g.points) == 0 and not g.has_colors()
    nv = len(sx.extract_voxel_point_cloud(ref)[0])
    assert nv > 0 and len(vol.extract_voxel_point_cloud().points) == nv


@pytest.mark.parametrize("color_type", [tx.NO_COLOR, tx.RGB8, tx.GRAY32], ids=["NoColor", "RGB8", "Gray32"])
def test_uniform_volume_agrees_voxel_for_voxel(color_type):
    """the second witness, on the GPU, that the two volumes apply one rule, for every colour type: of the exact scene's
    69 units (they depend on the depth alone) the 63 inside a UniformTSDFVolume of 128^3 equal its voxels at
    16*key + 64 bit for bit (tsdf, weight, colour; a NoColor volume reports the starting colour on both sides)"""
    from cupoch_amd import geometry, integration
    d, c, E = exact_scene()
    c = {tx.NO_COLOR: None, tx.RGB8: c, tx.GRAY32: np.ascontiguousarray(c[..., 0].astype(F))}[color_type]
    K = intrinsic_of("64x48")
    sv = gpu_volume("dyadic", color_type, 4)
    uv = integration.UniformTSDFVolume(2.0, 128, 0.05, integration.TSDFVolumeColorType(color_type), (0.0, 0.0, 0.0))
    for _ in range(2):
        assert sv.integrate(geometry.RGBDImage(c, d), K, E) and uv.integrate(geometry.RGBDImage(c, d), K, E)
    keys, t, w, col = sv.get_volume_units()
    ut, uw, uc = uv.get_voxels()
    ut, uw, uc = ut.reshape(128, 128, 128), uw.reshape(128, 128, 128), uc.reshape(128, 128, 128, 3)
    assert len(keys) == 69
    inside = 0
    for e, k in enumerate(keys):
        lo = 16 * k.astype(np.int64) + 64
        if lo.min() < 0 or lo.max() + 16 > 128:
            continue
        inside += 1
        s = tuple(slice(int(l), int(l) + 16) for l in lo)
        assert same(t[e].reshape(16, 16, 16), ut[s]) and same(w[e].reshape(16, 16, 16), uw[s])
        assert same(col[e].reshape(16, 16, 16, 3), uc[s])
    assert inside == 63


def run_frames(vol, image, kind, color_type, on_device=False):
    import torch
    from cupoch_amd import geometry
    K = intrinsic_of(image)
    for k in range(3):
        d, c, E = frame(image, kind, k, color_type)
        if on_device:
            img = geometry.RGBDImage(None if c is None else torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda())
        else:
            img = geometry.RGBDImage(c, d)
        assert vol.integrate(img, K, E)


def snapshot(vol):
    pc, vc = vol.extract_point_cloud(), vol.extract_voxel_point_cloud()
    out = [np.ascontiguousarray(a) for a in vol.get_volume_units()]
    out += [to_np(pc.points), to_np(pc.normals), to_np(pc.colors), to_np(vc.points), to_np(vc.colors)]
    return [a.tobytes() for a in out]


def test_determinism_reset_and_memory_kinds():
    """two fresh volumes fed the same frames hold the same bytes, whether the images are numpy arrays or device
    tensors; reset() and the same frames give the bytes of a fresh volume; both volumes live on one context"""
    a, b = gpu_volume("0.02", tx.RGB8, 3), gpu_volume("0.02", tx.RGB8, 3)
    assert a._eng is b._eng
    run_frames(a, "70x50", "amid", tx.RGB8)
    run_frames(b, "70x50", "amid", tx.RGB8, on_device=True)
    sa = snapshot(a)
    assert a.num_volume_units()[0] >= 10 and sa == snapshot(b)
    a.reset()
    assert a.num_volume_units() == (0, 1000) and len(a.extract_voxel_point_cloud().points) == 0
    assert snapshot(b) == sa                                # b is untouched by a's reset
    run_frames(a, "70x50", "amid", tx.RGB8)
    assert snapshot(a) == sa
    # the engine's host-side outputs (MI_ICP_HOST) equal its device-side ones
    eng = a._eng
    hp = eng.stsdf_extract_point_cloud(a._vol, True, on_device=False)
    dp = a.extract_point_cloud()
    assert isinstance(hp[0], np.ndarray) and same(dp.points, hp[0]) and same(dp.normals, hp[1]) and same(dp.colors, hp[2])
    hv = eng.stsdf_extract_voxel_point_cloud(a._vol, on_device=False)
    assert same(a.extract_voxel_point_cloud().points, hv[0])
    du = eng.stsdf_get_units(a._vol, True, on_device=True)
    for x, y in zip(du, a.get_volume_units()):
        assert to_np(x).tobytes() == y.tobytes()


def test_bad_formats_and_arguments_are_error_returns():
    import ctypes as C
    from cupoch_amd import geometry, integration, integration_scalable
    from cupoch_amd._lib import MiIcpError
    from cupoch_amd.engine import Engine
    d, c, E = frame("64x48", "identity", 0, tx.RGB8)
    K, K2 = intrinsic_of("64x48"), intrinsic_of("70x50")
    gray = np.ascontiguousarray(c[..., 0].astype(F))
    vol = gpu_volume("dyadic", tx.RGB8)
    bad = [geometry.RGBDImage(c, (d * 1000).astype(np.uint16)),          # depth not float32
           geometry.RGBDImage(c, np.stack([d, d], -1)),                   # two depth channels
           geometry.RGBDImage(gray, d),                                   # Gray32 colour into an RGB8 volume
           geometry.RGBDImage(c[:, :32], d),                              # colour size
           geometry.RGBDImage(None, d)]                                   # no colour
    for img in bad:
        assert vol.integrate(img, K, E) is False
    assert vol.integrate(geometry.RGBDImage(c, d), K2, E) is False        # sizes differ from the intrinsic's
    assert vol.num_volume_units()[0] == 0                                 # nothing was opened
    vg = gpu_volume("dyadic", tx.GRAY32)
    assert vg.integrate(geometry.RGBDImage(c, d), K, E) is False          # RGB8 colour into a Gray32 volume
    assert vg.integrate(geometry.RGBDImage(gray, d), K, E) is True
    # a bad frame after a good one leaves the volume as it was
    assert vol.integrate(geometry.RGBDImage(c, d), K, E) is True
    before = snapshot(vol)
    assert vol.integrate(geometry.RGBDImage(gray, d), K, E) is False
    singular = np.zeros((4, 4), F)
    with pytest.raises(MiIcpError):
        vol.integrate(geometry.RGBDImage(c, d), K, singular)
    assert snapshot(vol) == before
    # the constructor
    T = integration.TSDFVolumeColorType
    for args in ((0.0, 0.04, T.RGB8), (-0.01, 0.04, T.RGB8), (float("nan"), 0.04, T.RGB8), (float("inf"), 0.04, T.RGB8),
                 (0.01, 0.0, T.RGB8), (0.01, float("inf"), T.RGB8), (0.01, 0.17, T.RGB8),      # sdf_trunc > 16 voxels
                 (0.01, 0.04, T.RGB8, 0), (0.01, 0.04, T.RGB8, 4, 0)):
        with pytest.raises(MiIcpError):
            integration_scalable.ScalableTSDFVolume(*args)
    assert integration_scalable.ScalableTSDFVolume(0.01, 0.16, T.NoColor).num_volume_units() == (0, 1000)   # sdf_trunc == L
    # the C ABI: status codes, not crashes
    eng, L = vol._eng, vol._eng._L
    m = C.c_int64(-1)
    assert L.mi_icp_stsdf_extract_point_cloud(eng._ctx, None, None, None, None, 0, C.byref(m)) == -1
    other = C.c_void_p()
    assert L.mi_icp_stsdf_create(eng._ctx, 0.01, 0.04, 7, 4, 1000, C.byref(other)) == -1            # colour type
    with pytest.raises(MiIcpError):
        eng.stsdf_get_units(gpu_volume("dyadic", tx.NO_COLOR)._vol, True)                         # no colour planes
    # a volume is only accepted by the context that made it
    second = Engine(eng.device)
    try:
        with pytest.raises(MiIcpError):
            second.stsdf_reset(vol._vol)
        with pytest.raises(MiIcpError):
            second.stsdf_extract_voxel_point_cloud(vol._vol)
    finally:
        second.close()
    assert snapshot(vol) == before
    # capacity rule: too small a capacity writes nothing and reports the count
    need = C.c_int64(0)
    assert L.mi_icp_stsdf_extract_voxel_point_cloud(eng._ctx, vol._vol, None, None, 0, C.byref(need)) == 0
    assert need.value > 1
    import torch
    P = lambda t: C.c_void_p(t.data_ptr())                                # (this family's arrays are device pointers)
    buf = torch.full((need.value, 3), -7.0, dtype=torch.float32, device="cuda")
    got = C.c_int64(0)
    assert L.mi_icp_stsdf_extract_voxel_point_cloud(eng._ctx, vol._vol, P(buf), P(buf), need.value - 1, C.byref(got)) == 0
    assert got.value == need.value and bool((buf == -7.0).all())
    keys = torch.full((vol.num_volume_units()[0], 3), -7, dtype=torch.int32, device="cuda")
    assert L.mi_icp_stsdf_get_units(eng._ctx, vol._vol, P(keys), None, None, None, len(keys) - 1, C.byref(got)) == 0
    assert got.value == len(keys) and bool((keys == -7).all())
    assert L.mi_icp_stsdf_get_units(eng._ctx, vol._vol, P(keys), None, None, None, len(keys), C.byref(got)) == 0
    assert np.array_equal(keys.cpu().numpy(), vol.get_volume_units()[0])


def test_real_frame_with_the_examples_parameters():
    """Frame 0 of tests/golden/rgbd with the parameters of the reference's reconstruction example (voxel 4/512,
    sdf_trunc 0.04, RGB8, stride 4), through RGBDImage.create_from_color_and_depth: unit keys and contents exact, and
    both extractions.  The whole 640x480 frame is kept (the restatement takes about half a second); it opens 1077
    units (1081 while the depth was value / 1000: under the rule the reference's own vector pins, value * fl(1 / 1000),
    184531 of the frame's 267129 non-zero depths are one ulp larger and four fewer units are opened;
    tests/scalable_tsdf_exact.py gives both counts)."""
    from PIL import Image
    from cupoch_amd import camera, geometry, integration, integration_scalable
    raw_d = np.asarray(Image.open(os.path.join(RGBD, "depth", "00000.png")))
    raw_c = np.ascontiguousarray(np.asarray(Image.open(os.path.join(RGBD, "color", "00000.jpg")).convert("RGB")))
    rgbd = geometry.RGBDImage.create_from_color_and_depth(raw_c, raw_d, 1000.0, 4.0, False)
    d, c, E = tx.load_rgbd_frames(RGBD)[0]
    assert same(rgbd.depth, d) and np.array_equal(to_np(rgbd.color), c)
    vol = integration_scalable.ScalableTSDFVolume(4.0 / 512.0, 0.04, integration.TSDFVolumeColorType.RGB8, 4)
    ref = sx.Volume(4.0 / 512.0, 0.04, sx.RGB8, 4)
    K = camera.PinholeCameraIntrinsic(*tx.PRIMESENSE)
    n_new, upd = sx.integrate(ref, d, c, *tx.PRIMESENSE, E)
    assert vol.integrate(rgbd, K, E)
    assert n_new == 1077 and vol.num_volume_units() == (1077, 2000) and upd > 1000000
    check_units(vol, ref)
    nv, idx = check_clouds(vol, ref)
    assert nv > 100000 and len(idx) > 50000
