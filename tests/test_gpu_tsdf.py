"""integration::UniformTSDFVolume on the GPU against the numpy fp32 restatement of its contract (tests/tsdf_exact.py):
every voxel after every frame, both extractions and every raycast pixel bit for bit; the reference's RealData values;
memory kinds, determinism, several volumes on one context, error returns, and the raycast cloud as an ICP target."""
import os

import numpy as np
import pytest

import tsdf_exact as tx
from conftest import ROOT

pytestmark = pytest.mark.gpu
F = np.float32
RGBD = os.path.join(ROOT, "tests", "golden", "rgbd")

# the scene, in world coordinates: two planes and a sphere inside a volume of edge 3
PLANES = [((0.0, 0.0, 1.0), 1.0), ((1.0, 0.0, 0.0), 0.9)]
SPHERE = ((-0.2, 0.1, 0.7), 0.25)
LENGTH, TRUNC = 3.0, 0.12
IMAGES = {"70x50": (70, 50, 66.0, 64.0, 34.3, 25.1), "64x48": (64, 48, 60.0, 60.0, 31.5, 23.5)}


def extrinsic(kind, k=0):
    """(a) identity; (b) rotated, the frustum cutting the volume's faces with columns wholly outside; (c) a camera
    inside the volume with voxels behind it.  Frame k of a sequence is shifted a little."""
    s = 0.03 * k
    if kind == "identity":
        E = np.eye(4, dtype=F)
        E[0, 3] = F(-s)
        return E
    if kind == "rotated":
        return tx.look_at((-2.4 + s, -0.9, -2.2), (0.3, 0.1, 0.6))
    return tx.look_at((0.35, 0.2 + s, -0.55), (-0.1, 0.0, 0.8))


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def same(a, b):
    """bit-equal arrays of float32, NaN positions included"""
    a, b = np.ascontiguousarray(to_np(a), F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


def gpu_volume(res, color_type, origin):
    from cupoch_amd import integration
    return integration.UniformTSDFVolume(LENGTH, res, TRUNC, integration.TSDFVolumeColorType(color_type), origin)


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


def check_voxels(vol, ref):
    t, w, c = vol.get_voxels()
    assert same(t, ref.tsdf), "tsdf differs at %d voxels" % int((to_np(t) != ref.tsdf).sum())
    assert same(w, ref.weight)
    assert same(c, ref.color)


def check_clouds(vol, ref, image, E, truncs):
    from cupoch_amd import integration
    vp, vc = tx.extract_voxel_point_cloud(ref)
    g = vol.extract_voxel_point_cloud()
    assert len(g.points) == len(vp) and same(g.points, vp) and same(g.colors, vc) and not g.has_normals()
    p, n, c = tx.extract_point_cloud(ref)
    g = vol.extract_point_cloud()
    assert len(g.points) == len(p)
    if len(p):
        assert same(g.points, p) and same(g.normals, n)
    if ref.color_type == tx.NO_COLOR:
        assert not g.has_colors()
    elif len(p):
        assert same(g.colors, c)
    w, h, fx, fy, cx, cy = IMAGES[image]
    K = intrinsic_of(image)
    hits = 0
    for trunc in truncs:
        P, N, C, _ = tx.raycast(ref, w, h, fx, fy, cx, cy, E, trunc)
        full = vol.raycast(K, E, trunc, False)
        assert same(full.points, P) and same(full.normals, N) and same(full.colors, C)
        ok = np.isfinite(P).all(1)
        cut = vol.raycast(K, E, trunc, True)
        assert len(cut.points) == int(ok.sum())
        if ok.any():
            assert same(cut.points, P[ok]) and same(cut.normals, N[ok]) and same(cut.colors, C[ok])
        hits += int(ok.sum())
    return len(vp), len(p), hits


CASES = [  # resolution, image, origin, extrinsic, colour type, frames
    (30, "70x50", (0.0, 0.0, 0.0), "identity", tx.RGB8, 1),
    (33, "64x48", (0.13, -0.07, 0.21), "rotated", tx.GRAY32, 4),
    (64, "70x50", (0.0, 0.0, 0.0), "inside", tx.NO_COLOR, 4),
    (100, "64x48", (0.13, -0.07, 0.21), "rotated", tx.RGB8, 4),
    (33, "70x50", (0.0, 0.0, 0.0), "inside", tx.RGB8, 1),
    (64, "64x48", (0.13, -0.07, 0.21), "identity", tx.GRAY32, 1),
    (100, "70x50", (0.0, 0.0, 0.0), "identity", tx.NO_COLOR, 1),
    (30, "64x48", (0.13, -0.07, 0.21), "inside", tx.NO_COLOR, 4),
    (64, "64x48", (0.0, 0.0, 0.0), "rotated", tx.RGB8, 1),
]


@pytest.mark.parametrize("res,image,origin,kind,color_type,frames", CASES)
def test_integrate_extract_raycast_bit_equal(res, image, origin, kind, color_type, frames):
    """After every frame the tsdf, weight and colour planes equal the restatement at every voxel; then both
    extractions in count, order and every value, and the raycast from the last pose at every pixel, with
    project_valid_depth_only both ways, at the volume's sdf_trunc and twice it."""
    from cupoch_amd import geometry
    ref = tx.Volume(LENGTH, res, TRUNC, color_type, origin)
    vol = gpu_volume(res, color_type, origin)
    w, h, fx, fy, cx, cy = IMAGES[image]
    K = intrinsic_of(image)
    updated = 0
    for k in range(frames):
        d, c, E = frame(image, kind, k, color_type)
        updated += tx.integrate(ref, d, c, w, h, fx, fy, cx, cy, E)
        assert vol.integrate(geometry.RGBDImage(c, d), K, E)
        check_voxels(vol, ref)
    assert updated > 0                                  # the frames do reach the volume
    nv, npnt, hits = check_clouds(vol, ref, image, E, (TRUNC, 2 * TRUNC))
    print("res %d %s %s: %d voxels updated, %d valid, %d surface points, %d raycast hits" %
          (res, image, kind, updated, nv, npnt, hits))
    assert nv > 0 and npnt > 0 and hits > 0
    vol.reset()
    ref.reset()
    check_voxels(vol, ref)
    assert len(vol.extract_point_cloud().points) == 0 and len(vol.extract_voxel_point_cloud().points) == 0


Z_CHUNK = 256      # tsdf_integrate walks a z-column in chunks of 256 voxels (one block each, four waves of 64)
TALL_CASES = [     # resolution, origin, extrinsic, frames -> (voxels updated at z >= 256 per frame, columns they lie in)
    ((257, (0.0, 0.0, -0.5), "rotated", 1), ([45350], 45350)),           # the second chunk is the single layer z = 256
    ((257, (0.0, 0.0, -0.5), "inside", 1), ([15442], 15442)),
    ((300, (0.13, -0.07, -0.4), "inside", 2), ([783443, 791964], 27774)),  # its only wave is partial: z 256..299
    ((320, (0.0, 0.0, 0.0), "inside", 1), ([513557], 30168)),            # a full second wave
]


@pytest.mark.parametrize("case,counts", TALL_CASES, ids=["%d-%s" % (c[0], c[2]) for c, _ in TALL_CASES])
def test_resolutions_above_one_z_chunk_bit_equal(case, counts):
    """Resolutions above 256 (KinfuOption's default is 512): the second z-chunk's block index, its waves' span test and
    its partial last wave.  RGB8, the 64x48 image; every voxel after every frame, then both extractions and the
    raycasts.  From the restatement alone: voxels at z >= 256 are updated (the counts were worked out with
    tests/tsdf_exact.py) and some columns have none there, so neither a chunk that never runs nor a span test that
    lets everything through or nothing could pass."""
    from cupoch_amd import geometry
    res, origin, kind, frames = case
    ref = tx.Volume(LENGTH, res, TRUNC, tx.RGB8, origin)
    vol = gpu_volume(res, tx.RGB8, origin)
    w, h, fx, fy, cx, cy = IMAGES["64x48"]
    K = intrinsic_of("64x48")
    high, touched = [], np.zeros((res, res), bool)
    for k in range(frames):
        d, c, E = frame("64x48", kind, k, tx.RGB8)
        before = ref.grid(ref.weight)[:, :, Z_CHUNK:].copy()
        tx.integrate(ref, d, c, w, h, fx, fy, cx, cy, E)
        upd = ref.grid(ref.weight)[:, :, Z_CHUNK:] != before              # (every update adds 1 to the weight)
        high.append(int(upd.sum()))
        touched |= upd.any(2)
        assert vol.integrate(geometry.RGBDImage(c, d), K, E)
        check_voxels(vol, ref)
    print("res %d %s: voxels updated at z >= 256 per frame %s, in %d of %d columns" % (res, kind, high, int(touched.sum()), res * res))
    assert min(high) > 0 and 0 < int(touched.sum()) < res * res
    assert (high, int(touched.sum())) == counts
    nv, npnt, hits = check_clouds(vol, ref, "64x48", E, (TRUNC, 2 * TRUNC))
    assert nv > 0 and npnt > 0 and hits > 0


def scene_volume(res=64, color_type=tx.RGB8, origin=(0.0, 0.0, 0.0), kinds=("rotated", "identity")):
    from cupoch_amd import geometry
    ref, vol = tx.Volume(LENGTH, res, TRUNC, color_type, origin), gpu_volume(res, color_type, origin)
    w, h, fx, fy, cx, cy = IMAGES["64x48"]
    for kind in kinds:
        d, c, E = frame("64x48", kind, 0, color_type)
        tx.integrate(ref, d, c, w, h, fx, fy, cx, cy, E)
        assert vol.integrate(geometry.RGBDImage(c, d), intrinsic_of("64x48"), E)
    return ref, vol


def raycast_both(ref, vol, K, E, trunc):
    P, N, C, _ = tx.raycast(ref, K.width, K.height, *K.as4(), E, trunc)
    g = vol.raycast(K, E, trunc, False)
    assert same(g.points, P) and same(g.normals, N) and same(g.colors, C)
    ok = np.isfinite(P).all(1)
    g = vol.raycast(K, E, trunc, True)
    assert len(g.points) == int(ok.sum())
    if ok.any():
        assert same(g.points, P[ok]) and same(g.normals, N[ok]) and same(g.colors, C[ok])
    return int(ok.sum())


def test_raycast_special_cases():
    """cx, cy integral and an unrotated camera (the central ray has two zero direction components: IEEE quotients);
    a camera outside the volume looking away (every pixel invalid); a camera inside; a pyramid-level intrinsic."""
    from cupoch_amd import camera
    ref, vol = scene_volume(origin=(0.3, 0.4, 0.2))
    K = camera.PinholeCameraIntrinsic(64, 48, 60.0, 60.0, 32.0, 24.0)
    E = np.eye(4, dtype=F)
    E[:3, 3] = (-1.0, -1.1, 0.9)                        # unrotated, at (1.0, 1.1, -0.9)
    n_axis = raycast_both(ref, vol, K, E, TRUNC)
    away = tx.look_at((-4.0, -4.0, -4.0), (-9.0, -9.0, -9.0))
    assert raycast_both(ref, vol, K, away, TRUNC) == 0
    inside = extrinsic("inside")
    n_in = raycast_both(ref, vol, K, inside, 2 * TRUNC)
    K1 = intrinsic_of("64x48").create_pyramid_level(1)
    assert (K1.width, K1.height) == (32, 24)
    n_pyr = raycast_both(ref, vol, K1, extrinsic("rotated"), TRUNC)
    print("raycast hits: axis camera %d, inside %d, pyramid level %d" % (n_axis, n_in, n_pyr))
    assert n_axis > 0 and n_in > 0 and n_pyr > 0       # none of the cases is vacuous


def test_empty_volume_gives_empty_clouds():
    vol = gpu_volume(30, tx.RGB8, (0.0, 0.0, 0.0))
    assert len(vol.extract_point_cloud().points) == 0
    assert len(vol.extract_voxel_point_cloud().points) == 0
    assert len(vol.raycast(intrinsic_of("64x48"), np.eye(4, dtype=F), TRUNC).points) == 0
    t, w, c = vol.get_voxels()
    assert not t.any() and not w.any() and (c == 1).all()


def test_real_frames_give_the_references_counts_and_colour_sums():
    """the reference's RealData test on the GPU: 4488 and 2227 points exactly, colour sums within its 0.1"""
    from cupoch_amd import camera, geometry, integration
    vol = integration.UniformTSDFVolume(8.0, 200, 0.04, integration.TSDFVolumeColorType.RGB8)
    K = camera.PinholeCameraIntrinsic(*tx.PRIMESENSE)
    for d, c, E in tx.load_rgbd_frames(RGBD):
        assert vol.integrate(geometry.RGBDImage(c, d), K, E)
    v = vol.extract_voxel_point_cloud()
    assert len(v.points) == 4488 and len(v.colors) == 4488
    assert np.abs(to_np(v.colors).astype(np.float64).sum(0) - 2096.428416).max() <= 0.1
    p = vol.extract_point_cloud()
    assert len(p.points) == 2227 and len(p.colors) == 2227 and len(p.normals) == 2227
    csum = to_np(p.colors).astype(np.float64).sum(0)
    assert np.abs(csum - np.array([1877.673116, 1862.126057, 1862.190616])).max() <= 0.1


def test_memory_kinds_and_determinism():
    """host and device images give the same volume; two runs give the same bytes"""
    import torch
    from cupoch_amd import geometry
    d, c, E = frame("70x50", "rotated", 0, tx.RGB8)
    K = intrinsic_of("70x50")
    out = []
    for on_device in (False, True, True):
        vol = gpu_volume(33, tx.RGB8, (0.1, 0.0, -0.1))
        img = geometry.RGBDImage(torch.from_numpy(c).cuda(), torch.from_numpy(d).cuda()) if on_device \
            else geometry.RGBDImage(c, d)
        assert vol.integrate(img, K, E)
        t, w, col = vol.get_voxels()
        pc, ray = vol.extract_point_cloud(), vol.raycast(K, E, TRUNC, False)
        out.append([t, w, col, to_np(pc.points), to_np(pc.normals), to_np(pc.colors), to_np(ray.points)])
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert same(a, b)
    # the engine's host-side outputs (MI_ICP_HOST) equal its device-side ones
    eng = vol._eng
    hp = eng.tsdf_extract_point_cloud(vol._vol, True, on_device=False)
    assert isinstance(hp[0], np.ndarray) and same(hp[0], out[0][3]) and same(hp[1], out[0][4]) and same(hp[2], out[0][5])
    hr = eng.tsdf_raycast(vol._vol, K.width, K.height, K.as4(), E, TRUNC, False, on_device=False)
    assert isinstance(hr[0], np.ndarray) and same(hr[0], out[0][6])
    hv = eng.tsdf_extract_voxel_point_cloud(vol._vol, on_device=False)
    assert same(hv[0], to_np(vol.extract_voxel_point_cloud().points))


def test_two_volumes_on_one_context_and_a_following_registration():
    from cupoch_amd import geometry, registration
    from conftest import make_pair
    ref_a, vol_a = scene_volume(res=33, color_type=tx.RGB8)
    ref_b, vol_b = scene_volume(res=30, color_type=tx.NO_COLOR, origin=(0.2, 0.1, 0.0), kinds=("inside",))
    assert vol_a._eng is vol_b._eng
    check_voxels(vol_a, ref_a)
    check_voxels(vol_b, ref_b)
    cloud = vol_a.extract_point_cloud()
    d = make_pair(5000, seed=3)
    src, tgt = geometry.PointCloud(d["src"]), geometry.PointCloud(d["tgt"])
    res = registration.registration_icp(src, tgt, d["max_dist"], np.eye(4, dtype=F))
    assert np.linalg.norm(np.asarray(res.transformation) - d["T_gt"]) < 1e-3
    check_voxels(vol_a, ref_a)                          # the registration left the volumes alone
    check_voxels(vol_b, ref_b)
    assert same(vol_a.extract_point_cloud().points, to_np(cloud.points))


def test_raycast_cloud_is_an_icp_target():
    """the model cloud a raycast makes registers a frame cloud of the same view onto itself"""
    from cupoch_amd import geometry, kinfu, registration
    opt = kinfu.KinfuOption(num_pyramid_levels=2, tsdf_length=LENGTH, tsdf_resolution=64, sdf_trunc=TRUNC,
                            tsdf_color_type=0, tsdf_origin=(0.3, 0.4, 0.2))
    vol = kinfu.create_volume(opt)
    K = intrinsic_of("64x48")
    E = np.eye(4, dtype=F)
    E[:3, 3] = (-1.0, -1.1, 0.9)
    d, _ = tx.render_scene(K.width, K.height, *K.as4(), E, [((0.0, 0.0, 1.0), 0.6)], holes=False)
    model = kinfu.integrate_and_raycast(vol, opt, geometry.RGBDImage(None, d), K, E)
    assert len(model) == 2 and len(model[0].points) > 100 and model[0].has_normals()
    assert len(model[1].points) > 20
    src = geometry.PointCloud(to_np(model[0].points) + np.array([0.0, 0.0, 0.01], F))
    res = registration.registration_icp(src, model[0], 0.1, np.eye(4, dtype=F),
                                        registration.TransformationEstimationPointToPlane())
    assert res.fitness > 0.9 and abs(float(np.asarray(res.transformation)[2, 3]) + 0.01) < 2e-3


def test_bad_formats_are_error_returns():
    import ctypes as C
    from cupoch_amd import geometry, integration
    from cupoch_amd._lib import MiIcpError
    d, c, E = frame("64x48", "identity", 0, tx.RGB8)
    K, K2 = intrinsic_of("64x48"), intrinsic_of("70x50")
    gray = np.ascontiguousarray(c[..., 0].astype(F))
    vol = gpu_volume(30, tx.RGB8, (0.0, 0.0, 0.0))
    bad = [geometry.RGBDImage(c, (d * 1000).astype(np.uint16)),          # depth not float32
           geometry.RGBDImage(c, np.stack([d, d], -1)),                   # two depth channels
           geometry.RGBDImage(gray, d),                                   # Gray32 colour into an RGB8 volume
           geometry.RGBDImage(c[:, :32], d),                              # colour size
           geometry.RGBDImage(None, d)]                                   # no colour
    for img in bad:
        assert vol.integrate(img, K, E) is False
    assert vol.integrate(geometry.RGBDImage(c, d), K2, E) is False        # sizes differ from the intrinsic's
    t, w, _ = vol.get_voxels()
    assert not w.any() and not t.any()                                    # nothing was integrated
    vg = gpu_volume(30, tx.GRAY32, (0.0, 0.0, 0.0))
    assert vg.integrate(geometry.RGBDImage(c, d), K, E) is False          # RGB8 colour into a Gray32 volume
    assert vg.integrate(geometry.RGBDImage(gray, d), K, E) is True
    # the C ABI: status codes, not crashes
    eng, L = vol._eng, vol._eng._L
    m = C.c_int64(-1)
    assert L.mi_icp_tsdf_extract_point_cloud(eng._ctx, None, None, None, None, 0, C.byref(m), 0) == -1
    other = C.c_void_p()
    assert L.mi_icp_tsdf_create(eng._ctx, 1.0, 2, 0.1, 0, None, C.byref(other)) == -1       # resolution < 3
    assert L.mi_icp_tsdf_create(eng._ctx, 1.0, 16, 0.0, 0, None, C.byref(other)) == -1      # sdf_trunc
    assert L.mi_icp_tsdf_create(eng._ctx, 1.0, 16, 0.1, 7, None, C.byref(other)) == -1      # colour type
    plain = gpu_volume(30, tx.NO_COLOR, (0.0, 0.0, 0.0))
    from cupoch_amd import camera
    for w, h in ((1, 40000), (40000, 2)):                               # a side beyond MI_ICP_TSDF_MAX_IMAGE_SIDE
        with pytest.raises(MiIcpError):
            vol.raycast(camera.PinholeCameraIntrinsic(w, h, 60.0, 60.0, 0.0, 0.0), E, TRUNC)
    with pytest.raises(MiIcpError):
        vol.raycast(K, E, 1e-9)                                           # a march of 2^30 steps is turned away
    with pytest.raises(MiIcpError):
        eng.tsdf_get_voxels(plain._vol, 27000, True)                      # no colour planes
    # capacity rule: too small a capacity writes nothing and reports the count
    assert vol.integrate(geometry.RGBDImage(c, d), K, E)
    need = C.c_int64(0)
    assert L.mi_icp_tsdf_extract_voxel_point_cloud(eng._ctx, vol._vol, None, None, 0, C.byref(need), 0) == 0
    assert need.value > 1
    buf = np.full((need.value, 3), -7.0, F)
    got = C.c_int64(0)
    assert L.mi_icp_tsdf_extract_voxel_point_cloud(eng._ctx, vol._vol, buf.ctypes.data_as(C.c_void_p),
                                                   buf.ctypes.data_as(C.c_void_p), need.value - 1, C.byref(got), 0) == 0
    assert got.value == need.value and (buf == -7.0).all()
