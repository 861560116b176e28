"""GPU: depth / RGB-D image -> point cloud (PointCloud::CreateFromDepthImage, CreateFromRGBDImage,
pointcloud_factory.cu:286-376) held to the numpy restatement of its contract (tests/depth_exact.py, which
test_depth_exact_cpu.py pins to the C oracle and to hand-worked images): the count and the pixel order first, then every
word of the points, normals and colours of every pixel, from numpy arrays and from device tensors.  And the KinFu pose
estimation that feeds those clouds to RegistrationICP level by level (kinfu.cpp:105-143), whose bounds are ICP's."""
import numpy as np
import pytest
import torch

import depth_exact as dx
from conftest import render_depth, small_pose
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

K = [525.0, 525.0, 319.5, 239.5]


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def to_np(v):
    return None if v is None else np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def on_device(a):
    if a is None:
        return None
    if a.dtype == np.uint16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.uint16)
    return torch.from_numpy(a).cuda()


def held(got, want, width):
    """got = (points, normals, colors) of the library, want = depth_exact.cloud's four: count and order, then every word"""
    wp, wn, wc, pix = want
    gp, gn, gc = (to_np(g) for g in got)
    assert len(gp) == len(wp), "%d points, the restatement has %d" % (len(gp), len(wp))
    for what, g, w in (("points", gp, wp), ("normals", gn, wn), ("colors", gc, wc)):
        assert (g is None) == (w is None), what
        if w is not None:
            msg = dx.difference(what, g, w, pix, width)
            assert msg is None, msg


def both_kinds(eng, d, K4, E, color, kw, want, **u16):
    """the call from numpy arrays and from device tensors: each exact, and the two the same bytes"""
    out = []
    for dev in (False, True):
        got = eng.create_from_depth(on_device(d) if dev else d, K4, E, color=(on_device(color) if dev else color), **kw, **u16)
        assert all(g is None or torch.is_tensor(g) == dev for g in got)
        held(got, want, d.shape[1])
        out.append([to_np(g) for g in got])
    for a, b in zip(*out):
        assert (a is None and b is None) or a.tobytes() == b.tobytes()


def _depth_with_defects(w=640, h=480, seed=3):
    d = render_depth(w, h, K, np.eye(4), holes=0.05, seed=seed)
    rng = np.random.default_rng(seed + 1)
    bad = rng.random(d.shape)
    d[bad < 0.01] = -1.0
    d[(bad > 0.01) & (bad < 0.02)] = np.nan
    d[(bad > 0.02) & (bad < 0.025)] = np.inf
    return d


@pytest.mark.parametrize("stride", [1, 2, 3, 7])
@pytest.mark.parametrize("with_extrinsic", [False, True])
def test_depth_image_float(eng, stride, with_extrinsic):
    d = _depth_with_defects()
    E = np.linalg.inv(small_pose(0.3, 0.5)).astype(np.float32) if with_extrinsic else None
    want = dx.cloud(d, K, E, stride=stride)
    both_kinds(eng, d, K, E, None, dict(stride=stride), want)
    assert 0 < len(want[0]) < (640 // stride) * (480 // stride)


@pytest.mark.parametrize("c", dx.depth_cases(), ids=dx.case_id)
def test_depth_form_exact(eng, c):
    """rgbd = 0 at the sizes, strides, extrinsics and intrinsics of depth_exact.depth_cases"""
    d, K4, E, kw, _ = dx.case_inputs(c, False)
    want = dx.cloud(d, K4, E, **kw)
    both_kinds(eng, d, K4, E, None, kw, want)
    assert (len(want[0]) > 0) == (c["stride"] <= c["w"])


def test_depth_image_u16_scale_and_trunc(eng):
    """values up to 65535; depth_scale and depth_trunc are held as ints (999.7 is 999, 2.9 is 2, 4.5 is 4)"""
    u = dx.u16_image()
    counts = []
    for scale, trunc in dx.U16_PARAMS:
        want = dx.cloud(dx.u16_to_float(u, scale, trunc), dx.U16_K, None)
        both_kinds(eng, u, dx.U16_K, None, None, {}, want, depth_scale=scale, depth_trunc=trunc)
        counts.append(len(want[0]))
    assert counts[0] > counts[1] > counts[3] > counts[2] > 0
    # the reference holds depth_trunc as an int: 2.9 behaves as 2
    a, _, _ = eng.create_from_depth(u, dx.U16_K, None, depth_trunc=2.9)
    b, _, _ = eng.create_from_depth(u, dx.U16_K, None, depth_trunc=2.0)
    assert len(a) > 0 and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("valid_only", [True, False])
@pytest.mark.parametrize("color_kind", ["u8", "f32", None])
def test_rgbd_image_colors_normals_cutoff(eng, valid_only, color_kind):
    d = _depth_with_defects(seed=9)
    col = dx.colors_of(color_kind, 640, 480, 5)
    E = np.linalg.inv(small_pose(0.1, 0.2)).astype(np.float32)
    kw = dict(depth_cutoff=3.0, rgbd=True, compute_normals=True, valid_only=valid_only)
    want = dx.cloud(d, K, E, color=col, **kw)
    both_kinds(eng, d, K, E, col, kw, want)
    wp, wn = want[0], want[1]
    assert (wn[:, 2] <= 0).all() and (wn != 0).any(1).sum() > len(wn) // 4    # (the scene is not mostly background)
    if valid_only:
        assert np.isfinite(wp).all() and len(wp) < 640 * 480
    else:
        assert len(wp) == 640 * 480


@pytest.mark.parametrize("c", dx.rgbd_cases(), ids=dx.case_id)
def test_rgbd_form_exact(eng, c):
    """rgbd = 1: the cross of colour x cutoff x valid_only x compute_normals at 37x23 (3 blocks + 83), KinFu's setting
    and its valid_only = 0 twin at the other sizes (70x50 crosses a block and the scan tile)"""
    d, K4, E, kw, color = dx.case_inputs(c, True)
    want = dx.cloud(d, K4, E, color=color, **kw)
    both_kinds(eng, d, K4, E, color, kw, want)


def test_last_row_and_column_conventions(eng):
    """the reference's loose bounds test (pointcloud_factory.cu:173): the right neighbour of the last column is the next
    row's first pixel, the lower neighbour of the last row is zero, a rejected neighbour counts as (0, 0, 0)"""
    images = dx.convention_images() + [(name, d, dx.HAND_K, -1.0) for name, d in dx.hand_images()]
    for name, d, K4, cutoff in images:
        for valid_only in (False, True):
            kw = dict(rgbd=True, depth_cutoff=cutoff, compute_normals=True, valid_only=valid_only)
            both_kinds(eng, d, K4, None, None, kw, dx.cloud(d, K4, None, **kw))
    d = images[0][1]
    _, n, _ = eng.create_from_depth(d, images[0][2], rgbd=True, compute_normals=True, valid_only=False)
    n = n.reshape(6, 8, 3)
    assert (n[0] == 0).all() and (n[:, 0] == 0).all()          # first row / column: zero normal
    assert (n[1:5, 1:7, 2] < 0).all()                           # interior: facing the camera
    assert np.abs(n[5, 1:7]).sum() > 0                          # last row: lower neighbour taken as zero


def test_one_engine_a_sequence(eng):
    """a large compacted call, a small uncompacted one, a middle compacted one, the large one again: no flag, position
    or staged image of an earlier call is read by a later one"""
    cases = {(c["w"], c["h"], c["valid_only"]): c for c in dx.rgbd_cases() if c["cutoff"] > 0 and c["normals"]}
    order = [cases[640, 480, True], cases[8, 6, False], cases[70, 50, True], cases[640, 480, True]]
    wants = {}
    for dev in (False, True):
        for c in order:
            d, K4, E, kw, color = dx.case_inputs(c, True)
            if dx.case_id(c) not in wants:
                wants[dx.case_id(c)] = dx.cloud(d, K4, E, color=color, **kw)
            got = eng.create_from_depth(on_device(d) if dev else d, K4, E, color=(on_device(color) if dev else color), **kw)
            held(got, wants[dx.case_id(c)], c["w"])


def test_argument_errors(eng):
    from cupoch_amd import MiIcpError
    d = np.ones((4, 4), np.float32)
    with pytest.raises(MiIcpError):
        eng.create_from_depth(d, K, stride=0)
    with pytest.raises(MiIcpError):
        eng.create_from_depth(d.astype(np.uint16), K, rgbd=True)
    with pytest.raises(MiIcpError):
        eng.create_from_depth(d, K, compute_normals=True)              # normals belong to the RGB-D form
    with pytest.raises(MiIcpError):
        eng.create_from_depth(d, K, np.zeros((4, 4), np.float32))       # singular extrinsic
    p, _, _ = eng.create_from_depth(np.zeros((4, 4), np.float32), K)
    assert len(p) == 0
    p, _, _ = eng.create_from_depth(np.zeros((0, 0), np.float32), K)
    assert len(p) == 0


def test_python_factories_and_pyramid_intrinsics():
    from cupoch_amd import camera, geometry
    intr = camera.PinholeCameraIntrinsic(640, 480, *K)
    for level in range(4):
        w, h, fx, fy, cx, cy = orc.pyramid_level_intrinsic(640, 480, *K, level)
        lv = intr.create_pyramid_level(level)
        assert (lv.width, lv.height) == (w, h)
        np.testing.assert_array_equal(np.float32(lv.as4()), np.float32([fx, fy, cx, cy]))
    d, K4 = dx.scene(70, 50, 21), dx.intrinsic_of(70, 50)
    intr = camera.PinholeCameraIntrinsic(70, 50, *[float(v) for v in K4])
    E = dx.extrinsic_of("rigid")
    pc = geometry.PointCloud.create_from_depth_image(geometry.Image(d), intr, E, 1000.0, 1000.0, 2)
    held((pc.points, None, None), dx.cloud(d, K4, E, stride=2), 70)
    assert not pc.has_normals() and not pc.has_colors() and len(pc.points) > 0
    col = dx.colors_of("u8", 70, 50, 1)
    pc = geometry.PointCloud.create_from_rgbd_image(geometry.RGBDImage(col, torch.from_numpy(d)), intr, E,
                                                    compute_normals=True, depth_cutoff=dx.CUTOFF)
    assert pc.has_normals() and pc.has_colors()
    held((pc.points, pc.normals, pc.colors),
         dx.cloud(d, K4, E, color=col, rgbd=True, compute_normals=True, depth_cutoff=dx.CUTOFF), 70)
    bad = geometry.PointCloud.create_from_depth_image(np.zeros((4, 4, 3), np.uint8), intr)
    assert bad.is_empty()


def test_kinfu_point_cloud_pyramid_exact():
    """kinfu.point_cloud_pyramid on three levels (70x50, 35x25, 17x12): each level is CreateFromRGBDImage with that
    level's intrinsic, the identity, the option's cutoff, normals, valid points only"""
    from cupoch_amd import camera, kinfu
    K4 = dx.intrinsic_of(70, 50)
    intr = camera.PinholeCameraIntrinsic(70, 50, *[float(v) for v in K4])
    sizes = [(70, 50), (35, 25), (17, 12)]
    depth = [dx.scene(w, h, 31 + i) for i, (w, h) in enumerate(sizes)]
    color = [dx.colors_of("f32", w, h, 41 + i) for i, (w, h) in enumerate(sizes)]
    opt = kinfu.KinfuOption(num_pyramid_levels=3, depth_cutoff=dx.CUTOFF)
    for cols in (color, None):
        clouds = kinfu.point_cloud_pyramid(depth, intr, opt, cols)
        assert len(clouds) == 3
        for i, (w, h) in enumerate(sizes):
            lv = intr.create_pyramid_level(i)
            assert (lv.width, lv.height) == (w, h)
            want = dx.cloud(depth[i], np.float32(lv.as4()), np.eye(4, dtype=np.float32), color=(cols[i] if cols else None),
                            rgbd=True, depth_cutoff=dx.CUTOFF, compute_normals=True)
            pc = clouds[i]
            assert pc.has_normals() and pc.has_colors() == (cols is not None) and 0 < len(want[0]) < w * h
            held((pc.points, pc.normals, pc.colors if cols else None), want, w)


def _pyramids(levels, pose_b, scale):
    """frame A at the identity pose (the 'model'), frame B at pose_b (the new frame); every
    level rendered with its own intrinsics (the half-pixel convention of CreatePyramidLevel)"""
    from cupoch_amd import camera
    intr = camera.PinholeCameraIntrinsic(640, 480, *K)
    da, db = [], []
    for i in range(levels):
        lv = intr.create_pyramid_level(i)
        da.append(render_depth(lv.width, lv.height, lv.as4(), np.eye(4), scale=scale))
        db.append(render_depth(lv.width, lv.height, lv.as4(), pose_b, scale=scale))
    return intr, da, db


@pytest.mark.parametrize("colored", [False, True])
def test_kinfu_pose_estimation_matches_oracle_and_truth(colored):
    """Scene in centimetres: the reference's fp32 colour-gradient fit is ill-conditioned at
    metre scale (tests/test_gpu_colored.py), and a tracker test should not hinge on that."""
    from cupoch_amd import kinfu, registration
    levels, S = 3, 100.0
    pose_b = small_pose(0.02, 0.03 * S)
    intr, depth_a, depth_b = _pyramids(levels, pose_b, S)
    opt = kinfu.KinfuOption(num_pyramid_levels=levels, depth_cutoff=6.0 * S, distance_threshold=0.03 * S,
                            icp_iterations=(10, 10, 10),
                            tf_type=(registration.TransformationEstimationType.ColoredICP if colored
                                     else registration.TransformationEstimationType.PointToPlane))
    cols_a = cols_b = None
    if colored:   # a smooth world-space texture, so both frames see consistent colours
        cols_a, cols_b = [], []
        for i in range(levels):
            for dd, pose, dst in ((depth_a[i], np.eye(4), cols_a), (depth_b[i], pose_b, cols_b)):
                k = intr.create_pyramid_level(i).as4()
                p, _, _ = orc.create_from_depth(dd, k, np.linalg.inv(pose), rgbd=True, valid_only=False)
                p = np.where(np.isfinite(p), p, 0.0) / S
                v = 0.5 + 0.25 * np.sin(3.0 * p[:, 0]) + 0.25 * np.cos(2.0 * p[:, 1] + p[:, 2])
                dst.append(v.astype(np.float32).reshape(dd.shape))
    model = kinfu.point_cloud_pyramid(depth_a, intr, opt, cols_a)
    frame = kinfu.point_cloud_pyramid(depth_b, intr, opt, cols_b)
    assert [len(p.points) for p in model] == [int((d > 0).sum()) for d in depth_a]
    T, ok = kinfu.pose_estimation(opt, np.eye(4, dtype=np.float32), frame, model)
    assert ok

    def err(A, B):
        D = np.asarray(A, np.float64) - np.asarray(B, np.float64)
        D[:3, 3] /= S
        return np.linalg.norm(D)
    # truth: the new frame's camera -> world pose (its points are in its camera frame);
    # a threshold as wide as the occlusion shadows (0.1 m) would bias this to 7e-3
    assert err(T, pose_b) < 2e-3
    as_dict = lambda pcs: [dict(points=p.points.cpu(), normals=p.normals.cpu(),
                                colors=(p.colors.cpu() if p.has_colors() else None)) for p in pcs]
    T_ref = orc.kinfu_pose_estimation(np.eye(4, dtype=np.float32), as_dict(frame), as_dict(model),
                                      distance_threshold=0.03 * S, icp_iterations=(10, 10, 10), colored=colored)
    assert err(T, T_ref) < 1e-4
