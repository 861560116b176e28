"""Inputs and CPU references of the exact RGB-D odometry checks (tests/test_gpu_odometry_exact.py, the oracle's
self-checks): frames that put the kernels of csrc/odometry.h on every grid regime and a large share of the pixels on
the knife edge of the correspondence rule, and what oracle/odometry_oracle.c makes of them.

  CASES                      (w, h, levels): one-pixel and sub-wave images, one block, fewer rows / columns than a 3x3
                             kernel, the last atomic grid (96 blocks) and the first row-total grid (97), odd sizes at
                             two levels, exactly kOdMaxBlocks = 512 blocks, the first capped grid (515 -> 512, some
                             threads take a second pixel) and 640x480 (1200 -> 512, 2-3 pixels per thread)
  frames(w, h, seed, init)   source colour / depth, target colour / depth
  intrinsic(w, h)            fx, fy, cx, cy
  INITS                      identity and small_pose(0.02, 0.03): warps leave the image, u_t != u_s
  case(w, h, levels, init)   the frames, the oracle's images of every level, the correspondence count and the
                             information matrix at the init (cached: computed once, shared, never written to)
  rendered(w, h)             two frames of conftest.render_rgbd's room, the second from small_pose(0.02, 0.03)
  whole_run(w, h, it, kind)  the oracle's whole run on them; asserts that the oracle itself recovers the truth

The depth is 2.0 + 0.3 sin(u/7) + 0.2 cos(v/5) plus N(0, 0.01) noise per frame; in each frame about 1% of the pixels
each are 0, NaN, -1, +inf and 9.0 (above max_depth = 4): every way PreprocessDepth can reject a pixel.  With
max_depth_diff = 0.01 the two frames' noise decides the depth test for a large share of the pixels, so one ulp in
the warp shows up as another count.

For an init other than the identity the surface has to be seen through that init, or nothing corresponds (the surface
changes by 0.04 per pixel, the test allows 0.01; measured: 1-2% of the pixels): the source's noise-free depth is then
the depth whose warp under the init lands on its target pixel's surface value (_source_surface).  At the identity
that is the surface itself.

case() asserts that the oracle keeps between 15% and 75% of the pixels as correspondences: inputs outside that range
would let a test pass without exercising the rule.  Measured: 30-43% everywhere from 16x16 up, 57-60% at 7x5.  The
(size, init) pairs in GEOMETRY cannot be in the range whatever their depth holds, each for the reason given there;
they run all the same (a call in which every warp leaves the image is an edge of its own) and case() asserts that
they are where that reason puts them.

This is a helper module of the suite, not a conftest: tests import it by name."""
import functools

import numpy as np

from conftest import render_rgbd, small_pose
from oracle import oracle as orc

F32 = np.float32
MIN_DEPTH, MAX_DEPTH, MAX_DEPTH_DIFF = 0.0, 4.0, 0.01
SHARE = (0.15, 0.75)

# blocks of a level-0 grid = ceil(w h / 256)
CASES = [(1, 1, 1), (7, 5, 1), (16, 16, 3), (2048, 3, 2), (3, 2048, 2), (192, 128, 2), (193, 128, 2), (323, 243, 3),
         (512, 256, 1), (364, 362, 2), (640, 480, 4)]
INITS = {"identity": np.eye(4, dtype=F32), "small": small_pose(0.02, 0.03)}
SEEDS = {(1, 1): 1, (7, 5): 1}        # (w, h) -> seed where the default, w * 1000 + h, does not meet the share condition
# (w, h, init) whose share the geometry decides, whatever the depth values: the range cannot be asked of them
GEOMETRY = {(1, 1, "identity"): "one pixel: the share is 0 or 1 (the seed makes it 1)",
            (1, 1, "small"): "one pixel: the share is 0 or 1 (the seed makes it 1)",
            (2048, 3, "small"): "fy = 0.82 w = 1679: the init's 0.02 shift in y moves every pixel by 17 of the 3 rows, all "
                                "warps leave the image and the call runs on zero correspondences (NaN colour mean)",
            (3, 2048, "small"): "fy = 0.82 w = 2.46 over 2048 rows is a field of view of 179.7 degrees: off the middle "
                                "rows the init's rotation multiplies the warped depth, 1.8% correspond"}


def case_id(c):
    return "%dx%d_L%d" % c


def intrinsic(w, h):
    return [0.82 * w, 0.82 * w, (w - 1) / 2.0, (h - 1) / 2.0]


def _surface(u, v):
    return 2.0 + 0.3 * np.sin(u / 7.0) + 0.2 * np.cos(v / 5.0)


def _source_surface(w, h, T0):
    """The noise-free SOURCE depth for the init T0: per source pixel the depth whose warp under T0 (the rule of
    compute_correspondence_map, in fp64) lands on its target pixel at that pixel's surface depth, found by fixed-point
    iteration; a pixel whose warp leaves the image keeps the surface's own value.  At the identity this is the
    surface itself."""
    fx, fy, cx, cy = intrinsic(w, h)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    T = np.asarray(T0, np.float64)
    KRK, Kt = K @ T[:3, :3] @ np.linalg.inv(K), K @ T[:3, 3]
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ray = np.stack([u, v, np.ones_like(u)], -1) @ KRK.T
    d = _surface(u, v)
    for _ in range(8):
        uv = d[..., None] * ray + Kt
        ut, vt = np.floor(uv[..., 0] / uv[..., 2] + 0.5), np.floor(uv[..., 1] / uv[..., 2] + 0.5)
        inside = (ut >= 0) & (ut < w) & (vt >= 0) & (vt < h)
        d = np.where(inside, d + (_surface(ut, vt) - uv[..., 2]), d)
    return d


def frames(w, h, seed, init="identity"):
    """source colour, source depth, target colour, target depth.  The target's depth is the surface, the source's the
    same surface as the init sees it (_source_surface: at the identity, the surface); then noise and invalid pixels"""
    rng = np.random.default_rng(seed)
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    depth = []
    for base in (_source_surface(w, h, INITS[init]), _surface(u, v)):
        d = base + rng.normal(0.0, 0.01, (h, w))
        r = rng.random((h, w))
        for k, bad in enumerate((0.0, np.nan, -1.0, np.inf, 9.0)):
            d[(r >= 0.01 * k) & (r < 0.01 * (k + 1))] = bad
        depth.append(np.ascontiguousarray(d, F32))
    cs = rng.random((h, w))
    ct = cs + rng.normal(0.0, 0.02, (h, w))
    return np.ascontiguousarray(cs, F32), depth[0], np.ascontiguousarray(ct, F32), depth[1]


def seed_of(w, h):
    return SEEDS.get((w, h), w * 1000 + h)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def inputs(w, h, init="identity"):
    return tuple(_frozen(a) for a in frames(w, h, seed_of(w, h), init))


@functools.lru_cache(maxsize=None)
def case(w, h, levels, init):
    """dict: frames (cs, ds, ct, dt), K, T0, images[level][which], count, share, info (at T0, zero iterations)"""
    fr = inputs(w, h, init)
    K, T0 = intrinsic(w, h), INITS[init]
    images = orc.od_images(*fr, K, T0, levels, MIN_DEPTH, MAX_DEPTH, MAX_DEPTH_DIFF)
    for lvl in images:
        for a in lvl.values():
            _frozen(a)
    K3 = [[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]]
    count = len(orc.od_correspondence(K3, T0, images[0][1], images[0][3], MAX_DEPTH_DIFF))
    share = count / float(w * h)
    if w * h == 1:
        assert share == 1.0
    elif (w, h, init) in GEOMETRY:
        assert share < SHARE[0]
    else:
        assert SHARE[0] <= share <= SHARE[1], "broken input %dx%d %s: the oracle keeps %.3f of the pixels" % (w, h, init, share)
    ok, T, info = orc.compute_rgbd_odometry(*fr, K, odo_init=T0, iterations=(0,) * levels, max_depth_diff=MAX_DEPTH_DIFF,
                                            min_depth=MIN_DEPTH, max_depth=MAX_DEPTH)
    assert ok and np.array_equal(T, T0)
    return dict(frames=fr, K=K, T0=T0, images=images, count=count, share=share, info=_frozen(info))


def same_bits(a, b):
    """None when the two float32 images have the same NaN mask and the same bits elsewhere, else what differs"""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return "shape %s != %s" % (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        y, x = np.argwhere(na != nb)[0]
        return "%d pixels NaN in one image only, first (x %d, y %d)" % (int((na != nb).sum()), x, y)
    d = (a.view(np.uint32) != b.view(np.uint32)) & ~na
    if d.any():
        y, x = np.argwhere(d)[0]
        return "%d of %d pixels differ, first (x %d, y %d): %r != %r" % (int(d.sum()), d.size, x, y, a[y, x], b[y, x])
    return None


RENDER_SEEDS = (7, 8)         # of the two frames' 2% holes
TRUTH_FACTOR = {"colour": 0.5, "hybrid": 0.1, "weighted": 0.1}    # of the motion: tests/test_gpu_odometry.py


@functools.lru_cache(maxsize=None)
def rendered(w, h):
    """(truth, K, colour a, depth a, colour b, depth b): frame b is the source, frame a the target, as in
    tests/test_gpu_odometry.py"""
    K = intrinsic(w, h)
    pose_b = small_pose(0.02, 0.03)
    with np.errstate(invalid="ignore"):
        ca, da = render_rgbd(w, h, K, np.eye(4), holes=0.02, seed=RENDER_SEEDS[0])
        cb, db = render_rgbd(w, h, K, pose_b, holes=0.02, seed=RENDER_SEEDS[1])
    return (pose_b, K) + tuple(_frozen(a) for a in (ca, da, cb, db))


@functools.lru_cache(maxsize=None)
def whole_run(w, h, iterations, kind):
    """The oracle's whole run on rendered(w, h): (ok, T, twist or None, info).  Condition, as for the share above: the
    ORACLE must itself end within 0.8 of the factor asked of the engine, or the frames cannot tell a right engine from
    a wrong one -- after so few iterations the run is in mid-convergence and where it stands depends on the holes
    (oracle alone, hybrid, 323x243 after (10, 5, 3): 0.140, 0.133, 0.079, 0.071 of the motion for the seed pairs (1, 2),
    (3, 4), (5, 6), (7, 8); 640x480 after (20, 10, 5): 0.013, 0.098, 0.014, 0.011).  An engine within 1e-4 of the oracle
    is within 0.0025 of the motion of it."""
    pose_b, K, ca, da, cb, db = rendered(w, h)
    if kind == "weighted":
        ok, T, tw, info = orc.compute_weighted_rgbd_odometry(cb, db, ca, da, K, iterations=iterations, max_depth=6.0)
    else:
        jac = orc.OD_COLOR_TERM if kind == "colour" else orc.OD_HYBRID_TERM
        ok, T, info = orc.compute_rgbd_odometry(cb, db, ca, da, K, jacobian=jac, iterations=iterations, max_depth=6.0)
        tw = None
    to_truth = np.linalg.norm(T - pose_b) / np.linalg.norm(np.eye(4) - pose_b)
    assert ok and to_truth <= 0.8 * TRUTH_FACTOR[kind], "broken input %dx%d %s: the oracle ends at %.3f of the motion" % (w, h, kind, to_truth)
    return ok, _frozen(T), tw, _frozen(info)
