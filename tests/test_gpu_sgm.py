"""GPU: imageproc.SemiGlobalMatching and PointCloud.create_from_disparity against the numpy restatement of the stereo
contract (tests/sgm_exact.py).  Semi-global matching is integer arithmetic from the census to the disparity image, so
every comparison is on the bytes: the census planes, the summed path costs S (which localises a fault to the paths) and
the final image, at the smallest sizes at which borders, the disparity range running off the left edge, the tiles of
the winner-takes-all kernel and the small-image rules can go wrong, and once at 640x480.  The cloud is compared on the
words, non-finite values in the same places."""
import copy
import functools

import numpy as np
import pytest

import sgm_exact as sx

pytestmark = pytest.mark.gpu

DEFAULTS = dict(p1=10, p2=120, uniqueness=0.95, disp_size=128, path8=True, min_disp=0, lr_max_diff=1)
CENSUS_SIZES = [(8, 6), (9, 7), (13, 7), (37, 23), (65, 17), (130, 40)]            # (width, height)
SUM_CASES = [(37, 23, 64), (65, 17, 64), (130, 40, 128), (130, 40, 256)]           # (width, height, disp_size)
FINAL_CASES = ([(w, h, dict(disp_size=d, path8=p8)) for (w, h, d) in SUM_CASES for p8 in (False, True)] +
               [(13, 7, dict(disp_size=64)), (2, 2, dict(disp_size=64)), (13, 7, {}), (2, 2, dict(disp_size=256)),
                (200, 64, dict(min_disp=3, disp_size=64)), (200, 64, dict(lr_max_diff=-1)), (200, 64, dict(lr_max_diff=0)),
                (200, 64, dict(uniqueness=1.0)), (200, 64, dict(p1=0, p2=0)), (200, 64, dict(p1=224, p2=224)),
                (200, 64, dict(min_disp=3, disp_size=64, path8=False, lr_max_diff=-1, uniqueness=1.0, p1=5, p2=60)),
                (640, 480, {})])


def case_id(c):
    return "%dx%d-%s" % (c[0], c[1], ",".join("%s=%s" % kv for kv in sorted(c[2].items())) or "defaults")


@functools.lru_cache(maxsize=None)
def images(w, h):
    return sx.pair(w, h, 3)[:2]


@functools.lru_cache(maxsize=None)
def _reference(w, h, key):
    stages = {}
    left, right = images(w, h)
    out = sx.sgm(left, right, stages=stages, **dict(key))
    return out, stages


def reference(w, h, opts):
    """(disparity image, stages) of the restatement, computed once per case and left unchanged"""
    return _reference(w, h, tuple(sorted({**DEFAULTS, **opts}.items())))


def put(a, side):
    import torch
    return a if side == "numpy" else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def matcher(w, h, opts):
    from cupoch_amd import imageproc as ip
    o = {**DEFAULTS, **opts}
    return ip.SemiGlobalMatching(ip.SGMOption(w, h, o["p1"], o["p2"], o["uniqueness"], ip.DisparitySizeType(o["disp_size"]),
                                              ip.PathType.ScanPath8 if o["path8"] else ip.PathType.ScanPath4, o["min_disp"],
                                              o["lr_max_diff"]))


def run(m, left, right, side="numpy"):
    from cupoch_amd import geometry as g
    out = m.process_frame(g.Image(put(left, side)), g.Image(put(right, side)))
    return np.ascontiguousarray(np.asarray(out))


@pytest.mark.parametrize("side", ["numpy", "cuda"])
@pytest.mark.parametrize("w,h", CENSUS_SIZES, ids=["%dx%d" % s for s in CENSUS_SIZES])
def test_census_words(w, h, side):
    from cupoch_amd import geometry as g, imageproc as ip
    for image in images(w, h):
        got = ip.census(g.Image(put(image, side))).cpu().numpy().view(np.uint32)
        want = sx.census(image)
        assert got.shape == want.shape and got.tobytes() == want.tobytes()
    if (w, h) == (8, 6):
        assert not want.any()
    if (w, h) == (9, 7):
        assert np.count_nonzero(want) <= 1 and want[3, 4] == want.max()


@pytest.mark.parametrize("path8", [False, True], ids=["path4", "path8"])
@pytest.mark.parametrize("w,h,disp_size", SUM_CASES, ids=["%dx%d-D%d" % c for c in SUM_CASES])
def test_summed_path_costs(w, h, disp_size, path8):
    opts = dict(disp_size=disp_size, path8=path8)
    want = reference(w, h, opts)[1]["S"]
    m = matcher(w, h, opts)
    run(m, *images(w, h))
    got = m.get_sums().cpu().numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "S differs at %d places, first (y, x, d) = %s: got %d, want %d" % (
        len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize("case", FINAL_CASES, ids=[case_id(c) for c in FINAL_CASES])
def test_disparity_bytes(case):
    w, h, opts = case
    want = reference(w, h, opts)[0]
    got = run(matcher(w, h, opts), *images(w, h), side="cuda" if w == 37 else "numpy")
    assert got.shape == want.shape and got.dtype == np.uint8
    bad = np.argwhere(got != want)
    assert len(bad) == 0, "%d bytes differ, first (y, x) = %s: got %d, want %d" % (
        len(bad), tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])])


def test_the_large_frame_is_matched():
    """not only equal to the restatement: the 640x480 result is the pair's disparity"""
    out = reference(640, 480, {})[0]
    truth = sx.pair(640, 480, 3)[2]
    valid = out != 255
    assert valid.mean() >= 0.90 and (np.abs(out.astype(np.int32) - truth) <= 1)[valid].mean() >= 0.95


def test_no_state_leaks_through_the_workspace():
    w, h, opts = 130, 40, dict(disp_size=128)
    a = images(w, h)
    b = tuple(np.ascontiguousarray(x[::-1, ::-1]) for x in sx.pair(w, h, 8, bg=9, fg=31)[:2])
    m = matcher(w, h, opts)
    first, second, again = run(m, *a), run(m, *b), run(m, *a)
    assert first.tobytes() == reference(w, h, opts)[0].tobytes()
    assert second.tobytes() == run(matcher(w, h, opts), *b).tobytes() == sx.sgm(*b, **{**DEFAULTS, **opts}).tobytes()
    assert second.tobytes() != first.tobytes()
    assert again.tobytes() == first.tobytes() == run(matcher(w, h, opts), *a).tobytes()


def test_the_same_frame_twice_gives_the_same_bytes():
    w, h = 200, 64
    m = matcher(w, h, {})
    one = run(m, *images(w, h))
    sums = m.get_sums().cpu().numpy().tobytes()
    two = run(m, *images(w, h), side="cuda")
    assert one.tobytes() == two.tobytes() and sums == m.get_sums().cpu().numpy().tobytes()


def test_error_paths_return_an_empty_image(capfd):
    from cupoch_amd import MiIcpError, geometry as g, imageproc as ip
    left, right = images(37, 23)
    bad = [ip.SGMOption(), ip.SGMOption(37, 0), ip.SGMOption(37, 23, p1=11, p2=10), ip.SGMOption(37, 23, p1=-1),
           ip.SGMOption(37, 23, p2=225), ip.SGMOption(37, 23, min_disp=-1),
           ip.SGMOption(37, 23, disp_size=ip.DisparitySize256, min_disp=1),
           ip.SGMOption(37, 23, disp_size=ip.DisparitySize128, min_disp=129)]
    for option in bad:
        m = ip.SemiGlobalMatching(option)
        assert "Invalid SGM parameters" in capfd.readouterr().out
        assert m.process_frame(g.Image(left), g.Image(right)).is_empty()
        assert "[SemiGlobalMatching::ProcessFrame] Invalid SGM parameters." in capfd.readouterr().out
    assert not ip.SemiGlobalMatching(ip.SGMOption(37, 23, p1=0, p2=224, disp_size=ip.DisparitySize128, min_disp=128)).process_frame(
        g.Image(left), g.Image(right)).is_empty()
    m = matcher(37, 23, dict(disp_size=64))
    other = images(65, 17)
    rgb = np.repeat(left[:, :, None], 3, axis=2)
    for a, b in ((other[0], other[1]), (left, other[1]), (rgb, right), (left, rgb), (left.astype(np.uint16), right),
                 (left, right.astype(np.float32))):
        assert m.process_frame(g.Image(a), g.Image(b)).is_empty()
        assert "[SemiGlobalMatching::ProcessFrame] Unsupport image type." in capfd.readouterr().out
    assert run(m, left, right).tobytes() == reference(37, 23, dict(disp_size=64))[0].tobytes()     # still usable
    with pytest.raises(TypeError):
        copy.copy(m)
    with pytest.raises(TypeError):
        copy.deepcopy(m)
    eng = g.get_engine()
    with pytest.raises(MiIcpError):
        eng.sgm_get_sums(eng.sgm_create(16, 16), 16, 16, 128)                # no frame yet
    assert eng.sgm_limits() == (8192, sx.MAX_P2)


CLOUD_SIZES = [(5, 3), (37, 23), (640, 480)]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16], ids=["rgb8", "rgb16"])
@pytest.mark.parametrize("w,h", CLOUD_SIZES, ids=["%dx%d" % s for s in CLOUD_SIZES])
def test_create_from_disparity_words(w, h, dtype):
    from cupoch_amd import camera, geometry as g
    rng = np.random.default_rng(w + h)
    disp = rng.integers(0, 256, (h, w)).astype(np.uint8)
    disp[0, 0] = 0
    disp[h // 2, w // 2] = 0
    color = rng.integers(0, np.iinfo(dtype).max + 1, (h, w, 3)).astype(dtype)
    # equal principal points: disparity 0 gives w = 0; then fx != fy and cx != cx_right
    for fx, fy, cx, cy, cxr, baseline in ((525.0, 525.0, 319.5, 239.5, 319.5, 0.12), (517.3, 531.9, 318.6, 255.3, 301.25, 0.0754)):
        li, ri = camera.PinholeCameraIntrinsic(w, h, fx, fy, cx, cy), camera.PinholeCameraIntrinsic(w, h, fx, fy, cxr, cy)
        want_p, want_c = sx.points_from_disparity(disp, color, fx, fy, cx, cy, cxr, baseline)
        for side in ("numpy", "cuda"):
            pc = g.PointCloud.create_from_disparity(g.Image(put(disp, side)), g.Image(put(color, side)), li, ri, baseline)
            got_p, got_c = np.asarray(pc.points.cpu()), np.asarray(pc.colors.cpu())
            assert got_p.shape == (w * h, 3) and got_c.shape == (w * h, 3)              # no compaction
            assert (np.isfinite(got_p) == np.isfinite(want_p)).all() and (np.isinf(got_p) == np.isinf(want_p)).all()
            assert sx.same_words(got_p, want_p) and sx.same_words(got_c, want_c)
        if cx == cxr:
            assert not np.isfinite(got_p[0]).all() and not np.isfinite(want_p[0]).all()
            clean = pc.remove_none_finite_points()
            assert 0 < len(np.asarray(clean.points.cpu())) < w * h


def test_create_from_disparity_turns_away_other_formats(capfd):
    from cupoch_amd import camera, geometry as g
    k = camera.PinholeCameraIntrinsic(8, 4, 500.0, 500.0, 4.0, 2.0)
    disp, color = np.zeros((4, 8), np.uint8), np.zeros((4, 8, 3), np.uint8)
    for d, c in ((disp.astype(np.uint16), color), (disp, color[:, :, 0]), (disp, color.astype(np.float32)),
                 (disp, color[:3]), (color, color), (disp, np.zeros((4, 8, 4), np.uint8))):
        pc = g.PointCloud.create_from_disparity(g.Image(d), g.Image(np.ascontiguousarray(c)), k, k, 0.1)
        assert not pc.has_points() and not pc.has_colors()
        assert "[PointCloud::CreateFromDisparity] Unsupported image format." in capfd.readouterr().out
