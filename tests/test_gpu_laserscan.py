"""geometry.LaserScanBuffer on the GPU, through the Python mirror and the C ABI, against the numpy restatement of the
contract (tests/laserscan_exact.py): points, colours, bins and filtered ranges equal bit for bit, the path of the bin
reduction as the library's limits say, the ring as the model keeps it, and scans -> cloud -> OccupancyGrid end to end.

The bin tests' INPUT CONDITION (not a tolerance): points are generated from chosen bins so that, in fp64, their
fractional bin position lies in [0.05, 0.95] on the angle and the height axis, their range lies 1 % inside the limits
and angle_increment >= 2^-9 rad; the margin, 0.05 * 2^-9 ~ 1e-4 rad, is some fifty times any admissible atan2f error
at |angle| <= pi, so device atan2f and the restatement's float64 arctan2 choose the same bin."""
import ctypes as C
import math

import numpy as np
import pytest

import laserscan_exact as lx

pytestmark = pytest.mark.gpu
F = np.float32
PI_F = float(F(np.pi))


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def same(a, b):
    a, b = np.ascontiguousarray(to_np(a), F), np.ascontiguousarray(b, F)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd import geometry
    return geometry.get_engine()


@pytest.fixture(scope="module")
def limits():
    from cupoch_amd.engine import Engine
    return Engine.laserscan_limits()


def dev(eng, a, cols=1):
    return eng._vg_dev(np.ascontiguousarray(a, F), F, cols)


# ---- scans -> points -------------------------------------------------------------------------------------------------
MIN_A, MAX_A, MIN_R, MAX_R = -2.1, 2.3, 0.5, 20.0


def _readings(rng, steps):
    r = rng.uniform(1.0, 15.0, steps).astype(F)
    for k, v in enumerate((np.nan, np.inf, 0.1, 25.0, MIN_R, MAX_R, -1.0)):     # the limits themselves are kept
        if steps > 7 or k < steps:
            r[(k * 5 + 1) % steps] = v
    return r


def _origin(rng, k):
    a, b = rng.uniform(-1, 1, 2)
    R = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]]) @ \
        np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    O = np.eye(4, dtype=F)
    O[:3, :3] = R
    O[:3, 3] = rng.uniform(-3, 3, 3)
    if k == 1:
        O[0, 0] = F(3e38)       # r * c * 3e38 overflows for most readings: those points are removed, the others stay
    return O


def _storage(model, steps):
    """the model's raw slots as the arrays the entry point takes"""
    n = model.num_max_scans
    r, o = np.full((n, steps), np.nan, F), np.tile(np.eye(4, dtype=F), (n, 1, 1))
    v = np.zeros((n, steps), F)
    for s, slot in enumerate(model.slots):
        if slot is not None:
            r[s], o[s] = slot[0], slot[1]
            if slot[2] is not None:
                v[s] = slot[2]
    return r, o, v


def _fill(rng, steps, max_scans, adds, pops, with_int):
    from cupoch_amd import geometry as g
    scan, model = g.LaserScanBuffer(steps, max_scans, MIN_A, MAX_A), lx.RingModel(steps, max_scans)
    for k in range(adds):
        r, O = _readings(rng, steps), _origin(rng, k)
        v = rng.random(steps).astype(F) if with_int else None
        scan.add_ranges(dev(scan._eng(), r) if k % 2 else r, O, v)      # device rows and host rows alike
        model.add(r, O, v)
    for _ in range(pops):
        scan.pop_one_scan()
        model.pop()
    return scan, model


@pytest.mark.parametrize("steps", [2, 63, 64, 65, 1081])
def test_to_points_is_bit_equal(eng, steps):
    from cupoch_amd import geometry as g
    rng = np.random.default_rng(steps)
    for max_scans, adds, pops in ((4, 1, 0), (4, 3, 0), (4, 6, 1)):          # one scan, three, a wrapped ring
        for with_int in (False, True):
            scan, model = _fill(rng, steps, max_scans, adds, pops, with_int)
            assert (scan.top_, scan.bottom_) == (model.top, model.bottom)
            r, o, v = _storage(model, steps)
            pts, cols = lx.to_points(r, v if with_int else None, o, model.top % max_scans, model.num_scans, MIN_A, MAX_A,
                                     MIN_R, MAX_R)
            cloud = g.PointCloud.create_from_laserscanbuffer(scan, MIN_R, MAX_R)
            assert len(pts) > 0 or steps == 2
            assert same(cloud.points.tensor, pts), (steps, adds, with_int)
            assert cloud.has_colors() == (with_int and len(pts) > 0)
            if with_int and len(pts):
                assert same(cloud.colors.tensor, cols)
            if adds == 3 and steps > 2:
                assert 0 < len(pts) < 3 * steps - 3 * 4                       # the overflowing origin removed points


def _raw_to_points(eng, r, o, steps, max_scans, first, num, capacity, out):
    from cupoch_amd import _lib
    m = C.c_int64(-1)
    O = np.ascontiguousarray(np.asarray(o, F).transpose(0, 2, 1))
    rc = _lib.load().mi_icp_laserscan_to_points(eng._ctx, eng._ptr(r), None, O.ctypes.data_as(C.c_void_p), steps, max_scans,
                                                first, num, MIN_A, MAX_A, MIN_R, MAX_R, eng._ptr(out), None, capacity,
                                                C.byref(m))
    return rc, int(m.value)


def test_to_points_errors(eng, capsys):
    import torch
    from cupoch_amd import geometry as g
    rng = np.random.default_rng(5)
    steps = 65
    scan, model = _fill(rng, steps, 4, 3, 0, False)
    r, o, _ = _storage(model, steps)
    want, _ = lx.to_points(r, None, o, 0, 3, MIN_A, MAX_A, MIN_R, MAX_R)
    k = len(want)
    out = torch.full((k, 3), -7.0, device=scan._ranges.device)
    rc, m = _raw_to_points(eng, scan._ranges, o, steps, 4, 0, 3, k - 1, out)   # too little room: only the count
    eng.synchronize()
    assert rc == 0 and m == k and bool((out == -7.0).all())
    rc, m = _raw_to_points(eng, scan._ranges, o, steps, 4, 0, 3, k, out)
    eng.synchronize()
    assert rc == 0 and m == k and same(out, want)
    rc, m = _raw_to_points(eng, scan._ranges, o, 1, 4 * steps, 0, 3, k, out)   # num_steps = 1
    assert rc == -1 and m == 0
    capsys.readouterr()
    assert g.PointCloud.create_from_laserscanbuffer(scan, 2.0, 2.0).is_empty()
    assert "[PointCloud::CreateFromLaserScanBuffer] min_range must be smaller than max_range." in capsys.readouterr().err
    assert g.PointCloud.create_from_laserscanbuffer(g.LaserScanBuffer(steps), 0.0, 1.0).is_empty()
    assert "Empty scan, return empty pointcloud." in capsys.readouterr().err
    rc, m = _raw_to_points(eng, scan._ranges, o, steps, 4, 0, 0, k, out)       # no live scan
    assert rc == 0 and m == 0


# ---- points -> bins --------------------------------------------------------------------------------------------------
MIN_H, MAX_H, BMIN_R, BMAX_R = -0.5, 1.5, 0.3, 30.0
MAX_STEPS = 3000      # angle_increment >= 2^-9 over the full circle allows 2 pi * 512 = 3216 steps


def _grid_with(bins, step):
    """the first bin count from `bins` on (in direction `step`) that is steps x divisions with steps <= MAX_STEPS"""
    while True:
        for div in range(1, 65):
            if bins % div == 0 and bins // div <= MAX_STEPS:
                return bins // div, div
        bins += step


def _grid(name, limits):
    if name == "7x1":
        return dict(steps=7, div=1, min_a=-1.0, max_a=1.0)
    if name == "1081x16":
        return dict(steps=1081, div=16, min_a=-np.pi, max_a=np.pi)
    steps, div = _grid_with(limits[0], -1) if name == "lds_max" else _grid_with(limits[0] + 1, 1)
    return dict(steps=steps, div=div, min_a=-np.pi, max_a=np.pi)


def _params(gr):
    inc = F((F(gr["max_a"]) - F(gr["min_a"])) / F(gr["steps"] - 0.5))
    assert lx.num_steps_for(inc, gr["min_a"], gr["max_a"]) == gr["steps"] and inc >= F(2.0 ** -9)
    return dict(angle_inc=float(inc), min_h=MIN_H, max_h=MAX_H, divisions=gr["div"], min_range=BMIN_R, max_range=BMAX_R,
                min_angle=gr["min_a"], max_angle=gr["max_a"])


def _run_bins(eng, p, pts):
    return eng.laserscan_from_points(dev(eng, pts, 3), p["angle_inc"], p["min_h"], p["max_h"], p["divisions"], p["min_range"],
                                     p["max_range"], p["min_angle"], p["max_angle"])


def _want_bins(p, pts):
    return lx.from_points(pts, p["angle_inc"], p["min_h"], p["max_h"], p["divisions"], p["min_range"], p["max_range"],
                          p["min_angle"], p["max_angle"])


@pytest.mark.parametrize("grid", ["7x1", "1081x16", "lds_max", "global_min"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 200000])
def test_from_points_is_bit_equal_on_the_expected_path(eng, limits, grid, n):
    gr = _grid(grid, limits)
    p = _params(gr)
    bins = gr["steps"] * gr["div"]
    if grid == "lds_max":
        assert bins == limits[0]
    if grid == "global_min":
        assert limits[0] < bins <= limits[0] + 4
    rng = np.random.default_rng(n + bins)
    pts = lx.points_in_bins(rng, n, **p) if n else np.zeros((0, 3), F)
    got, path = _run_bins(eng, p, pts)
    want = _want_bins(p, pts)
    assert path == (0 if bins <= limits[0] else 1)
    assert same(got, want)
    assert (~np.isnan(want)).sum() == (len(np.unique(_flat_bins(p, pts, gr["steps"]))) if n else 0)


def _flat_bins(p, pts, steps):
    fa = (np.arctan2(pts[:, 1].astype(np.float64), pts[:, 0].astype(np.float64)) - float(F(p["min_angle"]))) / float(F(p["angle_inc"]))
    fh = (pts[:, 2].astype(np.float64) - float(F(p["min_h"]))) / (float(F(p["max_h"]) - F(p["min_h"])) / p["divisions"])
    return np.floor(fh).astype(np.int64) * steps + np.floor(fa).astype(np.int64)


@pytest.mark.parametrize("grid", ["1081x16", "global_min"])
def test_from_points_contention_ties_and_determinism(eng, limits, grid):
    gr = _grid(grid, limits)
    p = _params(gr)
    rng = np.random.default_rng(77)
    one = 5 * gr["steps"] + 333
    pts = lx.points_in_bins(rng, 10000, bins=[one], **p)
    assert len(np.unique(_flat_bins(p, pts, gr["steps"]))) == 1
    low = pts[np.argmin(np.hypot(pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)))]
    pts = np.concatenate([pts[:5000], np.tile(low, (7, 1)), pts[5000:], np.tile(low, (3, 1))])       # ties on the minimum
    want = _want_bins(p, pts)
    assert (~np.isnan(want)).sum() == 1 and want.reshape(-1)[one] == np.sqrt(low[0] * low[0] + low[1] * low[1])
    a, path = _run_bins(eng, p, pts)
    b, _ = _run_bins(eng, p, pts)
    assert path == (0 if gr["steps"] * gr["div"] <= limits[0] else 1)
    assert same(a, want) and to_np(a).tobytes() == to_np(b).tobytes()


@pytest.mark.parametrize("grid", ["7x1", "global_min"])
def test_from_points_drops_what_lies_outside_one_limit_at_a_time(eng, limits, grid):
    gr = _grid(grid, limits)
    gr.update(min_a=-1.0, max_a=1.0)                      # an angular window, so that there are angles outside it
    if grid != "7x1":
        gr.update(steps=min(gr["steps"], 1000))
        gr.update(div=limits[0] // gr["steps"] + 1)
    p = _params(gr)
    rng = np.random.default_rng(9)
    base = lx.points_in_bins(rng, 600, **p)
    z = 0.5
    nan, inf = np.nan, np.inf
    out = np.array([[0.1, 0.0, z], [0.0, -0.2, z],                       # range < min_range
                    [40.0, 1.0, z], [inf, 0.0, z],                       # range > max_range; not finite
                    [math.cos(2.0) * 3, math.sin(2.0) * 3, z], [math.cos(-2.0) * 3, math.sin(-2.0) * 3, z], [-3.0, 0.0, z],
                    [2.0, 0.1, MIN_H - 0.3], [2.0, 0.1, -1e30],          # below min_height
                    [2.0, 0.1, MAX_H + 0.3], [2.0, 0.1, 1e30],           # j >= num_vertical_divisions
                    [nan, 1.0, z], [1.0, nan, z], [1.0, 0.5, nan], [1.0, inf, z], [1.0, 0.5, inf], [1.0, 0.5, -inf],
                    [-inf, 1.0, z]], F)
    pts = np.concatenate([base[:300], out, base[300:]])
    want = _want_bins(p, pts)
    assert want.tobytes() == _want_bins(p, base).tobytes()               # the restatement drops every one of them
    got, path = _run_bins(eng, p, pts)
    assert path == (0 if gr["steps"] * gr["div"] <= limits[0] else 1) and same(got, want)


def test_from_points_at_exactly_max_angle(eng):
    """atan2f(+0, -1) is pi rounded to float, which is max_angle: inside the angle limits.  With an increment that
    divides the span (pi / 256: 512 steps) its index is 512 = num_steps and the point is dropped -- the reference writes
    out of bounds there; with 1080.5 increments in the span it lands in the last bin."""
    pts = np.array([[-1.0, 0.0, 0.25], [-2.0, 0.0, 0.25]], F)
    inc = float(F(np.pi) / F(256))
    assert lx.num_steps_for(inc, -np.pi, np.pi) == 512
    got, _ = eng.laserscan_from_points(dev(eng, pts, 3), inc, 0.0, 1.0, 2)
    want = lx.from_points(pts, inc, 0.0, 1.0, 2)
    assert np.isnan(want).all() and same(got, want)
    inc = float((F(np.pi) - F(-np.pi)) / F(1080.5))
    got, _ = eng.laserscan_from_points(dev(eng, pts, 3), inc, 0.0, 1.0, 2)
    want = lx.from_points(pts, inc, 0.0, 1.0, 2)
    assert want[0, 1080] == 1.0 and (~np.isnan(want)).sum() == 1 and same(got, want)


def test_from_points_refuses_invalid_parameters(eng, limits):
    from cupoch_amd import MiIcpError
    pts = dev(eng, np.array([[1.0, 0.0, 0.5]], F), 3)
    good = dict(angle_increment=0.1, min_height=0.0, max_height=1.0, num_vertical_divisions=1, min_range=0.0, max_range=10.0,
                min_angle=-1.0, max_angle=1.0)
    assert eng.laserscan_from_points(pts, **good)[0].shape == (1, 20)
    for bad in (dict(angle_increment=0.0), dict(angle_increment=-0.1), dict(min_height=1.0), dict(min_range=10.0),
                dict(min_angle=1.0), dict(num_vertical_divisions=0), dict(angle_increment=1e-9),
                dict(num_vertical_divisions=limits[1] // 20 + 1)):
        args = dict(good)
        args.update(bad)
        with pytest.raises(MiIcpError) as e:
            eng.laserscan_from_points(pts, **args)
        assert e.value.code == -1, bad


# ---- depth -> bins ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def frames():
    import tsdf_exact as tx
    out = {}
    for (w, h) in ((64, 48), (70, 50)):
        K = (60.0, 60.0, w / 2 - 0.5, h / 2 - 0.5)
        E = np.eye(4, dtype=F)
        E[:3, 3] = (0.1, -0.05, 0.0)
        d, _ = tx.render_scene(w, h, *K, E, [((0, 0, 1), 2.2), ((1, 0, 0.3), 1.4)], sphere=((0.2, 0.1, 1.6), 0.35), holes=True)
        out[(w, h)] = (d, K)
    return out


DEPTH = dict(angle_inc=0.01, min_y=-1.0, max_y=1.2, min_range=0.4, max_range=2.6, min_angle=-2.7, max_angle=-0.4)


@pytest.mark.parametrize("size", [(64, 48), (70, 50)])
@pytest.mark.parametrize("u16", [False, True])
def test_from_depth_is_bit_equal(eng, frames, size, u16):
    import torch
    from cupoch_amd import geometry as g
    from cupoch_amd.camera import PinholeCameraIntrinsic
    d, K = frames[size]
    scale, trunc = 1000.0, 3.0
    if u16:
        d = np.round(d.astype(np.float64) * 1000.0).astype(np.uint16)
    for div in (1, 3):
        dd = lx.condition_depth(d, K, DEPTH["angle_inc"], DEPTH["min_y"], DEPTH["max_y"], div, DEPTH["min_range"],
                                DEPTH["max_range"], DEPTH["min_angle"], scale, trunc)
        t = torch.from_numpy(dd.view(np.int16) if u16 else dd).cuda()
        t = t.view(torch.uint16) if u16 else t
        for stride in (1, 4):
            want = lx.from_depth(dd, K, DEPTH["angle_inc"], DEPTH["min_y"], DEPTH["max_y"], div, DEPTH["min_range"],
                                 DEPTH["max_range"], DEPTH["min_angle"], DEPTH["max_angle"], scale, trunc, stride)
            assert (~np.isnan(want)).sum() >= 10
            scan = g.LaserScanBuffer.create_from_depth_image(
                g.Image(t), PinholeCameraIntrinsic(size[0], size[1], *K), DEPTH["angle_inc"], DEPTH["min_y"], DEPTH["max_y"], div,
                DEPTH["min_range"], DEPTH["max_range"], DEPTH["min_angle"], DEPTH["max_angle"], scale, trunc, stride)
            assert (scan.num_steps, scan.num_max_scans, scan.num_scans) == (want.shape[1], 50, div)
            assert same(scan.ranges, want.reshape(-1)), (size, u16, div, stride)
            org = lx.factory_origins(DEPTH["min_y"], DEPTH["max_y"], div, 50, lx.QUARTER_TURN_X)
            assert scan._origins.tobytes() == org.tobytes()
            for i in (0, div - 1):                      # the stated matrices: the quarter turn, the height along +y
                h = F(DEPTH["min_y"]) + ((F(DEPTH["max_y"]) - F(DEPTH["min_y"])) * F(i)) / F(div)
                assert np.array_equal(org[i], np.array([[1, 0, 0, 0], [0, 0, 1, h], [0, -1, 0, 0], [0, 0, 0, 1]], F))


def test_from_points_factory_origins_and_slots(eng):
    from cupoch_amd import geometry as g
    rng = np.random.default_rng(4)
    p = dict(angle_inc=0.02, min_h=0.0, max_h=2.0, divisions=60, min_range=0.2, max_range=9.0, min_angle=-1.5, max_angle=1.5)
    pts = lx.points_in_bins(rng, 5000, **p)
    scan = g.LaserScanBuffer.create_from_point_cloud(g.PointCloud(pts), 0.02, 0.0, 2.0, 60, 0.2, 9.0, -1.5, 1.5)
    assert (scan.num_max_scans, scan.num_scans, scan.num_steps) == (60, 60, 150)       # max(50, divisions) slots
    assert same(scan.ranges, _want_bins(p, pts).reshape(-1))
    assert scan._origins.tobytes() == lx.factory_origins(0.0, 2.0, 60, 60).tobytes()
    assert scan._origins[30, 2, 3] == F(1.0) and np.array_equal(scan._origins[30, :3, :3], np.eye(3))
    small = g.LaserScanBuffer.create_from_point_cloud(g.PointCloud(pts), 0.02, 0.0, 2.0, 2, 0.2, 9.0, -1.5, 1.5)
    assert (small.num_max_scans, small.num_scans) == (50, 2)


# ---- filters ---------------------------------------------------------------------------------------------------------
def _filter_scans(steps=200):
    rng = np.random.default_rng(21)
    a = np.linspace(-1.2, 1.2, steps)
    rows = []
    for k in range(3):                                      # three scans that differ: a wrong scan index shows
        r = (2.0 + k + 0.3 * np.sin(3 * a + k)).astype(F)
        r[40 + 10 * k:80] += F(3.0)                         # step edges
        r[120:123 + k] = F(0.4)                             # a thin near object: px <= 0 for its neighbours
        r[rng.integers(0, steps, 6)] = np.nan
        r[150 + k] = np.inf
        rows.append(r)
    return np.stack(rows)


def _filter_buffer(rows):
    from cupoch_amd import geometry as g
    scan = g.LaserScanBuffer(rows.shape[1], 3, -1.2, 1.2)
    for k, r in enumerate(rows):
        scan.add_ranges(r, lx.pose_matrix(k, -k, 0.1 * k), np.full(rows.shape[1], k, F))
    return scan


def test_range_filter_is_bit_equal_and_keeps_the_rest():
    rows = _filter_scans()
    scan = _filter_buffer(rows)
    out = scan.range_filter(1.0, 4.5)
    want = lx.range_filter(rows, 1.0, 4.5)
    assert np.isnan(want).sum() > np.isnan(rows).sum() + 10
    assert same(out.ranges, want.reshape(-1)) and same(scan.ranges, rows.reshape(-1))
    assert (out.top_, out.bottom_) == (0, 3) and out.has_intensities() and same(out.intensities, to_np(scan.intensities))
    assert out._origins.tobytes() == scan._origins.tobytes()


@pytest.mark.parametrize("window", [1, 5])
@pytest.mark.parametrize("neighbors", [0, 2])
@pytest.mark.parametrize("remove", [False, True])
def test_shadow_filter_is_bit_equal(window, neighbors, remove):
    rows = _filter_scans()
    scan = _filter_buffer(rows)
    lo, hi = math.radians(12), math.radians(168)
    out = scan.scan_shadow_filter(lo, hi, window, neighbors, remove)
    want = lx.shadow_filter(rows, -1.2, 1.2, lo, hi, window, neighbors, remove)
    if neighbors or remove:
        assert all(np.isnan(want[k]).sum() > np.isnan(rows[k]).sum() for k in range(3))
    else:
        assert want.tobytes() == rows.tobytes()
    assert same(out.ranges, want.reshape(-1)), (window, neighbors, remove)
    assert same(scan.ranges, rows.reshape(-1)) and out._origins.tobytes() == scan._origins.tobytes()


# ---- the ring and the transforms through the GPU object -----------------------------------------------------------------
def _scan_row(k, steps=3):
    return np.full(steps, float(k), F)


def test_ring_through_the_gpu_object(capsys):
    from cupoch_amd import geometry as g
    s, m = g.LaserScanBuffer(3, 4), lx.RingModel(3, 4)

    def agree():
        assert (s.top_, s.bottom_, s.num_scans, s.is_full()) == (m.top, m.bottom, m.num_scans, m.is_full())
        assert same(s.ranges, m.ranges()) and same(s.get_ranges(), m.ranges())
    agree()
    s.add_ranges(np.zeros(2, F))
    assert "[AddRanges] Invalid size of input ranges." in capsys.readouterr().err
    for k in range(6):
        s.add_ranges(_scan_row(k), intensities=_scan_row(10 + k))
        m.add(_scan_row(k))
    agree()
    assert s.has_intensities() and to_np(s.intensities).tolist() == [12] * 3 + [13] * 3 + [14] * 3 + [15] * 3
    s.add_ranges(_scan_row(9))
    assert "[AddRanges] Invalid size of intensities." in capsys.readouterr().err
    agree()
    one = s.pop_one_scan()
    assert to_np(one.ranges).tolist() == m.pop()[0].tolist() == [2, 2, 2] and one.num_scans == 1
    assert to_np(one.intensities).tolist() == [12, 12, 12]
    agree()
    other, mo = g.LaserScanBuffer(3, 4), lx.RingModel(3, 4)
    s.merge(other)
    assert "[Merge] Input buffer is empty." in capsys.readouterr().err and not m.merge(mo)
    for k in (7, 8):
        other.add_ranges(_scan_row(k), intensities=_scan_row(k))
        mo.add(_scan_row(k))
    s.merge(other)
    assert "[Merge] Buffer is full." in capsys.readouterr().err and not m.merge(mo)
    agree()
    r, v = other.pop_host_one_scan()
    mo.pop()
    assert r.tolist() == [7, 7, 7] and v.tolist() == [7, 7, 7]
    s.merge(other)
    assert m.merge(mo)
    agree()
    assert to_np(s.ranges).tolist() == [3] * 3 + [4] * 3 + [5] * 3 + [8] * 3
    s.merge(g.LaserScanBuffer(5, 4).add_ranges(np.zeros(5, F)))
    assert "[Merge] Input buffer has different num_steps." in capsys.readouterr().err
    plain = g.LaserScanBuffer(3, 4).add_ranges(_scan_row(1))
    s.merge(plain)
    assert "[Merge] Input buffer has different intensities." in capsys.readouterr().err
    s.add_ranges(_scan_row(9), intensities=_scan_row(19))
    m.add(_scan_row(9))
    agree()
    s.clear()
    assert s.is_empty() and not s.has_intensities() and len(to_np(s.ranges)) == 0


def test_transforms_then_to_points_are_bit_equal():
    from cupoch_amd import geometry as g
    rng = np.random.default_rng(8)
    steps = 90
    scan, model = _fill(rng, steps, 4, 6, 1, True)
    T = _origin(rng, 0)
    T[3] = (0, 0, 0, 1)
    R = _origin(rng, 2)[:3, :3]
    t = np.array([0.5, -1.25, 2.0], F)
    scan.transform(T).translate(t).rotate(R).scale(1.5)
    r, o, v = _storage(model, steps)
    for s in range(4):
        o[s] = lx.matmul4(o[s], T)
        o[s, :3, 3] = o[s, :3, 3] + t
        o[s] = lx.rotate4(o[s], R)
    r = (r * F(1.5)).astype(F)
    assert scan._origins.tobytes() == o.tobytes()
    pts, cols = lx.to_points(r, v, o, model.top % 4, model.num_scans, MIN_A, MAX_A, MIN_R, MAX_R)
    cloud = g.PointCloud.create_from_laserscanbuffer(scan, MIN_R, MAX_R)
    assert len(pts) > steps and same(cloud.points.tensor, pts) and same(cloud.colors.tensor, cols)


# ---- end to end ------------------------------------------------------------------------------------------------------
def test_scans_to_cloud_to_occupancy_grid():
    """a square room scanned from three poses, each scan's cloud inserted from its pose: every occupied voxel lies within
    one voxel of a wall, and every half-metre wall segment has an occupied voxel"""
    from cupoch_amd import geometry as g
    half, vs, res, steps, z = 4.05, 0.1, 128, 1441, 0.05
    poses = [(0.0, 0.0, 0.0), (1.5, -2.0, 0.7), (-2.5, 1.0, -2.1)]
    scan = g.LaserScanBuffer(steps, 10)
    for p in poses:
        scan.add_ranges(lx.render_room(p, half, steps), lx.pose_matrix(*p, z=z))
    whole = g.PointCloud.create_from_laserscanbuffer(scan, 0.0, 100.0)
    assert len(whole.points) == 3 * steps
    grid = g.OccupancyGrid(vs, res)
    for p in poses:
        cloud = g.PointCloud.create_from_laserscanbuffer(scan.pop_one_scan(), 0.0, 100.0)
        assert len(cloud.points) == steps
        grid.insert(cloud, np.array([p[0], p[1], z], F))
    idx, _ = grid.extract_occupied_voxels().cpu()
    centre = (idx - res // 2 + 0.5) * vs
    assert len(centre) > 200 and (idx[:, 2] == res // 2).all()
    wall = np.minimum(np.abs(np.abs(centre[:, 0]) - half), np.abs(np.abs(centre[:, 1]) - half))
    assert wall.max() <= vs
    for axis in (0, 1):
        for side in (-half, half):
            on = centre[np.abs(centre[:, axis] - side) <= vs]
            for lo in np.arange(-4.0, 4.0, 0.5):
                assert ((on[:, 1 - axis] >= lo) & (on[:, 1 - axis] < lo + 0.5)).any(), (axis, side, lo)
