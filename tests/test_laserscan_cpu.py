"""geometry.LaserScanBuffer without a GPU: the numpy restatement (tests/laserscan_exact.py) against plain geometry, the
ring model's bookkeeping, the Python type's names, defaults and printed errors, and the bit-order fact the bin reduction
rests on."""
import inspect
import math
import os

import numpy as np

import laserscan_exact as lx
from conftest import ROOT

F = np.float32
HALF = 4.0
POSES = [(0.0, 0.0, 0.0), (1.5, -2.0, 0.7), (-2.5, 1.0, -2.1)]


def _wall_distance(p):
    """distance of 2-D points from the square's boundary (points are inside or on it up to rounding)"""
    return np.minimum(np.abs(np.abs(p[:, 0]) - HALF), np.abs(np.abs(p[:, 1]) - HALF))


def test_room_scan_converts_to_points_on_the_walls():
    """Error budget per coordinate, u = 2^-24, r <= the room's diagonal: the rendered range is rounded once (u), the
    table entry once (u), r*c once (u); the origin's entry is a rounded cosine (u) and its product rounds (u): 5u per
    term, two terms, plus the two sums (3u): under 16 u r_max."""
    steps = 361
    store = np.stack([lx.render_room(p, HALF, steps) for p in POSES])
    origins = np.stack([lx.pose_matrix(*p, z=0.25) for p in POSES])
    pts, cols = lx.to_points(store, None, origins, 0, 3, -np.pi, np.pi, 0.0, 100.0)
    assert cols is None and pts.shape == (3 * steps, 3) and pts.dtype == F
    bound = 16 * 2.0 ** -24 * (2 * HALF * math.sqrt(2))
    assert _wall_distance(pts.astype(np.float64)).max() <= bound
    assert (pts[:, 2] == F(0.25)).all()
    for wall in (-HALF, HALF):             # every wall is seen from inside
        assert (np.abs(pts[:, 0] - wall) <= bound).any() and (np.abs(pts[:, 1] - wall) <= bound).any()


def test_points_convert_back_to_the_same_bins():
    """A scan's points, binned on a grid shifted by half a step (so that step i sits in the middle of bin i), fall into
    their own steps, and the range comes back within the rounding of x, y, the squares, the sum and the root (4 ulp)."""
    steps = 180
    r = lx.render_room(POSES[1], HALF, steps, -2.0, 2.0)
    r[10:14] = np.nan
    r[100] = np.inf
    eye = np.eye(4, dtype=F)[None]
    pts, _ = lx.to_points(r[None], None, eye, 0, 1, -2.0, 2.0, 0.0, 50.0)
    kept = np.isfinite(r)
    assert len(pts) == kept.sum()
    inc = lx.angle_increment(-2.0, 2.0, steps)
    lo, hi = F(-2.0) - inc / F(2), F(2.0) + inc / F(2)
    bins = lx.from_points(pts, inc, -1.0, 1.0, 1, 0.0, 50.0, lo, hi)[0]
    assert len(bins) in (steps, steps + 1) and np.isnan(bins[steps:]).all()
    back = bins[:steps]
    assert (np.isnan(back) == ~kept).all()
    ulp = np.abs(back[kept].view(np.int32).astype(np.int64) - r[kept].view(np.int32).astype(np.int64))
    assert ulp.max() <= 4


def test_restated_bins_take_the_exact_minimum_and_drop_what_the_contract_drops():
    args = dict(angle_inc=0.5, min_height=0.0, max_height=2.0, divisions=2, min_range=0.5, max_range=10.0, min_angle=-1.0,
                max_angle=1.0)
    pts = np.array([[3, 0.1, 0.5], [2, 0.1, 0.5], [2.5, 0.1, 0.5],     # one bin: the minimum wins whatever the order
                    [2, 0.1, 1.5],                                     # the upper division
                    [0.1, 0.0, 0.5], [20, 0, 0.5],                     # range limits
                    [-1, 0.5, 0.5],                                    # angle limits
                    [2, 0, -0.1], [2, 0, 2.5],                         # below min_height; j >= divisions
                    [np.nan, 0, 0.5], [1, np.inf, 0.5], [1, 0, -np.inf]], F)
    b = lx.from_points(pts, **args)
    steps = lx.num_steps_for(0.5, -1.0, 1.0)
    assert b.shape == (2, steps) == (2, 4)
    want = np.full((2, 4), np.nan, F)
    want[0, 2] = np.sqrt(F(2) * F(2) + F(0.1) * F(0.1))
    want[1, 2] = want[0, 2]
    assert b.tobytes() == want.tobytes()
    assert lx.from_points(pts[::-1], **args).tobytes() == b.tobytes()


def test_nan_pattern_orders_above_every_range():
    """the reduction's premise: non-negative floats order as their bit patterns, and the quiet NaN lies above +inf"""
    v = np.array([0.0, 1e-45, 1e-30, 0.5, 1.0, 3.5, 1e30, np.inf], F)
    bits = v.view(np.uint32)
    assert (np.diff(bits.astype(np.int64)) > 0).all()
    assert np.array([np.nan], F).view(np.uint32)[0] == lx.NAN_BITS == 0x7FC00000
    assert lx.NAN_BITS > bits.max() and bits.max() == 0x7F800000
    rng = np.random.default_rng(3)
    a, b = np.abs(rng.standard_normal(1000)).astype(F), np.abs(rng.standard_normal(1000)).astype(F)
    assert ((a < b) == (a.view(np.uint32) < b.view(np.uint32))).all()


def test_filters_restated():
    r = np.array([[1, 2, np.nan, 9, np.inf, 0.1]], F)
    out = lx.range_filter(r, 0.5, 5.0)
    assert np.array_equal(np.isnan(out[0]), [False, False, True, True, True, True]) and out[0, 1] == 2
    # a step edge seen at a grazing angle: the far reading next to the near surface is a shadow
    steps = 41
    r = np.full((1, steps), 2.0, F)
    r[0, 20:] = 6.0
    r[0, 20] = 4.0                                                   # the veiling reading between the two surfaces
    assert lx.shadow_filter(r, -1.0, 1.0, math.radians(10), math.radians(170), 1).tobytes() == r.tobytes()   # neighbors = 0
    out = lx.shadow_filter(r, -1.0, 1.0, math.radians(10), math.radians(170), 1, 0, True)
    assert np.isnan(out).any() and not np.isnan(out[0, :15]).any() and not np.isnan(out[0, 26:]).any()
    assert lx.shadow_filter(np.full((1, steps), 2.0, F), -1.0, 1.0, math.radians(10), math.radians(170), 2).tobytes() == \
        np.full((1, steps), 2.0, F).tobytes()


# ---- the ring --------------------------------------------------------------------------------------------------------
def _scan(k, steps=3):
    return np.full(steps, float(k), F)


def test_ring_model_add_wrap_pop_merge():
    m = lx.RingModel(3, 4)
    assert m.num_scans == 0 and not m.is_full() and m.pop() is None
    assert not m.add(np.zeros(2, F))                                  # wrong size: refused
    for k in range(6):
        assert m.add(_scan(k))
    assert (m.top, m.bottom, m.num_scans, m.is_full()) == (2, 6, 4, True)
    assert m.ranges().tolist() == [2] * 3 + [3] * 3 + [4] * 3 + [5] * 3      # oldest first across the wrap
    assert m.pop()[0].tolist() == [2, 2, 2] and m.num_scans == 3 and not m.is_full()
    assert m.ranges().tolist() == [3] * 3 + [4] * 3 + [5] * 3
    other = lx.RingModel(3, 4)
    assert not m.merge(other)                                          # empty
    other.add(_scan(7))
    other.add(_scan(8))
    assert not m.merge(other)                                          # 3 + 2 > 4
    other.pop()
    assert m.merge(other) and m.is_full()
    assert m.ranges().tolist() == [3] * 3 + [4] * 3 + [5] * 3 + [8] * 3
    assert not m.merge(lx.RingModel(5, 4))
    m.add(_scan(9))                                                    # full: the oldest goes
    assert m.ranges().tolist() == [4] * 3 + [5] * 3 + [8] * 3 + [9] * 3


# ---- the Python type (no GPU is touched) -------------------------------------------------------------------------------
def test_python_type_names_and_defaults():
    from cupoch_amd import geometry as g
    L = g.LaserScanBuffer
    for name in ("is_full", "add_ranges", "add_host_ranges", "merge", "pop_one_scan", "pop_host_one_scan", "range_filter",
                 "scan_shadow_filter", "create_from_point_cloud", "create_from_depth_image", "transform", "translate",
                 "rotate", "scale", "clear", "is_empty", "get_min_bound", "get_max_bound", "get_center",
                 "get_axis_aligned_bounding_box", "has_intensities", "get_angle_increment", "get_num_scans"):
        assert callable(getattr(L, name)), name
    for name in ("num_steps", "num_max_scans", "num_scans", "ranges", "intensities"):
        assert isinstance(inspect.getattr_static(L, name), property), name
    assert callable(g.PointCloud.create_from_laserscanbuffer)
    s = L(1081)
    assert (s.num_steps, s.num_max_scans, s.num_scans) == (1081, 10, 0)
    assert s.min_angle == float(F(-np.pi)) and s.max_angle == float(F(np.pi))     # not the reference binding's +pi
    assert s.is_empty() and not s.is_full() and not s.has_intensities()
    assert s.get_angle_increment() == float((F(np.pi) - F(-np.pi)) / F(1080))
    sig = inspect.signature(L.scan_shadow_filter).parameters
    assert sig["neighbors"].default == 0 and sig["remove_shadow_start_point"].default is False
    sig = inspect.signature(L.create_from_point_cloud).parameters
    assert (sig["num_vertical_divisions"].default, sig["min_range"].default, sig["max_range"].default) == (1, 0.0, float("inf"))
    assert (sig["min_angle"].default, sig["max_angle"].default) == (-np.pi, np.pi)
    sig = inspect.signature(L.create_from_depth_image).parameters
    assert (sig["depth_scale"].default, sig["depth_trunc"].default, sig["stride"].default) == (1000.0, 1000.0, 1)
    with open(os.path.join(ROOT, "cupoch_amd", "cpp", "include", "cupoch", "geometry", "laserscanbuffer.h")) as f:
        assert "DEFAULT_NUM_MAX_SCANS = 50" in f.read()          # the C++ default; the Python one is the binding's 10


def test_python_type_prints_errors_and_does_not_raise(capsys):
    from cupoch_amd import geometry as g
    s = g.LaserScanBuffer(5, 3)
    assert s.add_ranges([1.0, 2.0]) is s and s.num_scans == 0
    assert "[AddRanges] Invalid size of input ranges." in capsys.readouterr().err
    assert s.pop_one_scan() is None
    assert "[PopRange] Buffer is empty." in capsys.readouterr().err
    r, i = s.pop_host_one_scan()
    assert len(r) == 0 and len(i) == 0 and "[PopRange] Buffer is empty." in capsys.readouterr().err
    assert s.merge(g.LaserScanBuffer(5, 3)) is s
    assert "[Merge] Input buffer is empty." in capsys.readouterr().err
    assert np.array_equal(s.get_min_bound(), np.zeros(3)) and np.array_equal(s.get_center(), np.zeros(3))
    err = capsys.readouterr().err
    assert "LaserScanBuffer::GetMinBound is not supported" in err and "LaserScanBuffer::GetCenter is not supported" in err
    for kw, msg in ((dict(angle_increment=0.0), "angle_increment must be positive."),
                    (dict(min_height=1.0, max_height=1.0), "min_height must be smaller than max_height."),
                    (dict(min_range=2.0, max_range=1.0), "min_range must be smaller than max_range."),
                    (dict(min_angle=1.0, max_angle=-1.0), "min_angle must be smaller than max_angle.")):
        args = dict(angle_increment=0.1, min_height=0.0, max_height=1.0)
        args.update(kw)
        assert g.LaserScanBuffer.create_from_point_cloud(None, **args) is None
        assert "[LaserScanBuffer::CreateFromPointCloud] " + msg in capsys.readouterr().err
    assert g.LaserScanBuffer.create_from_depth_image(None, None, 0.1, 1.0, 0.0) is None
    assert "[LaserScanBuffer::CreateFromDepthImage] min_y must be smaller than max_y." in capsys.readouterr().err
    s.transform(np.eye(4)).translate([1, 2, 3]).rotate(np.eye(3)).scale(2.0)      # an empty buffer: host arithmetic only
    assert s.is_empty()
