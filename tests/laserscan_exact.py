"""geometry::LaserScanBuffer's numeric contract (include/mi_icp.h "laserscan") restated in numpy fp32: every product
and sum is a separate float32 operation in the order the header writes it, the host tables come from math.cos /
math.sin / math.tan on Python floats, and the bin angle from float64 arctan2.  Also a pure-Python model of the ring
and the generators of inputs that meet the tests' input condition.  A helper, not a test."""
import math

import numpy as np

F = np.float32
NAN_BITS = np.uint32(0x7FC00000)
QUARTER_TURN_X = np.array([[1, 0, 0, 0], [0, 0, 1, 0], [0, -1, 0, 0], [0, 0, 0, 1]], F)


def angle_increment(min_angle, max_angle, num_steps):
    return (F(max_angle) - F(min_angle)) / F(num_steps - 1)


def cos_sin_table(min_angle, max_angle, num_steps):
    inc = angle_increment(min_angle, max_angle, num_steps)
    ang = [F(min_angle) + F(i) * inc for i in range(num_steps)]
    return (np.array([math.cos(float(a)) for a in ang], F), np.array([math.sin(float(a)) for a in ang], F))


def num_steps_for(angle_inc, min_angle, max_angle):
    return int(np.ceil((F(max_angle) - F(min_angle)) / F(angle_inc)))


# ---- scans -> points -----------------------------------------------------------------------------------------------
def to_points(ranges, intensities, origins, first_slot, num_scans, min_angle, max_angle, min_range, max_range):
    """ranges [num_max_scans, num_steps] (the raw storage), origins [num_max_scans, 4, 4] row-major -> (points [m, 3],
    colours [m, 3] or None)"""
    ranges = np.asarray(ranges, F)
    max_scans, steps = ranges.shape
    assert steps >= 2
    if not F(min_range) < F(max_range) or num_scans == 0:
        return np.zeros((0, 3), F), (None if intensities is None else np.zeros((0, 3), F))
    c, s = cos_sin_table(min_angle, max_angle, steps)
    pts, cols = [], []
    with np.errstate(all="ignore"):
        for k in range(num_scans):
            slot = (first_slot + k) % max_scans
            r = ranges[slot]
            O = np.asarray(origins[slot], F)
            keep = ~np.isnan(r) & ~(r < F(min_range)) & ~(F(max_range) < r)
            x, y = r * c, r * s
            p = np.stack([(O[q, 0] * x + O[q, 1] * y) + O[q, 3] for q in range(3)], 1).astype(F)
            keep &= np.isfinite(p).all(1)
            pts.append(p[keep])
            if intensities is not None:
                v = np.asarray(intensities, F)[slot][keep]
                cols.append(np.stack([v, v, v], 1))
    return np.concatenate(pts), (np.concatenate(cols) if intensities is not None else None)


# ---- points / depth pixels -> bins -----------------------------------------------------------------------------------
def _bin(x, y, z, angle_inc, min_h, max_h, divisions, min_range, max_range, min_angle, max_angle, steps):
    """-> bins [divisions, steps] float32: NaN, or the exact minimum range of the kept points of the bin"""
    x, y, z = (np.asarray(v, F).reshape(-1) for v in (x, y, z))
    out = np.full(divisions * steps, NAN_BITS, np.uint32)
    with np.errstate(all="ignore"):
        h_inc = (F(max_h) - F(min_h)) / F(divisions)
        rng = np.sqrt(x * x + y * y).astype(F)
        ang = np.arctan2(y.astype(np.float64), x.astype(np.float64)).astype(F)
        keep = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
        keep &= ~((rng < F(min_range)) | (rng > F(max_range)))
        keep &= ~((ang < F(min_angle)) | (ang > F(max_angle)))
        keep &= ~(z < F(min_h))
        fj = ((z - F(min_h)) / h_inc).astype(F)
        fi = ((ang - F(min_angle)) / F(angle_inc)).astype(F)
        keep &= (fj < F(2.0e9)) & (fi < F(2.0e9))
        j = np.where(keep, fj, 0).astype(np.int64)
        i = np.where(keep, fi, 0).astype(np.int64)
        keep &= (j < divisions) & (i < steps)
    # ranges are >= 0: their bit patterns order as unsigned integers, the NaN pattern above +inf's
    np.minimum.at(out, (j * steps + i)[keep], rng[keep].view(np.uint32))
    return out.view(F).reshape(divisions, steps)


def from_points(points, angle_inc, min_height, max_height, divisions=1, min_range=0.0, max_range=np.inf,
                min_angle=-np.pi, max_angle=np.pi):
    p = np.asarray(points, F).reshape(-1, 3)
    steps = num_steps_for(angle_inc, min_angle, max_angle)
    return _bin(p[:, 0], p[:, 1], p[:, 2], angle_inc, min_height, max_height, divisions, min_range, max_range, min_angle,
                max_angle, steps)


def depth_values(depth, depth_scale, depth_trunc):
    """mi_icp_create_from_depth's rule: U16 value * the correctly rounded reciprocal of (int)depth_scale, values
    >= (int)depth_trunc dropped (0)"""
    if depth.dtype == np.uint16:
        with np.errstate(all="ignore"):
            d = depth.astype(F) * F(np.float64(1.0) / np.float64(F(int(depth_scale))))
        return np.where(d >= F(int(depth_trunc)), F(0), d).astype(F)
    return np.asarray(depth, F)


def depth_scan_points(depth, intrinsic4, depth_scale=1000.0, depth_trunc=1000.0, stride=1):
    """the scan-frame point (x, -z, y) of every selected pixel and whether its depth is kept (not <= 0)"""
    fx, fy, cx, cy = (F(v) for v in intrinsic4)
    h, w = depth.shape
    rows, cols = np.arange(h // stride) * stride, np.arange(w // stride) * stride
    d = depth_values(depth, depth_scale, depth_trunc)[np.ix_(rows, cols)]
    cc, rr = np.meshgrid(cols.astype(F), rows.astype(F))
    with np.errstate(all="ignore"):
        x = ((cc - cx) * d) / fx
        y = ((rr - cy) * d) / fy
    return x.reshape(-1), (-d).reshape(-1), y.reshape(-1), ~(d <= 0).reshape(-1)


def from_depth(depth, intrinsic4, angle_inc, min_y, max_y, divisions=1, min_range=0.0, max_range=np.inf, min_angle=-np.pi,
               max_angle=np.pi, depth_scale=1000.0, depth_trunc=1000.0, stride=1):
    x, y, z, ok = depth_scan_points(depth, intrinsic4, depth_scale, depth_trunc, stride)
    steps = num_steps_for(angle_inc, min_angle, max_angle)
    return _bin(x[ok], y[ok], z[ok], angle_inc, min_y, max_y, divisions, min_range, max_range, min_angle, max_angle, steps)


def matmul4(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    out = np.empty((4, 4), F)
    for r in range(4):
        for c in range(4):
            out[r, c] = ((a[r, 0] * b[0, c] + a[r, 1] * b[1, c]) + a[r, 2] * b[2, c]) + a[r, 3] * b[3, c]
    return out


def rotate4(o, R):
    o, R = np.array(o, F), np.asarray(R, F)
    a = o[:3, :3].copy()
    for r in range(3):
        for c in range(3):
            o[r, c] = (a[r, 0] * R[0, c] + a[r, 1] * R[1, c]) + a[r, 2] * R[2, c]
    return o


def factory_origins(low, high, divisions, num_slots, left=None):
    out = np.tile(np.eye(4, dtype=F), (num_slots, 1, 1))
    for i in range(num_slots):
        out[i, 2, 3] = F(low) + ((F(high) - F(low)) * F(i)) / F(divisions)
        if left is not None:
            out[i] = matmul4(left, out[i])
    return out


# ---- the input condition of the bit-equal bin tests -------------------------------------------------------------------
def bin_fractions(x, y, z, angle_inc, min_h, max_h, divisions, min_angle):
    """in float64, from the float32 coordinates: the fractional position of every point inside its bin on the angle axis
    and on the height axis"""
    x, y, z = (np.asarray(v, np.float64) for v in (x, y, z))
    with np.errstate(all="ignore"):
        fa = (np.arctan2(y, x) - float(F(min_angle))) / float(F(angle_inc))
        fh = (z - float(F(min_h))) / (float(F(max_h) - F(min_h)) / divisions)
    return fa - np.floor(fa), fh - np.floor(fh)


def well_inside(x, y, z, angle_inc, min_h, max_h, divisions, min_angle, min_range, max_range):
    """the condition: both fractions in [0.05, 0.95] and the float64 range at least 1 % inside [min_range, max_range]"""
    fa, fh = bin_fractions(x, y, z, angle_inc, min_h, max_h, divisions, min_angle)
    r = np.hypot(np.asarray(x, np.float64), np.asarray(y, np.float64))
    lo = float(F(min_range)) * 1.01 if min_range > 0 else 0.0
    hi = float(F(max_range)) * 0.99 if np.isfinite(max_range) else np.inf
    with np.errstate(all="ignore"):
        return (fa >= 0.05) & (fa <= 0.95) & (fh >= 0.05) & (fh <= 0.95) & (r >= lo) & (r <= hi) & (r > 0 if min_range <= 0 else True)


def points_in_bins(rng, n, angle_inc, min_h, max_h, divisions, min_range, max_range, min_angle, max_angle, bins=None):
    """n float32 points generated from chosen bins (`bins`: flat indices to draw from, default all) that meet the input
    condition; asserted"""
    assert F(angle_inc) >= F(2.0 ** -9)
    steps = num_steps_for(angle_inc, min_angle, max_angle)
    span = float(F(max_angle)) - float(F(min_angle))
    inc = float(F(angle_inc))
    flat = rng.integers(0, divisions * steps, n) if bins is None else np.asarray(bins)[rng.integers(0, len(bins), n)]
    j, i = flat // steps, flat % steps
    last = span / inc - (steps - 1)                       # the last angular bin may be narrower than the others
    width = np.where(i == steps - 1, min(last, 1.0), 1.0)
    ang = float(F(min_angle)) + (i + (0.15 + 0.7 * rng.random(n)) * width) * inc
    z = float(F(min_h)) + (j + 0.15 + 0.7 * rng.random(n)) * (float(F(max_h) - F(min_h)) / divisions)
    hi = min(float(max_range), max(float(min_range), 0.5) * 20.0)
    r = float(min_range) * 1.05 + 0.02 + rng.random(n) * (hi * 0.95 - float(min_range) * 1.05 - 0.02)
    p = np.stack([r * np.cos(ang), r * np.sin(ang), z], 1).astype(F)
    ok = well_inside(p[:, 0], p[:, 1], p[:, 2], angle_inc, min_h, max_h, divisions, min_angle, min_range, max_range)
    p = p[ok]                                            # (a narrow last bin can push a point out: those are redrawn away)
    assert len(p) >= 0.9 * n, (len(p), n)
    if len(p) < n:
        p = np.concatenate([p, p[rng.integers(0, len(p), n - len(p))]]) if len(p) else p
    return np.ascontiguousarray(p)


def condition_depth(depth, intrinsic4, angle_inc, min_y, max_y, divisions, min_range, max_range, min_angle,
                    depth_scale=1000.0, depth_trunc=1000.0):
    """the depth frame with every pixel whose point misses the input condition set to 0 (both sides skip those); at least
    half of the pixels must remain"""
    x, y, z, ok = depth_scan_points(depth, intrinsic4, depth_scale, depth_trunc, 1)
    good = ok & well_inside(x, y, z, angle_inc, min_y, max_y, divisions, min_angle, min_range, max_range)
    out = np.where(good.reshape(depth.shape), depth, depth.dtype.type(0))
    assert good.sum() * 2 >= depth.size, (int(good.sum()), depth.size)
    return np.ascontiguousarray(out)


# ---- filters ---------------------------------------------------------------------------------------------------------
def range_filter(ranges, min_range, max_range):
    r = np.asarray(ranges, F)
    with np.errstate(invalid="ignore"):
        return np.where((r < F(min_range)) | (r > F(max_range)), F(np.nan), r).astype(F)


def shadow_filter(ranges, scan_min_angle, scan_max_angle, min_angle, max_angle, window, neighbors=0, remove_start=False):
    r = np.asarray(ranges, F)
    rows, steps = r.shape
    min_tan = F(abs(F(math.tan(float(F(min_angle))))))
    max_tan = F(-abs(F(math.tan(float(F(max_angle))))))
    inc = angle_increment(scan_min_angle, scan_max_angle, steps)
    out = r.copy()
    nan = F(np.nan)
    with np.errstate(all="ignore"):
        for n in range(rows):
            for i in range(steps):
                shadow = False
                for y in range(-window, window + 1):
                    j = i + y
                    if j < 0 or j >= steps or j == i:
                        continue
                    a = float(F(y) * inc)
                    py = r[n, j] * F(math.sin(a))
                    px = r[n, i] - r[n, j] * F(math.cos(a))
                    t = F(abs(py)) / px
                    if (t < min_tan) if t > 0 else (t > max_tan):
                        shadow = True
                if not shadow:
                    continue
                for index in range(max(i - neighbors, 0), min(i + neighbors, steps - 1) + 1):
                    if r[n, i] < r[n, index]:
                        out[n, index] = nan
                if remove_start:
                    out[n, i] = nan
    return out


# ---- the ring --------------------------------------------------------------------------------------------------------
class RingModel:
    """the ring's bookkeeping in plain Python: storage slots hold (ranges, origin, intensities) or None"""

    def __init__(self, num_steps, num_max_scans):
        self.num_steps, self.num_max_scans = num_steps, num_max_scans
        self.top = self.bottom = 0
        self.slots = [None] * num_max_scans

    @property
    def num_scans(self):
        return self.bottom - self.top

    def is_full(self):
        return self.num_scans == self.num_max_scans

    def add(self, ranges, origin=None, intensities=None):
        if len(ranges) != self.num_steps:
            return False
        if self.is_full():
            self.top += 1
        self.slots[self.bottom % self.num_max_scans] = (np.asarray(ranges, F), origin, intensities)
        self.bottom += 1
        return True

    def pop(self):
        if self.num_scans == 0:
            return None
        out = self.slots[self.top % self.num_max_scans]
        self.top += 1
        return out

    def live(self):
        return [self.slots[(self.top + k) % self.num_max_scans] for k in range(self.num_scans)]

    def merge(self, other):
        if other.num_scans == 0 or other.num_steps != self.num_steps or other.num_scans + self.num_scans > self.num_max_scans:
            return False
        for s in other.live():
            self.add(*s)
        return True

    def ranges(self):
        live = self.live()
        return np.concatenate([s[0] for s in live]) if live else np.zeros(0, F)


# ---- a 2-D room for the geometric checks -----------------------------------------------------------------------------
def render_room(pose_xy_yaw, half, num_steps, min_angle=-np.pi, max_angle=np.pi):
    """the scan of a square room |x| <= half, |y| <= half seen from (px, py, yaw), in float64 along the float32 step
    angles -> ranges float32 [num_steps]"""
    px, py, yaw = pose_xy_yaw
    inc = angle_increment(min_angle, max_angle, num_steps)
    out = np.empty(num_steps, F)
    for i in range(num_steps):
        a = float(F(min_angle) + F(i) * inc) + yaw
        dx, dy = math.cos(a), math.sin(a)
        best = np.inf
        for d, p in ((dx, px), (dy, py)):
            for wall in (-half, half):
                if abs(d) > 1e-12:
                    t = (wall - p) / d
                    if t > 0:
                        best = min(best, t)
        out[i] = best
    return out


def pose_matrix(px, py, yaw, z=0.0):
    c, s = math.cos(yaw), math.sin(yaw)
    return np.array([[c, -s, 0, px], [s, c, 0, py], [0, 0, 1, z], [0, 0, 0, 1]], F)
