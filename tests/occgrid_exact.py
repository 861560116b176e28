"""geometry::OccupancyGrid restated in numpy fp32: the numeric contract of include/mi_icp.h (mi_icp_occgrid_*), step by
step in the order written there, vectorised over the rays with a masked loop for the walk.  The kernels are held to it
bit for bit.  Nothing here reads the product."""
import numpy as np

F = np.float32
MAX_NDIV = 4096            # MI_ICP_OCCGRID_MAX_NDIV
MAX_RESOLUTION = 1024      # MI_ICP_OCCGRID_MAX_RESOLUTION
KNOWN, FREE, OCCUPIED = 0, 1, 2


class Refused(ValueError):
    """what the C ABI answers with MI_ICP_ERR_INVALID; the grid is unchanged"""


def floor_int(x):
    """floor to int with the value held inside +-1e9 first (NaN -> -1e9)"""
    x = np.floor(np.asarray(x, F))
    x = np.where(np.isnan(x), F(-1.0e9), x)
    return np.clip(x, F(-1.0e9), F(1.0e9)).astype(np.int64)


class Grid:
    def __init__(self, voxel_size=0.05, resolution=512, origin=(0.0, 0.0, 0.0), dense=True):
        if resolution < 2 or resolution > MAX_RESOLUTION:
            raise Refused("resolution")
        self.voxel_size = F(voxel_size)
        self.resolution = int(resolution)
        self.origin = np.asarray(origin, F).reshape(3).copy()
        self.clamping_thres_min, self.clamping_thres_max = F(-2.0), F(3.5)
        self.prob_hit_log, self.prob_miss_log, self.occ_prob_thres_log = F(0.85), F(-0.4), F(0.0)
        self.h = self.resolution // 2
        # dense: the whole plane; else a dict linear index -> log-odds (the reference's scenarios at 512^3 on the CPU)
        self.dense = dense
        self.clear()

    def clear(self):
        r = self.resolution
        self.prob = np.full(r * r * r, np.nan, F) if self.dense else {}
        self.min_bound = np.full(3, self.h, np.int64)
        self.max_bound = np.full(3, self.h, np.int64)

    # ---- storage ------------------------------------------------------------------------------------------------
    def _check(self):
        if not (self.voxel_size > 0 and np.isfinite(self.voxel_size)) or not np.isfinite(self.origin).all():
            raise Refused("voxel_size / origin")

    def _get(self, lin):
        lin = np.asarray(lin, np.int64)
        if self.dense:
            return self.prob[lin]
        return np.array([self.prob.get(int(i), F(np.nan)) for i in lin.ravel()], F).reshape(lin.shape)

    def _put(self, lin, val):
        if self.dense:
            self.prob[lin] = val
        else:
            for i, v in zip(np.asarray(lin).ravel(), np.asarray(val, F).ravel()):
                self.prob[int(i)] = F(v)

    def linear(self, ijk):
        ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
        r = self.resolution
        return (ijk[:, 0] * r + ijk[:, 1]) * r + ijk[:, 2]

    def inside(self, ijk):
        ijk = np.asarray(ijk, np.int64).reshape(-1, 3)
        return ((ijk >= 0) & (ijk < self.resolution)).all(1)

    def _update(self, lin, step, clamp=True):
        """the step-5 update of each voxel in lin (distinct), and nothing else"""
        if len(lin) == 0:
            return
        p = self._get(lin)
        p = np.where(np.isnan(p), F(0.0), p).astype(F)
        p = (p + F(step)).astype(F)
        if clamp:
            p = np.where(p < self.clamping_thres_min, self.clamping_thres_min, p).astype(F)
            p = np.where(p > self.clamping_thres_max, self.clamping_thres_max, p).astype(F)
        self._put(lin, p)

    def _widen(self, lin):
        if len(lin) == 0:
            return
        r = self.resolution
        ijk = np.stack([lin // (r * r), (lin // r) % r, lin % r], 1)
        self.min_bound = np.minimum(self.min_bound, ijk.min(0))
        self.max_bound = np.maximum(self.max_bound, ijk.max(0))


# ---- Insert -------------------------------------------------------------------------------------------------------
def ranged_points(points, viewpoint, max_range):
    """step 1: (q [n,3], hit [n], keep [n]) -- keep is False for a point with a coordinate that is not finite"""
    p = np.asarray(points, F).reshape(-1, 3)
    vp = np.asarray(viewpoint, F).reshape(3)
    mr = F(max_range)
    keep = np.isfinite(p).all(1)
    with np.errstate(all="ignore"):
        d = (p - vp).astype(F)
        dist = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).astype(F) + d[:, 2] * d[:, 2]).astype(F)).astype(F)
        hit = (dist <= mr) if not mr < 0 else np.ones(len(p), bool)
        cut = (vp + ((d / dist[:, None]).astype(F) * mr).astype(F)).astype(F)
    q = np.where(hit[:, None], p, np.where((dist == 0)[:, None], vp[None, :], cut)).astype(F)
    return q, hit & keep, keep


def traversal(start, ends, vs, n_buf):
    """VoxelTraversal for every end: a list of [k,3] int64 arrays of emitted voxels (before + h), and per ray whether
    the walk left the bounding box of its start and end voxels"""
    vs = F(vs)
    ends = np.asarray(ends, F).reshape(-1, 3)
    n = len(ends)
    start = np.broadcast_to(np.asarray(start, F).reshape(1, 3), (n, 3))
    with np.errstate(all="ignore"):
        ray = (ends - start).astype(F)
        length = np.sqrt(((ray[:, 0] * ray[:, 0] + ray[:, 1] * ray[:, 1]).astype(F) + ray[:, 2] * ray[:, 2]).astype(F)).astype(F)
        alive = length != 0
        ray = (ray / length[:, None]).astype(F)
        cur = floor_int((start / vs).astype(F))
        last = floor_int((ends / vs).astype(F))
        step = np.where(ray > 0, 1, np.where(ray < 0, -1, 0)).astype(np.int64)
        boundary = ((cur.astype(np.float64) + 0.5 * step.astype(np.float64)) * np.float64(vs)).astype(F)
        tmax = np.where(step != 0, ((boundary - start).astype(F) / ray).astype(F), F(np.inf)).astype(F)
        tdelta = np.where(step != 0, (vs / np.abs(ray)).astype(F), F(np.inf)).astype(F)
    emitted = [[] for _ in range(n)]
    rows = np.nonzero(alive)[0]
    for i in rows:
        emitted[i].append(cur[i].copy())
    count = 1
    while count < n_buf and len(rows):
        tx, ty, tz = tmax[rows, 0], tmax[rows, 1], tmax[rows, 2]
        axis = np.where(tx < ty, np.where(tx < tz, 0, 2), np.where(ty < tz, 1, 2))
        cur[rows, axis] += step[rows, axis]
        with np.errstate(all="ignore"):
            tmax[rows, axis] = (tmax[rows, axis] + tdelta[rows, axis]).astype(F)
        at_last = (cur[rows] == last[rows]).all(1)
        t = tmax[rows]
        tmin = np.where(t[:, 0] < t[:, 1], t[:, 0], t[:, 1])
        tmin = np.where(tmin < t[:, 2], tmin, t[:, 2])
        go = ~at_last & ~(tmin > length[rows])
        rows = rows[go]
        for i in rows:
            emitted[i].append(cur[i].copy())
        count += 1
    out, left = [], np.zeros(n, bool)
    c0 = floor_int((start / vs).astype(F))
    lo, hi = np.minimum(c0, last), np.maximum(c0, last)
    for i in range(n):
        e = np.array(emitted[i], np.int64).reshape(-1, 3)
        out.append(e)
        left[i] = bool(len(e)) and bool(((e < lo[i]) | (e > hi[i])).any())
    return out, left


_SETS = {}   # insert_sets' results: the same cloud inserted again walks the same voxels


def insert_sets(g, p, vp, max_range):
    """steps 1-4 of Insert: (free minus occupied, occupied) as ascending linear indices, and what the non-vacuity checks
    ask about.  Depends on the grid's frame only, not on its voxels."""
    key = (p.tobytes(), vp.tobytes(), float(max_range), float(g.voxel_size), g.origin.tobytes(), g.resolution)
    if key in _SETS:
        return _SETS[key]
    q, hit, keep = ranged_points(p, vp, max_range)
    q, hit = q[keep], hit[keep]
    vs, h = g.voxel_size, g.h
    with np.errstate(all="ignore"):
        r = np.abs((q - vp).astype(F)).max(1) if len(q) else np.zeros(0, F)
        max_r = r.max() if len(r) else F(0.0)           # (np.max hands a NaN on)
        nd = np.ceil(F(max_r) / vs)
    if not nd <= MAX_NDIV:
        raise Refused("n_div")
    n_div = int(nd)
    n_buf = 3 * (n_div + 1)
    free = np.zeros(0, np.int64)
    left = np.zeros(len(q), bool)
    walked_out = np.zeros(len(q), bool)
    if n_div > 0 and len(q):
        vox, left = traversal((vp - g.origin).astype(F), (q - g.origin).astype(F), vs, n_buf)
        walked_out = np.array([bool(len(v)) and not g.inside(v + h).all() for v in vox])
        allv = np.concatenate(vox) + h
        free = np.unique(g.linear(allv[g.inside(allv)]))
    occ_ijk = floor_int(((q[hit] - g.origin).astype(F) / vs).astype(F)) + h
    occ = np.unique(g.linear(occ_ijk[g.inside(occ_ijk)]))
    free_only = np.setdiff1d(free, occ)
    stats = dict(free=len(free_only), occupied=len(occ), both=len(np.intersect1d(free, occ)), left_box=int(left.sum()),
                 left_grid=int(walked_out.sum()), n_div=n_div)
    if len(_SETS) > 64:
        _SETS.clear()
    _SETS[key] = (free_only, occ, stats)
    return _SETS[key]


def insert(g, points, viewpoint, max_range=-1.0, stats=None):
    """Insert; stats (a dict) receives the sizes the non-vacuity checks ask about"""
    g._check()
    p = np.ascontiguousarray(np.asarray(points, F).reshape(-1, 3))
    if len(p) == 0:
        return
    vp = np.asarray(viewpoint, F).reshape(3)
    if not np.isfinite(vp).all() or np.isnan(F(max_range)):
        raise Refused("viewpoint / max_range")
    free_only, occ, st = insert_sets(g, p, vp, max_range)
    g._update(free_only, g.prob_miss_log)
    g._update(occ, g.prob_hit_log)
    g._widen(np.concatenate([free_only, occ]))
    if stats is not None:
        stats.update(st)


def add_voxels(g, indices, occupied=False):
    g._check()
    ijk = np.asarray(indices, np.int64).reshape(-1, 3)
    if len(ijk) == 0:
        return
    if not g.inside(ijk).all():
        raise Refused("index")
    lin = np.unique(g.linear(ijk))
    g._update(lin, g.prob_hit_log if occupied else g.prob_miss_log)
    g._widen(lin)


def set_free_area(g, lo, hi):
    g._check()
    lo, hi = np.asarray(lo, F).reshape(3), np.asarray(hi, F).reshape(3)
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        raise Refused("corner")
    imin = np.maximum(floor_int(((lo - g.origin).astype(F) / g.voxel_size).astype(F)) + g.h, 0)
    imax = np.minimum(floor_int(((hi - g.origin).astype(F) / g.voxel_size).astype(F)) + g.h, g.resolution - 1)
    g.min_bound, g.max_bound = imin, imax
    lin = box_linear(g)
    g._update(lin, g.prob_miss_log, clamp=False)


def box_linear(g):
    """linear indices of the bounds box, ascending; empty where min > max on an axis"""
    if (g.min_bound > g.max_bound).any():
        return np.zeros(0, np.int64)
    ax = [np.arange(g.min_bound[k], g.max_bound[k] + 1, dtype=np.int64) for k in range(3)]
    r = g.resolution
    return ((ax[0][:, None, None] * r + ax[1][None, :, None]) * r + ax[2][None, None, :]).ravel()


def voxel_of(g, points):
    p = np.asarray(points, F).reshape(-1, 3)
    return floor_int(((p - g.origin).astype(F) / g.voxel_size).astype(F)) + g.h


def query(g, points):
    """-> (log-odds [n], NaN for unknown or outside on any axis; index [n,3])"""
    ijk = voxel_of(g, points)
    ok = g.inside(ijk)
    out = np.full(len(ijk), np.nan, F)
    if ok.any():
        out[ok] = g._get(g.linear(ijk[ok]))
    return out, ijk


def extract(g, which):
    """-> (grid_index [m,3] int32, prob_log [m], points [m,3])"""
    lin = box_linear(g)
    p = g._get(lin) if len(lin) else np.zeros(0, F)
    known = ~np.isnan(p)
    with np.errstate(invalid="ignore"):
        sel = known if which == KNOWN else (known & (p <= g.occ_prob_thres_log) if which == FREE
                                            else known & (p > g.occ_prob_thres_log))
    lin, p = lin[sel], p[sel]
    r = g.resolution
    ijk = np.stack([lin // (r * r), (lin // r) % r, lin % r], 1).astype(np.int32).reshape(-1, 3)
    c = F(0.5 - g.h)
    pts = (((ijk.astype(F) + c).astype(F) * g.voxel_size).astype(F) + g.origin).astype(F)
    return ijk, p.astype(F), pts


def get_min_bound(g):
    return ((g.min_bound - g.h).astype(F) * g.voxel_size + g.origin).astype(F)


def get_max_bound(g):
    return ((g.max_bound - (g.h - 1)).astype(F) * g.voxel_size + g.origin).astype(F)


# ---- the scenes of the GPU tests ------------------------------------------------------------------------------------
RESOLUTIONS = (16, 33, 64)
COUNTS = (1, 63, 64, 65, 257, 5000)     # what crosses a lane, a wave and a block
SCENES = "abcdefgh"
ORIGINS = {16: (0.0, 0.0, 0.0), 33: (0.013, -0.027, 0.041), 64: (0.2, -0.1, 0.3)}   # 33: no multiple of the voxel
VOXEL = 0.1


def new_grid(res):
    return Grid(VOXEL, res, ORIGINS[res])


def scene(name, res, n, seed=3):
    """the calls of scene `name` on new_grid(res) with clouds of n points: a list of
    ("insert", points, viewpoint, max_range) | ("free", lo, hi) | ("add", indices, occupied) | ("set", {attribute: value})
      a  a shell of points around a viewpoint at the grid's centre: every ray shares its first voxels
      b  a viewpoint outside the grid, about half the points outside too: rays enter, leave, some never touch it
      c  axis-parallel rays, rays with one and two zero direction components, a point equal to the viewpoint, a
         point inside the viewpoint's own voxel; then shell points
      d  max_range below most distances, then max_range = 0 (with a point at the viewpoint itself)
      e  the same cloud 12 times: both clamps bind
      f  other log-odds parameters and threshold, two viewpoints
      g  set_free_area over a box partly outside the grid, then an insert
      h  an insert, then add_voxels with duplicates, occupied and free"""
    rng = np.random.default_rng(seed * 1000 + res * 10 + SCENES.index(name))
    c = np.asarray(ORIGINS[res], F)
    e = F(res * VOXEL / 2)               # half the grid's side

    def shell(k, centre, radius, jitter):
        d = rng.standard_normal((k, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        r = radius * (1.0 + jitter * rng.uniform(-1.0, 1.0, (k, 1)))
        return (np.asarray(centre, np.float64) + d * r).astype(F)

    vp = (c + np.array([0.031, -0.017, 0.023], F)).astype(F)
    if name == "a":
        return [("insert", shell(n, vp, 0.6 * e, 0.3), vp, -1.0)]
    if name == "b":
        vp = (c + np.array([1.7, 0.35, -0.25], F) * e).astype(F)
        pts = (c + rng.uniform(-1.25, 1.25, (n, 3)) * e).astype(F)
        pts[0] = c + np.array([-0.9, -0.2, 0.1], F) * e     # the first ray crosses the grid, whatever the draw
        return [("insert", pts, vp, -1.0)]
    if name == "c":
        vp = (c + np.array([0.05, 0.05, 0.05], F)).astype(F)
        special = np.array([[0.5 * e, 0, 0], [0, -0.5 * e, 0], [0, 0, 0.4 * e], [0.3 * e, 0.3 * e, 0],
                            [0, -0.2 * e, 0.45 * e], [0, 0, 0], [0.01, 0.02, -0.01]], F)
        pts = np.concatenate([(vp + special).astype(F), shell(max(n - len(special), 0), vp, 0.55 * e, 0.3)])[:n]
        return [("insert", np.ascontiguousarray(pts), vp, -1.0)]
    if name == "d":
        pts = shell(n, vp, 0.6 * e, 0.6)
        at_vp = np.concatenate([vp[None, :], pts])[:n]
        return [("insert", pts, vp, float(0.45 * e)), ("insert", np.ascontiguousarray(at_vp), vp, 0.0)]
    if name == "e":
        return [("insert", shell(n, vp, 0.6 * e, 0.3), vp, -1.0)] * 12
    if name == "f":
        vp2 = (c + np.array([-0.3, 0.2, 0.1], F) * e).astype(F)
        pts = shell(n, vp, 0.6 * e, 0.3)
        return [("set", dict(clamping_thres_min=-1.3, clamping_thres_max=2.2, prob_hit_log=0.7, prob_miss_log=-0.55,
                             occ_prob_thres_log=0.3)),
                ("insert", pts, vp, -1.0), ("insert", pts, vp2, -1.0), ("insert", pts, vp, -1.0)]
    if name == "g":
        lo = (c + np.array([0.2, -0.5, -1.4], F) * e).astype(F)
        hi = (c + np.array([1.5, 0.4, 0.3], F) * e).astype(F)
        return [("free", lo, hi), ("insert", shell(n, vp, 0.6 * e, 0.3), vp, -1.0)]
    if name == "h":
        idx = rng.integers(0, res, (max(n // 4, 1), 3)).astype(np.int32)
        dup = np.concatenate([idx, idx[rng.permutation(len(idx))], idx[:1]])
        return [("insert", shell(n, vp, 0.6 * e, 0.3), vp, -1.0), ("add", dup, True), ("add", dup[::-1].copy(), False),
                ("add", dup[: len(dup) // 2 + 1], True)]
    raise KeyError(name)


def apply(g, op, stats=None):
    """one call of a scene on the restatement"""
    if op[0] == "insert":
        st = {}
        insert(g, op[1], op[2], op[3], st)
        if stats is not None:
            stats.append(st)
    elif op[0] == "free":
        set_free_area(g, op[1], op[2])
    elif op[0] == "add":
        add_voxels(g, op[1], op[2])
    else:
        for k, v in op[1].items():
            setattr(g, k, F(v))
