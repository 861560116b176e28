"""The numeric contract of integration::ScalableTSDFVolume (include/mi_icp.h) restated in numpy fp32.  The per-voxel
update is tsdf_exact.integrate on a 16^3 tsdf_exact.Volume per unit (h = 0, origin = key * L), so it stays the rule
that is pinned to the reference's RealData values; the open rule, both extractions and GetTSDFAt / GetNormalAt across
units are restated from the contract text.  A helper for test_scalable_tsdf_cpu.py and test_gpu_scalable_tsdf.py, not
a test."""
import numpy as np

import tsdf_exact as tx
from depth_exact import depth_points, invert4          # noqa: F401 (the pose and stage 1's points: one restatement)

F = np.float32
NO_COLOR, RGB8, GRAY32 = tx.NO_COLOR, tx.RGB8, tx.GRAY32
RES, UNIT = 16, 4096
KEY_MAX = (1 << 20) - 1


def keys_of_points(p, sdf_trunc, L):
    """the units within sdf_trunc of the points: a sorted list of (x, y, z) tuples"""
    p, t, L = np.asarray(p, F).reshape(-1, 3), F(sdf_trunc), F(L)
    lo = tx._floor_int((p - t) / L)
    hi = tx._floor_int((p + t) / L)
    out = set()
    span = int((hi - lo).max()) + 1 if len(p) else 0
    assert span <= 4
    for dx in range(span):
        for dy in range(span):
            for dz in range(span):
                k = lo + np.array([dx, dy, dz])
                m = (k <= hi).all(1) & (np.abs(k) <= KEY_MAX).all(1)
                out.update(map(tuple, k[m].tolist()))
    return sorted(out)


class Volume:
    def __init__(self, voxel_length, sdf_trunc, color_type, depth_sampling_stride=4):
        self.vl = F(voxel_length)
        self.half = F(F(0.5) * self.vl)
        self.L = F(self.vl * F(16.0))
        self.trunc = F(sdf_trunc)
        self.color_type = int(color_type)
        self.stride = int(depth_sampling_stride)
        self.units = {}            # key -> tsdf_exact.Volume of 16^3 (h = 0)
        self.mult, self.mult_key = None, None

    def reset(self):
        self.units = {}

    def keys(self):
        return sorted(self.units)

    def arrays(self):
        """(keys [m, 3] int32 ascending, tsdf [m, 4096], weight [m, 4096], color [m, 4096, 3])"""
        ks = self.keys()
        m = len(ks)
        t, w, c = np.zeros((m, UNIT), F), np.zeros((m, UNIT), F), np.ones((m, UNIT, 3), F)
        for e, k in enumerate(ks):
            t[e], w[e], c[e] = self.units[k].tsdf, self.units[k].weight, self.units[k].color
        return np.array(ks, np.int32).reshape(m, 3), t, w, c


def open_units(vol, depth, width, height, fx, fy, cx, cy, extrinsic):
    """stage 1; returns the new keys, ascending"""
    p = depth_points(depth, width, height, fx, fy, cx, cy, extrinsic, vol.stride)
    new = [k for k in keys_of_points(p, vol.trunc, vol.L) if k not in vol.units]
    for k in new:
        u = tx.Volume(vol.L, RES, vol.trunc, vol.color_type, [F(k[a]) * vol.L for a in range(3)])
        u.h = 0
        assert u.vl == vol.vl and u.half == vol.half
        vol.units[k] = u
    return new


def integrate(vol, depth, color, width, height, fx, fy, cx, cy, extrinsic):
    """one frame: open, then the uniform volume's rule in every open unit.  Returns (new units, voxels updated)."""
    new = open_units(vol, depth, width, height, fx, fy, cx, cy, extrinsic)
    key = (width, height, F(fx), F(fy), F(cx), F(cy))
    if vol.mult_key != key:
        vol.mult, vol.mult_key = tx.multiplier(width, height, F(fx), F(fy), F(cx), F(cy)), key
    updated = 0
    for u in vol.units.values():
        u.mult, u.mult_key = vol.mult, key           # (one multiplier image for all units)
        updated += tx.integrate(u, depth, color, width, height, fx, fy, cx, cy, extrinsic)
    return len(new), updated


# ---- extraction ------------------------------------------------------------------------------------------------------
def _pack(k):
    k = np.asarray(k, np.int64)
    return ((k[..., 0] + (1 << 20)) << 42) | ((k[..., 1] + (1 << 20)) << 21) | (k[..., 2] + (1 << 20))


class _Grid:
    """the open units as dense arrays in the canonical order, and the directory's lookup"""

    def __init__(self, vol):
        self.keys, t, w, c = vol.arrays()
        self.m = len(self.keys)
        self.T = t.reshape(self.m, RES, RES, RES)
        self.W = w.reshape(self.m, RES, RES, RES)
        self.C = c.reshape(self.m, RES, RES, RES, 3)
        self.packed = _pack(self.keys) if self.m else np.zeros(0, np.int64)

    def find(self, k):
        """unit indices of keys k [n, 3] (int64), -1 where the unit is not open"""
        k = np.asarray(k, np.int64)
        ok = (np.abs(k) <= KEY_MAX).all(-1)
        q = _pack(np.where(ok[..., None], k, 0))
        if self.m == 0:
            return np.full(q.shape, -1, np.int64)
        at = np.clip(np.searchsorted(self.packed, q), 0, self.m - 1)
        return np.where(ok & (self.packed[at] == q), at, -1)

    def next_along(self, ax):
        """per voxel the (tsdf, weight, colour) of the voxel at +1 along ax: in the same unit, or coordinate 0 of the
        next unit, weight 0 / tsdf 0 where that unit is not open"""
        step = np.zeros(3, np.int64)
        step[ax] = 1
        nb = self.find(self.keys.astype(np.int64) + step)
        has = nb >= 0
        sl_hi = [slice(None)] * 4
        sl_hi[ax + 1] = slice(1, RES)
        sl_lo = [slice(None)] * 4
        sl_lo[ax + 1] = slice(0, RES - 1)
        first = [slice(None)] * 4
        first[ax + 1] = 0
        last = [slice(None)] * 4
        last[ax + 1] = RES - 1
        out = []
        for A, fill in ((self.T, F(0)), (self.W, F(0)), (self.C, F(0))):
            B = np.full_like(A, fill)
            B[tuple(sl_lo)] = A[tuple(sl_hi)]
            face = A[np.where(has, nb, 0)][tuple(first)]
            mask = has.reshape((-1,) + (1,) * (face.ndim - 1))
            B[tuple(last)] = np.where(mask, face, fill)
            out.append(B)
        return out


def _valid(w, t):
    return (w != F(0)) & (t < F(0.98)) & (t >= F(-0.98))


def extract_voxel_point_cloud(vol):
    """-> (points [n, 3], colors [n, 3]): units ascending, then ascending voxel index"""
    g = _Grid(vol)
    e, x, y, z = np.nonzero(_valid(g.W, g.T)) if g.m else (np.zeros(0, np.int64),) * 4
    xyz = np.stack([x, y, z], 1).reshape(-1, 3)
    k = g.keys[e].astype(F).reshape(-1, 3)
    pts = (vol.half + vol.vl * xyz.astype(F)) + k * vol.L
    c = ((g.T[e, x, y, z].astype(np.float64) + 1.0) * 0.5).astype(F)
    return pts.astype(F), np.stack([c, c, c], 1).reshape(-1, 3)


def tsdf_at(vol, g, p):
    """GetTSDFAt at the world points p [n, 3]"""
    p = np.asarray(p, F).reshape(-1, 3)
    q = p - vol.half
    with np.errstate(all="ignore"):
        u = tx._floor_int(q / vol.L)
    e0 = g.find(u)
    gr = (q - u.astype(F) * vol.L) / vol.vl
    i = np.clip(tx._floor_int(gr), 0, RES - 1)
    r = gr - i.astype(F)
    f = {}
    for dx in (0, 1):
        for dy in (0, 1):
            for dz in (0, 1):
                c = i + np.array([dx, dy, dz])
                wrap = c >= RES
                e = np.where(wrap.any(1), g.find(u + wrap), e0)
                cc = c - RES * wrap
                val = g.T[np.where(e >= 0, e, 0), cc[:, 0], cc[:, 1], cc[:, 2]] if g.m else np.zeros(len(p), F)
                f[(dx, dy, dz)] = np.where(e >= 0, val, F(0)).astype(F)
    one = F(1)
    r0, r1, r2 = r[:, 0], r[:, 1], r[:, 2]
    a0, a1, a2 = one - r0, one - r1, one - r2
    s = a0 * (a1 * (a2 * f[0, 0, 0] + r2 * f[0, 0, 1]) + r1 * (a2 * f[0, 1, 0] + r2 * f[0, 1, 1])) + \
        r0 * (a1 * (a2 * f[1, 0, 0] + r2 * f[1, 0, 1]) + r1 * (a2 * f[1, 1, 0] + r2 * f[1, 1, 1]))
    return np.where(e0 >= 0, s, F(0)).astype(F)


def normal_at(vol, g, p):
    """GetNormalAt at the world points p [n, 3]"""
    p = np.asarray(p, F).reshape(-1, 3)
    gap = F(0.99 * np.float64(vol.vl))
    n = np.zeros((len(p), 3), F)
    for k in range(3):
        hi, lo = p.copy(), p.copy()
        hi[:, k] = p[:, k] + gap
        lo[:, k] = p[:, k] - gap
        n[:, k] = tsdf_at(vol, g, hi) - tsdf_at(vol, g, lo)
    zz = (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]
    with np.errstate(all="ignore"):
        return np.where((zz > F(0))[:, None], n / np.sqrt(zz)[:, None], n).astype(F)


def extract_point_cloud(vol, with_index=False):
    """-> (points, normals, colors or None): units ascending, then ascending voxel index, then the axis; with_index:
    also [n, 5] = (unit, x, y, z, axis) of every point"""
    g = _Grid(vol)
    if g.m == 0:
        z = np.zeros((0, 3), F)
        out = (z, z.copy(), (None if vol.color_type == NO_COLOR else z.copy()))
        return out + (np.zeros((0, 5), np.int64),) if with_index else out
    v0 = _valid(g.W, g.T)
    cross = np.zeros((g.m, RES, RES, RES, 3), bool)
    nxt = [g.next_along(ax) for ax in range(3)]
    for ax in range(3):
        T1, W1, _ = nxt[ax]
        cross[..., ax] = v0 & _valid(W1, T1) & (g.T * T1 < F(0))
    e, x, y, z, ax = np.nonzero(cross)
    n = len(e)
    f0 = g.T[e, x, y, z]
    f1 = np.zeros(n, F)
    c0 = g.C[e, x, y, z]
    c1 = np.zeros((n, 3), F)
    for a in range(3):
        m = ax == a
        f1[m] = nxt[a][0][e[m], x[m], y[m], z[m]]
        c1[m] = nxt[a][2][e[m], x[m], y[m], z[m]]
    r0, r1 = np.abs(f0), np.abs(f1)
    rs = r0 + r1
    xyz = np.stack([x, y, z], 1)
    p = ((vol.half + vol.vl * xyz.astype(F)) + g.keys[e].astype(F) * vol.L).astype(F)
    rows = np.arange(n)
    pa = p[rows, ax]
    p[rows, ax] = (pa * r1 + (pa + vol.vl) * r0) / rs
    cols = None
    if vol.color_type != NO_COLOR:
        cols = (c0 * r1[:, None] + c1 * r0[:, None]) / rs[:, None]
        if vol.color_type == RGB8:
            cols = cols / F(255)
        cols = cols.astype(F)
    out = (p, normal_at(vol, g, p), cols)
    return out + (np.stack([e, x, y, z, ax], 1),) if with_index else out
