"""The collision contract of include/mi_icp.h restated in numpy, fp32 in the order written there: cell boxes, the five
predicates, ComputeIntersection as an all-pairs brute force (smallest other index, ascending enumerated index),
GetAxisAlignedBoundingBox and CreateVoxelGrid.  The yardstick of test_collision_cpu.py (which holds it to the
reference's unit tests and to outside definitions in fp64) and of the GPU tests (which hold the library to it exactly).
Nothing here knows about candidate cells: every enumerated element meets every element of the other side.

Sides:  ("voxel", keys int32[m, 3], voxel_size, origin[3])
        ("occ", indices int32[m, 3] of the occupied voxels in ascending linear order, resolution, voxel_size, origin[3])
        ("lines", points float32[n, 3], lines int32[l, 2])
        ("prims", [Prim, ...])
Settled here where the issue's wording left room: (radius + margin)^2 is the fp32 sum times itself; the capsule's
stationary sums start from 0; a box whose rotation is not orthonormal within 1e-4 is refused (ValueError); a box's bounding box
is |rot| * half lengths (the reference's |rot * half| does not contain a rotated box)."""
from collections import namedtuple

import numpy as np

F = np.float32
EPS = F(np.finfo(np.float32).eps)
UNSPECIFIED, BOX, SPHERE, CAPSULE, CYLINDER, MESH = 0, 1, 2, 3, 4, 5
BOX_ORTHO_TOL = F(1.0e-4)

Prim = namedtuple("Prim", "type transform param")     # transform: 4x4 (row, column), param: 3 floats


def prim(ptype, transform=None, param=(0, 0, 0)):
    t = np.eye(4, dtype=F) if transform is None else np.asarray(transform, F).reshape(4, 4).copy()
    p = np.zeros(3, F)
    p[:len(np.atleast_1d(param))] = np.atleast_1d(param)
    return Prim(int(ptype), t, p)


def box(lengths, transform=None):
    return prim(BOX, transform, lengths)


def sphere(radius, center=(0, 0, 0)):
    t = np.eye(4, dtype=F)
    t[:3, 3] = center
    return prim(SPHERE, t, (radius,))


def capsule(radius, height, transform=None):
    return prim(CAPSULE, transform, (radius, height))


def cylinder(radius, height, transform=None):
    return prim(CYLINDER, transform, (radius, height))


def prim_records(prims):
    """-> the 80-byte mi_icp_primitive records as a structured array (transform column-major)"""
    rec = np.zeros(len(prims), dtype=[("type", np.int32), ("transform", F, 16), ("param", F, 3)])
    for i, p in enumerate(prims):
        rec["type"][i] = p.type
        rec["transform"][i] = p.transform.T.reshape(16)
        rec["param"][i] = p.param
    return rec


# ---------------------------------------------------------------------------------------------- cell boxes
def cell_bounds(keys, voxel_size, origin):
    """lo = (float)k * vs + origin, hi = (float)(k + 1) * vs + origin"""
    keys = np.asarray(keys, np.int64).reshape(-1, 3)
    o = np.asarray(origin, F).reshape(1, 3)
    vs = F(voxel_size)
    return keys.astype(F) * vs + o, (keys + 1).astype(F) * vs + o


def side_cells(side):
    """a grid side -> (lo, hi, index): the cell boxes and the index each has in a pair"""
    if side[0] == "voxel":
        _, keys, vs, origin = side
        lo, hi = cell_bounds(keys, vs, origin)
        return lo, hi, np.arange(len(lo), dtype=np.int64)
    _, idx, res, vs, origin = side
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    lo, hi = cell_bounds(idx - res // 2, vs, origin)
    return lo, hi, (idx[:, 0] * res + idx[:, 1]) * res + idx[:, 2]


# ---------------------------------------------------------------------------------------------- predicates
def cell_cell(alo, ahi, blo, bhi):
    return ((alo <= bhi) & (blo <= ahi)).all(axis=-1)


def segment_cell(p0, p1, lo, hi):
    """LineSegmentAABB on [lo, hi] (already inflated); arrays broadcast over [..., 3]"""
    with np.errstate(all="ignore"):
        center = (lo + hi) * F(0.5)
        ext = hi - center
        mid = (p0 + p1) * F(0.5)
        dst = p1 - mid
        mid = mid - center
        ad = np.abs(dst)
        ok = ~(np.abs(mid) > ext + ad).any(axis=-1)
        ad = ad + EPS
        for a, b in ((1, 2), (2, 0), (0, 1)):
            lhs = np.abs(mid[..., a] * dst[..., b] - mid[..., b] * dst[..., a])
            ok &= ~(lhs > ext[..., a] * ad[..., b] + ext[..., b] * ad[..., a])
    return ok


def point_cell_d2(q, lo, hi):
    e = np.maximum(np.maximum(lo - q, q - hi), F(0))
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def segment_cell_d2(p, d, lo, hi):
    """min over the 34 parameters of point_cell_d2(p + t * d); p, d: [3] or [m, 3]; lo, hi: [m, 3]"""
    p, d = np.asarray(p, F).reshape(-1, 3), np.asarray(d, F).reshape(-1, 3)
    m = len(lo)
    ts = [np.zeros(m, F), np.ones(m, F)]
    with np.errstate(all="ignore"):
        for a in range(3):
            for b in (lo, hi):
                ts.append((b[:, a] - p[:, a]) / d[:, a])
        for code in range(1, 27):
            c = (code // 9, (code // 3) % 3, code % 3)
            num, den = np.zeros(m, F), np.zeros(len(d), F)
            for a in range(3):
                if c[a] == 0:
                    continue
                b = lo[:, a] if c[a] == 1 else hi[:, a]
                num = num + d[:, a] * (p[:, a] - b)
                den = den + d[:, a] * d[:, a]
            ts.append(-num / den)
        best = None
        for t in ts:
            t = np.where(np.isfinite(t), np.minimum(np.maximum(t, F(0)), F(1)), F(0)).astype(F)
            q = p + t[:, None] * d
            d2 = point_cell_d2(q, lo, hi)
            best = d2 if best is None else np.where(d2 < best, d2, best)
    return best


def box_cell(T, ea, cc, eb):
    """the fifteen axes; T 4x4, ea [3], cc / eb [m, 3]"""
    R = T[:3, :3].T.astype(F)            # R[i][j] = rot[j][i]
    A = np.abs(R) + EPS
    dc = cc - T[:3, 3][None, :]
    t = [(R[i, 0] * dc[:, 0] + R[i, 1] * dc[:, 1]) + R[i, 2] * dc[:, 2] for i in range(3)]
    ok = np.ones(len(cc), bool)
    for i in range(3):
        ok &= ~(np.abs(t[i]) > ea[i] + ((eb[:, 0] * A[i, 0] + eb[:, 1] * A[i, 1]) + eb[:, 2] * A[i, 2]))
    for j in range(3):
        ok &= ~(np.abs((t[0] * R[0, j] + t[1] * R[1, j]) + t[2] * R[2, j]) >
                ((ea[0] * A[0, j] + ea[1] * A[1, j]) + ea[2] * A[2, j]) + eb[:, j])
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            ok &= ~(np.abs(t[i2] * R[i1, j] - t[i1] * R[i2, j]) >
                    (ea[i1] * A[i2, j] + ea[i2] * A[i1, j]) + (eb[:, j1] * A[i, j2] + eb[:, j2] * A[i, j1]))
    return ok


def box_rotation_ok(T):
    for i in range(3):
        for j in range(3):
            g = (T[0, i] * T[0, j] + T[1, i] * T[1, j]) + T[2, i] * T[2, j]
            if not (abs(F(g - F(1.0 if i == j else 0.0))) <= BOX_ORTHO_TOL):
                return False
    return True


def primitive_live(P):
    if P.type not in (BOX, SPHERE, CAPSULE):
        return False
    if not (np.isfinite(P.transform).all() and np.isfinite(P.param).all()):
        return False
    return P.type != BOX or box_rotation_ok(P.transform)


def primitive_cells(P, lo, hi, margin):
    """one primitive against the cells [lo, hi] (not inflated) -> bool[m]"""
    if not primitive_live(P) or len(lo) == 0:
        return np.zeros(len(lo), bool)
    T, margin = P.transform, F(margin)
    with np.errstate(all="ignore"):
        if P.type == SPHERE:
            rr = F(P.param[0] + margin)
            return point_cell_d2(T[:3, 3][None, :], lo, hi) <= rr * rr
        if P.type == CAPSULE:
            rr, hh = F(P.param[0] + margin), F(F(0.5) * P.param[1])
            z = T[:3, 2]
            return segment_cell_d2(T[:3, 3] - hh * z, P.param[1] * z, lo, hi) <= rr * rr
        cc = (lo + hi) * F(0.5)
        eb = (hi - cc) + margin
        return box_cell(T, P.param * F(0.5), cc, eb)


# ---------------------------------------------------------------------------------------------- ComputeIntersection
def _accept_matrix_rows(en, ot, margin):
    """yields, per enumerated element i, the bool vector over the other side's elements (in the other side's order)
    and the other side's pair indices"""
    margin = F(margin)
    if ot[0] == "prims":
        elo, ehi, _ = side_cells(en)
        cols = [primitive_cells(P, elo, ehi, margin) for P in ot[1]]
        acc = np.stack(cols, axis=1) if cols else np.zeros((len(elo), 0), bool)
        return acc, np.arange(len(ot[1]), dtype=np.int64)
    olo, ohi, oidx = side_cells(ot)
    if en[0] in ("voxel", "occ"):
        elo, ehi, _ = side_cells(en)
        acc = np.zeros((len(elo), len(olo)), bool)
        for s in range(0, len(elo), 256):
            acc[s:s + 256] = cell_cell((elo[s:s + 256] - margin)[:, None, :], (ehi[s:s + 256] + margin)[:, None, :],
                                       olo[None, :, :], ohi[None, :, :])
        return acc, oidx
    if en[0] == "lines":
        pts, lines = np.asarray(en[1], F).reshape(-1, 3), np.asarray(en[2], np.int64).reshape(-1, 2)
        if len(lines) and (lines.min() < 0 or lines.max() >= len(pts)):
            raise ValueError("a line's point index is out of range")
        p0, p1 = pts[lines[:, 0]], pts[lines[:, 1]]
        fin = np.isfinite(p0).all(axis=1) & np.isfinite(p1).all(axis=1)
        acc = np.zeros((len(lines), len(olo)), bool)
        ilo, ihi = olo - margin, ohi + margin
        for s in range(0, len(lines), 64):
            acc[s:s + 64] = segment_cell(p0[s:s + 64, None, :], p1[s:s + 64, None, :], ilo[None], ihi[None])
        acc[~fin] = False
        return acc, oidx
    acc = np.stack([primitive_cells(P, olo, ohi, margin) for P in en[1]], axis=0) if len(en[1]) else np.zeros((0, len(olo)), bool)
    return acc, oidx


def side_count(side):
    return len(side[2]) if side[0] == "lines" else len(side[1])


def compute_intersection(a, b, margin=0.0):
    """-> pairs int32[m, 2]: column 0 indexes a, column 1 indexes b"""
    if not (np.isfinite(margin) and margin >= 0):
        raise ValueError("the margin must be finite and >= 0")
    kinds = (a[0], b[0])
    grids = ("voxel", "occ")
    ok = (a[0] in grids and b[0] in grids and kinds != ("occ", "occ")) or \
         (a[0] in grids and b[0] in ("lines", "prims")) or (b[0] in grids and a[0] in ("lines", "prims"))
    if not ok:
        raise ValueError("this pair of kinds is not built")
    a_enum = a[0] == "lines"
    en, ot = (a, b) if a_enum else (b, a)
    if side_count(a) == 0 or side_count(b) == 0:
        return np.zeros((0, 2), np.int32)
    for side in (a, b):
        if side[0] == "prims" and any(P.type == BOX and np.isfinite(P.transform).all() and np.isfinite(P.param).all() and
                                      not box_rotation_ok(P.transform) for P in side[1]):
            raise ValueError("a box's rotation is not orthonormal")
    acc, oidx = _accept_matrix_rows(en, ot, margin)
    if en[0] in grids:
        eidx = side_cells(en)[2]
    else:
        eidx = np.arange(acc.shape[0], dtype=np.int64)
    if acc.shape[1] == 0:
        return np.zeros((0, 2), np.int32)
    big = np.iinfo(np.int64).max
    other = np.where(acc, oidx[None, :], big).min(axis=1)
    rows = np.flatnonzero(other != big)
    pairs = np.stack([eidx[rows], other[rows]] if a_enum else [other[rows], eidx[rows]], axis=1)
    return pairs.astype(np.int32)


# ---------------------------------------------------------------------------------------------- bounding boxes, CreateVoxelGrid
def primitive_aabb(P):
    T, q = P.transform, P.param
    t = T[:3, 3]
    with np.errstate(all="ignore"):
        if P.type == BOX:
            h = np.array([(abs(T[k, 0]) * F(F(0.5) * q[0]) + abs(T[k, 1]) * F(F(0.5) * q[1])) + abs(T[k, 2]) * F(F(0.5) * q[2])
                          for k in range(3)], F)
            return -np.abs(h) + t, np.abs(h) + t
        if P.type == SPHERE:
            return -q[0] + t, q[0] + t
        if P.type == CAPSULE:
            pa = T[:3, 2] * F(F(0.5) * q[1])
            return (np.minimum(pa, -pa) - q[0]) + t, (np.maximum(pa, -pa) + q[0]) + t
        if P.type == CYLINDER:
            pa = T[:3, 2] * F(F(0.5) * q[1])
            a = -pa - pa
            n2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
            e = q[0] * np.sqrt(F(1) - a * a / n2)
            return np.minimum(pa - e, -pa - e) + t, np.maximum(pa + e, -pa + e) + t
    return np.zeros(3, F), np.zeros(3, F)


def voxelize_counts(P, voxel_size):
    vs = F(voxel_size)
    mn, mx = primitive_aabb(P)
    origin = P.transform[:3, 3].copy()
    min_b = (mn - origin) - vs * F(0.5)
    max_b = (mx - origin) + vs * F(0.5)
    cells = (max_b - min_b) / vs
    num = [int(np.floor(float(c) + 0.5)) for c in cells]       # roundf of a positive value
    return [n if n >= 1 else 0 for n in num], origin


def create_voxel_grid(P, voxel_size):
    """-> (keys int32[m, 3] ascending, origin[3])"""
    if not (voxel_size > 0 and np.isfinite(voxel_size)) or P.type not in (BOX, SPHERE, CAPSULE) or \
            not (np.isfinite(P.transform).all() and np.isfinite(P.param).all()):
        raise ValueError("refused")
    if P.type == BOX and not box_rotation_ok(P.transform):
        raise ValueError("refused")
    (nw, nh, nd), origin = voxelize_counts(P, voxel_size)
    total = nw * nh * nd
    if total > 2147483647:
        raise ValueError("refused")
    if total == 0:
        return np.zeros((0, 3), np.int32), origin
    idx = np.arange(total, dtype=np.int64)
    keys = np.stack([idx // (nh * nd) - nw // 2, (idx % (nh * nd)) // nd - nh // 2, idx % nd - nd // 2], axis=1)
    T0 = P.transform.copy()
    T0[:3, 3] = 0
    lo, hi = cell_bounds(keys, voxel_size, np.zeros(3, F))
    keep = primitive_cells(Prim(P.type, T0, P.param), lo, hi, 0.0)
    return keys[keep].astype(np.int32), origin


# ---------------------------------------------------------------------------------------------- scenes the tests share
def rotation(rng):
    """a random rotation in fp32 (orthonormal to a few 1e-7)"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))[None, :]
    if np.linalg.det(q) < 0:
        q[:, 2] = -q[:, 2]
    return q.astype(F)


def pose(rng, center, identity=False):
    T = np.eye(4, dtype=F)
    if not identity:
        T[:3, :3] = rotation(rng)
    T[:3, 3] = center
    return T


def shell_keys(rng, n, radius=14.0, noise=1.2):
    """about n distinct voxels of a noisy sphere shell around (-3, 2, -5): negative keys among them; ascending"""
    d = rng.normal(size=(n * 2, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = d * (radius + rng.normal(size=(n * 2, 1)) * noise) + np.array([-3.0, 2.0, -5.0])
    keys = np.unique(np.floor(p).astype(np.int32), axis=0)
    keys = keys[np.sort(rng.choice(len(keys), size=min(n, len(keys)), replace=False))]
    return np.ascontiguousarray(keys[np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))])


def mixed_primitives(rng, n, lo, hi):
    """n primitives around the box [lo, hi]: rotated and axis-aligned boxes, spheres, capsules, and at fixed places a
    sphere larger than the box, a capsule of height 0, a cylinder and a primitive with a NaN field"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    size = float((hi - lo).max())
    out = []
    for i in range(n):
        c = lo + rng.uniform(-0.1, 1.1, 3) * (hi - lo)
        kind = i % 4
        if i == 3:
            out.append(sphere(size * 1.2, (lo + hi) / 2))
        elif i == 5:
            out.append(capsule(size * 0.04, 0.0, pose(rng, c)))
        elif i == 6:
            out.append(cylinder(size * 0.2, size * 0.5, pose(rng, (lo + hi) / 2)))
        elif i == 7:
            T = pose(rng, c)
            T[1, 3] = np.nan
            out.append(sphere(size * 0.3, c)._replace(transform=T))
        elif kind == 0:
            out.append(box(rng.uniform(0.01, 0.12, 3) * size, pose(rng, c, identity=(i % 8 == 0))))
        elif kind == 1:
            out.append(sphere(rng.uniform(0.005, 0.08) * size, c))
        elif kind == 2:
            out.append(capsule(rng.uniform(0.005, 0.04) * size, rng.uniform(0.0, 0.3) * size, pose(rng, c)))
        else:
            out.append(box(rng.uniform(0.005, 0.05, 3) * size, pose(rng, c)))
    return out


SCENE_VS, SCENE_ORIGIN, SCENE_RES, SCENE_MARGIN = 0.1, np.array([0.3, -0.2, 0.1], F), 32, 0.02
SCENE_VS_B = 0.17


def scene_inputs():
    """what the C++ and pybind11 tests share: a_keys (ascending), b_keys (any order), points + lines, primitives, the
    cloud an occupancy grid of SCENE_RES sees from its origin, and a capsule to voxelise"""
    rng = np.random.default_rng(77)
    a_keys = shell_keys(rng, 500, radius=6.0, noise=0.8)
    b_keys = rng.integers(-6, 5, (300, 3)).astype(np.int32)
    centre = SCENE_ORIGIN + np.array([-0.3, 0.2, -0.5], F)
    pts = (centre + rng.uniform(-0.9, 0.9, (60, 3))).astype(F)
    lines = rng.integers(0, 60, (80, 2)).astype(np.int32)
    prims = mixed_primitives(rng, 24, centre - 0.8, centre + 0.8)
    d = rng.normal(size=(400, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    cloud = (SCENE_ORIGIN + d * 0.5).astype(F)
    cap = capsule(0.11, 0.37, pose(rng, (-0.4, 0.1, 0.2)))
    return a_keys, b_keys, pts, lines, prims, cloud, cap


def scene_expected(occ_index):
    """-> {name: pairs} for the scene, given the occupied voxels the grid lists"""
    a_keys, b_keys, pts, lines, prims, _, cap = scene_inputs()
    a = ("voxel", a_keys, SCENE_VS, SCENE_ORIGIN)
    b = ("voxel", b_keys, SCENE_VS_B, SCENE_ORIGIN + F(0.037))
    rev = ("voxel", np.ascontiguousarray(a_keys[::-1]), SCENE_VS, SCENE_ORIGIN)
    ls, pr = ("lines", pts, lines), ("prims", prims)
    occ = ("occ", np.asarray(occ_index, np.int32).reshape(-1, 3), SCENE_RES, SCENE_VS, SCENE_ORIGIN)
    m = SCENE_MARGIN
    return {"vv": compute_intersection(a, b, m), "vl": compute_intersection(a, ls, m), "lv": compute_intersection(ls, a, m),
            "vo": compute_intersection(a, occ, m), "ov": compute_intersection(occ, a, m), "ol": compute_intersection(occ, ls, m),
            "lo": compute_intersection(ls, occ, m), "pv": compute_intersection(pr, a, m), "vp": compute_intersection(a, pr, m),
            "po": compute_intersection(pr, occ, m), "op": compute_intersection(occ, pr, m),
            "rl": compute_intersection(rev, ls, m), "rp": compute_intersection(rev, pr, m), "rv": compute_intersection(rev, b, m),
            "capsule": create_voxel_grid(cap, 0.05)[0]}
