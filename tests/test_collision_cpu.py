"""The collision contract without a GPU: the numpy restatement (tests/collision_exact.py) against the reference's two
unit tests and against outside definitions in fp64 -- dense sampling of the segment for segments and capsules, linear
programming for boxes, the closed form for spheres; the lattice, ordering, bounding-box and CreateVoxelGrid rules
against brute force; the predicates' header (csrc/collision_predicates.h) against the restatement in a stand-alone
program built with AddressSanitizer and UBSan and run directly; the C ABI's prototypes and statuses.

UNDECIDABLE CASES.  A case whose fp64 answer changes when both shapes grow and shrink by 1e-5 (coordinates are of order
1, so that is about 100 fp32 ulps) is skipped; at most 1 % of a case set may be, and outside them agreement is exact.
The sampled distance is the minimum over 1001 points of the segment and 1001 more between the neighbours of the best
one -- the distance to a box is convex along a segment -- so it is within 2 * 0.6 / 1e6 = 1.2e-6 of the true minimum;
a sampled answer is "distance <= bound + 1.5e-6"."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import collision_exact as ex

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DELTA, SAMPLING = 1.0e-5, 1.5e-6


# ---------------------------------------------------------------------------------------------- the reference's unit tests
def test_reference_unit_test_voxel_voxel():
    o = np.zeros(3, F)
    empty = ("voxel", np.zeros((0, 3), np.int32), 0.0, o)
    assert len(ex.compute_intersection(empty, empty)) == 0
    v1, v2 = ("voxel", np.array([[0, 0, 0]], np.int32), 1.0, o), ("voxel", np.array([[0, 0, 0]], np.int32), 1.0, o)
    assert len(ex.compute_intersection(v1, v2)) == 1
    v1 = ("voxel", np.array([[0, 0, 0], [5, 0, 0]], np.int32), 1.0, o)
    v2 = ("voxel", np.array([[0, 0, 0], [10, 0, 0]], np.int32), 1.0, o)
    assert ex.compute_intersection(v1, v2).tolist() == [[0, 0]]


def test_reference_unit_test_voxel_lineset():
    o = np.zeros(3, F)
    assert len(ex.compute_intersection(("voxel", np.zeros((0, 3), np.int32), 0.0, o),
                                       ("lines", np.zeros((0, 3), F), np.zeros((0, 2), np.int32)))) == 0
    v = ("voxel", np.array([[0, 0, 0], [5, 0, 0]], np.int32), 1.0, o)
    pts = np.array([[-0.1, -0.1, -0.1], [-0.1, -0.1, 1.1], [1.1, 1.1, 1.1]], F)
    ls = ("lines", pts, np.array([[0, 1], [0, 2]], np.int32))
    assert ex.compute_intersection(v, ls).tolist() == [[0, 1]]
    assert ex.compute_intersection(ls, v).tolist() == [[1, 0]]       # the lines are enumerated either way


# ---------------------------------------------------------------------------------------------- the case sets
def _cells(rng, n):
    lo = rng.uniform(-1, 1, (n, 3)).astype(F)
    return lo, (lo + F(0.05)).astype(F)


def _directions(rng, n):
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ax = np.flatnonzero(rng.random(n) < 0.1)                           # a tenth are axis-aligned
    d[ax] = np.eye(3)[rng.integers(0, 3, len(ax))] * rng.choice([-1.0, 1.0], (len(ax), 1))
    return d


def _segments(rng, lo, hi):
    n = len(lo)
    c = (lo.astype(float) + hi) / 2 + rng.normal(size=(n, 3)) * 0.15
    length = rng.uniform(0, 0.6, n)
    length[rng.random(n) < 0.02] = 0.0                                 # some have length 0
    d = _directions(rng, n) * length[:, None] / 2
    return (c - d).astype(F), (c + d).astype(F)


def _dist_to_box(q, lo, hi):
    e = np.maximum(np.maximum(lo - q, q - hi), 0.0)
    return np.sqrt((e * e).sum(axis=-1))


def _sampled_distance(p0, p1, lo, hi):
    """fp64: min over the segment of the distance to [lo, hi]: 1001 samples, then 1001 between the best one's neighbours"""
    p0, p1, lo, hi = (np.asarray(a, np.float64) for a in (p0, p1, lo, hi))
    out = np.empty(len(p0))
    for s in range(0, len(p0), 500):
        a, b, l, h = p0[s:s + 500, None], p1[s:s + 500, None], lo[s:s + 500, None], hi[s:s + 500, None]
        t = np.linspace(0, 1, 1001)[None, :, None]
        d = _dist_to_box(a + t * (b - a), l, h)
        k = d.argmin(axis=1)
        t0, t1 = np.maximum(k - 1, 0) / 1000.0, np.minimum(k + 1, 1000) / 1000.0
        t = (t0[:, None] + (t1 - t0)[:, None] * np.linspace(0, 1, 1001)[None, :])[:, :, None]
        out[s:s + 500] = np.minimum(d.min(axis=1), _dist_to_box(a + t * (b - a), l, h).min(axis=1))
    return out


def _hold(got, grown, shrunk, what):
    """got: the restatement; grown / shrunk: the fp64 answers with both shapes grown / shrunk by DELTA"""
    undecidable = grown != shrunk
    frac = undecidable.mean()
    print("%s: %d cases, %d undecidable (%.3f %%), %d hits" % (what, len(got), undecidable.sum(), 100 * frac, got.sum()))
    assert frac <= 0.01
    bad = np.flatnonzero(~undecidable & (got != grown))
    assert len(bad) == 0, "%s: %d decidable cases disagree, first %s" % (what, len(bad), bad[:5])
    assert min(got.sum(), (~got).sum()) >= len(got) // 100               # (the set does hold both answers)


def test_segments_against_dense_sampling():
    rng = np.random.default_rng(11)
    n = 20000
    lo, hi = _cells(rng, n)
    p0, p1 = _segments(rng, lo, hi)
    margin = np.where(rng.random(n) < 0.5, F(0), F(0.02)).astype(F)[:, None]
    got = ex.segment_cell(p0, p1, lo - margin, hi + margin)
    m64 = margin.astype(float)
    ans = [_sampled_distance(p0, p1, lo - m64 - g, hi + m64 + g) <= SAMPLING for g in (DELTA, -DELTA)]
    _hold(got, ans[0], ans[1], "segments")


def _capsule_set(rng, n):
    lo, hi = _cells(rng, n)
    c = (lo.astype(float) + hi) / 2 + rng.normal(size=(n, 3)) * 0.15
    prims = [ex.capsule(rng.uniform(0.01, 0.2), 0.0 if rng.random() < 0.02 else rng.uniform(0, 0.6),
                        ex.pose(rng, c[i], identity=rng.random() < 0.1)) for i in range(n)]
    return lo, hi, prims


def _capsule_axis(prims):
    T = np.stack([P.transform for P in prims])
    q = np.stack([P.param for P in prims])
    return T, q


def test_capsules_against_dense_sampling():
    rng = np.random.default_rng(12)
    n = 20000
    lo, hi, prims = _capsule_set(rng, n)
    T, q = _capsule_axis(prims)
    margin = F(0.0)
    hh = (F(0.5) * q[:, 1]).astype(F)
    p = (T[:, :3, 3] - hh[:, None] * T[:, :3, 2]).astype(F)
    d = (q[:, 1:2] * T[:, :3, 2]).astype(F)
    rr = (q[:, 0] + margin).astype(F)
    got = ex.segment_cell_d2(p, d, lo, hi) <= rr * rr
    one = np.array([ex.primitive_cells(prims[i], lo[i:i + 1], hi[i:i + 1], 0.0)[0] for i in range(0, n, 97)])
    assert np.array_equal(one, got[::97])                               # (primitive_cells is that rule)
    T64, q64 = T.astype(float), q.astype(float)
    a = T64[:, :3, 3] - 0.5 * q64[:, 1:2] * T64[:, :3, 2]
    b = T64[:, :3, 3] + 0.5 * q64[:, 1:2] * T64[:, :3, 2]
    ans = [_sampled_distance(a, b, lo.astype(float) - g, hi.astype(float) + g) <= q64[:, 0] + g + SAMPLING for g in (DELTA, -DELTA)]
    _hold(got, ans[0], ans[1], "capsules")


def test_spheres_against_the_closed_form():
    rng = np.random.default_rng(13)
    n = 20000
    lo, hi = _cells(rng, n)
    c = ((lo.astype(float) + hi) / 2 + rng.normal(size=(n, 3)) * 0.15).astype(F)
    r = rng.uniform(0.01, 0.2, n).astype(F)
    margin = np.where(rng.random(n) < 0.5, F(0), F(0.02)).astype(F)
    rr = (r + margin).astype(F)
    got = ex.point_cell_d2(c, lo, hi) <= rr * rr
    ans = [_dist_to_box(c.astype(float), lo.astype(float) - g, hi.astype(float) + g) <= rr.astype(float) + g for g in (DELTA, -DELTA)]
    _hold(got, ans[0], ans[1], "spheres")
    P = ex.sphere(r[0], c[0])
    assert ex.primitive_cells(P, lo[:1], hi[:1], margin[0])[0] == got[0]


def _box_depth(T, half, lo, hi):
    """fp64: the largest s such that some point lies s inside all twelve half-spaces (scipy's HiGHS); < 0: separated by
    -s.  Growing both shapes by g adds g."""
    from scipy.optimize import linprog
    T, half, lo, hi = (np.asarray(a, np.float64) for a in (T, half, lo, hi))
    A, b = [], []
    for k in range(3):
        e = np.eye(3)[k]
        A += [np.append(e, 1.0), np.append(-e, 1.0)]
        b += [hi[k], -lo[k]]
        u = T[:3, k] / np.linalg.norm(T[:3, k])
        A += [np.append(u, 1.0), np.append(-u, 1.0)]
        b += [half[k] + u @ T[:3, 3], half[k] - u @ T[:3, 3]]
    res = linprog([0, 0, 0, -1.0], A_ub=np.array(A), b_ub=np.array(b), bounds=[(None, None)] * 3 + [(None, 1.0)], method="highs")
    assert res.status == 0
    return res.x[3]


def test_boxes_against_linear_programming():
    rng = np.random.default_rng(14)
    n = 3000
    lo, hi = _cells(rng, n)
    c = (lo.astype(float) + hi) / 2 + rng.normal(size=(n, 3)) * 0.25
    got, depth = np.zeros(n, bool), np.zeros(n)
    for i in range(n):
        half = rng.uniform(0.01, 0.3, 3)
        P = ex.box(2 * half, ex.pose(rng, c[i], identity=(i % 10 == 0)))
        margin = 0.0 if i % 2 else 0.02
        got[i] = ex.primitive_cells(P, lo[i:i + 1], hi[i:i + 1], margin)[0]
        depth[i] = _box_depth(P.transform, P.param.astype(float) / 2, lo[i].astype(float) - margin, hi[i].astype(float) + margin)
    _hold(got, depth + DELTA >= 0, depth - DELTA >= 0, "boxes")


# ---------------------------------------------------------------------------------------------- other rules
def test_same_lattice_touching():
    o = np.array([0.3, -1.7, 2.9], F)
    vs = 0.05
    nb = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.int32) + np.array([4, -7, 2], np.int32)
    centre = ("voxel", np.array([[4, -7, 2]], np.int32), vs, o)
    got = ex.compute_intersection(centre, ("voxel", nb, vs, o))
    assert got[:, 1].tolist() == list(range(27)) and (got[:, 0] == 0).all()      # itself and all 26 neighbours
    far = ("voxel", np.array([[6, -7, 2]], np.int32), vs, o)
    assert len(ex.compute_intersection(centre, far, 0.0)) == 0
    assert len(ex.compute_intersection(centre, far, 0.049)) == 0
    assert len(ex.compute_intersection(centre, far, 0.0501)) == 1               # margin >= vs (and its rounding)
    with pytest.raises(ValueError):
        ex.compute_intersection(centre, far, -0.1)
    with pytest.raises(ValueError):
        ex.compute_intersection(centre, far, float("nan"))


def _brute_pairs(n_enum, n_other, accept, enum_first):
    out = []
    for i in range(n_enum):
        for j in range(n_other):
            if accept(i, j):
                out.append([i, j] if enum_first else [j, i])
                break
    return out


def test_smallest_index_and_ascending_order_against_brute_force():
    rng = np.random.default_rng(15)
    o = np.array([0.1, 0.2, -0.3], F)
    a_keys = rng.permutation(ex.shell_keys(rng, 150, radius=4.0, noise=0.8))      # unsorted
    b_keys = ex.shell_keys(rng, 120, radius=4.0, noise=0.8)
    a, b = ("voxel", a_keys, 0.1, o), ("voxel", b_keys, 0.13, o + F(0.037))
    alo, ahi = ex.cell_bounds(a_keys, 0.1, o)
    blo, bhi = ex.cell_bounds(b_keys, 0.13, o + F(0.037))
    for margin in (0.0, 0.02, 0.24):
        m = F(margin)
        want = _brute_pairs(len(b_keys), len(a_keys), lambda i, j: bool(((blo[i] - m <= ahi[j]) & (alo[j] <= bhi[i] + m)).all()), False)
        got = ex.compute_intersection(a, b, margin)
        assert got.tolist() == want and len(want) > 0
        assert (np.diff(got[:, 1]) > 0).all()
    pts = (rng.uniform(-0.6, 0.6, (40, 3)) + o).astype(F)
    lines = rng.integers(0, 40, (60, 2)).astype(np.int32)
    ls = ("lines", pts, lines)
    want = _brute_pairs(60, len(a_keys), lambda i, j: bool(ex.segment_cell(pts[lines[i, 0]], pts[lines[i, 1]], alo[j], ahi[j])), False)
    assert ex.compute_intersection(a, ls).tolist() == want and len(want) > 0
    assert ex.compute_intersection(ls, a).tolist() == [[q, p] for p, q in want]
    prims = ex.mixed_primitives(rng, 24, o - 0.6, o + 0.6)
    acc = np.stack([ex.primitive_cells(P, alo, ahi, 0.03) for P in prims])
    want = _brute_pairs(24, len(a_keys), lambda i, j: bool(acc[i, j]), False)
    assert ex.compute_intersection(a, ("prims", prims), 0.03).tolist() == want and len(want) > 0
    want = _brute_pairs(len(a_keys), 24, lambda i, j: bool(acc[j, i]), False)
    assert ex.compute_intersection(("prims", prims), a, 0.03).tolist() == want and len(want) > 0
    # an occupancy grid's voxels are named by their linear index
    idx = np.array([[3, 4, 5], [3, 4, 6], [9, 1, 1]], np.int32)
    occ = ("occ", idx, 16, 0.1, o)
    got = ex.compute_intersection(a, occ, 0.5)
    assert set(got[:, 1].tolist()) <= {(3 * 16 + 4) * 16 + 5, (3 * 16 + 4) * 16 + 6, (9 * 16 + 1) * 16 + 1} and len(got) > 0
    with pytest.raises(ValueError):
        ex.compute_intersection(occ, occ)
    with pytest.raises(ValueError):
        ex.compute_intersection(("prims", prims), ("prims", prims))
    with pytest.raises(ValueError):
        ex.compute_intersection(a, ("lines", pts, np.array([[0, 40]], np.int32)))


def _surface(P, rng, n=4000):
    """fp64 points on the primitive's surface"""
    T = P.transform.astype(float)
    if P.type == ex.BOX:
        u = rng.uniform(-1, 1, (n, 3))
        u[np.arange(n), rng.integers(0, 3, n)] = rng.choice([-1.0, 1.0], n)
        local = u * P.param.astype(float) / 2
    elif P.type == ex.SPHERE:
        d = rng.normal(size=(n, 3))
        local = d / np.linalg.norm(d, axis=1, keepdims=True) * float(P.param[0])
    else:
        r, h = float(P.param[0]), float(P.param[1])
        d = rng.normal(size=(n, 3))
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        z = rng.uniform(-h / 2, h / 2, n)
        if P.type == ex.CAPSULE:
            local = d * r + np.array([0, 0, 1.0]) * (np.sign(d[:, 2]) * h / 2)[:, None]
            side = rng.random(n) < 0.5
            ring = d[:, :2] / np.linalg.norm(d[:, :2], axis=1, keepdims=True) * r
            local[side] = np.concatenate([ring, z[:, None]], axis=1)[side]
        else:
            ring = d[:, :2] / np.linalg.norm(d[:, :2], axis=1, keepdims=True) * r
            rim = np.concatenate([ring * rng.random((n, 1)), (np.sign(d[:, 2]) * h / 2)[:, None]], axis=1)
            local = np.where((rng.random(n) < 0.5)[:, None], np.concatenate([ring, z[:, None]], axis=1), rim)
    return local @ T[:3, :3].T + T[:3, 3]


def test_bounding_boxes_contain_the_sampled_surface():
    rng = np.random.default_rng(16)
    for i in range(60):
        T = ex.pose(rng, rng.uniform(-2, 2, 3), identity=(i % 10 == 0))
        P = [ex.box(rng.uniform(0.05, 1.0, 3), T), ex.sphere(rng.uniform(0.05, 1.0), T[:3, 3]),
             ex.capsule(rng.uniform(0.05, 0.5), rng.uniform(0, 1.5), T), ex.cylinder(rng.uniform(0.05, 0.5), rng.uniform(0.1, 1.5), T)][i % 4]
        mn, mx = ex.primitive_aabb(P)
        s = _surface(P, rng)
        tol = 1e-5
        assert (s >= mn.astype(float) - tol).all() and (s <= mx.astype(float) + tol).all(), (i, P.type)
        assert (s.min(axis=0) <= mn + 0.12 * (mx - mn)).all() and (s.max(axis=0) >= mx - 0.12 * (mx - mn)).all()   # and is tight
    assert all((v == 0).all() for v in ex.primitive_aabb(ex.prim(ex.MESH)))


@pytest.mark.parametrize("which", ["box", "sphere", "capsule"])
def test_create_voxel_grid_equals_brute_force(which):
    rng = np.random.default_rng(17)
    P = {"box": ex.box((0.31, 0.22, 0.4), ex.pose(rng, (0.3, -0.2, 1.0), identity=True)),
         "sphere": ex.sphere(0.23, (1.0, 2.0, -0.5)),
         "capsule": ex.capsule(0.11, 0.37, ex.pose(rng, (-0.4, 0.1, 0.2)))}[which]
    vs = 0.05
    keys, origin = ex.create_voxel_grid(P, vs)
    assert np.array_equal(origin, P.transform[:3, 3]) and len(keys) > 20
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    assert np.array_equal(order, np.arange(len(keys)))                    # ascending
    (nw, nh, nd), _ = ex.voxelize_counts(P, vs)
    T0 = P.transform.copy()
    T0[:3, 3] = 0
    P0 = ex.Prim(P.type, T0, P.param)
    want = []
    for w in range(-(nw // 2), nw - nw // 2):
        for h in range(-(nh // 2), nh - nh // 2):
            for d in range(-(nd // 2), nd - nd // 2):
                lo, hi = ex.cell_bounds(np.array([[w, h, d]]), vs, np.zeros(3, F))
                if ex.primitive_cells(P0, lo, hi, 0.0)[0]:
                    want.append([w, h, d])
    assert keys.tolist() == want
    with pytest.raises(ValueError):
        ex.create_voxel_grid(P, 0.0)
    with pytest.raises(ValueError):
        ex.create_voxel_grid(ex.cylinder(0.1, 0.2), vs)


# ---------------------------------------------------------------------------------------------- the header
def _case(kind, margin=0.0, lo=(0, 0, 0), hi=(0, 0, 0), p0=(0, 0, 0), p1=(0, 0, 0), P=None):
    c = np.zeros(34, F)
    c[0], c[1], c[2:5], c[5:8], c[8:11], c[11:14] = kind, margin, lo, hi, p0, p1
    if P is not None:
        c[14], c[15:31], c[31:34] = P.type, P.transform.T.reshape(16), P.param
    return c


_SLAB_SHORT = 4000


def _slab_cases(rng, cases):
    """kind 4 of the host program: _SLAB_SHORT short segments (half length 3e-5 .. 3e-3, a fifth 1e-7 .. 0.1) through the
    corners and edges of a lattice of size 0.1 at origin 0 and 1, some nearly perpendicular to x, a quarter with a
    margin; then 1000 long ones, some with no extent along an axis.  -> how many"""
    def case(margin, origin, K, p0, p1):
        c = np.zeros(34, F)
        c[0], c[1], c[2:5], c[5], c[6], c[8:11], c[11:14] = 4, margin, origin, 0.1, K, p0, p1
        return c
    for i in range(_SLAB_SHORT):
        origin = float(i % 2)
        corner = rng.integers(-4, 5, 3) * 0.1 + origin
        if i % 3 == 0:
            corner = corner + np.array([0, 0, rng.uniform(0, 0.1)])
        hl = 10 ** rng.uniform(np.log10(3e-5), np.log10(3e-3)) if i % 5 else 10 ** rng.uniform(-7, -1)
        d = rng.normal(size=3)
        if i % 7 == 0:
            d[0] *= 10 ** rng.uniform(-7, -2)
        d /= np.linalg.norm(d)
        c0 = corner + rng.normal(size=3) * hl * 0.3
        cases.append(case(0.0 if i % 4 else 0.013, [origin] * 3, 6, c0 - d * hl, c0 + d * hl))
    for i in range(1000):
        origin = rng.uniform(-1, 1, 3)
        p0, p1 = rng.uniform(-1.2, 1.2, 3) + origin, rng.uniform(-1.2, 1.2, 3) + origin
        if i % 5 == 0:
            p1[0] = p0[0] + rng.normal() * 1e-6
        if i % 11 == 0:
            p1[1] = p0[1]
        cases.append(case(0.02 if i % 2 else 0.0, origin, 8, p0, p1))
    return _SLAB_SHORT + 1000


def test_header_equals_restatement_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_collision_predicates")
    src = os.path.join(ROOT, "tests", "cpp", "test_collision_predicates.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cupoch_amd", "csrc"), src, "-o", exe])
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["collision_predicates.h"]
    rng = np.random.default_rng(18)
    n = 3000
    lo, hi = _cells(rng, n)
    p0, p1 = _segments(rng, lo, hi)
    cases, want = [], []
    for i in range(n):
        cases.append(_case(0, 0.02 if i % 2 else 0.0, lo[i], hi[i], p0[i], p1[i]))
    m = np.where(np.arange(n) % 2 == 1, F(0.02), F(0)).astype(F)[:, None]
    want += ex.segment_cell(p0, p1, lo - m, hi + m).astype(float).tolist()
    prims = ex.mixed_primitives(rng, 1500, (-1, -1, -1), (1, 1, 1))
    plo, phi = _cells(rng, len(prims))
    for i, P in enumerate(prims):       # cells near the primitive, so that both answers occur
        c = P.transform[:3, 3] if np.isfinite(P.transform).all() else np.zeros(3, F)
        plo[i] = (c + rng.normal(size=3) * 0.1).astype(F)
        phi[i] = plo[i] + F(0.05)
        cases.append(_case(1, 0.03 if i % 3 == 0 else 0.0, plo[i], phi[i], P=P))
        want.append(float(ex.primitive_cells(P, plo[i:i + 1], phi[i:i + 1], 0.03 if i % 3 == 0 else 0.0)[0]))
    for P in prims[:200]:
        cases.append(_case(2, P=P))
    ranges = []
    for i in range(300):
        vs, origin = F(rng.uniform(0.01, 0.3)), F(rng.uniform(-3, 3))
        a = F(rng.uniform(-3, 3))
        b = F(a + rng.uniform(0, 1.0))
        klo, khi = int(rng.integers(-60, 0)), int(rng.integers(0, 60))
        ranges.append((a, b, vs, origin, klo, khi))
        cases.append(_case(3, vs, (a, 0, 0), (b, 0, 0), (klo, khi, origin)))
    n_slab = _slab_cases(rng, cases)
    inp, outp = str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")
    np.stack(cases).astype(F).tofile(inp)
    out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "ok"
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
    got = np.fromfile(outp, F).reshape(-1, 8)
    k = n + len(prims)
    assert np.array_equal(got[:k, 0], np.array(want, F))
    assert 0.01 < got[:n, 0].mean() < 0.99 and 0.01 < got[n:k, 0].mean() < 0.99      # (both answers occur)
    for j, P in enumerate(prims[:200]):
        mn, mx = ex.primitive_aabb(P)
        assert np.array_equal(got[k + j, :3], mn.astype(F), equal_nan=True) and np.array_equal(got[k + j, 3:6], mx.astype(F), equal_nan=True)
        assert bool(got[k + j, 6]) == ex.primitive_live(P)
    for j, (a, b, vs, origin, klo, khi) in enumerate(ranges):     # the candidate range is exactly the keys that pass
        keys = np.arange(klo, khi + 1)
        clo, chi = keys.astype(F) * vs + origin, (keys + 1).astype(F) * vs + origin
        ok = keys[(chi >= a) & (clo <= b)]
        k0, k1 = int(got[k + 200 + j, 0]), int(got[k + 200 + j, 1])
        assert (list(range(k0, k1 + 1)) == ok.tolist()) if len(ok) else (k0 > k1)
    # the line kernel's walk (segment_cells, segment_slab_cells per x) visits every cell segment_cell accepts -- short
    # segments through lattice corners and edges, where the predicate's FLT_EPSILON admits cells far from the segment,
    # among them -- and stays near the segment: a long segment's walk is a small part of its box
    slab = got[k + 200 + len(ranges):]
    assert len(slab) == n_slab and slab[:, 0].sum() > 5 * n_slab
    assert slab[:, 1].sum() == 0, np.flatnonzero(slab[:, 1])[:10]
    long_ = slab[_SLAB_SHORT:]
    assert long_[:, 2].sum() <= 3 * long_[:, 0].sum() and long_[:, 3].sum() >= 10 * long_[:, 0].sum()


# ---------------------------------------------------------------------------------------------- the surface
def test_abi_family_is_declared_exported_and_bound():
    from cupoch_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    names = re.findall(r"MI_ICP_API int (mi_icp_collision_\w+|mi_icp_primitive_\w+)\(", hdr)
    assert sorted(names) == ["mi_icp_collision_compute", "mi_icp_collision_sort_keys", "mi_icp_collision_voxelize_primitive",
                             "mi_icp_primitive_aabb"]
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(names) == set(re.findall(r" T (mi_icp_collision_\w+|mi_icp_primitive_\w+)", out))
    assert all(n in _lib.SIGNATURES for n in names)
    assert C.sizeof(_lib.Primitive) == 80
    L = _lib.load()
    assert all(hasattr(L, n) for n in _lib.SIGNATURES)
    for word in ("Not built: CreateFromVoxelGrid.  The collision queries are", "visualisation; OccupancyGrid::CreateFromVoxelGrid"):
        assert word in hdr


def test_statuses_and_bounding_boxes_without_a_device():
    from cupoch_amd import _lib, collision, geometry
    L = _lib.load()
    m = C.c_int64(7)
    side = _lib.CollisionSide()
    assert L.mi_icp_collision_compute(None, C.byref(side), C.byref(side), 0.0, None, 0, C.byref(m)) == _lib.MI_ICP_ERR_INVALID
    assert L.mi_icp_collision_voxelize_primitive(None, None, 0.1, None, None, 0, C.byref(m), None) == _lib.MI_ICP_ERR_INVALID
    assert L.mi_icp_primitive_aabb(None, None, None) == _lib.MI_ICP_ERR_INVALID
    rng = np.random.default_rng(19)
    T = ex.pose(rng, (0.5, -1.0, 2.0))
    for mine, theirs in ((collision.Box((0.3, 0.2, 0.7), T), ex.box((0.3, 0.2, 0.7), T)),
                         (collision.Sphere(0.4, (1, 2, 3)), ex.sphere(0.4, (1, 2, 3))),
                         (collision.Capsule(0.1, 0.8, T), ex.capsule(0.1, 0.8, T)),
                         (collision.Cylinder(0.1, 0.8, T), ex.cylinder(0.1, 0.8, T))):
        box = mine.get_axis_aligned_bounding_box()
        mn, mx = ex.primitive_aabb(theirs)
        assert np.array_equal(box.get_min_bound(), mn) and np.array_equal(box.get_max_bound(), mx)
        assert mine._record().tobytes() == ex.prim_records([theirs]).tobytes()
    assert collision.CollitionResult is collision.CollisionResult
    r = collision.CollisionResult()
    assert not r.is_collided() and r.get_collision_index_pairs().shape == (0, 2)
    assert [t.name for t in collision.Primitive.Type] == ["Unspecified", "Box", "Sphere", "Capsule", "Cylinder", "Mesh"]
    arr = collision.PrimitiveArray()
    arr.append(collision.Sphere(1.0))
    assert len(arr) == 1 and arr._records().nbytes == 80
    assert hasattr(geometry, "LineSet")
