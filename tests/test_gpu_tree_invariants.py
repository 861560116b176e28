"""GPU: invariants of the target tree as built (mi_icp_debug_get_tree) -- the facts the search's
exactness argument rests on (cupoch_amd/csrc/traverse.h):
  * the leaf lines hold every point exactly once, padding elsewhere;
  * a record's child boxes are the exact bounding boxes of the children's points;
  * a node's REGION (record floats 48..53, flag 54) contains no point of any other node in its
    interior -- what lets a lane whose search cube lies inside it stop looking elsewhere."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def get_tree(eng):
    info = (C.c_int64 * 5)()
    eng._chk(eng._L.mi_icp_debug_get_tree(eng._ctx, info, None, None))
    nts, nleaf, leaf_first, nrec, nt = [int(v) for v in info]
    rec = np.empty((nrec, 64), np.float32)
    lines = np.empty((nleaf, 32), np.float32)
    eng._chk(eng._L.mi_icp_debug_get_tree(eng._ctx, info, rec.ctypes.data_as(C.c_void_p), lines.ctypes.data_as(C.c_void_p)))
    return nts, nleaf, leaf_first, rec, lines, nt


def record_index(node):
    h = 1
    while h * 8 <= node:
        h *= 8
    return node - h + (h - 1) // 7


def check_tree(eng, pts, expect_all_flagged):
    eng.set_target(pts)
    nts, nleaf, leaf_first, rec, lines, nt = get_tree(eng)
    assert nt == len(pts) and nleaf == (nts + 7) // 8
    nts = nleaf * 8
    xyz = np.stack([lines[:, 0:8], lines[:, 8:16], lines[:, 16:24]], -1).reshape(-1, 3)      # slot -> coordinates
    orig = lines[:, 24:32].copy().view(np.int32).reshape(-1)
    real = orig >= 0
    assert np.array_equal(np.sort(orig[real]), np.arange(len(pts)))                           # a permutation
    assert np.array_equal(xyz[real], pts[orig[real]])
    assert np.isinf(xyz[~real]).all()

    # leaf-level records: child c of node leaf_first + a is leaf 8a + c
    n_ll = (nleaf + 7) // 8
    for a in np.random.default_rng(0).permutation(n_ll)[:300]:
        r = rec[record_index(leaf_first + a)]
        for c in range(8):
            L = 8 * a + c
            p = xyz[L * 8:(L + 1) * 8][real[L * 8:(L + 1) * 8]] if L < nleaf else np.zeros((0, 3), np.float32)
            pair, ab = c >> 1, c & 1
            mn = r[pair * 12 + np.array([0, 2, 4]) + ab]
            mx = r[pair * 12 + np.array([6, 8, 10]) + ab]
            if len(p):
                assert np.array_equal(mn, p.min(0)) and np.array_equal(mx, p.max(0))
            else:
                assert (mn > mx).all()                                                        # inverted: never hit

    # regions, level by level: node `first + t` covers slots [t * span, (t + 1) * span)
    finite = np.isfinite(xyz).all(1) & real
    flagged = total = excused = 0
    first, span = leaf_first, 64
    while first >= 1:
        count = (nts + span - 1) // span
        for t in range(count):
            r = rec[record_index(first + t)]
            lo, hi, flag = r[48:51], r[51:54], r[54:55].view(np.uint32)[0]
            mine = np.zeros(len(xyz), bool)
            mine[t * span:(t + 1) * span] = True
            if not (mine & real).any() or first == 1:      # (the root's own record is never consulted)
                continue
            total += 1
            if flag == 0:
                # (a TRI layout -- 3 * 2^k cells, kd_descend.h -- has kd-subtree nodes only inside its three parts: a node
                # that spans more cells than a part keeps its points' box and no flag)
                cells = nts // 4096
                if nts % 4096 == 0 and cells % 3 == 0 and span // 4096 > cells // 3:
                    excused += 1
                continue
            flagged += 1
            others = xyz[finite & ~mine]
            strictly_inside = ((others > lo) & (others < hi)).all(1)
            assert not strictly_inside.any(), (first, t, int(strictly_inside.sum()))
            own = xyz[finite & mine]
            inside = ((own >= lo) & (own <= hi)).all(1)
            # (near-ties at a median may sit outside: at most 1 % of the node's points -- and one point of a 64-slot node)
            assert len(own) - int(inside.sum()) <= max(1, len(own) // 100), (first, t, len(own), int(inside.sum()))
        if first == 1:
            break
        first //= 8
        span *= 8
    if expect_all_flagged:
        assert flagged + excused == total
    check_leaf_regions(eng, nleaf, xyz, finite)
    check_leaf_halos(eng, nleaf, xyz, finite)
    return flagged, total


def halo_reaches(wa, wb):
    """The eight reaches packed into a region record's floats 3 and 7 (nn_search.h: halo_reach_fraction)."""
    wa, wb = int(wa), int(wb)
    unit = np.array([wb & 0xffff0000], np.uint32).view(np.float32)[0] * np.float32(1.0 / 64.0)
    q = [(wa >> (6 * k)) & 63 for k in range(5)] + [(wb >> (6 * k)) & 63 for k in range(2)] + [(wa >> 30) | (((wb >> 12) & 15) << 2)]
    return [np.float32(unit * np.float32(v)) for v in q]


def check_leaf_halos(eng, nleaf, xyz, finite):
    """The halo lines (leaf_halo.h) of a leaf with region R hold points of OTHER leaves with their true
    coordinates and slots, ascending in slot inside a line; EVERY point of another leaf that is nearer to R
    (L-infinity distance to the box) than reach k -- packed into the region record -- is in the lines 0 .. k;
    the reaches ascend."""
    NL = 8
    halos = np.empty((nleaf, NL, 32), np.float32)
    eng._chk(eng._L.mi_icp_debug_get_leaf_halos(eng._ctx, halos.ctypes.data_as(C.c_void_p)))
    reg = np.empty((nleaf, 8), np.float32)
    eng._chk(eng._L.mi_icp_debug_get_leaf_regions(eng._ctx, reg.ctypes.data_as(C.c_void_p)))
    lo, hi = reg[:, 0:3], reg[:, 4:7]
    wa, wb = reg[:, 3].copy().view(np.uint32), reg[:, 7].copy().view(np.uint32)
    have = np.flatnonzero(wb != 0)
    leaf_of = np.arange(len(xyz)) // 8
    pts = xyz.astype(np.float64)
    with_points = long_reach = 0
    for L in np.random.default_rng(6).permutation(have)[:300]:
        foreign = finite & (leaf_of != L)
        up = pts - hi[L].astype(np.float64)                   # >= 0: on or beyond the upper face
        dn = lo[L].astype(np.float64) - pts                   # >= 0: on or beyond the lower face
        with np.errstate(invalid="ignore"):
            dist = np.maximum(np.maximum(up, dn).max(1), 0.0)
        reaches = halo_reaches(wa[L], wb[L])
        assert all(reaches[k] <= reaches[k + 1] for k in range(NL - 1)), (int(L), reaches)
        seen = set()
        for k in range(NL):
            must = np.flatnonzero(foreign & (dist < float(reaches[k])))
            line = halos[L, k]
            slots = line[24:32].copy().view(np.int32)
            used = slots >= 0
            assert (np.diff(slots[used]) > 0).all(), (int(L), k, slots)
            assert used.all() or not used[np.argmin(used):].any()                         # unused entries at the end
            got = np.stack([line[0:8], line[8:16], line[16:24]], -1)
            assert np.array_equal(got[used], xyz[slots[used]]), (int(L), k)
            assert np.isinf(got[~used]).all()
            assert foreign[slots[used]].all(), (int(L), k, "the leaf's own point, or padding")
            assert not (seen & set(slots[used].tolist()))
            seen |= set(slots[used].tolist())
            assert set(must.tolist()) <= seen, (int(L), k, float(reaches[k]), must[:5])
            with_points += int(used.any())
        long_reach += int(float(reaches[NL - 1]) > 0)
    assert len(have) == 0 or (with_points > 0 and long_reach > 0)
    return len(have)


def check_leaf_regions(eng, nleaf, xyz, finite):
    """A LEAF's region (mi_icp_debug_get_leaf_regions: what finishes a seeded query without a tree
    walk, nn_search.h) holds no point of any other leaf strictly inside; invalid ones are empty."""
    reg = np.empty((nleaf, 8), np.float32)
    eng._chk(eng._L.mi_icp_debug_get_leaf_regions(eng._ctx, reg.ctypes.data_as(C.c_void_p)))
    lo, hi = reg[:, 0:3], reg[:, 4:7]
    valid = (lo <= hi).all(1)
    leaf_of = np.arange(len(xyz)) // 8
    pts, owner = xyz[finite], leaf_of[finite]
    order = np.random.default_rng(5).permutation(np.flatnonzero(valid))[:400]
    for L in order:
        inside = ((pts > lo[L]) & (pts < hi[L])).all(1)
        assert not (inside & (owner != L)).any(), (int(L), int((inside & (owner != L)).sum()))
    # own points: inside the closed region except near-ties at a median
    own_ok = own_n = 0
    for L in order[:200]:
        mine = pts[owner == L]
        own_n += len(mine)
        own_ok += int(((mine >= lo[L]) & (mine <= hi[L])).all(1).sum())
    assert own_n == 0 or own_ok >= 0.98 * own_n
    return int(valid.sum())


def test_regions_uniform_cloud(eng):
    rng = np.random.default_rng(1)
    f, t = check_tree(eng, rng.random((60000, 3), dtype=np.float32), True)
    assert t > 900


def _layout_cells(n, fill=3300):
    """kd_cells.h cell_layout_for: the fewest cells -- 2^d or 3 * 2^k -- whose mean fill stays within `fill`"""
    d = 0
    while (fill << d) < n:
        d += 1
    k = 0
    while (3 * fill << k) < n:
        k += 1
    return (3 << k) if (3 << k) < (1 << d) else (1 << d)


def test_regions_small_and_tiny_clouds(eng):
    rng = np.random.default_rng(2)
    for n in (1, 9, 100, 3300, 3301, 4097, 6601, 9000, 9901, 13201):
        check_tree(eng, rng.random((n, 3), dtype=np.float32), True)


@pytest.mark.parametrize("n", [6601, 26401, 60000, 160000, 307200, 1000000, 5000000])
def test_cell_layouts_fill_their_groups_without_overflow(eng, n):
    """Round 5: 2^d or 3 * 2^k cells (kd_descend.h TRI) with planes from histograms over the sample (kd_planes.h): on
    uniform data every cell stays within its one 4096-slot group -- the tree has exactly as many groups as the layout
    has cells -- although the mean fill now goes up to 80 % (it was held below two thirds because the sampled medians
    left the counts +-12 %); the fullest cell says how much room is left."""
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3), dtype=np.float32)
    eng.set_target(pts)
    nts, nleaf, leaf_first, rec, lines, nt = get_tree(eng)
    cells = _layout_cells(n)
    assert nts == cells * 4096, (n, nts // 4096, cells)          # one group per cell: no cell overflowed
    idx = lines[:, 24:32].copy().view(np.int32).reshape(cells, 4096)
    counts = (idx >= 0).sum(1)
    assert counts.sum() == n
    mean = n / cells
    assert counts.max() <= 4096 and counts.max() <= 1.25 * mean + 64, (n, cells, int(counts.max()), mean)
    assert counts.min() >= 0.75 * mean - 64, (n, cells, int(counts.min()), mean)


def test_regions_clustered_planar_and_quantised(eng):
    rng = np.random.default_rng(3)
    clustered = np.concatenate([c + rng.normal(0, 0.003, (s, 3)).astype(np.float32)
                                for c, s in zip(rng.random((40, 3)).astype(np.float32), rng.integers(5, 3000, 40))])
    check_tree(eng, clustered, False)
    planar = rng.random((30000, 3), dtype=np.float32)
    planar[:, 2] = 0.25                                                                       # one axis constant
    check_tree(eng, planar, False)
    grid = np.round(rng.random((40000, 3)) * 32).astype(np.float32) / 32                      # many equal coordinates
    check_tree(eng, grid, False)


def test_overflowing_cell_has_no_regions_but_the_rest_does(eng):
    rng = np.random.default_rng(4)
    pts = np.concatenate([rng.random((30000, 3), dtype=np.float32),
                          np.tile(np.array([[0.5, 0.5, 0.5]], np.float32), (20000, 1))])    # 20k copies: several groups
    flagged, total = check_tree(eng, pts, False)
    assert 0 < flagged < total


@pytest.mark.parametrize("n", [70000, 307200, 1000000, 3000000])
def test_locate_by_planes_finds_the_leaf_a_target_point_lives_in(eng, n):
    """The binary descent through the cell planes and the group's own planes (nn_search.h locate_by_planes; seeds of a
    first pass with halos and of every re-location) must land in the leaf that HOLDS a point when the query is that
    point: any leaf is a valid seed, so the search tests cannot see a descent that lands next door -- only its cost
    does.  The target's own points as the source, under the identity: all but a handful (a coordinate equal to a plane
    through a quantised median, kd_refine.h) are found where they are stored."""
    rng = np.random.default_rng(n + 7)
    pts = rng.random((n, 3), dtype=np.float32)
    eng.set_target(pts)
    eng.set_source(pts)
    nts, nleaf, leaf_first, rec, lines, nt = get_tree(eng)
    orig = lines[:, 24:32].copy().view(np.int32).reshape(-1)
    lives = np.empty(n, np.int64)
    real = orig >= 0
    lives[orig[real]] = np.nonzero(real)[0] >> 3
    got = np.empty(n, np.int32)
    eng._chk(eng._L.mi_icp_debug_locate(eng._ctx, None, got.ctypes.data_as(C.c_void_p)))
    wrong = np.nonzero(got != lives)[0]
    assert len(wrong) <= max(4, n // 20000), (n, len(wrong), got[wrong[:8]], lives[wrong[:8]])
    # ... and the search that starts from those seeds finds every point at distance 0
    idx, d2, _ = eng.search_radius_1nn(0.01, None)
    assert (d2 == 0.0).all() and (pts[idx] == pts).all()
    # A query a hair away from a target point (a converged registration's: 0.005 point spacings per coordinate) is
    # still found in that point's leaf unless the point lies that close to one of the leaf's faces (~1.5 %).  While a
    # split's plane was the median element's own coordinate one point in eight lay exactly ON a plane and its
    # neighbourhood fell on either side: 92 % instead of 98.5 (kd_refine.h kd_plane_between).
    s = float(n) ** (-1.0 / 3.0)
    near = (pts + rng.normal(0.0, 0.005 * s, pts.shape)).astype(np.float32)
    eng.set_source(near)
    eng._chk(eng._L.mi_icp_debug_locate(eng._ctx, None, got.ctypes.data_as(C.c_void_p)))
    right = float((got == lives).mean())
    assert right >= 0.97, (n, right)
