"""collision.compute_intersection and create_voxel_grid on the GPU, through the Python mirror, against the numpy
restatement of the contract (tests/collision_exact.py): the pairs are array_equal, always.  Voxels against voxels at
three size ratios, three margins, sorted and shuffled targets and every enumerated count around a wave and a block;
occupancy grids whose bounds box cuts the occupied set, as either argument; lines (random, on cell faces, of length
zero, far outside, not finite, one diagonal across a 128^3 grid) and primitives (rotated boxes, a sphere larger than the
grid, a capsule of height 0, a cylinder) against both grid types in both orders; the edge rules; CreateVoxelGrid."""
import ctypes as C

import numpy as np
import pytest

import collision_exact as ex

pytestmark = pytest.mark.gpu
F = np.float32
VS, ORIGIN = 0.1, np.array([0.3, -0.2, 0.1], F)


def to_np(v):
    return np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def vgrid(keys, vs, origin, is_sorted):
    """a geometry.VoxelGrid with these keys: through add_voxels (ascending, flagged sorted) or taken as given"""
    from cupoch_amd import geometry
    g = geometry.VoxelGrid()
    g.voxel_size, g.origin = float(vs), np.asarray(origin, F)
    keys = np.ascontiguousarray(keys, np.int32).reshape(-1, 3)
    if len(keys) == 0:
        return g
    if is_sorted:
        g.add_voxels((keys, np.ones((len(keys), 3), F)))
        assert g._sorted and np.array_equal(to_np(g.voxels.grid_index), keys)
    else:
        g.voxels = (keys, np.ones((len(keys), 3), F))
        assert not g._sorted
    return g


def lineset(points, lines):
    from cupoch_amd import geometry
    return geometry.LineSet(np.ascontiguousarray(points, F), np.ascontiguousarray(lines, np.int32))


def primitive_array(prims):
    from cupoch_amd import collision
    out = collision.PrimitiveArray()
    for P in prims:
        if P.type == ex.BOX:
            out.append(collision.Box(P.param, P.transform))
        elif P.type == ex.SPHERE:
            s = collision.Sphere(P.param[0])
            s.transform = P.transform.copy()
            out.append(s)
        elif P.type == ex.CAPSULE:
            out.append(collision.Capsule(P.param[0], P.param[1], P.transform))
        else:
            out.append(collision.Cylinder(P.param[0], P.param[1], P.transform))
    assert out._records().tobytes() == ex.prim_records(prims).tobytes()
    return out


def pairs_of(a, b, margin=0.0):
    from cupoch_amd import collision
    r = collision.compute_intersection(a, b, margin)
    p = r.get_collision_index_pairs()
    assert r.is_collided() == (len(p) > 0) and p.dtype == np.int32 and p.shape[1:] == (2,)
    assert np.array_equal(r.get_first_collision_indices(), p[:, 0]) and np.array_equal(r.get_second_collision_indices(), p[:, 1])
    return p, r


def pairs_from(acc, eidx, oidx, enumerated_first):
    """the contract's result from an acceptance matrix [enumerated, other] and the two sides' pair indices"""
    big = np.iinfo(np.int64).max
    other = np.where(acc, np.asarray(oidx, np.int64)[None, :], big).min(axis=1) if acc.shape[1] else np.full(len(acc), big)
    rows = np.flatnonzero(other != big)
    cols = [np.asarray(eidx)[rows], other[rows]] if enumerated_first else [other[rows], np.asarray(eidx)[rows]]
    return np.stack(cols, axis=1).astype(np.int32)


# ---------------------------------------------------------------------------------------------- voxels against voxels
@pytest.fixture(scope="module")
def shell():
    return ex.shell_keys(np.random.default_rng(1), 3000)


@pytest.mark.parametrize("ratio", [0.3, 1.0, 3.3])
@pytest.mark.parametrize("margin_voxels", [0.0, 0.2, 2.4])
def test_voxels_against_voxels(shell, ratio, margin_voxels):
    rng = np.random.default_rng(int(ratio * 10) * 7 + int(margin_voxels * 10))
    vs_q, origin_q, margin = VS * ratio, ORIGIN + F(0.37 * VS), margin_voxels * VS
    reach = (np.array([[-19.0, -14.0, -21.0], [13.0, 18.0, 11.0]]) * VS + ORIGIN - origin_q) / vs_q   # the shell's box and a rim
    q_keys = rng.integers(np.floor(reach[0] - 2), np.ceil(reach[1] + 2), (4097, 3)).astype(np.int32)
    shuffle = rng.permutation(len(shell))
    a_sorted, a_shuffled = vgrid(shell, VS, ORIGIN, True), vgrid(shell[shuffle], VS, ORIGIN, False)
    acc, _ = ex._accept_matrix_rows(("voxel", q_keys, vs_q, origin_q), ("voxel", shell, VS, ORIGIN), margin)
    position = np.empty(len(shell), np.int64)
    position[shuffle] = np.arange(len(shell))                        # where a sorted voxel sits in the shuffled grid
    hits = 0
    for n in (1, 63, 64, 65, 4097):
        b = vgrid(q_keys[:n], vs_q, origin_q, False)
        want = pairs_from(acc[:n], np.arange(n), np.arange(len(shell)), False)
        got, r = pairs_of(a_sorted, b, margin)
        assert np.array_equal(got, want), (n, len(got), len(want))
        assert np.array_equal(pairs_of(a_shuffled, b, margin)[0], pairs_from(acc[:n], np.arange(n), position, False)), n
        hits += len(want)
    assert r.first.name == "VoxelGrid" and r.second.name == "VoxelGrid" and 0 < hits < 5 * 4097
    assert np.array_equal(want, ex.compute_intersection(("voxel", shell, VS, ORIGIN), ("voxel", q_keys, vs_q, origin_q), margin))


def test_reference_unit_tests_and_the_lattice():
    from cupoch_amd import geometry
    o = np.zeros(3, F)
    assert len(pairs_of(geometry.VoxelGrid(), geometry.VoxelGrid())[0]) == 0
    v1, v2 = vgrid([[0, 0, 0], [5, 0, 0]], 1.0, o, False), vgrid([[0, 0, 0], [10, 0, 0]], 1.0, o, False)
    assert pairs_of(v1, v2)[0].tolist() == [[0, 0]]
    assert len(pairs_of(geometry.VoxelGrid(), geometry.LineSet())[0]) == 0
    ls = lineset([[-0.1, -0.1, -0.1], [-0.1, -0.1, 1.1], [1.1, 1.1, 1.1]], [[0, 1], [0, 2]])
    assert pairs_of(v1, ls)[0].tolist() == [[0, 1]] and pairs_of(ls, v1)[0].tolist() == [[1, 0]]
    nb = np.array([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.int32) + np.array([4, -7, 2], np.int32)
    centre, ring = vgrid([[4, -7, 2]], 0.05, ORIGIN, True), vgrid(nb, 0.05, ORIGIN, True)
    assert pairs_of(centre, ring)[0].tolist() == [[0, i] for i in range(27)]
    far = vgrid([[6, -7, 2]], 0.05, ORIGIN, True)
    assert [len(pairs_of(centre, far, m)[0]) for m in (0.0, 0.049, 0.0501)] == [0, 0, 1]


# ---------------------------------------------------------------------------------------------- occupancy grids
def occupancy(res, seed):
    """-> (OccupancyGrid, its side for the restatement): a noisy sphere seen from inside, then a free box that cuts it"""
    from cupoch_amd import geometry
    rng = np.random.default_rng(seed)
    g = geometry.OccupancyGrid(VS, res, ORIGIN)
    d = rng.normal(size=(4000, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    half = res * VS / 2
    g.insert((d * (0.62 * half + rng.normal(size=(4000, 1)) * 0.04) + ORIGIN).astype(F), ORIGIN + F(0.01))
    everything = len(g.extract_occupied_voxels())
    g.set_free_area(ORIGIN + F(-0.75 * half), ORIGIN + np.array([0.55, 0.8, 0.35], F) * F(half))
    idx = to_np(g.extract_occupied_voxels().grid_index).astype(np.int32)
    assert 50 < len(idx) < everything                                   # the bounds box cuts the occupied set
    return g, ("occ", idx, res, VS, ORIGIN)


@pytest.fixture(scope="module", params=[32, 33, 64])
def occ(request):
    return occupancy(request.param, request.param)


def test_occupancy_grid_against_voxels_either_way(occ, shell):
    g, side = occ
    res = side[2]
    rng = np.random.default_rng(res)
    keys = np.unique(rng.integers(-res // 3, res // 3, (700, 3)), axis=0).astype(np.int32)
    vs_v, origin_v = VS * 1.7, ORIGIN + F(0.037)
    keys = (keys / 1.7).astype(np.int32)
    keys = np.unique(keys, axis=0)
    for is_sorted in (True, False):
        k = keys if is_sorted else rng.permutation(keys)
        v, vside = vgrid(k, vs_v, origin_v, is_sorted), ("voxel", k, vs_v, origin_v)
        for margin in (0.0, 0.03):
            want = ex.compute_intersection(vside, side, margin)
            got, r = pairs_of(v, g, margin)
            assert np.array_equal(got, want) and len(want) > 0
            assert r.first.name == "VoxelGrid" and r.second.name == "OccupancyGrid"
            want = ex.compute_intersection(side, vside, margin)
            assert np.array_equal(pairs_of(g, v, margin)[0], want) and len(want) > 0
    from cupoch_amd import MiIcpError
    with pytest.raises(MiIcpError):
        pairs_of(g, g)


# ---------------------------------------------------------------------------------------------- lines
def line_scene(rng, lo, hi, vs, origin):
    span = hi - lo
    pts = [rng.uniform(lo - 0.15 * span, hi + 0.15 * span, (700, 3))]
    lines = [rng.integers(0, 700, (500, 2))]
    n = 700

    def add(p, q):
        nonlocal n
        pts.append(np.array([p, q], float))
        lines.append(np.array([[n, n + 1]]))
        n += 2
    for i in range(30):                                                # axis-aligned, lying on cell faces
        k = rng.integers(-6, 6, 3)
        a = (k.astype(F) * F(vs) + origin).astype(float)
        b = a.copy()
        b[i % 3] += float(rng.integers(1, 9)) * vs
        add(a, b)
    for i in range(20):                                                # of length zero: in space, and on lattice corners
        p = rng.uniform(lo, hi) if i % 2 else (rng.integers(-6, 6, 3).astype(F) * F(vs) + origin).astype(float)
        add(p, p)
    for i in range(10):                                                # end points far outside the grid
        d = rng.normal(size=3)
        c = rng.uniform(lo + 0.3 * span, hi - 0.3 * span)
        add(c - d * 1.0e4, c + d * (1.0e4 if i % 2 else 0.0))
    add([np.nan, 0, 0], (lo + hi) / 2)
    add((lo + hi) / 2, [0, np.inf, 0])
    return np.concatenate(pts).astype(F), np.concatenate(lines).astype(np.int32)


def test_lines_against_both_grids(occ, shell):
    g, side = occ
    res = side[2]
    rng = np.random.default_rng(100 + res)
    half = res * VS / 2
    pts, lines = line_scene(rng, ORIGIN - 0.8 * half, ORIGIN + 0.8 * half, VS, ORIGIN)
    ls, lside = lineset(pts, lines), ("lines", pts, lines)
    for margin in (0.0, 0.03):
        want = ex.compute_intersection(side, lside, margin)
        got, r = pairs_of(g, ls, margin)
        assert np.array_equal(got, want) and 20 < len(want) < len(lines), (len(got), len(want))
        assert r.first.name == "OccupancyGrid" and r.second.name == "LineSet"
        assert np.array_equal(pairs_of(ls, g, margin)[0], want[:, ::-1])        # the lines are enumerated either way
    if res != 64:
        return
    pts, lines = line_scene(rng, ORIGIN - 1.6, ORIGIN + 1.6, VS, ORIGIN)
    ls, lside = lineset(pts, lines), ("lines", pts, lines)
    shuffle = rng.permutation(len(shell))
    for is_sorted in (True, False):
        k = shell if is_sorted else shell[shuffle]
        v, vside = vgrid(k, VS, ORIGIN, is_sorted), ("voxel", k, VS, ORIGIN)
        for margin in (0.0, 0.03):
            want = ex.compute_intersection(vside, lside, margin)
            assert np.array_equal(pairs_of(v, ls, margin)[0], want) and len(want) > 20
            assert np.array_equal(pairs_of(ls, v, margin)[0], want[:, ::-1])


@pytest.mark.parametrize("origin", [0.0, 1.0])
def test_short_segments_through_lattice_corners_and_edges(origin):
    """segment_cell adds FLT_EPSILON to |dst| before its cross-axis tests, so a segment of length 1e-4 that passes a
    corner diagonally is accepted by cells about 1e-4 away from it, which its own slab-by-slab y / z range does not
    reach: the walk has to widen by that term.  Half the lattice is occupied, so such a cell is often the only hit or
    the one with the smallest index."""
    from cupoch_amd import geometry
    rng = np.random.default_rng(300 + int(origin))
    o3 = np.full(3, origin, F)
    n = 2000
    corner = rng.integers(-4, 5, (n, 3)) * VS + origin
    corner[::3, 2] += rng.uniform(0, VS, len(corner[::3]))                          # on an edge, not a corner
    hl = 10 ** rng.uniform(np.log10(3e-5), np.log10(3e-3), (n, 1))
    d = rng.normal(size=(n, 3))
    d[::7, 0] *= 10 ** rng.uniform(-7, -2, len(d[::7]))                             # nearly perpendicular to x
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c0 = corner + rng.normal(size=(n, 3)) * hl * 0.3
    pts = np.concatenate([c0 - d * hl, c0 + d * hl]).astype(F)
    lines = np.stack([np.arange(n), np.arange(n) + n], axis=1).astype(np.int32)
    ls, lside = lineset(pts, lines), ("lines", pts, lines)
    full = np.stack(np.meshgrid(*[np.arange(-6, 6)] * 3, indexing="ij"), axis=-1).reshape(-1, 3).astype(np.int32)
    keys = full[rng.random(len(full)) < 0.5]
    shuffle = rng.permutation(len(keys))
    res = 16
    g = geometry.OccupancyGrid(VS, res, o3)
    idx = keys[np.abs(keys + 0.5).max(axis=1) < 6] + res // 2
    g.add_voxels(idx, occupied=True)
    assert np.array_equal(to_np(g.extract_occupied_voxels().grid_index), idx)
    for margin in (0.0, 0.013):
        want = ex.compute_intersection(("voxel", keys, VS, o3), lside, margin)
        assert n // 2 < len(want) <= n
        assert np.array_equal(pairs_of(vgrid(keys, VS, o3, True), ls, margin)[0], want)
        k = keys[shuffle]
        assert np.array_equal(pairs_of(ls, vgrid(k, VS, o3, False), margin)[0], ex.compute_intersection(lside, ("voxel", k, VS, o3), margin))
        assert np.array_equal(pairs_of(g, ls, margin)[0], ex.compute_intersection(("occ", idx, res, VS, o3), lside, margin))


def test_a_diagonal_across_a_plane_of_a_128_grid():
    from cupoch_amd import geometry
    res, x = 128, 70
    g = geometry.OccupancyGrid(VS, res, ORIGIN)
    yz = np.stack(np.meshgrid(np.arange(res), np.arange(res), indexing="ij"), axis=-1).reshape(-1, 2)
    idx = np.concatenate([np.full((len(yz), 1), x), yz], axis=1).astype(np.int32)
    g.add_voxels(idx, occupied=True)
    assert np.array_equal(to_np(g.extract_occupied_voxels().grid_index), idx)
    half = res * VS / 2
    corner = np.array([half, half, half], F)
    pts = np.stack([ORIGIN - corner, ORIGIN + corner, ORIGIN + corner * np.array([1, -1, 1], F), ORIGIN - corner * np.array([1, -1, 1], F),
                    ORIGIN + np.array([0.61, -half, 0.25], F), ORIGIN + np.array([0.61, half, 0.25], F),    # inside the plane's slab
                    ORIGIN + np.array([0.2, -1, 0.2], F), ORIGIN + np.array([0.4, 1, 3.0], F)]).astype(F)   # beside it
    lines = np.array([[0, 1], [2, 3], [1, 0], [4, 5], [6, 7]], np.int32)
    side, lside = ("occ", idx, res, VS, ORIGIN), ("lines", pts, lines)
    for margin in (0.0, 0.03, 0.5):
        want = ex.compute_intersection(side, lside, margin)
        assert np.array_equal(pairs_of(g, lineset(pts, lines), margin)[0], want)
        if margin == 0.0:
            assert want[:, 1].tolist() == [0, 1, 2, 3] and want[3, 0] == (x * res + 0) * res + 66


# ---------------------------------------------------------------------------------------------- primitives
def test_primitives_against_both_grids(occ, shell):
    g, side = occ
    res = side[2]
    rng = np.random.default_rng(200 + res)
    half = res * VS / 2
    n = 200 if res == 64 else 60
    prims = ex.mixed_primitives(rng, n, ORIGIN - 0.7 * half, ORIGIN + 0.7 * half)
    arr = primitive_array(prims)
    olo, ohi, oidx = ex.side_cells(side)
    for margin in (0.0, 0.03):
        acc = np.stack([ex.primitive_cells(P, olo, ohi, margin) for P in prims])
        assert acc[3].all() and not acc[6].any() and not acc[7].any()          # the large sphere; the cylinder; the NaN
        want = pairs_from(acc, np.arange(n), oidx, False)
        got, r = pairs_of(g, arr, margin)
        assert np.array_equal(got, want) and 3 < len(want) < n, (len(got), len(want))
        assert r.first.name == "OccupancyGrid" and r.second.name == "Primitives"
        want = pairs_from(acc.T, oidx, np.arange(n), False)
        assert np.array_equal(pairs_of(arr, g, margin)[0], want) and len(want) == len(oidx)
    if res != 64:
        return
    prims = ex.mixed_primitives(rng, 200, ORIGIN - 1.7, ORIGIN + 1.5)
    arr = primitive_array(prims)
    shuffle = rng.permutation(len(shell))
    position = np.empty(len(shell), np.int64)
    position[shuffle] = np.arange(len(shell))
    slo, shi = ex.cell_bounds(shell, VS, ORIGIN)
    v_sorted, v_shuffled = vgrid(shell, VS, ORIGIN, True), vgrid(shell[shuffle], VS, ORIGIN, False)
    for margin in (0.0, 0.03):
        acc = np.stack([ex.primitive_cells(P, slo, shi, margin) for P in prims])
        want = pairs_from(acc, np.arange(200), np.arange(len(shell)), False)
        assert np.array_equal(pairs_of(v_sorted, arr, margin)[0], want) and len(want) > 10
        assert np.array_equal(pairs_of(v_shuffled, arr, margin)[0], pairs_from(acc, np.arange(200), position, False))
        want = pairs_from(acc.T, np.arange(len(shell)), np.arange(200), False)
        assert np.array_equal(pairs_of(arr, v_sorted, margin)[0], want) and len(want) == len(shell)
        assert np.array_equal(pairs_of(arr, v_shuffled, margin)[0], pairs_from(acc.T[shuffle], np.arange(len(shell)), np.arange(200), False))
    # a box whose rotation is scaled is refused, as either argument and when voxelised; the same box unscaled collides
    from cupoch_amd import MiIcpError, _lib, collision
    T = ex.pose(rng, ORIGIN + np.array([0, 0, 1.4], F))
    good, bad = ex.box((0.5, 0.5, 0.5), T), ex.box((0.5, 0.5, 0.5), T * np.array([1.01, 1.01, 1.01, 1], F)[None, :])
    assert len(pairs_of(v_sorted, primitive_array([good]))[0]) == 1
    for args in ((v_sorted, primitive_array([good, bad])), (primitive_array([bad]), v_sorted), (g, primitive_array([bad]))):
        with pytest.raises(MiIcpError) as e:
            pairs_of(*args)
        assert e.value.code == _lib.MI_ICP_ERR_INVALID
    with pytest.raises(ValueError):
        ex.compute_intersection(("voxel", shell, VS, ORIGIN), ("prims", [good, bad]))
    with pytest.raises(ValueError):
        ex.create_voxel_grid(bad, 0.05)
    assert len(collision.create_voxel_grid(primitive_array([bad])[0], 0.05)) == 0       # (logged, as the other refusals are)
    assert len(pairs_of(v_sorted, primitive_array([good]))[0]) == 1                   # the context still works


# ---------------------------------------------------------------------------------------------- edge rules
def test_edge_rules(shell):
    from cupoch_amd import MiIcpError, _lib, collision, geometry
    v = vgrid(shell, VS, ORIGIN, True)
    assert len(pairs_of(v, geometry.VoxelGrid())[0]) == 0 and len(pairs_of(geometry.VoxelGrid(), v)[0]) == 0
    assert len(pairs_of(v, geometry.LineSet())[0]) == 0 and len(pairs_of(collision.PrimitiveArray(), v)[0]) == 0
    assert len(pairs_of(v, lineset(np.zeros((2, 3)), np.zeros((0, 2))))[0]) == 0
    for margin in (-0.01, float("nan"), float("inf")):
        with pytest.raises(MiIcpError) as e:
            pairs_of(v, v, margin)
        assert e.value.code == _lib.MI_ICP_ERR_INVALID
    with pytest.raises(MiIcpError):
        collision.compute_intersection(collision.PrimitiveArray([collision.Sphere(1.0)]), collision.PrimitiveArray([collision.Sphere(1.0)]))
    with pytest.raises(TypeError):
        collision.compute_intersection(v, 3)
    # the capacity rule, and an out-of-range line index: nothing is written
    import torch
    eng = v._eng()
    pts = ((shell[:40].astype(F) + F(0.5)) * F(VS) + ORIGIN).astype(F)                 # voxel centres
    lines = np.stack([np.arange(0, 40, 2), np.arange(1, 40, 2)], axis=1).astype(np.int32)
    want = ex.compute_intersection(("voxel", shell, VS, ORIGIN), ("lines", pts, lines))
    assert len(want) == 20                                                          # every line starts inside a voxel
    a = eng.collision_voxel_side(v._arrays()[0], VS, ORIGIN, True)
    out = torch.full((32, 2), -7, dtype=torch.int32, device="cuda")
    for capacity, written in ((0, False), (19, False), (20, True)):
        b = eng.collision_lineset_side(pts, lines)
        out.fill_(-7)
        m = C.c_int64(-1)
        rc = eng._L.mi_icp_collision_compute(eng._ctx, C.byref(a[0]), C.byref(b[0]), 0.0, C.c_void_p(out.data_ptr()), capacity, C.byref(m))
        eng.synchronize()
        assert rc == 0 and m.value == 20
        host = out.cpu().numpy()
        assert np.array_equal(host[:20], want) if written else (host == -7).all()
        assert (host[20:] == -7).all()
    for bad in ([[0, 40]], [[-1, 3]]):
        b = eng.collision_lineset_side(pts, np.concatenate([lines, np.array(bad, np.int32)]))
        out.fill_(-7)
        m = C.c_int64(-1)
        rc = eng._L.mi_icp_collision_compute(eng._ctx, C.byref(a[0]), C.byref(b[0]), 0.0, C.c_void_p(out.data_ptr()), 32, C.byref(m))
        eng.synchronize()
        assert rc == _lib.MI_ICP_ERR_INVALID and m.value == 0 and (out.cpu().numpy() == -7).all()
    assert np.array_equal(pairs_of(v, lineset(pts, lines))[0], want)                # the context still works


def test_far_apart_voxels_cost_by_the_voxels_that_exist(shell):
    """three voxels 9e8 keys apart: a line or a primitive that spans them is walked over the x that have a key (three
    slabs, not 1.8e9), and a voxel query whose inflated box covers key extents of 2e9 x 2e9 walks the three voxels
    between the corners (the count of columns there does not fit 64 bits times 8).  Pairs equal the restatement's."""
    eng = vgrid(shell[:4], VS, ORIGIN, True)._eng()
    zero = np.zeros(3, F)

    def run(a, b, margin=0.0):
        return to_np(eng.collision_compute(a, b, margin))
    far = 900000000
    keys = np.array([[-far, 0, 0], [0, 0, 0], [far, 0, 0]], np.int32)
    pts = np.array([[-1e9, 0.5, 0.5], [1e9, 0.5, 0.5], [1e8, 0.5, 0.5], [-1e9, 1e6, 0.5], [1e9, 1e6, 0.5]], F)
    lines = np.array([[0, 1], [2, 1], [3, 4], [1, 0]], np.int32)
    want = ex.compute_intersection(("voxel", keys, 1.0, zero), ("lines", pts, lines))
    assert want.tolist() == [[0, 0], [2, 1], [0, 3]]
    assert np.array_equal(run(eng.collision_voxel_side(keys, 1.0, zero, True), eng.collision_lineset_side(pts, lines)), want)
    prims = [ex.sphere(2e9), ex.sphere(1000.0, (far, 0, 0)), ex.sphere(10.0, (4e8, 0, 0)), ex.box((2e9, 1, 1)), ex.capsule(1.0, 2e9)]
    want = ex.compute_intersection(("voxel", keys, 1.0, zero), ("prims", prims))
    assert want.tolist() == [[0, 0], [2, 1], [0, 3], [1, 4]]
    assert np.array_equal(run(eng.collision_voxel_side(keys, 1.0, zero, True), eng.collision_primitives_side(ex.prim_records(prims))), want)
    wide = np.array([[-1000000000, -1000000000, 0], [0, 0, 0], [1000000000, 1000000000, 0]], np.int32)
    query = np.array([[0, 0, 0], [5, 5, 0]], np.int32)
    for margin in (0.0, 3e9):
        want = ex.compute_intersection(("voxel", wide, 1.0, zero), ("voxel", query, 1.0, zero), margin)
        assert want.tolist() == ([[1, 0]] if margin == 0 else [[0, 0], [0, 1]])
        assert np.array_equal(run(eng.collision_voxel_side(wide, 1.0, zero, True), eng.collision_voxel_side(query, 1.0, zero, True), margin), want)


# ---------------------------------------------------------------------------------------------- CreateVoxelGrid, LineSet
@pytest.mark.parametrize("which", ["box", "rotated_box", "sphere", "capsule"])
def test_create_voxel_grid(which):
    from cupoch_amd import collision
    rng = np.random.default_rng(17)
    P = {"box": ex.box((0.31, 0.22, 0.4), ex.pose(rng, (0.3, -0.2, 1.0), identity=True)),
         "rotated_box": ex.box((0.31, 0.22, 0.4), ex.pose(rng, (0.3, -0.2, 1.0))),
         "sphere": ex.sphere(0.23, (1.0, 2.0, -0.5)),
         "capsule": ex.capsule(0.11, 0.37, ex.pose(rng, (-0.4, 0.1, 0.2)))}[which]
    mine = primitive_array([P])[0]
    for vs in (0.05, 0.013):
        keys, origin = ex.create_voxel_grid(P, vs)
        g = collision.create_voxel_grid(mine, vs)
        assert np.array_equal(to_np(g.voxels.grid_index), keys) and len(keys) > 20
        assert (to_np(g.voxels.color) == 1).all() and np.array_equal(g.origin, origin) and g.voxel_size == float(F(vs)) and g._sorted
    assert len(collision.create_voxel_grid(mine, 0.0)) == 0 and len(collision.create_voxel_grid(mine, -1.0)) == 0
    assert len(collision.create_voxel_grid(collision.Cylinder(0.1, 0.3), 0.05)) == 0


def test_lineset_surface():
    from cupoch_amd import geometry
    rng = np.random.default_rng(5)
    pts = rng.uniform(-1, 1, (50, 3)).astype(F)
    lines = rng.integers(0, 50, (30, 2)).astype(np.int32)
    ls = lineset(pts, lines)
    assert ls.has_points() and ls.has_lines() and not ls.has_colors() and not ls.is_empty() and geometry.LineSet().is_empty()
    assert np.array_equal(ls.get_min_bound(), pts.min(axis=0)) and np.array_equal(ls.get_max_bound(), pts.max(axis=0))
    box = ls.get_axis_aligned_bounding_box()
    assert np.array_equal(box.get_min_bound(), pts.min(axis=0))
    a, b = ls.get_line_coordinate(7)
    assert np.array_equal(a, pts[lines[7, 0]]) and np.array_equal(b, pts[lines[7, 1]])
    ls.paint_uniform_color((0.1, 0.2, 0.3))
    assert ls.has_colors() and np.array_equal(to_np(ls.colors), np.repeat(np.array([[0.1, 0.2, 0.3]], F), 30, axis=0))
    pc = geometry.PointCloud(pts.copy())
    T = ex.pose(rng, (0.5, 0.25, -1.0))
    for move in (lambda x: x.translate((1.0, -2.0, 0.5)), lambda x: x.scale(1.5), lambda x: x.rotate(T[:3, :3]), lambda x: x.transform(T)):
        move(ls), move(pc)
        assert np.array_equal(to_np(ls.points), to_np(pc.points))
    edges = geometry.LineSet.create_from_axis_aligned_bounding_box(box)
    assert len(edges.points) == 8 and len(edges.lines) == 12
    p, l = to_np(edges.points), to_np(edges.lines)
    d = np.abs(p[l[:, 0]] - p[l[:, 1]])
    assert ((d > 0).sum(axis=1) == 1).all() and np.array_equal(p.min(axis=0), box.get_min_bound())
    a, b = ls.get_line_coordinate(30)                                   # out of range: zeros, as the C++ surface gives
    assert not a.any() and not b.any()
