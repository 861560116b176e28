"""Inputs and references for the exact tests of VoxelDownSample (tests/test_voxel_exact_cpu.py holds this module against
the CPU oracle, tests/test_gpu_voxel_exact.py holds the kernels against it).  numpy only.

Every general-path kernel of the downsample adds in fp64 and rounds once, (float)(sum / count).  On a cloud whose fp64
sums are exact in ANY order there is one right answer per output float, whatever kernel ran and however it grouped the
additions: `lattice_cloud` builds such clouds, `restated` computes that answer in ten lines of numpy.

The lattice: coordinates base + q * voxel / 8 with an integer q >= 0, voxel a power of two, base a multiple of
voxel / 8, everything below 2^24 lattice units -- so every coordinate, the grid's origin (min - voxel / 2), every
p - origin, every quotient by the voxel size and every fp64 sum of up to 2^20 coordinates is exact.  Written
as q = 8 c + u with c the cell before the half-voxel shift and u = 0 .. 7, points with u >= 4 land in cell c + 1.
The builder draws the CELL k = floor((q + 4) / 8) and then an offset inside it (q = 8 k + r, r = -4 .. 3, q >= 0), which
is the same family with the grid's cell count under control: cells 0 .. cells_axis - 1 occur, a point is planted at
q = 0 and one in the last cell of every axis, and voxel_grid_fit's cell count is cells_axis + 1 -- b bits on an axis
for 2^(b-1) <= cells_axis <= 2^b - 1.

A consequence that shapes the table below: the largest cell index of an axis is at most 2^b - 2, so the key's low L
bits take all 2^L values only where the z axis has MORE than L bits.  A cloud of at most 5 key bits (no sort at all,
L = bits) can therefore never fill a run's mask; the full masks of 16 and 32 voxels are pinned at 12 and 13 bits
(bits_z = 10 and 11) instead, and the clouds of 4 and 5 bits pin every voxel the grid can hold, and the lowest with
the highest one alone."""
import functools

import numpy as np

F32 = np.float32


# ---- the reference --------------------------------------------------------------------------------------------------
def restated(pts, voxel, nrm=None, col=None):
    """PointCloud::VoxelDownSample restated: a dict of points / colors (float32 means of fp64 sums), normals (FLOAT64:
    w / |w| in fp64 from the float32 means w; NaN where w = 0), count per voxel, bits (x, y, z) per voxel_grid_fit's
    definition, and inverse (the voxel of every input point).  Voxels in lexicographic (x, y, z) order."""
    pts = np.ascontiguousarray(pts, F32).reshape(-1, 3)
    voxel = F32(voxel)
    mn, mx = np.fmin.reduce(pts, axis=0), np.fmax.reduce(pts, axis=0)      # (NaN ignored, as fminf / fmaxf)
    origin = (mn - voxel * F32(0.5)).astype(F32)
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.floor(((pts - origin).astype(F32) / voxel).astype(F32))
    cell = np.where(np.isfinite(q), q, 0.0).astype(np.int64)                 # (voxel_cell: not finite -> cell 0)
    cells = np.floor((mx.astype(np.float64) - origin.astype(np.float64)) / np.float64(voxel)) + 2.0
    bits = tuple(max(1, int(np.ceil(np.log2(c)))) for c in cells)
    assert all(2.0 ** b >= c and (b == 1 or 2.0 ** (b - 1) < c) for b, c in zip(bits, cells))
    # lexicographic order of the cells: rank every axis (ranks < n), pack the ranks
    rank = [np.unique(cell[:, k], return_inverse=True)[1].reshape(-1).astype(np.int64) for k in range(3)]
    n = len(pts)
    _, inv = np.unique((rank[0] * n + rank[1]) * n + rank[2], return_inverse=True)
    inv = inv.reshape(-1)
    cnt = np.bincount(inv).astype(np.float64)

    def means(a):
        S = np.zeros((len(cnt), 3), np.float64)
        np.add.at(S, inv, np.asarray(a, F32).astype(np.float64))
        return (S / cnt[:, None]).astype(F32)

    out = dict(points=means(pts), normals=None, colors=None, count=cnt.astype(np.int64), bits=bits, inverse=inv)
    if nrm is not None:
        w = means(nrm).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["normals"] = w / np.sqrt((w * w).sum(1))[:, None]
        out["normal_length"] = np.sqrt((w * w).sum(1))
    if col is not None:
        out["colors"] = means(col)
    return out


def ulps(got, want):
    """|got - want| in units of the float32 spacing at `want` (want may be float64); NaN on both sides counts 0, on
    one side inf"""
    got = np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want) / np.spacing(np.abs(want).astype(F32)).astype(np.float64)
    both = np.isnan(got) & np.isnan(want)
    one = np.isnan(got) ^ np.isnan(want)
    return np.where(both, 0.0, np.where(one, np.inf, d))


# ---- lattice clouds -------------------------------------------------------------------------------------------------
def lattice_cloud(n, cells, voxel, base, seed, sub=8, cell_fn=None):
    """n float32 points on the lattice of the module's docstring.  cells: occupied cells per axis; sub: lattice points
    per voxel edge (8; 2 for the grids of 21 and 22 bits an axis, whose coordinates then stay below 2^24 units of
    voxel / 2); cell_fn(rng, n, k) -> (n, 3) cells of the points, k the uniform draw (the default) to start from."""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells, np.int64)
    k = rng.integers(0, cells, size=(n, 3))
    if cell_fn is not None:
        k = np.asarray(cell_fn(rng, n, k), np.int64).reshape(n, 3)
    assert (k >= 0).all() and (k < cells).all()
    k[0] = 0                                                                # the origin is known ...
    step = 8 // sub
    r = rng.integers(-4 // step, (3 // step) + 1, size=(n, 3)) * step       # sub 8: -4 .. 3, sub 2: -4, 0
    if n > 1:
        k[1] = cells - 1                                                    # ... and so is the grid's far corner
    q = np.maximum(8 * k + r, 0)
    q[0] = 0
    voxel = float(voxel)
    assert np.log2(voxel) == int(np.log2(voxel)) and (base / (voxel / 8)) == int(base / (voxel / 8))
    p64 = base + q.astype(np.float64) * (voxel / 8)
    pts = p64.astype(F32)
    assert np.array_equal(pts.astype(np.float64), p64)                      # exact in float32
    assert np.abs(p64 / (voxel / sub)).max() < 2 ** 24 and np.array_equal(p64 / (voxel / sub), np.rint(p64 / (voxel / sub)))
    assert np.array_equal((q + 4) // 8, k)
    return np.ascontiguousarray(pts), k


def lattice_payload(n, cell, seed, cancel=True):
    """colours (1, (i mod 4096) / 4096, h12(i) / 4096), h12 = the top 12 bits of i * 2654435761 mod 2^32: channel 0's
    mean is exactly 1 in every voxel, and a point lost, doubled or credited to another voxel changes an exact sum.
    Normals from {-1, -0.5, 0, 0.5, 1}; cancel: the normals of the voxel of point 0 add up to exactly zero."""
    i = np.arange(n, dtype=np.uint64)
    h12 = ((i * np.uint64(2654435761)) % np.uint64(1 << 32)) >> np.uint64(20)
    col = np.stack([np.ones(n), (i % np.uint64(4096)).astype(np.float64) / 4096.0, h12.astype(np.float64) / 4096.0], 1).astype(F32)
    rng = np.random.default_rng(seed + 7919)
    nrm = rng.choice(F32([-1, -0.5, 0, 0.5, 1]), size=(n, 3)).astype(F32)
    if cancel:
        mine = np.flatnonzero((cell == cell[0]).all(1))
        half = len(mine) // 2
        nrm[mine[half:2 * half]] = -nrm[mine[:half]]
        nrm[mine[2 * half:]] = 0.0
    return np.ascontiguousarray(nrm), np.ascontiguousarray(col)


def random_cloud(n, ext, off, seed):
    """the non-dyadic family: float32 uniform points in [off, off + ext), off >= 0, colours in [0, 1), Gaussian normals"""
    assert off >= 0
    rng = np.random.default_rng(seed)
    pts = (rng.random((n, 3), dtype=F32) * np.asarray(ext, F32) + F32(off)).astype(F32)
    nrm = rng.standard_normal((n, 3)).astype(F32)
    col = rng.random((n, 3), dtype=F32)
    return pts, nrm, col


def face_cloud(n, voxel, seed):
    """half of the points ON the faces of the cells of a non-dyadic voxel or one ulp beside them (as
    test_gpu_voxel_dense.test_points_exactly_on_cell_faces_...): the quotient is an integer or one ulp off it"""
    rng = np.random.default_rng(seed)
    voxel = F32(voxel)
    pts = rng.random((n, 3), dtype=F32)
    origin = pts.min(axis=0) - voxel * F32(0.5)
    k = rng.integers(0, 80, size=(n // 2, 3)).astype(F32)
    on_face = origin + k * voxel
    on_face = np.nextafter(on_face, on_face + rng.choice(F32([-1, 0, 1]), size=on_face.shape)).astype(F32)
    pts[: n // 2] = np.clip(on_face, pts.min(axis=0), pts.max(axis=0))
    nrm = rng.standard_normal((n, 3)).astype(F32)
    col = rng.random((n, 3), dtype=F32)
    return np.ascontiguousarray(pts), nrm, col


# ---- the cases ------------------------------------------------------------------------------------------------------
# plan = (path, key bits, L, sort passes, sort kind, means kernel) as mi_icp_debug_last_voxel_plan reports them:
# sort kind 0 none, 1 payload radix (8-bit digits), 2 wide sort (11-bit digits), 3 64-bit pairs, 4 three sorts;
# means 0 vx_finish (dense), 1 voxel_means_wave, 2 voxel_means_runs, 3 voxel_means_thread, 4 voxel_means.
def _dup(rng, n, k):
    """fine grids: the second half of the cloud shares the cells of the first (runs of two and more points)"""
    k[n - n // 2:] = k[: n // 2]
    return k


def _only(*corner):
    """every point in one of the given cells"""
    def fn(rng, n, k):
        c = np.asarray(corner, np.int64)
        return c[rng.integers(0, len(c), size=n)]
    return fn


def _masks(L):
    """bits (1, 1, z): the run z >> L == 1 holds every one of its 2^L voxels twice, in input order v, v, v + 1, v + 1,
    ... (the run's first 2^L places name half of its voxels only); the run z >> L == 2 holds its first voxel once and
    its last one twice, and nothing else; the points drawn into either run move four runs up"""
    w = 1 << L

    def fn(rng, n, k):
        z = k[:, 2]
        z[(z >= w) & (z < 3 * w)] += 4 * w
        z[2:2 + 2 * w] = w + np.arange(2 * w) // 2
        z[2 + 2 * w:2 + 2 * w + 3] = (2 * w, 3 * w - 1, 3 * w - 1)
        return k
    return fn


def _case(id, row, n, bits, cells, plan, voxel=0.25, base=None, sub=8, cell_fn=None, no_dense=False, cancel=True):
    base = (-5.0 * voxel + 3 * voxel / 8) if base is None else base
    return dict(id=id, row=row, n=n, bits=bits, cells=cells, plan=plan, voxel=voxel, base=base, sub=sub, cell_fn=cell_fn,
                no_dense=no_dense, cancel=cancel, host=row in "bdhj")


BIG = 1 << 21
LATTICE = [
    # a: below the n / 8 rule -- one voxel, L = 0, one pass, a thread
    _case("a-n1", "a", 1, (1, 1, 1), (1, 1, 1), (0, 3, 0, 1, 1, 3)),
    _case("a-n7", "a", 7, (1, 1, 1), (1, 1, 1), (0, 3, 0, 1, 1, 3)),
    # b: no sort, L = 3, the wave kernel: one run of 1, 1, 2 and 4 chunks (64 | 65: the chunk's edge)
    _case("b-n9", "b", 9, (1, 1, 1), (1, 1, 1), (0, 3, 3, 0, 0, 1)),
    _case("b-n64", "b", 64, (1, 1, 1), (1, 1, 1), (0, 3, 3, 0, 0, 1), cancel=False),
    _case("b-n65", "b", 65, (1, 1, 1), (1, 1, 1), (0, 3, 3, 0, 0, 1), cancel=False),
    _case("b-n200", "b", 200, (1, 1, 1), (1, 1, 1), (0, 3, 3, 0, 0, 1), cancel=False),
    # c: no sort, L = 4 / 5: every voxel such a grid can hold (mask 0b111 / 0x7f); the lowest and the highest alone
    # (key 0 and 2 << 2: mask bits 0 and 8; key 0 and 6 << 2: bits 0 and 24)
    _case("c-4bits-all", "c", 300, (1, 1, 2), (1, 1, 3), (0, 4, 4, 0, 0, 1)),
    _case("c-4bits-ends", "c", 300, (2, 1, 1), (3, 1, 1), (0, 4, 4, 0, 0, 1), cell_fn=_only((0, 0, 0), (2, 0, 0))),
    _case("c-5bits-all", "c", 300, (1, 1, 3), (1, 1, 7), (0, 5, 5, 0, 0, 1)),
    _case("c-5bits-ends", "c", 300, (3, 1, 1), (7, 1, 1), (0, 5, 5, 0, 0, 1), cell_fn=_only((0, 0, 0), (6, 0, 0))),
    # d: one pass, L = 1 .. 5, the wave kernel, rmax = 256, n AT the edge 2^(bits - L) <= n / 8; at 12 and 13 bits a
    # run with all 16 / 32 voxels and one with its first and last voxel alone
    _case("d-9bits", "d", 2048, (3, 3, 3), (7, 7, 7), (0, 9, 1, 1, 1, 1)),
    _case("d-10bits", "d", 2048, (4, 3, 3), (12, 6, 5), (0, 10, 2, 1, 1, 1)),
    _case("d-11bits", "d", 2048, (4, 4, 3), (9, 13, 7), (0, 11, 3, 1, 1, 1)),
    _case("d-12bits", "d", 2048, (1, 1, 10), (1, 1, 1000), (0, 12, 4, 1, 1, 1), cell_fn=_masks(4)),
    _case("d-13bits", "d", 2048, (1, 1, 11), (1, 1, 2000), (0, 13, 5, 1, 1, 1), cell_fn=_masks(5)),
    # e: the other side of that edge
    _case("e-n2047", "e", 2047, (4, 4, 3), (9, 13, 7), (0, 11, 0, 2, 1, 3)),
    # f: one pass, L = 0, n > 16 voxels: 8 lanes per voxel; 2049: the scan tile's edge inside a run, the scalar tail
    _case("f-n200", "f", 200, (2, 2, 2), (2, 2, 2), (0, 6, 0, 1, 1, 2)),
    _case("f-n2049", "f", 2049, (3, 3, 2), (4, 4, 2), (0, 8, 0, 1, 1, 2)),
    # g: 2 / 3 / 4 passes of the payload radix, L = 0, a thread per voxel
    _case("g-16bits", "g", 4100, (6, 5, 5), (40, 20, 20), (0, 16, 0, 2, 1, 3)),
    _case("g-24bits", "g", 4100, (8, 8, 8), (200, 200, 200), (0, 24, 0, 3, 1, 3), cell_fn=_dup),
    _case("g-32bits", "g", 4100, (11, 11, 10), (2000, 2000, 1000), (0, 32, 0, 4, 1, 3), cell_fn=_dup),
    # h: 64-bit (key, index) pairs, both ends of their range
    _case("h-33bits", "h", 3000, (11, 11, 11), (2000, 1500, 1100), (0, 33, 0, 5, 3, 4), cell_fn=_dup),
    _case("h-64bits", "h", 3000, (22, 21, 21), (BIG + 5, BIG // 2 + 3, BIG // 2 + 9), (0, 64, 0, 8, 3, 4), voxel=0.5, base=0.0,
          sub=2, cell_fn=_dup),
    # i: three sorts, one per axis (3 passes each)
    _case("i-66bits", "i", 3000, (22, 22, 22), (BIG + 5, BIG + 3, BIG + 9), (0, 66, 0, 9, 4, 4), voxel=0.5, base=0.0, sub=2,
          cell_fn=_dup),
    # j, k: 2^17 points, the dense plan refuses (21 bits: 1024 buckets of 128 points; 24 bits: too many): the wide sort
    _case("j-21bits", "j", 131072, (7, 7, 7), (100, 100, 100), (0, 21, 0, 2, 2, 3)),
    _case("k-24bits", "k", 131072, (8, 8, 8), (200, 200, 200), (0, 24, 0, 3, 2, 3), cell_fn=_dup),
    # l: the smallest dense cloud, both ends of what the plan takes at this size.  (A voxel size of their own: a context
    # whose last call with THIS voxel size and a cloud of about this size was turned away by the dense plan -- rows j
    # and k -- does not try that path again, mi_voxel.hip "turned_away".)
    _case("l-15bits", "l", 131072, (5, 5, 5), (31, 31, 31), (1, 15, 0, 0, 0, 0), voxel=0.125),
    _case("l-20bits", "l", 131072, (7, 7, 6), (100, 100, 60), (1, 20, 0, 0, 0, 0), voxel=0.125),
    # m: the large L > 0 regime (the dense path switched off): two passes, rmax = 65536 = n / 8
    _case("m-17bits", "m", 524288, (6, 6, 5), (33, 32, 16), (0, 17, 1, 2, 1, 1), no_dense=True),
    _case("m-21bits", "m", 524288, (7, 7, 7), (100, 100, 100), (0, 21, 5, 2, 1, 1), no_dense=True),
]
LATTICE_IDS = [c["id"] for c in LATTICE]

# the non-dyadic family: (id, n, voxel, extent, offset, bits, plan, no_dense), one per row d, f, g, h, j, l, m
RANDOM = [
    dict(id="d-random", n=2048, voxel=0.1, ext=(1.0, 1.0, 0.5), off=0.0, bits=(4, 4, 3), plan=(0, 11, 3, 1, 1, 1)),
    dict(id="f-random", n=2049, voxel=0.25, ext=(1.0, 1.0, 0.3), off=0.0, bits=(3, 3, 2), plan=(0, 8, 0, 1, 1, 2)),
    dict(id="g-random", n=4100, voxel=0.005, ext=(1.0, 1.0, 1.0), off=0.0, bits=(8, 8, 8), plan=(0, 24, 0, 3, 1, 3)),
    dict(id="h-random", n=3000, voxel=0.0008, ext=(1.0, 1.0, 1.0), off=2.0, bits=(11, 11, 11), plan=(0, 33, 0, 5, 3, 4)),
    dict(id="j-random", n=131072, voxel=0.01, ext=(1.0, 1.0, 1.0), off=0.0, bits=(7, 7, 7), plan=(0, 21, 0, 2, 2, 3)),
    dict(id="l-random", n=131072, voxel=0.04, ext=(1.0, 1.0, 1.0), off=0.0, bits=(5, 5, 5), plan=(1, 15, 0, 0, 0, 0)),
    dict(id="m-random", n=524288, voxel=0.01, ext=(1.0, 1.0, 1.0), off=0.0, bits=(7, 7, 7), plan=(0, 21, 5, 2, 1, 1), no_dense=True),
]
RANDOM_IDS = [c["id"] for c in RANDOM]
FACES = dict(id="faces", n=4100, voxel=0.0125, bits=(7, 7, 7), plan=(0, 21, 0, 3, 1, 3))


def _seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def lattice(case_id):
    """(case, points, normals, colours, restated) of a lattice case, built once; the arrays are shared: do not write"""
    c = LATTICE[LATTICE_IDS.index(case_id)]
    pts, cell = lattice_cloud(c["n"], c["cells"], c["voxel"], c["base"], _seed(case_id), c["sub"], c["cell_fn"])
    nrm, col = lattice_payload(c["n"], cell, _seed(case_id), c["cancel"])
    ref = restated(pts, c["voxel"], nrm, col)
    for a in (pts, nrm, col):
        a.setflags(write=False)
    return c, pts, nrm, col, ref


@functools.lru_cache(maxsize=None)
def random_case(case_id):
    """(case, points, normals, colours) of a random-family case (the faces' cloud included)"""
    if case_id == "faces":
        c = FACES
        pts, nrm, col = face_cloud(c["n"], c["voxel"], 3)
    else:
        c = RANDOM[RANDOM_IDS.index(case_id)]
        pts, nrm, col = random_cloud(c["n"], c["ext"], c["off"], _seed(case_id))
    for a in (pts, nrm, col):
        a.setflags(write=False)
    return c, pts, nrm, col


# ---- bounds and centre ----------------------------------------------------------------------------------------------
BOUNDS_SIZES = [1, 255, 256, 257, 262144, 262145, 786432, 786433, 1048577]


def bounds_slots(n):
    """indices of a cloud of n points by the place bounds_partial (csrc/lbvh.h) reads them in: blocks = min(1024,
    ceil(n / 256)), stride = blocks * 256, thread t takes t, t + stride, ... four at a time while the fourth exists
    ("u0" .. "u3": the unrolled loop's slots), then one at a time ("tail").  Returns {place: index}, with "first" and
    "last" always there."""
    blocks = min(1024, (n + 255) // 256)
    stride = blocks * 256
    out = {"first": 0, "last": n - 1}
    for t in (5, 0, stride - 1, 1):
        if t >= n:
            continue
        i = t
        while i + 3 * stride < n:
            for s in range(4):
                out.setdefault("u%d" % s, i + s * stride)
            i += 4 * stride
        while i < n:
            if i >= stride:                                                   # (a thread's FIRST point is no tail)
                out.setdefault("tail", i)
            i += stride
    return out
