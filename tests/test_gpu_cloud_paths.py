"""GPU: the host-side paths every cloud-in, cloud-out entry point shares -- the argument checks, the staging of a cloud,
the scan and its total, the count-first emitters -- pinned at the scan's edges, in both memory kinds and through the
error returns, message by message."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F = np.float32
HOST, DEVICE = 0, 1
SIZES = [1, 255, 256, 257, 2047, 2048, 2049, 4097]     # the 256-thread block, kScanTile = 2048, two tiles plus one
PATTERNS = ["none", "all", "first", "last", "alternating", "random"]


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def to_np(v):
    return None if v is None else np.asarray(v.cpu() if hasattr(v, "cpu") else v)


def bits(a):
    return np.ascontiguousarray(to_np(a), F).view(np.uint32)


def same(a, b):
    """bit-equal arrays of float32, NaN and infinity included"""
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool((a == b).all())


def keep_pattern(n, pattern):
    keep = np.zeros(n, bool)
    if pattern == "all":
        keep[:] = True
    elif pattern == "first":
        keep[0] = True
    elif pattern == "last":
        keep[-1] = True
    elif pattern == "alternating":
        keep[::2] = True
    elif pattern == "random":
        keep = np.random.default_rng(n).random(n) < 0.5
    return keep


def cloud_for(keep, finite):
    """a cloud whose kept points lie inside the unit box and whose others do not: x = 2 (finite) or NaN / infinity"""
    n = len(keep)
    rng = np.random.default_rng(1000 + n)
    pts = rng.random((n, 3), dtype=F) * F(0.5) + F(0.25)
    nrm = rng.standard_normal((n, 3)).astype(F)
    col = rng.random((n, 3), dtype=F)
    if finite:
        pts[~keep, 0] = F(2.0)
    else:
        drop = np.flatnonzero(~keep)
        pts[drop[0::3], 0] = np.nan
        pts[drop[1::3], 1] = np.inf
        pts[drop[2::3], 2] = -np.inf
    return pts, nrm, col


# name, does it return the index list, does it need a finite cloud, the call given (engine, points, keep, attributes)
COMPACTORS = [
    ("select_by_mask", False, True, lambda e, p, keep, kw: e.select_by_mask(p, keep, **kw)),
    ("select_by_index", False, True, lambda e, p, keep, kw: e.select_by_index(p, np.flatnonzero(~keep), invert=True, **kw)),
    ("pass_through_filter", True, True, lambda e, p, keep, kw: e.pass_through_filter(p, 0, 0.0, 1.0, **kw)),
    ("crop_aabb", True, True, lambda e, p, keep, kw: e.crop_aabb(p, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), **kw)),
    ("remove_none_finite", True, False, lambda e, p, keep, kw: e.remove_none_finite(p, True, True, **kw)),
]


def check_compaction(eng, n, kind, attributes):
    wrap = (lambda a: torch.from_numpy(a).cuda()) if kind == DEVICE else (lambda a: a)
    for pattern in PATTERNS:
        keep = keep_pattern(n, pattern)
        for name, has_idx, finite, call in COMPACTORS:
            pts, nrm, col = cloud_for(keep, finite)
            kw = {}
            if "normals" in attributes:
                kw["normals"] = wrap(nrm)
            if "colors" in attributes:
                kw["colors"] = wrap(col)
            out = call(eng, wrap(pts), keep, kw)
            what = (name, n, pattern, kind, attributes)
            assert hasattr(out[0], "cpu") == (kind == DEVICE), what
            assert len(out[0]) == int(keep.sum()), what                  # m
            assert same(out[0], pts[keep]), what
            assert (out[1] is None) == ("normals" not in attributes) and (out[2] is None) == ("colors" not in attributes)
            if out[1] is not None:
                assert same(out[1], nrm[keep]), what
            if out[2] is not None:
                assert same(out[2], col[keep]), what
            if has_idx:
                idx = to_np(out[3])
                assert idx.dtype == np.int64 and np.array_equal(idx, np.flatnonzero(keep)), what


@pytest.mark.parametrize("kind", [HOST, DEVICE])
@pytest.mark.parametrize("n", SIZES)
def test_compaction_is_exact_at_the_scans_edges(eng, n, kind):
    check_compaction(eng, n, kind, ("normals", "colors"))


@pytest.mark.parametrize("kind", [HOST, DEVICE])
@pytest.mark.parametrize("attributes", [(), ("normals",), ("colors",)])
def test_compaction_with_every_attribute_set(eng, attributes, kind):
    check_compaction(eng, 2049, kind, attributes)       # (normals and colours together: the test above)


# ---- count-first emitters: the count comes back before anything is written
@pytest.mark.parametrize("w,h", [(1, 1), (45, 45), (64, 32), (64, 33)])
def test_create_from_depth_valid_only_counts_then_emits(eng, w, h):
    rng = np.random.default_rng(w * 100 + h)
    images = []
    depth = (rng.random((h, w), dtype=F) + F(0.5))
    depth[rng.random((h, w)) < 0.3] = F(0.0)
    images.append(depth)
    if w * h == 1:                                      # one pixel: the hole and the valid pixel, each on its own
        images = [np.zeros((1, 1), F), np.full((1, 1), 0.75, F)]
    else:
        depth[0, 0], depth[-1, -1] = F(0.0), F(1.0)
    K = (50.0, 52.0, w / 2.0 - 0.25, h / 2.0 + 0.25)
    for depth in images:
        valid = int(np.count_nonzero(depth > 0))
        host = eng.create_from_depth(depth, K, valid_only=True)[0]
        dev = eng.create_from_depth(torch.from_numpy(depth).cuda(), K, valid_only=True)[0]
        assert len(host) == valid and len(dev) == valid
        assert isinstance(host, np.ndarray) and dev.is_cuda
        assert same(host, dev)
        assert np.isfinite(host).all()


K4 = (14.0, 14.0, 15.5, 11.5)
IMG_W, IMG_H = 32, 24


@pytest.fixture(scope="module", params=[8, 16])
def volume(request, eng):
    """a volume of edge 2 centred in front of the camera with one synthetic frame in it: a wall at depth 1.5,
    in the half of the volume where the raycast's march begins, with a hole"""
    res = request.param
    vol = eng.tsdf_create(2.0, res, 4.8 / res, 1, (0.0, 0.0, 1.0))       # MI_ICP_TSDF_RGB8
    rng = np.random.default_rng(res)
    depth = np.full((IMG_H, IMG_W), 1.5, F) + rng.random((IMG_H, IMG_W), dtype=F) * F(0.05)
    depth[:4, :4] = F(0.0)
    color = rng.integers(0, 256, (IMG_H, IMG_W, 3), dtype=np.uint8)
    eng.tsdf_integrate(vol, depth, color, IMG_W, IMG_H, K4)
    yield res, vol
    eng.tsdf_destroy(vol)


def tsdf_calls(eng, vol):
    """name, number of output arrays, the call given (their pointers, capacity, m, kind)"""
    L, ctx = eng._L, eng._ctx
    K = (C.c_float * 4)(*K4)
    E = np.ascontiguousarray(np.eye(4, dtype=F))
    pE = E.ctypes.data_as(C.c_void_p)
    ray = lambda valid: lambda p, cap, m, kind: (E, L.mi_icp_tsdf_raycast(ctx, vol, IMG_W, IMG_H, K, pE, 0.3, valid, p[0], p[1],
                                                                         p[2], cap, m, kind))[1]
    return [
        ("extract_voxel_point_cloud", 2,
         lambda p, cap, m, kind: L.mi_icp_tsdf_extract_voxel_point_cloud(ctx, vol, p[0], p[1], cap, m, kind)),
        ("extract_point_cloud", 3,
         lambda p, cap, m, kind: L.mi_icp_tsdf_extract_point_cloud(ctx, vol, p[0], p[1], p[2], cap, m, kind)),
        ("raycast_every_pixel", 3, ray(0)),
        ("raycast_valid_only", 3, ray(1)),
    ]


def test_tsdf_emitters_count_first_and_honour_capacity(eng, volume):
    res, vol = volume
    SENTINEL = F(-77.0)
    raycast_points = None
    for name, narr, call in tsdf_calls(eng, vol):
        m = C.c_int64(-5)
        assert call([None] * narr, 0, C.byref(m), HOST) == 0, name           # no room: the count alone
        need = int(m.value)
        assert need > 1, (name, res)
        if name == "raycast_every_pixel":
            assert need == IMG_W * IMG_H
        results = {}
        for kind in (HOST, DEVICE):
            for cap in (need - 1, need):
                host = [np.full((need, 3), SENTINEL, F) for _ in range(narr)]
                arr = [torch.from_numpy(a).cuda() for a in host] if kind == DEVICE else host
                ptr = [C.c_void_p(a.data_ptr()) if kind == DEVICE else a.ctypes.data_as(C.c_void_p) for a in arr]
                m = C.c_int64(-5)
                rc = call(ptr, cap, C.byref(m), kind)
                torch.cuda.synchronize()
                got = [to_np(a) for a in arr]
                assert rc == 0 and int(m.value) == need, (name, res, kind, cap)
                if cap < need:                                               # too small: nothing is written
                    assert all(bool((g == SENTINEL).all()) for g in got), (name, res, kind)
                else:
                    results[kind] = got
        for h, d in zip(results[HOST], results[DEVICE]):
            assert same(h, d), (name, res)
        pts = results[HOST][0]
        if name == "raycast_every_pixel":
            assert np.isfinite(pts).all(1).any() and not np.isfinite(pts).all()   # hits, and misses kept as NaN
        else:
            assert np.isfinite(pts).all() and not bool((pts == SENTINEL).all(1).any()), (name, res)
        if name == "raycast_valid_only":
            assert need == int(np.isfinite(raycast_points).all(1).sum())
            assert same(pts, raycast_points[np.isfinite(raycast_points).all(1)])
        if name == "raycast_every_pixel":
            raycast_points = pts


# ---- the error table: code -1 (MI_ICP_ERR_INVALID) and the exact message, entry point by entry point
N = 64


def error_entries():
    """name, has it an m, has it an upper bound on n, the call given (xyz, normals, colors, n, out_xyz, out_normals,
    out_colors, m) -- every other argument valid"""
    idx = np.arange(N, dtype=np.int64)
    mask = np.ones(N, np.uint8)
    oidx = np.zeros(N, np.int64)
    stat = np.zeros(N, F)
    lo, hi = np.zeros(3, F), np.ones(3, F)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    keep = (idx, mask, oidx, stat, lo, hi)
    return [
        ("voxel_downsample", True, True, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_voxel_downsample(
            c, x, n, k, nn, 0.05, ox, on, ok, m, HOST)),
        ("select_by_index", True, True, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_select_by_index(
            c, x, n, k, nn, hp(idx), 8, 0, ox, on, ok, m, HOST)),
        ("select_by_mask", True, True, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_select_by_mask(
            c, x, n, k, nn, hp(mask), nn, 0, ox, on, ok, m, HOST)),
        # (no upper bound: a strided copy, no staging and no 32-bit index)
        ("uniform_downsample", True, False, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_uniform_downsample(
            c, x, n, k, nn, 2, ox, on, ok, m, HOST)),
        ("farthest_point_downsample", True, True, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_farthest_point_downsample(
            c, x, n, k, nn, 8, ox, on, ok, hp(oidx), m, HOST)),
        ("pass_through_filter", True, True, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_pass_through_filter(
            c, x, n, k, nn, 0, 0.0, 1.0, ox, on, ok, hp(oidx), m, HOST)),
        ("crop_aabb", True, True, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_crop_aabb(
            c, x, n, k, nn, hp(lo), hp(hi), ox, on, ok, hp(oidx), m, HOST)),
        ("remove_none_finite", True, True, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_remove_none_finite(
            c, x, n, k, nn, 1, 1, ox, on, ok, hp(oidx), m, HOST)),
        ("remove_statistical_outliers", True, True, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_remove_statistical_outliers(
            c, x, n, k, nn, 8, 2.0, ox, on, ok, hp(oidx), hp(stat), m, HOST)),
        ("remove_radius_outliers", True, True, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_remove_radius_outliers(
            c, x, n, k, nn, 4, 0.1, ox, on, ok, hp(oidx), hp(stat), m, HOST)),
        ("gaussian_filter", False, True, lambda L, c, x, n, k, nn, ox, on, ok, m: L.mi_icp_gaussian_filter(
            c, x, n, k, nn, 0.1, 0.01, 8, ox, on, ok, HOST)),
    ], keep


@pytest.mark.parametrize("name", [e[0] for e in error_entries()[0]])
def test_error_table(eng, name):
    entries, keep = error_entries()
    _, has_m, bounded, call = next(e for e in entries if e[0] == name)
    rng = np.random.default_rng(3)
    xyz, nrm, col = (rng.random((N, 3), dtype=F) for _ in range(3))
    oxyz, onrm, ocol = (np.full((N, 3), 7, F) for _ in range(3))
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    m = C.c_int64(7)
    good = dict(x=hp(xyz), n=hp(nrm), k=hp(col), nn=N, ox=hp(oxyz), on=hp(onrm), ok=hp(ocol), m=C.byref(m))
    cases = [("m is null", dict(m=None)), ("bad size", dict(nn=-1)), ("bad size", dict(nn=0x7fffff01)),
             ("null buffer", dict(x=None)), ("null buffer", dict(on=None)), ("null buffer", dict(ok=None))]
    ran = 0
    for message, change in cases:
        if ("m" in change and not has_m) or (change.get("nn") == 0x7fffff01 and not bounded):
            continue
        a = dict(good, **change)
        m.value = 7
        rc = call(eng._L, eng._ctx, a["x"], a["n"], a["k"], a["nn"], a["ox"], a["on"], a["ok"], a["m"])
        assert rc == -1, (name, change)
        assert eng._L.mi_icp_last_error(eng._ctx).decode() == "%s: %s" % (name, message), (name, change)
        if has_m and "m" not in change:
            assert m.value == 0                          # zeroed before the size is looked at
        for out in (oxyz, onrm, ocol):
            assert bool((out == 7).all())
        ran += 1
    assert ran == 6 - (0 if has_m else 1) - (0 if bounded else 1)
    # and with everything in place the call goes through
    m.value = 7
    assert call(eng._L, eng._ctx, good["x"], good["n"], good["k"], N, good["ox"], good["on"], good["ok"], good["m"]) == 0


def test_error_precedence(eng):
    """The entry points disagree on the order of their checks, and that order is part of the interface: the crop
    filters look at their own arguments before the buffers, the outlier filters at the buffers first."""
    L, ctx = eng._L, eng._ctx
    xyz = np.random.default_rng(4).random((N, 3), dtype=F)
    oidx, stat = np.zeros(N, np.int64), np.zeros(N, F)
    hp = lambda a: a.ctypes.data_as(C.c_void_p)
    m = C.c_int64(7)
    rc = L.mi_icp_pass_through_filter(ctx, hp(xyz), None, None, N, 3, 0.0, 1.0, None, None, None, hp(oidx), C.byref(m), HOST)
    assert rc == -1 and L.mi_icp_last_error(ctx).decode() == "pass_through_filter: axis_no must be 0, 1 or 2"
    rc = L.mi_icp_remove_statistical_outliers(ctx, hp(xyz), None, None, N, 0, 2.0, None, None, None, hp(oidx), hp(stat),
                                              C.byref(m), HOST)
    assert rc == -1 and L.mi_icp_last_error(ctx).decode() == "remove_statistical_outliers: null buffer"
