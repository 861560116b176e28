"""geometry::VoxelGrid without a GPU: the numpy restatement of the contract (tests/voxelgrid_exact.py) reproduces the
reference's three unit tests (src/tests/geometry/voxelgrid.cpp) and agrees with brute-force definitions (a dict of lists
for voxelisation and merging, a per-corner Python loop for carving); the carving scenes of the GPU tests each keep and
remove a real share of the voxels; the Python type surface; the C ABI's prototypes."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import voxelgrid_exact as vx
from conftest import ROOT

F = np.float32


# ---- the reference's unit tests on the restatement ----------------------------------------------------------------------
def test_restatement_bounds():
    """three AddVoxel at voxel_size 5: bounds (0, 0, 0) / (10, 15, 20)"""
    k, c = np.zeros((0, 3), np.int32), np.zeros((0, 3), F)
    for idx in ([1, 0, 0], [0, 2, 0], [0, 0, 3]):
        k, c = vx.merge(k, c, [idx], [[0, 0, 0]], vx.KEEP_FIRST)
    lo, hi, _ = vx.bounds(k, 5.0, (0, 0, 0))
    assert np.array_equal(lo, np.array([0, 0, 0], F)) and np.array_equal(hi, np.array([10, 15, 20], F))
    assert np.array_equal(k, np.array([[0, 0, 3], [0, 2, 0], [1, 0, 0]], np.int32))     # ascending, x most significant


def test_restatement_get_voxel():
    for x, want in ((0.0, 0), (1.0, 0), (4.9, 0), (5.0, 1), (5.1, 1), (-0.1, -1)):
        k, fin = vx.point_keys([[x, x, x]], 5.0, (0, 0, 0))
        assert fin[0] and tuple(k[0]) == (want, want, want)


def test_restatement_one_voxel_within_bounds():
    k, c = vx.from_points([[0.5, 0.5, 0.5]], None, 1.0, (-100, -100, -100), (100, 100, 100))
    assert len(k) == 1 and tuple(k[0]) == (100, 100, 100) and tuple(c[0]) == (1.0, 1.0, 1.0)


# ---- against brute-force definitions ----------------------------------------------------------------------------------
def _cloud(n, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3)) * spread).astype(F), rng.random((n, 3)).astype(F)


def test_voxelisation_against_a_dict():
    pts, col = _cloud(3000, 1)
    pts[5] = [np.nan, 0, 0]
    pts[17] = [0.2, np.inf, 0.1]
    vs, lo = F(0.07), np.array([0.31, 0.27, 0.4], F)         # min_bound inside the cloud: negative keys
    k, c = vx.from_points(pts, col, vs, lo, (2, 2, 2))
    cells = {}
    for i, p in enumerate(pts):
        if not np.isfinite(p).all():
            continue
        key = tuple(int(math.floor(float(F(F(p[d] - lo[d]) / vs)))) for d in range(3))
        cells.setdefault(key, []).append(i)
    want = sorted(cells)
    assert [tuple(r) for r in k.tolist()] == want and (k.min() < 0)
    for key, got in zip(want, c):
        s = np.zeros(3, np.float64)
        for i in cells[key]:
            s = s + col[i].astype(np.float64)
        assert np.array_equal((s / len(cells[key])).astype(F), got)
    k2, c2 = vx.from_points(pts, None, vs, lo, (2, 2, 2))
    assert np.array_equal(k2, k) and (c2 == 1).all()


def test_merge_against_a_dict():
    rng = np.random.default_rng(2)
    ka, kb = rng.integers(-3, 4, (60, 3)).astype(np.int32), rng.integers(-3, 4, (80, 3)).astype(np.int32)
    ca, cb = rng.random((60, 3)).astype(F), rng.random((80, 3)).astype(F)
    cells = {}
    for key, col in list(zip(map(tuple, ka.tolist()), ca)) + list(zip(map(tuple, kb.tolist()), cb)):
        cells.setdefault(key, []).append(col)
    want = sorted(cells)
    k, c = vx.merge(ka, ca, kb, cb, vx.AVERAGE)
    assert [tuple(r) for r in k.tolist()] == want
    for key, got in zip(want, c):
        s = cells[key][0].copy()
        for col in cells[key][1:]:
            s = (s + col).astype(F)
        assert np.array_equal((s / F(len(cells[key]))).astype(F), got)
    k, c = vx.merge(ka, ca, kb, cb, vx.KEEP_FIRST)
    assert [tuple(r) for r in k.tolist()] == want
    assert all(np.array_equal(cells[key][0], got) for key, got in zip(want, c))


def _carve_one(key, vs, o, img, K, E, keep):
    """compute_carve_functor for one voxel, scalar fp32 arithmetic"""
    H, W = img.shape[:2]
    r = F(vs / F(2))
    c = [F(F(F(key[d]) + F(0.5)) * vs + o[d]) for d in range(3)]
    for sg in vx.CORNER_SIGNS:
        p = [F(c[d] + (r if sg[d] > 0 else -r)) for d in range(3)]
        X = [F(F(F(F(E[d, 0] * p[0]) + F(E[d, 1] * p[1])) + F(E[d, 2] * p[2])) + E[d, 3]) for d in range(3)]
        uvz = [F(F(F(K[d, 0] * X[0]) + F(K[d, 1] * X[1])) + F(K[d, 2] * X[2])) for d in range(3)]
        z = uvz[2]
        with np.errstate(all="ignore"):
            u, v = F(uvz[0] / z), F(uvz[1] / z)
        within = img.ndim == 2 and img.dtype == np.float32 and u >= 0 and u <= F(W - 1) and v >= 0 and v <= F(H - 1)
        if not within:
            if keep:
                return True
            continue
        ui, vi = max(min(int(u), W - 2), 0), max(min(int(v), H - 2), 0)
        pu, pv = F(u - F(ui)), F(v - F(vi))
        one = F(1)
        a = F(F(img[vi, ui] * F(one - pv)) + F(img[vi + 1, ui] * pv))
        b = F(F(img[vi, ui + 1] * F(one - pv)) + F(img[vi + 1, ui + 1] * pv))
        d = F(F(a * F(one - pu)) + F(b * pu))
        if d > 0 and z >= d:
            return True
    return False


def test_carve_against_a_per_corner_loop():
    keys, _ = vx.dense(32, 32, 32)
    rng = np.random.default_rng(3)
    pick = keys[rng.choice(len(keys), 200, replace=False)]
    vs, o = F(vx.DENSE_VS), np.asarray(vx.DENSE_ORIGIN, F)
    for name, (intr, E, img) in vx.carve_scenes().items():
        K = vx.k3(intr)
        for keep in (False, True):
            got = vx.carve_stay(pick, vs, o, img, intr, E, keep)
            want = np.array([_carve_one(k, vs, o, img, K, E, keep) for k in pick])
            assert np.array_equal(got, want), (name, keep)


def test_carve_scenes_keep_and_remove_a_real_share():
    """else a constant answer would pass the GPU comparison"""
    keys, _ = vx.dense(32, 32, 32)
    assert len(keys) == 32768
    saw_nonpositive_z = False
    for name, (intr, E, img) in vx.carve_scenes().items():
        for keep in (False, True):
            share = vx.carve_stay(keys, vx.DENSE_VS, vx.DENSE_ORIGIN, img, intr, E, keep).mean()
            assert 0.05 <= share <= 0.95, (name, keep, share)
        if name == "inside":
            c = (keys.astype(F) + F(0.5)) * F(vx.DENSE_VS)
            z = c[:, 2] - F(vx.DENSE_VS / 2) + E[2, 3]
            saw_nonpositive_z = bool((z == 0).any() and (z < 0).any())
    assert saw_nonpositive_z
    for img in (np.ones((vx.IMG_H, vx.IMG_W), np.uint16), np.ones((vx.IMG_H, vx.IMG_W, 3), F)):   # never "within"
        intr, E, _ = vx.carve_scenes()["front"]
        assert not vx.carve_stay(keys, vx.DENSE_VS, vx.DENSE_ORIGIN, img, intr, E, False).any()
        assert vx.carve_stay(keys, vx.DENSE_VS, vx.DENSE_ORIGIN, img, intr, E, True).all()


def test_query_bounds_and_refusals_of_the_restatement():
    k, _ = vx.from_points(_cloud(500, 4)[0], None, 0.1, (0, 0, 0), (1, 1, 1))
    q = np.array([[0.05, 0.05, 0.05], [np.nan, 0, 0], [0.1, 0.2, 0.3], [5, 5, 5]], F)
    inc, idx = vx.query(k, 0.1, (0, 0, 0), q)
    assert not inc[1] and tuple(idx[1]) == (0, 0, 0) and not inc[3] and tuple(idx[3]) == (50, 50, 50)
    assert inc[0] == ((0, 0, 0) in set(map(tuple, k.tolist())))
    lo, hi, ce = vx.bounds(np.zeros((0, 3), np.int32), 0.5, (1, 2, 3))
    assert tuple(lo) == (1, 2, 3) and tuple(hi) == (1, 2, 3) and tuple(ce) == (0, 0, 0)
    assert vx.refused_from_points(0.0, (0, 0, 0), (1, 1, 1)) and vx.refused_from_points(-1.0, (0, 0, 0), (1, 1, 1))
    assert vx.refused_from_points(np.nan, (0, 0, 0), (1, 1, 1)) and vx.refused_from_points(1e-12, (0, 0, 0), (1, 1, 1))
    assert not vx.refused_from_points(0.1, (0, 0, 0), (1, 1, 1))
    far = np.array([[0, 0, 0], [3000000, 3000000, 3000000]], np.int32)
    assert vx.key_span_bits(far) == 66                        # (3e6 needs 22 bits an axis: beyond one 64-bit key)
    assert 32 < vx.key_span_bits(far * np.array([1, 1, 0], np.int32)) <= 64
    assert vx.key_span_bits(np.array([[-10 ** 9] * 3, [10 ** 9] * 3], np.int32)) > 64
    assert np.array_equal(vx.dense(2, 3, 4)[0][[0, 1, 4, 12, 23]], [[0, 0, 0], [0, 0, 1], [0, 1, 0], [1, 0, 0], [1, 2, 3]])
    assert len(vx.dense(0, 3, 4)[0]) == 0 and len(vx.dense(2, -1, 4)[0]) == 0


# ---- the Python type surface (no GPU is touched) ----------------------------------------------------------------------
def test_python_surface_names_defaults_and_repr():
    from cupoch_amd import camera, geometry, integration
    V = geometry.Voxel
    v = V()
    assert tuple(v.grid_index) == (0, 0, 0) and tuple(v.color) == (1.0, 1.0, 1.0)
    assert tuple(V([1, 2, 3]).grid_index) == (1, 2, 3) and tuple(V([1, 2, 3]).color) == (1.0, 1.0, 1.0)
    assert tuple(V(color=[0.5, 0.25, 0]).grid_index) == (0, 0, 0) and tuple(V(color=[0.5, 0.25, 0]).color) == (0.5, 0.25, 0.0)
    v = V([1, 2, 3], [0.25, 0.5, 0.75])
    assert repr(v) == "geometry::Voxel with grid_index: (1, 2, 3), color: (0.25, 0.5, 0.75)"
    g = geometry.VoxelGrid()
    assert g.voxel_size == 0.0 and np.array_equal(g.origin, np.zeros(3, F)) and g.origin.dtype == F
    assert repr(g) == "geometry::VoxelGrid with 0 voxels." and g.is_empty() and not g.has_voxels() and g.has_colors()
    assert len(g.voxels) == 0 and g.voxels.cpu()[0].shape == (0, 3)
    for name in ("voxels", "has_colors", "has_voxels", "get_voxel", "paint_uniform_color", "paint_indexed_color",
                 "check_if_included", "carve_depth_map", "carve_silhouette", "create_dense", "create_from_point_cloud",
                 "create_from_point_cloud_within_bounds", "create_from_occupancy_grid", "select_by_index", "add_voxel",
                 "add_voxels", "get_voxel_center_coordinate", "get_voxel_bounding_points", "get_min_bound", "get_max_bound",
                 "get_center", "get_axis_aligned_bounding_box", "translate", "scale", "transform", "rotate", "clear",
                 "is_empty", "__add__", "__iadd__"):
        assert hasattr(geometry.VoxelGrid, name), name
    import inspect
    for fn in (geometry.VoxelGrid.carve_depth_map, geometry.VoxelGrid.carve_silhouette):
        assert inspect.signature(fn).parameters["keep_voxels_outside_image"].default is False
    assert list(inspect.signature(geometry.VoxelGrid.create_dense).parameters)[:5] == ["origin", "voxel_size", "width", "height", "depth"]
    assert list(inspect.signature(geometry.VoxelGrid.create_from_point_cloud_within_bounds).parameters) == \
        ["input", "voxel_size", "min_bound", "max_bound"]
    g.voxel_size, g.origin = 5.0, np.zeros(3, F)
    assert [int(g.get_voxel([x, x, x])[0]) for x in (0, 1, 4.9, 5, 5.1)] == [0, 0, 0, 1, 1]
    g.translate([1.0, 0.0, -1.0]).scale(2.0)
    assert np.array_equal(g.origin, np.array([1, 0, -1], F)) and g.voxel_size == 10.0
    assert np.array_equal(g.get_min_bound(), g.origin) and np.array_equal(g.get_max_bound(), g.origin)
    assert np.array_equal(g.get_center(), np.zeros(3, F))
    with pytest.raises(RuntimeError):
        g.transform(np.eye(4))
    with pytest.raises(RuntimeError):
        g.rotate(np.eye(3))
    g.clear()
    assert g.voxel_size == 0.0 and np.array_equal(g.origin, np.zeros(3, F))
    # what stays unbuilt is not pretended
    assert not hasattr(geometry.OccupancyGrid, "create_from_voxel_grid")
    assert not hasattr(integration.UniformTSDFVolume, "extract_voxel_grid")
    assert not hasattr(geometry.VoxelGrid, "create_from_triangle_mesh")
    assert not hasattr(geometry.VoxelGrid, "get_oriented_bounding_box")
    assert "ScalableTSDFVolume" in integration.__doc__
    for doc in (geometry.__doc__, integration.__doc__):
        assert "no VoxelGrid type" not in doc
    p = camera.PinholeCameraParameters()
    assert isinstance(p.intrinsic, camera.PinholeCameraIntrinsic) and np.array_equal(p.extrinsic, np.eye(4, dtype=F))


# ---- ABI facts -------------------------------------------------------------------------------------------------------
FAMILY = ("from_points", "dense", "merge", "carve", "query", "bounds", "select_by_index", "paint")


def _prototypes():
    src = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return {m.group(1): m.group(2) for m in
            re.finditer(r"MI_ICP_API\s+[\w\s\*]+?\b(mi_icp_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_abi_family_is_declared_without_a_memory_kind_and_bound():
    from cupoch_amd import _lib, engine
    protos = _prototypes()
    names = ["mi_icp_voxelgrid_" + f for f in FAMILY]
    assert sorted(n for n in protos if n.startswith("mi_icp_voxelgrid_")) == sorted(names)
    for n in names:
        args = [a.strip() for a in protos[n].split(",")]
        assert "mem_kind" not in protos[n] and args[0] == "mi_icp_ctx* ctx"
        res, argtypes = _lib.SIGNATURES[n]
        assert res is C.c_int and len(argtypes) == len(args), n
        for a, t in zip(args, argtypes):
            if "*" in a:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (n, a)
            elif a.startswith("int64_t"):
                assert t is C.c_int64, (n, a)
            elif a.startswith("float"):
                assert t is C.c_float, (n, a)
            else:
                assert a.startswith("int ") and t is C.c_int, (n, a)
    hdr = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    assert re.search(r"#define\s+MI_ICP_VOXELGRID_AVERAGE\s+%d\b" % vx.AVERAGE, hdr)
    assert re.search(r"#define\s+MI_ICP_VOXELGRID_KEEP_FIRST\s+%d\b" % vx.KEEP_FIRST, hdr)
    assert (engine.Engine.VOXELGRID_AVERAGE, engine.Engine.VOXELGRID_KEEP_FIRST) == (vx.AVERAGE, vx.KEEP_FIRST)
    assert "mi_voxelgrid" in _lib.UNITS
    unit_map = open(os.path.join(ROOT, "cupoch_amd", "csrc", "ctx.h")).read().split("#pragma once")[0]
    assert "mi_voxelgrid.hip" in unit_map


def test_status_codes_without_a_device():
    """a null context is a status, with or without a GPU"""
    from cupoch_amd import _lib
    L = _lib.load()
    m = C.c_int64(7)
    assert L.mi_icp_voxelgrid_from_points(None, None, None, 0, 1.0, None, None, None, None, 0, C.byref(m)) == -1
    assert L.mi_icp_voxelgrid_dense(None, 1, 1, 1, None, None, 0, C.byref(m)) == -1
    assert L.mi_icp_voxelgrid_query(None, None, 0, 1, 1.0, None, None, 0, None, None) == -1
    assert L.mi_icp_voxelgrid_paint(None, None, 0, None, 0, None) == -1
