"""geometry::OccupancyGrid without a GPU: the numpy restatement of the contract (tests/occgrid_exact.py) reproduces the
reference's four unit tests (src/tests/geometry/occupancygrid.cpp) and the two facts the kernels' plan rests on; the
Python type surface; the C ABI's prototypes."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import occgrid_exact as ox
from conftest import ROOT

F = np.float32


# ---- the reference's unit tests on the restatement (a sparse grid: 512^3 voxels, a handful known) ------------------------
def test_restatement_bounds():
    g = ox.Grid(dense=False)
    assert g.voxel_size == F(0.05) and g.resolution == 512
    g.voxel_size = F(5)
    ox.add_voxels(g, [[0, 0, 0]])
    ox.add_voxels(g, [[511, 511, 511]])
    assert np.array_equal(ox.get_min_bound(g), np.full(3, -1280.0, F))
    assert np.array_equal(ox.get_max_bound(g), np.full(3, 1280.0, F))


def test_restatement_get_voxel():
    g = ox.Grid(dense=False)
    g.voxel_size = F(1.0)
    h = 512 // 2
    want = []
    for occupied in (True, True, False):
        ox.add_voxels(g, [[h + 1, h, h]], occupied)
        p, ijk = ox.query(g, [[1.5, 0.0, 0.0]])
        assert tuple(ijk[0]) == (h + 1, h, h) and not np.isnan(p[0])
        want.append(p[0])
    assert want[0] == F(0.85) and want[1] == F(F(0.85) + F(0.85)) and want[2] == F(F(1.7) + F(-0.4))
    np.testing.assert_allclose(want, [0.85, 1.70, 1.70 - 0.4], rtol=1e-6)
    # a point outside the grid on one axis is unknown, whatever its linear index would alias to
    assert np.isnan(ox.query(g, [[1.5, 256.5, 0.0]])[0][0])


def test_restatement_insert():
    g = ox.Grid(1.0, 512, (-0.5, -0.5, 0.0), dense=False)
    st = {}
    ox.insert(g, [[0.0, 0.0, 3.5]], [0.0, 0.0, 0.0], stats=st)
    ijk, p, _ = ox.extract(g, ox.KNOWN)
    assert len(ijk) == 4 and st["n_div"] == 4 and st["free"] == 3 and st["occupied"] == 1
    h = 256
    assert [tuple(v - h) for v in ijk] == [(0, 0, 0), (0, 0, 1), (0, 0, 2), (0, 0, 3)]
    assert list(p) == [F(-0.4)] * 3 + [F(0.85)]
    known = ~np.isnan(ox.query(g, [[0, 0, 0.5], [0, 0, 1.5], [0, 0, 2.5], [0, 0, 3.5], [0, 0, 4.5]])[0])
    assert list(known) == [True, True, True, True, False]
    assert len(ox.extract(g, ox.FREE)[0]) == 3 and len(ox.extract(g, ox.OCCUPIED)[0]) == 1


def test_restatement_set_free_area():
    g = ox.Grid(dense=False)
    ox.set_free_area(g, [0, 0, 0], [0.1, 0.1, 0.1])
    ijk, p, _ = ox.extract(g, ox.FREE)
    assert len(ijk) == 27 and (p == F(-0.4)).all() and len(ox.extract(g, ox.OCCUPIED)[0]) == 0
    assert tuple(g.min_bound) == (256, 256, 256) and tuple(g.max_bound) == (258, 258, 258)
    ox.set_free_area(g, [0, 0, 0], [0.1, 0.1, 0.1])          # no clamp, and the bounds are overwritten, not widened
    for _ in range(5):
        ox.set_free_area(g, [0, 0, 0], [0.01, 0.01, 0.01])
    assert tuple(g.max_bound) == (256, 256, 256)
    assert ox.query(g, [[0.01, 0.01, 0.01]])[0][0] < F(-2.0)


def test_walks_leave_the_box_of_their_end_voxels():
    """the half-voxel first boundary: of 20,000 random rays thousands emit a voxel outside the bounding box of their start
    and end voxels -- so neither the bounds nor a sweep's extent may come from the end points"""
    rng = np.random.default_rng(0)
    ends = rng.uniform(-1.0, 1.0, (20000, 3)).astype(F)
    start = np.array([0.013, -0.021, 0.007], F)
    vox, left = ox.traversal(start, ends, F(0.05), 3 * 41)
    assert 1000 < int(left.sum()) < 19000
    worst = 0
    c0, last = ox.floor_int(start / F(0.05)), ox.floor_int((ends / F(0.05)).astype(F))
    for i in np.nonzero(left)[0][:2000]:
        lo, hi = np.minimum(c0, last[i]), np.maximum(c0, last[i])
        worst = max(worst, int(np.maximum(lo - vox[i], vox[i] - hi).max()))
    assert worst == 1
    # the walk never emits its end voxel, always its start voxel, and never the same voxel twice
    for i in range(0, 20000, 97):
        v = vox[i]
        assert tuple(v[0]) == tuple(c0) and not (v == last[i]).all(1).any() and len(np.unique(v, axis=0)) == len(v)


def test_duplicates_and_refusals_in_the_restatement():
    g = ox.Grid(0.1, 16)
    ox.add_voxels(g, [[1, 2, 3], [1, 2, 3], [4, 5, 6], [1, 2, 3]], True)       # once per distinct voxel
    assert g.prob[g.linear([[1, 2, 3]])[0]] == F(0.85) and np.count_nonzero(~np.isnan(g.prob)) == 2
    before = g.prob.copy()
    with pytest.raises(ox.Refused):
        ox.add_voxels(g, [[1, 2, 3], [16, 0, 0]], True)
    with pytest.raises(ox.Refused):
        ox.insert(g, [[0.1 * (ox.MAX_NDIV + 2), 0, 0]], [0, 0, 0])
    with pytest.raises(ox.Refused):
        ox.Grid(0.1, 1)
    with pytest.raises(ox.Refused):
        ox.Grid(0.1, ox.MAX_RESOLUTION + 1)
    assert np.array_equal(before.view(np.uint32), g.prob.view(np.uint32))
    ox.insert(g, [[np.nan, 0, 0], [0.3, np.inf, 0]], [0, 0, 0])                # skipped points: nothing happens
    assert np.array_equal(before.view(np.uint32), g.prob.view(np.uint32))


# ---- the Python type surface (no GPU is touched) ----------------------------------------------------------------------
def test_python_surface_names_and_defaults():
    from cupoch_amd import geometry
    g = geometry.OccupancyGrid()
    assert g.voxel_size == float(F(0.05)) and g.resolution == 512 and np.array_equal(g.origin, np.zeros(3, F))
    assert (g.clamping_thres_min, g.clamping_thres_max, g.prob_hit_log, g.prob_miss_log, g.occ_prob_thres_log) == \
        (-2.0, 3.5, 0.85, -0.4, 0.0)
    assert g.visualize_free_area is True
    g2 = geometry.OccupancyGrid(0.2, 64, (1.0, 2.0, 3.0))
    assert g2.voxel_size == float(F(0.2)) and g2.resolution == 64 and np.array_equal(g2.origin, np.array([1, 2, 3], F))
    for name in ("voxel_size", "resolution", "origin", "clamping_thres_min", "clamping_thres_max", "prob_hit_log",
                 "prob_miss_log", "occ_prob_thres_log", "visualize_free_area"):
        setattr(g2, name, getattr(g, name))                  # read-write attributes
        assert np.array_equal(getattr(g2, name), getattr(g, name))
    for name in ("insert", "add_voxel", "add_voxels", "set_free_area", "get_voxel", "is_occupied", "is_unknown",
                 "extract_known_voxels", "extract_free_voxels", "extract_occupied_voxels", "voxels", "reconstruct", "clear",
                 "get_min_bound", "get_max_bound", "get_center", "translate", "scale", "transform", "rotate",
                 "min_bound", "max_bound"):
        assert hasattr(geometry.OccupancyGrid, name), name
    assert not hasattr(geometry.OccupancyGrid, "create_from_voxel_grid")      # not built, and not pretended
    assert callable(geometry.PointCloud.create_from_occupancy_grid)
    g2.translate([1.0, 0.0, -1.0])
    g2.scale(2.0)
    assert np.array_equal(g2.origin, np.array([1.0, 0.0, -1.0], F)) and g2.voxel_size == float(F(0.05) * F(2.0))
    assert np.array_equal(g2.get_center(), g2.origin)
    with pytest.raises(RuntimeError):
        g2.transform(np.eye(4))
    with pytest.raises(RuntimeError):
        g2.rotate(np.eye(3))

    V = geometry.OccupancyVoxel
    v = V()
    assert tuple(v.grid_index) == (0, 0, 0) and np.isnan(v.prob_log) and tuple(v.color) == (0.0, 0.0, 1.0)
    v = V([1, 2, 3])
    assert tuple(v.grid_index) == (1, 2, 3) and np.isnan(v.prob_log)
    v = V([1, 2, 3], 0.5)
    assert v.prob_log == 0.5 and tuple(v.color) == (0.0, 0.0, 1.0)
    v = V([1, 2, 3], 0.5, [0.25, 0.5, 0.75])
    assert tuple(v.color) == (0.25, 0.5, 0.75)
    assert repr(v) == "geometry::OccupancyVoxel with grid_index: (1, 2, 3), prob_log: 0.5, color: (0.25, 0.5, 0.75)"


# ---- ABI facts -------------------------------------------------------------------------------------------------------
FAMILY = ("create", "destroy", "reset", "reconstruct", "insert", "add_voxels", "set_free_area", "query", "extract",
          "get_bounds", "get_voxels")


def _prototypes():
    src = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return {m.group(1): m.group(2) for m in
            re.finditer(r"MI_ICP_API\s+[\w\s\*]+?\b(mi_icp_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_abi_family_is_declared_without_a_memory_kind_and_bound():
    from cupoch_amd import _lib
    protos = _prototypes()
    names = ["mi_icp_occgrid_" + f for f in FAMILY]
    assert sorted(n for n in protos if n.startswith("mi_icp_occgrid_")) == sorted(names)
    for n in names:
        args = [a.strip() for a in protos[n].split(",")]
        assert "mem_kind" not in protos[n]                   # device pointers only (the header's preamble says so)
        assert args[0] == "mi_icp_ctx* ctx"
        res, argtypes = _lib.SIGNATURES[n]
        assert res is C.c_int and len(argtypes) == len(args), n
        for a, t in zip(args, argtypes):                     # every pointer is bound as one, every scalar by its type
            if "*" in a:
                assert t is C.c_void_p or issubclass(t, C._Pointer), (n, a)
            elif a.startswith("int64_t"):
                assert t is C.c_int64, (n, a)
            elif a.startswith("float"):
                assert t is C.c_float, (n, a)
            else:
                assert a.startswith("int ") and t is C.c_int, (n, a)
    assert "mi_icp_debug_occupancy" in _lib.SIGNATURES       # the unrelated entry keeps its name
    hdr = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    assert "THE ONE EXCEPTION is the mi_icp_occgrid_* family" in hdr
    fields = [f for f, _ in _lib.OccGridParams._fields_]
    assert fields == ["voxel_size", "origin", "clamping_thres_min", "clamping_thres_max", "prob_hit_log", "prob_miss_log",
                      "occ_prob_thres_log"] and C.sizeof(_lib.OccGridParams) == 36
    for name, val in (("MI_ICP_OCCGRID_MAX_RESOLUTION", ox.MAX_RESOLUTION), ("MI_ICP_OCCGRID_MAX_NDIV", ox.MAX_NDIV)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, val), hdr)
    assert "mi_occgrid" in _lib.UNITS


def test_status_codes_without_a_device():
    """null handles and contexts are statuses, with or without a GPU"""
    from cupoch_amd import _lib
    L = _lib.load()
    assert L.mi_icp_occgrid_create(None, 16, None) == -1
    assert L.mi_icp_occgrid_reset(None, None) == -1
    assert L.mi_icp_occgrid_get_bounds(None, None, None, None) == -1
