"""geometry::DistanceTransform without a GPU: the two engines of the numpy restatement (tests/edt_exact.py) agree; the
per-line routine of the passes (csrc/edt_envelope.h) against an O(n^2) minimum in a stand-alone program built with
AddressSanitizer and UBSan and run directly; the Python type surface; the C ABI's prototypes and its statuses."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import edt_exact as ex
from conftest import ROOT

F = np.float32


# ---- the restatement ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res, n, seed", [(2, 1, 0), (3, 2, 1), (8, 5, 2), (9, 40, 3), (17, 1, 4), (17, 300, 5), (20, 8000, 6)])
def test_the_two_engines_agree(res, n, seed):
    rng = np.random.default_rng(seed)
    sites, dropped = ex.site_set(rng.integers(0, res, (n, 3)), res)
    assert dropped == 0 and 0 < len(sites) <= n
    a, b = ex.field_brute(sites, res), ex.field_scipy(sites, res)
    assert a.dtype == np.int64 and np.array_equal(a, b)
    lin = (sites[:, 0] * res + sites[:, 1]) * res + sites[:, 2]
    assert (a[lin] == 0).all() and np.count_nonzero(a == 0) == len(sites)


def test_restatement_rules():
    # no sites: no distance anywhere
    assert (ex.field_brute(np.zeros((0, 3)), 4) == -1).all() and (ex.field_scipy(np.zeros((0, 3)), 4) == -1).all()
    assert np.isposinf(ex.distance([-1], 0.5)[0]) and ex.distance([0, 4, 3], 0.5).tolist() == [0.0, 1.0, float(F(np.sqrt(F(3))) * F(0.5))]
    # cells outside the grid are dropped and counted, duplicates are one site
    sites, dropped = ex.site_set([[1, 1, 1], [1, 1, 1], [4, 0, 0], [0, -1, 0], [3, 3, 3]], 4)
    assert dropped == 2 and sites.tolist() == [[1, 1, 1], [3, 3, 3]]
    # the reference's unit test: key (5, 5, 5) at voxel_size 1 lands in cell 261 of a 512 grid
    assert ex.cells_of_keys([[5, 5, 5]], 1.0, (0, 0, 0), (0, 0, 0), 512).tolist() == [[261, 261, 261]]
    # the order of the fp32 steps matters: (key * vs + origin_grid) - origin_dt, then / vs
    k = np.array([[3, -7, 100]])
    c = ex.cells_of_keys(k, 0.1, (0.033, -0.05, 0.0), (0.1, 0.2, -0.3), 64)
    vs = F(0.1)
    want = [int(np.floor(F(F(F(F(k[0, a]) * vs) + F(o1)) - F(o2)) / vs)) + 32 for a, (o1, o2) in enumerate(zip((0.033, -0.05, 0.0), (0.1, 0.2, -0.3)))]
    assert c.tolist() == [want]
    # the query rule, a point on a cell boundary belongs to the upper cell; NaN goes outside
    q = ex.cells_of_points([[0.0, -0.5, 0.49], [np.nan, 0, 0]], 0.5, (0, 0, 0), 8)
    assert q[0].tolist() == [4, 3, 4] and not ex.inside(q[1:], 8)[0]
    # the checker: a wrong site, a non-site and a missing -1 are all caught
    sites = np.array([[0, 0, 0], [3, 3, 3]])
    d2 = ex.field_brute(sites, 4)
    near = np.where((d2 == ex.d2_brute(sites[:1], ex.grid_cells(4)))[:, None], sites[0], sites[1])
    assert ex.valid_nearest(near, sites, d2, res=4)[0]
    bad = near.copy()
    bad[-1] = [0, 0, 0]
    assert not ex.valid_nearest(bad, sites, d2, res=4)[0]
    bad[-1] = [3, 3, 2]
    assert not ex.valid_nearest(bad, sites, d2, res=4)[0]
    assert ex.valid_nearest(np.full((64, 3), -1), sites[:0], np.full(64, -1), res=4)[0]
    assert not ex.valid_nearest(np.zeros((64, 3)), sites[:0], np.full(64, -1), res=4)[0]


# ---- the per-line routine, on the host, under the sanitizers ----------------------------------------------------------
def test_envelope_of_every_line_shape_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_edt_envelope")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "cupoch_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "test_edt_envelope.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout[-1500:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "ok"
    assert "Sanitizer" not in out.stderr and "runtime error" not in out.stderr
    src = open(os.path.join(ROOT, "tests", "cpp", "test_edt_envelope.cpp")).read()
    assert re.findall(r'#include\s+"([^"]+)"', src) == ["edt_envelope.h"]      # nothing but that header
    hdr = open(os.path.join(ROOT, "cupoch_amd", "csrc", "edt_envelope.h")).read()
    assert "hip" not in re.sub(r"//[^\n]*", "", hdr).replace("__HIPCC__", "").lower()
    assert "float" not in re.sub(r"//[^\n]*", "", hdr) and "double" not in re.sub(r"//[^\n]*", "", hdr)


# ---- the Python type surface (no GPU is touched) ----------------------------------------------------------------------
def test_python_surface_names_and_defaults(capsys):
    from cupoch_amd import geometry
    d = geometry.DistanceTransform()
    assert d.voxel_size == float(F(0.05)) and d.resolution == 512 and np.array_equal(d.origin, np.zeros(3, F))
    assert repr(d) == "geometry::DistanceTransform with 512 resolution."
    d = geometry.DistanceTransform(0.2, 65, (1.0, 2.0, 3.0))
    assert d.voxel_size == float(F(0.2)) and d.resolution == 65 and np.array_equal(d.origin, np.array([1, 2, 3], F))
    assert repr(d) == "geometry::DistanceTransform with 65 resolution."
    for name in ("reconstruct", "compute_edt", "compute_voronoi_diagram", "get_distance", "get_distances", "get_voxel",
                 "create_from_occupancy_grid", "get_min_bound", "get_max_bound", "get_center",
                 "get_axis_aligned_bounding_box", "translate", "scale", "transform", "rotate", "clear", "is_empty", "voxels",
                 "get_nearest_index_plane", "get_distance_plane"):
        assert hasattr(geometry.DistanceTransform, name), name
    length = F(F(0.2) * F(65)) * F(0.5)
    assert np.array_equal(d.get_min_bound(), np.array([1, 2, 3], F) - length)
    assert np.array_equal(d.get_max_bound(), np.array([1, 2, 3], F) + length)
    assert np.array_equal(d.get_center(), d.origin) and not d.is_empty()
    d.translate([1.0, 0.0, -1.0])
    d.scale(2.0)
    assert np.array_equal(d.origin, np.array([2.0, 2.0, 2.0], F)) and d.voxel_size == float(F(0.2) * F(2.0))
    before = (d.voxel_size, d.resolution, d.origin.copy())
    capsys.readouterr()
    assert d.transform(np.eye(4)) is d and d.rotate(np.eye(3)) is d          # logged, nothing changes
    err = capsys.readouterr().err
    assert "DenseGrid::Transform is not supported" in err and "DenseGrid::Rotate is not supported" in err
    assert (d.voxel_size, d.resolution) == before[:2] and np.array_equal(d.origin, before[2])
    assert d.clear() is d                                                    # no cells made yet: nothing to do

    V = geometry.DistanceVoxel
    v = V()
    assert tuple(v.nearest_index) == (0, 0, 0) and v.distance == 0.0
    v = V([261, 261, 261], 1.5)
    assert repr(v) == "geometry::DistanceVoxel with nearest_index: (261, 261, 261), distance: 1.5)"
    v.nearest_index, v.distance = np.array([1, 2, 3]), 2.0                   # read-write, as in the reference
    assert tuple(v.nearest_index) == (1, 2, 3) and v.distance == 2.0

    # a voxel-size mismatch is logged and changes nothing -- before any device is asked for
    grid = geometry.VoxelGrid()
    grid.voxel_size = 0.3
    d = geometry.DistanceTransform(0.2, 16)
    assert d.compute_edt(grid) is d and d._dt is None
    assert "Unsupport computing Voronoi diagrams from different voxel size." in capsys.readouterr().err
    with pytest.raises(TypeError):
        d.compute_edt(np.zeros((2, 3), F))                                   # cells are integers
    with pytest.raises(ValueError):
        d.compute_edt(geometry.OccupancyGrid(0.2, 32))                       # another resolution


# ---- ABI facts -------------------------------------------------------------------------------------------------------
FAMILY = ("create", "destroy", "reconstruct", "compute_cells", "compute_voxelgrid", "compute_occgrid", "query", "get_voxels")


def _prototypes():
    src = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    src = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return {m.group(1): m.group(2) for m in
            re.finditer(r"MI_ICP_API\s+[\w\s\*]+?\b(mi_icp_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S)}


def test_abi_family_is_declared_exported_and_bound():
    from cupoch_amd import _lib
    _lib.build()
    protos = _prototypes()
    names = ["mi_icp_dt_" + f for f in FAMILY]
    assert sorted(n for n in protos if n.startswith("mi_icp_dt_")) == sorted(names)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert set(names) == set(re.findall(r" T (mi_icp_dt_\w+)", out))
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
    hdr = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    assert "mi_icp_dt_* families beside it" in hdr
    assert re.search(r"#define\s+MI_ICP_DT_MAX_RESOLUTION\s+1024\b", hdr)
    assert "mi_edt" in _lib.UNITS


def test_status_codes_without_a_device():
    """null handles and contexts are statuses, with or without a GPU"""
    from cupoch_amd import _lib
    L = _lib.load()
    assert L.mi_icp_dt_create(None, 16, None) == -1
    assert L.mi_icp_dt_destroy(None, None) == -1
    assert L.mi_icp_dt_reconstruct(None, None, 16) == -1
    assert L.mi_icp_dt_compute_cells(None, None, None, 0, None) == -1
    assert L.mi_icp_dt_compute_voxelgrid(None, None, 1.0, None, None, 0, 1.0, None, None) == -1
    assert L.mi_icp_dt_compute_occgrid(None, None, None, 0.0) == -1
    assert L.mi_icp_dt_query(None, None, 1.0, None, None, 0, None, None) == -1
    assert L.mi_icp_dt_get_voxels(None, None, 1.0, None, None) == -1
