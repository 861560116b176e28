"""CPU: the restatement of the outlier filters and the selections (tests/outlier_exact.py) on the reference's own test
cases and against O(n^2) restatements, and the ctypes rows of the four entry points against the header."""
import os
import re

import numpy as np
import pytest

import outlier_exact as ox

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32

CROSS = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [2, 0, 0]], F32)
PICKED = [3, 10, 24, 32, 47, 51, 66, 79, 85, 98]


def test_radius_outliers_on_the_reference_cross_keeps_only_the_origin():
    # tests/geometry/pointcloud.cpp:676-692 of the reference: RemoveRadiusOutliers(6, 1.1)
    cnt, keep = ox.radius(CROSS, 6, 1.1)
    assert np.flatnonzero(keep).tolist() == [0]
    assert cnt.tolist() == [7, 3, 2, 2, 2, 2, 2, 2]
    bcnt, bkeep = ox.brute_radius(CROSS, 6, 1.1)
    assert np.array_equal(cnt, bcnt) and np.array_equal(keep, bkeep)


def test_select_by_index_of_ten_from_a_hundred():
    # tests/geometry/pointcloud.cpp:303-334 of the reference: the selection is the points at those indices, in order
    pts = np.random.default_rng(0).random((100, 3), dtype=F32)
    sel = ox.select(100, PICKED)
    assert np.array_equal(pts[sel], pts[np.array(PICKED)])
    inv = ox.select(100, PICKED, invert=True)
    assert len(inv) == 90 and not set(inv.tolist()) & set(PICKED) and np.all(np.diff(inv) > 0)
    assert np.array_equal(ox.select(100, PICKED + PICKED[:3], invert=True), inv)   # repeats count once


def _lattice(n, seed, span=20):
    return (np.random.default_rng(seed).integers(-span, span + 1, (n, 3)) * 0.125).astype(F32)


@pytest.mark.parametrize("k", [1, 3, 8, 20])
@pytest.mark.parametrize("seed", [0, 1])
def test_statistic_equals_the_brute_force_restatement(k, seed):
    pts = _lattice(300, seed, span=6)                    # many ties and duplicates among the distances
    avg, thr, keep = ox.statistical(pts, k, 2.0)
    bavg, bthr, bkeep = ox.brute_statistical(pts, k, 2.0)
    assert np.array_equal(avg, bavg)
    assert thr == pytest.approx(bthr, rel=1e-12)
    assert np.array_equal(keep, bkeep)


def test_fewer_points_than_neighbours_averages_what_is_there():
    pts = _lattice(5, 3)
    avg, _, _ = ox.statistical(pts, 20, 1.0)
    bavg, _, _ = ox.brute_statistical(pts, 20, 1.0)
    assert np.array_equal(avg, bavg)
    D = ox.brute_d2(pts).astype(np.float64)
    assert np.allclose(avg, D.mean(1), rtol=1e-6)        # all five points, the point itself included


def test_all_duplicate_points_are_all_removed():
    pts = np.repeat(np.array([[0.5, -0.25, 2.0]], F32), 40, axis=0)
    avg, thr, keep = ox.statistical(pts, 8, 2.0)
    assert (avg == 0).all() and not keep.any()          # avg > 0 is required, as in the reference


def test_one_point_gives_an_empty_result():
    avg, thr, keep = ox.statistical(np.zeros((1, 3), F32), 4, 2.0)
    assert thr == -np.inf and not keep.any()
    avg, thr, keep = ox.statistical(np.zeros((0, 3), F32), 4, 2.0)
    assert len(keep) == 0


@pytest.mark.parametrize("nb", [1, 4, 12])
def test_radius_counts_equal_the_brute_force_restatement(nb):
    pts = _lattice(400, nb, span=8)
    r = 0.3                                               # r*r in fp32 lies off every lattice d2 (multiples of 1/64)
    cnt, keep = ox.radius(pts, nb, r)
    bcnt, bkeep = ox.brute_radius(pts, nb, r)
    assert np.array_equal(cnt, bcnt) and np.array_equal(keep, bkeep)


def test_uniform_indices():
    assert ox.uniform(10, 3).tolist() == [0, 3, 6]
    assert ox.uniform(5, 1).tolist() == [0, 1, 2, 3, 4]
    assert ox.uniform(5, 7).tolist() == []


def _declared_args():
    src = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"MI_ICP_API\s+int\s+(mi_icp_\w+)\s*\(([^)]*)\)", src):
        out[m.group(1)] = len([a for a in m.group(2).split(",") if a.strip()])
    return out


@pytest.mark.parametrize("name", ["mi_icp_remove_statistical_outliers", "mi_icp_remove_radius_outliers",
                                  "mi_icp_select_by_index", "mi_icp_uniform_downsample"])
def test_signature_rows_have_the_header_argument_counts(name):
    from cupoch_amd import _lib
    decl = _declared_args()
    assert name in decl and name in _lib.SIGNATURES
    restype, args = _lib.SIGNATURES[name]
    assert len(args) == decl[name]
