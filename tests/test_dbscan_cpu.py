"""PointCloud::ClusterDBSCAN without a GPU: the two CPU restatements of tests/dbscan_exact.py agree with each other, the
reference's quirks are pinned on hand-built clouds, and the surface exists under the reference's names."""
import inspect
import os
import re

import numpy as np
import pytest

import dbscan_exact as dx

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cloud(rng, n, dup):
    """integer points (exact distances) in a small box, some of them repeated"""
    p = rng.integers(0, 12, (n, 3)).astype(F32)
    if dup:
        p[rng.integers(0, n, n // 4)] = p[rng.integers(0, n, n // 4)]
    return p


@pytest.mark.parametrize("max_edges", [0, 1, 5, 100])
@pytest.mark.parametrize("min_points", [0, 1, 2, 10])
def test_literal_and_by_definition_agree(min_points, max_edges):
    rng = np.random.default_rng(1000 * min_points + max_edges)
    for t in range(12):
        n = int(rng.integers(1, 300))
        pts = _cloud(rng, n, dup=t % 2 == 0)
        eps = float(rng.choice([1.5, 2.5, 3.5]))
        a = dx.literal(pts, eps, min_points, max_edges)
        b = dx.by_definition(pts, eps, min_points, max_edges)
        assert np.array_equal(a[0], b[0]), (t, n, eps)
        assert np.array_equal(a[1], b[1]) and a[2] == b[2], (t, n, eps)


def test_truncated_rows_are_asymmetric_and_still_agree():
    rng = np.random.default_rng(7)
    pts = _cloud(rng, 600, dup=False)
    assert dx.asymmetric_edges(pts, 3.5, 2, 5) > 0
    a, b = dx.literal(pts, 3.5, 2, 5), dx.by_definition(pts, 3.5, 2, 5)
    assert np.array_equal(a[0], b[0]) and a[2] == b[2]


def test_a_later_root_relabels_an_earlier_cluster():
    # max_edges = 1: every row holds the point and its nearest.  0 and 1 are each other's nearest; 2's nearest is 1,
    # but 1's is 0: the edge 2 -> 1 is one way.  0 starts cluster 0 ({0, 1}); nothing smaller reaches 2, so 2 is a
    # root, starts cluster 1 and relabels 0 and 1.  Number 0 is on no point.
    pts = np.array([[0, 0, 0], [1, 0, 0], [2.5, 0, 0]], F32)
    for f in (dx.literal, dx.by_definition):
        labels, deg, nc = f(pts, 2.0, 1, 1)
        assert labels.tolist() == [1, 1, 1] and deg.tolist() == [1, 1, 1] and nc == 2, f.__name__


def test_border_point_takes_the_highest_cluster():
    # two cores 0 and 2 with 3 neighbours each, sharing the border point 1 (a non-core point: 2 neighbours)
    pts = np.array([[0, 0, 0], [2, 0, 0], [4, 0, 0], [-1, 0, 0], [0, 1, 0], [5, 0, 0], [4, 1, 0]], F32)
    for f in (dx.literal, dx.by_definition):
        labels, deg, nc = f(pts, 2.1, 3, 100)
        assert nc == 2 and labels[1] == 1 and labels[0] == 0 and labels[2] == 1, (f.__name__, labels)


def test_isolated_points_with_min_points_one_and_duplicates_past_the_row():
    pts = np.array([[0, 0, 0], [10, 0, 0], [20, 0, 0]], F32)
    for f in (dx.literal, dx.by_definition):
        assert f(pts, 1.0, 1, 100)[0].tolist() == [0, 1, 2]
        assert f(pts, 1.0, 2, 100)[0].tolist() == [-1, -1, -1]
    # three copies of one point, max_edges = 1: row(2) = {0, 1} without 2 itself, so deg(2) = 2
    dup = np.zeros((3, 3), F32)
    for f in (dx.literal, dx.by_definition):
        _, deg, _ = f(dup, 1.0, 1, 1)
        assert deg.tolist() == [1, 1, 2], f.__name__


# ---- the surface ------------------------------------------------------------------------------------------------------
def test_geometry_point_cloud_has_cluster_dbscan():
    from cupoch_amd import geometry
    sig = inspect.signature(geometry.PointCloud.cluster_dbscan)
    ps = sig.parameters
    assert list(ps)[1:] == ["eps", "min_points", "print_progress", "max_edges"]
    assert ps["print_progress"].default is False and ps["max_edges"].default == 100


def test_utility_int_vector_exists():
    from cupoch_amd import utility
    assert issubclass(utility.IntVector, utility.DeviceVector) and utility.IntVector.cols == 0


def test_engine_has_cluster_dbscan():
    from cupoch_amd.engine import Engine
    ps = inspect.signature(Engine.cluster_dbscan).parameters
    assert list(ps)[1:] == ["points", "eps", "min_points", "max_edges"] and ps["max_edges"].default == 100


def test_abi_entry_point_is_declared_and_bound():
    from cupoch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    assert re.search(r"MI_ICP_API int mi_icp_cluster_dbscan\(", hdr)
    res, args = _lib.SIGNATURES["mi_icp_cluster_dbscan"]
    assert len(args) == 10


def test_cpp_surface_declares_the_reference_signature():
    h = open(os.path.join(ROOT, "cupoch_amd", "cpp", "include", "cupoch", "geometry", "pointcloud.h")).read()
    assert re.search(r"std::unique_ptr<utility::device_vector<int>>\s+ClusterDBSCAN\(float eps, size_t min_points, "
                     r"bool print_progress = false,\s+size_t max_edges = knn::NUM_MAX_NN\) const;", h)
    py = open(os.path.join(ROOT, "cupoch_amd", "cpp", "src", "pybind_module.cpp")).read()
    assert '"cluster_dbscan"' in py and '"print_progress"_a = false' in py and '"max_edges"_a = knn::NUM_MAX_NN' in py
    assert 'py::class_<IntVector>(mu, "IntVector")' in py
