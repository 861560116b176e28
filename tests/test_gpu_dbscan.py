"""GPU: PointCloud::ClusterDBSCAN (include/mi_icp.h mi_icp_cluster_dbscan, knn_normals_kernel<4>, csrc/dbscan.h) held to
the CPU restatements of tests/dbscan_exact.py.

On dyadic clouds (tests/knn_exact.py) with a dyadic radius no squared distance equals eps^2 and every one is exact, so
rows, degrees, labels and the cluster count must equal the restatement exactly, at every candidate-list capacity and with
truncated, asymmetric rows.  The real scans and a 2M-point cloud are held to the same equality."""
import os

import numpy as np
import pytest
import torch

import dbscan_exact as dx
import knn_exact as kx

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLOUDS = {"volume": kx.cloud_volume, "graded": kx.cloud_graded, "sheet": kx.cloud_sheet, "outliers": kx.cloud_outliers,
          "duplicates": kx.cloud_duplicates}
MAX_EDGES = [0, 1, 9, 31, 32, 63, 64, 100]


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _radius_for(pts, target, seed=0):
    """a dyadic radius at which the cloud's points have about `target` neighbours on average"""
    rng = np.random.default_rng(seed)
    from scipy.spatial import cKDTree
    tree = cKDTree(pts.astype(np.float64))
    q = pts[rng.permutation(len(pts))[:400]].astype(np.float64)
    for steps in range(1, 400):
        r = kx.dyadic_radius(steps)
        if tree.query_ball_point(q, r, return_length=True).mean() >= target:
            return r
    return kx.dyadic_radius(400)


def _check(eng, pts, eps, min_points, max_edges, case, ref=dx.by_definition):
    lab, deg, nc = eng.cluster_dbscan(_dev(pts), eps, min_points, max_edges)
    rl, rd, rn = ref(pts, eps, min_points, max_edges)
    assert np.array_equal(_np(deg), rd), "%s: degrees differ at %d points" % (case, int((_np(deg) != rd).sum()))
    bad = np.flatnonzero(_np(lab) != rl)
    assert not len(bad), "%s: %d labels differ, first at %d (%d vs %d)" % (case, len(bad), bad[0], _np(lab)[bad[0]], rl[bad[0]])
    assert nc == rn, (case, nc, rn)
    return _np(lab)


# ---- exactness on dyadic clouds --------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_edges", MAX_EDGES)
@pytest.mark.parametrize("cloud", sorted(CLOUDS))
def test_labels_exact_on_dyadic_clouds(eng, cloud, max_edges):
    pts = CLOUDS[cloud](20_000, seed=max_edges + 11)
    # about as many neighbours as the row holds: some rows truncated, some not
    eps = _radius_for(pts, max(3, 0.8 * (max_edges + 1)))
    for mp in sorted({0, 1, 2, max(1, max_edges // 2), 10}):
        _check(eng, pts, eps, mp, max_edges, "%s max_edges=%d min_points=%d" % (cloud, max_edges, mp))


@pytest.mark.parametrize("max_edges", [1, 9, 31])
def test_truncated_asymmetric_rows_match_the_literal_loop(eng, max_edges):
    pts = kx.cloud_volume(3000, seed=5 + max_edges)
    eps = _radius_for(pts, 3 * (max_edges + 1))
    mp = max(1, max_edges // 2)
    assert dx.asymmetric_edges(pts, eps, mp, max_edges) > 0, "the case lost its one-way edges"
    _check(eng, pts, eps, mp, max_edges, "asymmetric max_edges=%d" % max_edges, ref=dx.literal)
    _check(eng, pts, eps, mp, max_edges, "asymmetric max_edges=%d" % max_edges)


def test_a_later_root_relabels_an_earlier_cluster(eng):
    pts = np.array([[0, 0, 0], [1, 0, 0], [2.5, 0, 0]], F32)
    lab, deg, nc = eng.cluster_dbscan(_dev(pts), 2.0, 1, 1)
    assert _np(lab).tolist() == [1, 1, 1] and _np(deg).tolist() == [1, 1, 1] and nc == 2


# ---- the reference benchmark's own call -------------------------------------------------------------------------------
def test_fragment_points_benchmark_call(eng):
    pts = np.load(os.path.join(GOLDEN, "fragment_points.npz"))["points"].astype(F32)
    lab = _check(eng, pts, 0.02, 10, 100, "fragment_points (0.02, 10)")
    assert lab.max() >= 1 and (lab == -1).any()


def test_fragment_every3rd_second_eps(eng):
    pts = np.load(os.path.join(GOLDEN, "fragment_every3rd.npz"))["points"].astype(F32)
    _check(eng, pts, 0.03, 10, 100, "fragment_every3rd (0.03, 10)")


# ---- scale ----------------------------------------------------------------------------------------------------------
def test_two_million_points_in_blobs_and_noise(eng):
    rng = np.random.default_rng(3)
    centres = rng.uniform(-50, 50, (200, 3))
    blobs = (centres[rng.integers(0, 200, 1_900_000)] + rng.normal(0, 0.6, (1_900_000, 3)))
    noise = rng.uniform(-60, 60, (100_000, 3))
    pts = np.concatenate([blobs, noise]).astype(F32)
    pts = pts[rng.permutation(len(pts))]
    _check(eng, pts, 0.16, 10, 100, "2M blobs")


# ---- memory kinds, determinism, isolation, errors ---------------------------------------------------------------------
def test_host_and_device_memory_agree(eng):
    pts = kx.cloud_graded(30_000, seed=2)
    eps = _radius_for(pts, 12)
    ld, dd, nd = eng.cluster_dbscan(_dev(pts), eps, 5)
    lh, dh, nh = eng.cluster_dbscan(pts, eps, 5)
    assert isinstance(lh, np.ndarray) and lh.dtype == np.int32 and ld.dtype == torch.int32 and ld.is_cuda
    assert np.array_equal(_np(ld), lh) and np.array_equal(_np(dd), dh) and nd == nh


def test_labels_are_deterministic(eng):
    from cupoch_amd.engine import Engine
    pts = kx.cloud_duplicates(50_000, seed=4)
    eps = _radius_for(pts, 20)
    a = _np(eng.cluster_dbscan(_dev(pts), eps, 8, 9)[0])
    b = _np(eng.cluster_dbscan(_dev(pts), eps, 8, 9)[0])
    e2 = Engine(0)
    try:
        c = _np(e2.cluster_dbscan(_dev(pts), eps, 8, 9)[0])
    finally:
        e2.close()
    assert a.tobytes() == b.tobytes() == c.tobytes()


def test_the_callers_target_survives(eng):
    rng = np.random.default_rng(9)
    tgt = rng.random((20_000, 3), dtype=F32)
    q = rng.random((3000, 3), dtype=F32)
    eng.set_target(_dev(tgt))
    before = eng.search_knn(_dev(q), 8)
    eng.cluster_dbscan(_dev(rng.random((40_000, 3), dtype=F32)), 0.03, 5)
    after = eng.search_knn(_dev(q), 8)
    for x, y in zip(before, after):
        assert np.array_equal(_np(x), _np(y))


def test_errors_and_edges(eng):
    from cupoch_amd._lib import MiIcpError
    pts = _dev(np.random.default_rng(1).random((1000, 3), dtype=F32))
    for eps, mp, me in [(0.0, 5, 100), (-0.1, 5, 100), (float("nan"), 5, 100), (float("inf"), 5, 100),
                        (0.1, -1, 100), (0.1, 5, -1), (0.1, 5, 101)]:
        with pytest.raises(MiIcpError):
            eng.cluster_dbscan(pts, eps, mp, me)
    lab, deg, nc = eng.cluster_dbscan(pts, 0.1, 5, 100)
    assert len(lab) == 1000
    lab, deg, nc = eng.cluster_dbscan(np.zeros((0, 3), F32), 0.1, 5)
    assert len(lab) == 0 and nc == 0
    lab, deg, nc = eng.cluster_dbscan(_dev(np.zeros((1, 3), F32)), 0.1, 1)
    assert _np(lab).tolist() == [0] and _np(deg).tolist() == [0] and nc == 1
    lab, deg, nc = eng.cluster_dbscan(_dev(np.zeros((1, 3), F32)), 0.1, 2)
    assert _np(lab).tolist() == [-1] and nc == 0


# ---- both front ends, the reference's clustering.py flow --------------------------------------------------------------
def test_both_front_ends_and_the_clustering_example():
    from cupoch_amd import geometry, pybind, utility
    pts = np.load(os.path.join(GOLDEN, "fragment_every3rd.npz"))["points"].astype(F32)
    ref, _, _ = dx.by_definition(pts, 0.02, 10, 100)
    outs = []
    for mod in (geometry, pybind.geometry):
        pcl = mod.PointCloud()
        pcl.points = (utility if mod is geometry else pybind.utility).Vector3fVector(pts)
        v = pcl.cluster_dbscan(eps=0.02, min_points=10, print_progress=True)
        assert type(v).__name__ == "IntVector"
        labels = np.array(v.cpu())
        assert labels.dtype == np.int32 and np.array_equal(labels, ref)
        max_label = labels.max()
        colors = np.stack([labels / (max_label if max_label > 0 else 1)] * 3, 1).astype(F32)
        colors[labels < 0] = 0
        pcl.colors = (utility if mod is geometry else pybind.utility).Vector3fVector(colors)
        assert max_label + 1 >= 1
        outs.append(labels)
    assert np.array_equal(outs[0], outs[1])
