"""The exact k-NN references of knn_exact.py, proven on the CPU against the oracle (no GPU needed).

The GPU file (test_gpu_knn_exact.py) holds the kernels to these references bit for bit; here they are held to the
oracle's own EstimateNormals and colour gradients, which share the oracle's neighbour sets exactly."""
import numpy as np
import pytest

import knn_exact as kx
from oracle import oracle as orc

F32 = np.float32


@pytest.fixture(scope="module")
def clouds():
    return {"volume": kx.cloud_volume(60000, 1), "graded": kx.cloud_graded(60000, 2), "sheet": kx.cloud_sheet(30000, 3),
            "duplicates": kx.cloud_duplicates(30000, 4), "outliers": kx.cloud_outliers(60000, 5)}


def test_cumulant_sums_of_the_dyadic_clouds_are_exact_in_fp32(clouds):
    """the premise: up to 100 coordinates, squares and products sum to integers below 2^24 lattice units, so every
    order of summation gives the same fp32 bits -- checked directly, forward against backward, on real neighbour sets"""
    for name, pts in clouds.items():
        kx.assert_exact_cumulants(pts, 100)
        idx, cnt, _, _ = kx.neighbour_sets(pts[:4000], 100)
        P = pts[idx].astype(F32)
        terms = np.concatenate([P, P[..., [0, 0, 0, 1, 1, 2]] * P[..., [0, 1, 2, 1, 2, 2]]], 2)
        fwd, bwd = np.zeros(terms.shape[::2], F32), np.zeros(terms.shape[::2], F32)
        for t in range(100):
            fwd += terms[:, t]
            bwd += terms[:, 99 - t]
        assert np.array_equal(fwd, bwd), name
        assert np.array_equal(fwd.astype(np.float64), terms.astype(np.float64).sum(1)), name


@pytest.mark.parametrize("k", [3, 30, 33, 64, 100])
def test_restated_knn_normals_are_the_oracles_bit_for_bit(clouds, k):
    """the restated phase C on the oracle's own neighbour sets, through eigen3.h on the host, is the oracle's
    EstimateNormals(KNN) bit for bit at every point of every cloud (ambiguous sets included: the oracle's search and
    its normals break ties alike)"""
    for name, pts in clouds.items():
        idx, cnt, _, _ = kx.neighbour_sets(pts, k)
        got = kx.restated_normals(pts, idx, cnt, -1)
        want = orc.estimate_normals_knn(pts, k)
        assert kx.bits_equal(got, want).all(), (name, k, int((~kx.bits_equal(got, want)).sum()))


@pytest.mark.parametrize("max_nn", [16, 33, 65, 100])
def test_restated_radius_normals_are_the_oracles_bit_for_bit(clouds, max_nn):
    """... and EstimateNormals(Radius) with radii that leave some points under 3 neighbours (the (0,0,1) fallback) and
    others over max_nn"""
    steps = int(round((max_nn / (0.008 * 4.19)) ** (1.0 / 3.0)))
    for name in ("graded", "sheet", "duplicates"):
        pts = clouds[name]
        r = kx.dyadic_radius(steps)
        idx, cnt, _, _ = kx.neighbour_sets(pts, max_nn, radius=r)
        got = kx.restated_normals(pts, idx, cnt, -1)
        want = orc.estimate_normals_radius(pts, r, max_nn)
        assert kx.bits_equal(got, want).all(), (name, max_nn)
        if name == "graded":
            assert (cnt < 3).any() and (cnt == max_nn).any()
            assert (got[cnt < 3] == F32([0, 0, 1])).all()


@pytest.mark.parametrize("k", [30, 100])
def test_the_exact_check_has_teeth(clouds, k):
    """one neighbour of each set swapped for the next one out changes the restated normal's bits at >= 90 % of the
    points: a kernel that dropped, doubled or misplaced one candidate could not pass a bit-exact comparison"""
    for name in ("volume", "sheet"):
        pts = clouds[name]
        _, idx, _ = orc.search_knn(pts, pts, k + 1)
        cnt = np.full(len(pts), k)
        base = kx.restated_normals(pts, idx[:, :k], cnt, -1)
        mut = idx[:, :k].copy()
        mut[:, k - 1] = idx[:, k]
        moved = ~kx.bits_equal(kx.restated_normals(pts, mut, cnt, -1), base)
        assert moved.mean() >= 0.9, (name, k, moved.mean())
        dropped = kx.restated_normals(pts, idx[:, :k], cnt - 1, -1)    # one neighbour fewer
        assert (~kx.bits_equal(dropped, base)).mean() >= 0.9, (name, k)


def test_ambiguity_classifier_on_duplicates_and_ties():
    """a set is ambiguous exactly when the tie at the k-th distance spans points at different places"""
    line = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 2, 0], [0, 2, 0], [0, -2, 0], [5, 5, 5]], F32) * F32(kx.SCALE)
    q = np.zeros((1, 3), F32)
    _, cnt, _, amb = kx.neighbour_sets(line, 2, queries=q)
    assert cnt[0] == 2 and amb[0]                         # 1 and 2 tie at the 2nd distance, different places
    _, _, _, amb = kx.neighbour_sets(line, 3, queries=q)
    assert not amb[0]                                     # {0, 1, 2}: the 4th is further
    _, _, _, amb = kx.neighbour_sets(line, 4, queries=q, extra=2)
    assert amb[0]                                         # (0,2,0) twice and (0,-2,0) tie
    two = line[[0, 1, 3, 4, 6]]
    _, _, _, amb = kx.neighbour_sets(two, 3, queries=q, extra=2)
    assert not amb[0]                                     # the tie is two copies of one point
    _, _, _, amb = kx.neighbour_sets(two, 3, queries=q, extra=0)
    assert amb[0]                                         # ... but the group is not seen to its end


@pytest.mark.parametrize("max_nn", [5, 30, 64, 100])
def test_gradient_reference_matches_the_oracle(max_nn):
    """the fp64 normal-equation gradient reference against the oracle's fp32 InitializePointCloudForColoredICP, every
    point within the per-point bound, and the same set of exact zeros (fewer than four others)"""
    pts, nrm, col, radius = kx.gradient_cloud(40000, max_nn, seed=max_nn)
    inten = orc.intensity(col)
    want = orc.color_gradients(pts, nrm, col, radius, max_nn)
    idx, cnt, _, amb = kx.neighbour_sets(pts, max_nn, radius=radius)
    assert not amb.any()
    ref, tol, zero = kx.gradient_reference(pts, nrm, inten, idx, cnt)
    assert np.array_equal((want == 0).all(1), zero)
    assert zero.any() and not zero.all()
    err = np.abs(want.astype(np.float64) - ref).max(1) / tol
    assert err.max() <= 1.0, (float(err.max()), int(err.argmax()))
