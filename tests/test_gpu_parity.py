"""GPU parity tests: the HIP path through the C ABI against the CPU oracle on
identical inputs, the reference's golden vectors, and edge cases.
Integer / index results are bit-exact (up to equal-distance ties, which the
reference resolves by traversal order); fp32 per-point values (d2) are
bit-exact; fp64-accumulated sums agree to 1e-9 relative; final transforms to
1e-5 Frobenius (the tolerance BASELINE.json's north_star states)."""
import numpy as np
import pytest
import torch

from conftest import make_pair
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

P2P, PT2PL, SYM, GICP = 1, 2, 3, 5


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def cuda(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def rigid(angle, axis, t):
    axis = np.asarray(axis, np.float64)
    axis /= np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)
    T[:3, 3] = t
    return T.astype(np.float32)


def check_nn(idx, d2, oi, od, src_t, tgt):
    """bit-exact d2; index equal, or a genuine tie (same d2 to a different point)."""
    oi, od = oi[:, 0], od[:, 0]
    assert np.array_equal(np.isinf(d2), np.isinf(od)), "hit/miss pattern differs"
    assert np.array_equal(idx < 0, oi < 0)
    hit = oi >= 0
    assert np.array_equal(d2[hit], od[hit]), "d2 not bit-exact: max diff %g" % np.abs(d2[hit] - od[hit]).max()
    diff = np.flatnonzero(idx != oi)
    if len(diff):
        # ties only: the engine's pick must be at exactly the same distance
        dd = src_t[diff] - tgt[idx[diff]]
        d_alt = (dd[:, 2] * dd[:, 2] + (dd[:, 1] * dd[:, 1] + dd[:, 0] * dd[:, 0])).astype(np.float32)
        assert np.allclose(d_alt, od[diff], rtol=1e-6), "index mismatch that is not a tie"
        # (in general position ties are rare; on a lattice or among duplicated points -- the fuzz test's fourth
        # cloud kind -- equidistant targets are the rule, and every one of them has just been checked)
        if len(np.unique(tgt[:, 0])) > 0.9 * len(tgt):
            assert len(diff) <= max(2, len(idx) // 1000)


# --------------------------------------------------------------------------- search
@pytest.mark.parametrize("n", [1, 5, 8, 9, 63, 64, 65, 513, 4096, 100000])
def test_radius_1nn_matches_oracle_bit_exact(eng, n):
    rng = np.random.default_rng(n)
    tgt = rng.random((n, 3), dtype=np.float32)
    m = max(1, n // 2 + 3)
    src = rng.random((m, 3), dtype=np.float32)
    radius = 1.5 * n ** (-1 / 3)
    eng.set_target(tgt)
    eng.set_source(src)
    idx, d2, stats = eng.search_radius_1nn(radius)
    cnt, oi, od = orc.search_radius(tgt, src, radius, 1)
    check_nn(idx, d2, oi, od, src, tgt)
    assert stats[0] == cnt and stats[2] == m
    np.testing.assert_allclose(stats[1], od[np.isfinite(od)].astype(np.float64).sum(), rtol=1e-12)


def test_radius_1nn_with_transform_and_device_inputs(eng):
    d = make_pair(300000, seed=5)
    T = rigid(0.3, [1, -2, 0.5], [0.05, -0.02, 0.01])
    eng.set_target(cuda(d["tgt"]))
    eng.set_source(cuda(d["src"]))
    idx, d2, stats = eng.search_radius_1nn(d["max_dist"], T)
    src_t = orc.transform_points(T, d["src"])
    cnt, oi, od = orc.search_radius(d["tgt"], src_t, d["max_dist"], 1)
    check_nn(idx, d2, oi, od, src_t, d["tgt"])
    assert 0 < cnt < len(src_t)                      # misses and hits both exercised
    cor = eng.get_correspondences()
    keep = oi[:, 0] >= 0
    ref = np.stack([np.flatnonzero(keep), idx[keep]], 1).astype(np.int32)
    np.testing.assert_array_equal(cor, ref)          # ascending in source index, stable


def test_outliers_of_the_source_under_a_generous_radius(eng):
    """Queries far from the target whose correspondence radius still reaches it: in the wave-uniform walk their cubes
    hold the target whole (1M points + 500 such queries: 86 ms per iteration instead of 0.06).  The walk's cubes are
    capped at ~10 point spacings (kd_build.h tree_scale) and lanes that found nothing that near finish on their own with
    L2 pruning (nn_search.h THE CAP, traverse.h solo_walk): unseeded, seeded and through a whole registration the
    matches are the oracle's, in a time of the usual order."""
    import time
    rng = np.random.default_rng(31)
    n = 200_000
    tgt = rng.random((n, 3), dtype=np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    far = (rng.random((300, 3), dtype=np.float32) * np.float32(40.0) - np.float32(20.0)).astype(np.float32)
    mid = (rng.random((300, 3), dtype=np.float32) * np.float32(3.0) - np.float32(1.0)).astype(np.float32)      # around and inside
    src = np.concatenate([tgt[:60000] + np.float32(0.003), far, mid])[rng.permutation(60600)]
    eng.set_target(cuda(tgt), cuda(nrm))
    eng.set_source(cuda(src))
    for radius in (50.0, 0.5):
        T = rigid(0.02, [0.2, 1, -0.4], [0.004, -0.003, 0.002])
        eng.drop_seeds()
        idx, d2, st = eng.search_radius_1nn(radius, T)                       # from the root
        src_t = orc.transform_points(T, src)
        cnt, oi, od = orc.search_radius(tgt, src_t, radius, 1)
        check_nn(idx, d2, oi, od, src_t, tgt)
        assert st[0] == cnt and (cnt == len(src)) == (radius == 50.0)
        T2 = rigid(0.021, [0.2, 1, -0.4], [0.0045, -0.003, 0.002])           # seeded by those matches
        idx, d2, st = eng.search_radius_1nn(radius, T2)
        assert eng.last_search_kind() == 1
        src_t = orc.transform_points(T2, src)
        cnt, oi, od = orc.search_radius(tgt, src_t, radius, 1)
        check_nn(idx, d2, oi, od, src_t, tgt)
    big_t = rng.random((1_000_000, 3), dtype=np.float32)
    big_n = np.tile(np.array([[0.0, 0.0, 1.0]], np.float32), (1_000_000, 1))
    big_s = np.concatenate([big_t + np.float32(0.002), (rng.random((500, 3), dtype=np.float32) * 40 - 20).astype(np.float32)])
    eng.set_target(cuda(big_t), cuda(big_n))
    eng.set_source(cuda(big_s))
    eng.registration_icp(PT2PL, 50.0, None, 0.0, 0.0, 10, -1.0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = eng.registration_icp(PT2PL, 50.0, None, 0.0, 0.0, 10, -1.0)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 0.1 and res.fitness == 1.0         # (3.5 ms; 860 ms with every lane in the wave's walk)


def test_search_golden_vectors(eng, golden):
    g = golden["lbvh_search_nn"]                     # src/tests/knn/lbvh_knn.cpp:47-86
    eng.set_target(np.asarray(g["points"], np.float32))
    eng.set_source(np.asarray([g["query"]], np.float32))
    idx, d2, _ = eng.search_radius_1nn(1e3)
    assert idx[0] == g["ref_index"] and abs(d2[0] - g["ref_distance2"]) <= 1e-9
    g = golden["kdtree_search_radius"]               # src/tests/knn/kdtree_flann.cpp:93-135, max_nn -> 1
    idx, d2, st = eng.search_radius_1nn(g["radius"])
    assert idx[0] == g["ref_indices"][0] and abs(d2[0] - g["ref_distance2"][0]) <= g["tol"]
    assert st[0] == 1


def test_search_edge_cases(eng):
    tgt = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0]], np.float32)
    eng.set_target(tgt)
    eng.set_source(np.zeros((1, 3), np.float32))
    idx, d2, st = eng.search_radius_1nn(1.0)          # d2 == r2 is NOT a match (strict <)
    assert idx[0] == -1 and np.isinf(d2[0]) and st[0] == 0
    idx, d2, st = eng.search_radius_1nn(1.0001)
    assert idx[0] in (0, 1, 2) and d2[0] == 1.0       # three-way tie: any of them is the reference's answer
    # all-equal points, collinear points, a far outlier
    pts = np.zeros((100, 3), np.float32)
    eng.set_target(pts)
    eng.set_source(pts[:10] + 0.5)
    idx, d2, _ = eng.search_radius_1nn(1.0)
    assert (idx >= 0).all() and np.allclose(d2, 0.75)
    line = np.stack([np.linspace(0, 1, 1000), np.zeros(1000), np.zeros(1000)], 1).astype(np.float32)
    line[-1] = [1e6, -1e6, 1e6]
    eng.set_target(line)
    q = np.array([[0.5004, 0.1, 0.0], [1e6, -1e6, 1e6 + 1], [-5, 0, 0]], np.float32)
    eng.set_source(q)
    idx, d2, _ = eng.search_radius_1nn(2.0)
    _, oi, od = orc.search_radius(line, q, 2.0, 1)
    check_nn(idx, d2, oi, od, q, line)
    # empty target -> every query misses; empty source is a state error on search
    eng.set_target(np.zeros((0, 3), np.float32))
    idx, d2, st = eng.search_radius_1nn(1.0)
    assert (idx == -1).all() and np.isinf(d2).all() and st[0] == 0
    assert len(eng.get_correspondences()) == 0


# --------------------------------------------------------------------------- systems
def _systems_inputs(n=60000, seed=9):
    d = make_pair(n, seed=seed, noise=0.05)
    d["src_cov"] = orc.covariances_from_normals(d["src_nrm"])
    d["tgt_cov"] = orc.covariances_from_normals(d["tgt_nrm"])
    return d


@pytest.mark.parametrize("est", [P2P, PT2PL, SYM, GICP])
def test_compute_system_matches_oracle(eng, est):
    d = _systems_inputs()
    T = rigid(0.01, [0.3, 1, -0.2], [0.002, 0.001, -0.003])
    eng.set_target(cuda(d["tgt"]), cuda(d["tgt_nrm"]), cuda(d["tgt_cov"]))
    eng.set_source(cuda(d["src"]), cuda(d["src_nrm"]), cuda(d["src_cov"]))
    idx, _, _ = eng.search_radius_1nn(d["max_dist"], T)
    got = eng.compute_system(est, T)
    cor = eng.get_correspondences()
    src_t = orc.transform_points(T, d["src"])
    nrm_t = orc.transform_normals(T, d["src_nrm"])
    cov_t = orc.rotate_covariances(T, d["src_cov"])
    ref = orc.compute_system(est, src_t, d["tgt"], cor, nrm_t, d["tgt_nrm"], cov_t, d["tgt_cov"])
    scale = np.abs(ref).max()
    tol = 1e-9 if est != GICP else 2e-5            # GICP goes through acosf/cosf: libm vs device ulps
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * scale)
    # the statistics do not go through GICP's weights: the count is exact and the sum of d^2 is held as everywhere else
    assert got[29] == len(cor)
    np.testing.assert_allclose(got[28], ref[28], rtol=1e-12)
    rm = eng.compute_rmse(est, T)
    rr = orc.compute_rmse(est, src_t, d["tgt"], cor, nrm_t, d["tgt_nrm"], cov_t, d["tgt_cov"])
    assert rm == pytest.approx(rr, rel=1e-5)
    # ComputeTransformation = system + host solve
    U = eng.compute_transformation(est, T, det_thresh=-1.0)
    if est == P2P:
        Uref = orc.kabsch_from_sums(ref, len(d["src"]))
    elif est == SYM:
        ok, half = orc.solve_system(ref, -1.0)
        Uref = np.eye(4, dtype=np.float32)
        Uref[:3, :3] = (half[:3, :3].astype(np.float64) @ half[:3, :3].astype(np.float64)).astype(np.float32)
        Uref[:3, 3] = half[:3, 3]
    else:
        _, Uref = orc.solve_system(ref, -1.0)
    np.testing.assert_allclose(U, Uref, atol=3e-6)


def test_gicp_system_on_covariances_the_eigen_solver_special_cases(eng):
    """GICP's rows are accumulated from S = W W without taking W (reduce.h, eigen3.h gicp_weight), which restates how
    FastEigen3x3 treats its input: scaled by its largest coefficient in general, taken as is when it has no
    off-diagonal entries, zero when nothing in it is positive.  Axis-aligned normals under a pure translation give
    exactly diagonal (Ct + Cs)^-1 (the unscaled branch), alone and mixed with general ones: against the oracle's
    row-by-row form."""
    n = 20000
    rng = np.random.default_rng(17)
    tgt = rng.random((n, 3), dtype=np.float32)
    src = (tgt + np.float32(0.004) * rng.standard_normal((n, 3)).astype(np.float32) + np.array([0.003, -0.002, 0.001], np.float32)).astype(np.float32)
    axes = np.eye(3, dtype=np.float32)
    nrm = axes[rng.integers(0, 3, n)]                               # axis-aligned: diagonal covariances
    gen = rng.standard_normal((n, 3)).astype(np.float32)
    gen /= np.linalg.norm(gen, axis=1, keepdims=True)
    mixed = np.where((np.arange(n) % 3 == 0)[:, None], gen, nrm).astype(np.float32)
    for normals in (nrm, mixed):
        cov = orc.covariances_from_normals(normals)
        T = np.eye(4, dtype=np.float32)
        T[:3, 3] = [0.001, 0.0005, -0.002]                          # no rotation: diagonal stays diagonal
        eng.set_target(cuda(tgt), cuda(normals), cuda(cov))
        eng.set_source(cuda(src), cuda(normals), cuda(cov))
        eng.search_radius_1nn(0.05, T)
        got = eng.compute_system(GICP, T)
        cor = eng.get_correspondences()
        ref = orc.compute_system(GICP, orc.transform_points(T, src), tgt, cor, orc.transform_normals(T, normals), normals,
                                 orc.rotate_covariances(T, cov), cov)
        assert np.isfinite(ref).all() and len(cor) > n // 2
        np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max())
        assert got[29] == len(cor)                                  # (the statistics do not go through the weights)
        np.testing.assert_allclose(got[28], ref[28], rtol=1e-12)


def test_gicp_system_on_singular_and_indefinite_covariances(eng):
    """ADVICE r3 / DESIGN deviation 6, pinned.  (a) A correspondence whose Ct + Cs is SINGULAR (both covariances zero)
    poisons the whole system in the reference's form -- (Ct+Cs)^-1 is not finite -- and here alike.  (b) One whose
    Ct + Cs is INDEFINITE (not a covariance: a negative eigenvalue) gives NaN rows in the reference (cwiseSqrt of a negative
    eigenvalue, eigenvalue.inl SqrtMatrix3x3) but a finite contribution here, because the rows are accumulated from
    S = W W without taking the root: the one place where the two can part on finite inputs, and only on inputs that
    are not covariances."""
    n = 3000
    rng = np.random.default_rng(23)
    tgt = rng.random((n, 3), dtype=np.float32)
    src = (tgt + np.float32(0.002) * rng.standard_normal((n, 3)).astype(np.float32)).astype(np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    cov = orc.covariances_from_normals(nrm)
    T = np.eye(4, dtype=np.float32)

    def systems(cs, ct):
        eng.set_target(cuda(tgt), cuda(nrm), cuda(ct))
        eng.set_source(cuda(src), cuda(nrm), cuda(cs))
        eng.search_radius_1nn(0.05, T)
        got = eng.compute_system(GICP, T)
        cor = eng.get_correspondences()
        ref = orc.compute_system(GICP, src, tgt, cor, nrm, nrm, cs, ct)
        return got, ref, cor

    got, ref, cor = systems(cov, cov)                                   # sane covariances: finite and equal
    assert np.isfinite(ref).all() and np.isfinite(got).all() and len(cor) == n
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max())
    # (a) one point with zero covariance on both sides (source i matches target i here)
    cs, ct = cov.copy(), cov.copy()
    cs[7] = 0.0
    ct[7] = 0.0
    got, ref, cor = systems(cs, ct)
    assert (cor[7] == [7, 7]).all()
    assert not np.isfinite(ref[:27]).all() and not np.isfinite(got[:27]).all()
    assert got[29] == ref[29] == n and np.isfinite(got[28])            # the statistics do not go through the weights
    # (b) one point whose summed covariance is indefinite
    cs, ct = cov.copy(), cov.copy()
    cs[11] = np.diag([1.0, 1.0, -0.8]).astype(np.float32)
    ct[11] = np.diag([0.1, 0.1, 0.1]).astype(np.float32)
    got, ref, cor = systems(cs, ct)
    assert not np.isfinite(ref[:27]).all()                              # the reference's form: NaN rows
    assert np.isfinite(got).all()                                       # here: a finite S = (Ct + Cs)^-1 (scaled)
    # ... and the finite system is the sane one plus that one correspondence's rows: removing the point restores parity
    keep = np.arange(n) != 11
    cor_wo = cor[keep]
    ref_wo = orc.compute_system(GICP, src, tgt, cor_wo, nrm, nrm, cs, ct)
    eng.set_correspondences(cor_wo)
    got_wo = eng.compute_system(GICP, T)
    np.testing.assert_allclose(got_wo, ref_wo, rtol=2e-5, atol=2e-5 * np.abs(ref_wo).max())


def test_explicit_correspondence_set(eng):
    d = _systems_inputs(5000, seed=2)
    eng.set_target(d["tgt"], d["tgt_nrm"])
    eng.set_source(d["src"], d["src_nrm"])
    rng = np.random.default_rng(0)
    cor = np.stack([rng.integers(0, 5000, 3000), rng.integers(0, 5000, 3000)], 1).astype(np.int32)
    eng.set_correspondences(cor)                     # arbitrary pairs, sources repeat
    for est in (P2P, PT2PL, SYM):
        got = eng.compute_system(est)
        ref = orc.compute_system(est, d["src"], d["tgt"], cor, d["src_nrm"], d["tgt_nrm"])
        np.testing.assert_allclose(got, ref, rtol=1e-9, atol=1e-9 * np.abs(ref).max())
    np.testing.assert_array_equal(eng.get_correspondences(), cor)
    eng.set_correspondences(np.zeros((0, 2), np.int32))
    np.testing.assert_array_equal(eng.compute_transformation(PT2PL), np.eye(4))   # empty -> identity


# --------------------------------------------------------------------------- ICP
@pytest.mark.parametrize("est", [P2P, PT2PL, SYM, GICP])
@pytest.mark.parametrize("n", [2000, 100000])
def test_icp_final_transform_matches_oracle(eng, est, n):
    d = make_pair(n, seed=21 + est, noise=0.02)
    kw, okw = {}, {}
    if est in (PT2PL, SYM):
        okw = dict(src_nrm=d["src_nrm"], tgt_nrm=d["tgt_nrm"])
    if est == GICP:
        sc, tc = orc.covariances_from_normals(d["src_nrm"]), orc.covariances_from_normals(d["tgt_nrm"])
        okw = dict(src_cov=sc, tgt_cov=tc)
    eng.set_target(d["tgt"], d["tgt_nrm"] if est != P2P else None, okw.get("tgt_cov"))
    eng.set_source(d["src"], d["src_nrm"] if est == SYM else None, okw.get("src_cov"))
    res = eng.registration_icp(est, d["max_dist"], None, 0.0, 0.0, 15, -1.0)
    T = np.array(res.transformation, np.float32).reshape(4, 4).T
    ref = orc.registration_icp(d["src"], d["tgt"], d["max_dist"], est=est, det_thresh=-1.0,
                               relative_fitness=0.0, relative_rmse=0.0, max_iteration=15, **okw)
    assert res.iterations == 15 and res.nn_passes == 16 and ref.iterations == 15
    err = np.linalg.norm(T - ref.transformation)
    assert err <= 1e-5, "||T - T_oracle||_F = %g" % err
    assert res.fitness == pytest.approx(ref.fitness, abs=2e-5)
    assert res.inlier_rmse == pytest.approx(ref.inlier_rmse, rel=1e-3, abs=1e-7)
    cor = eng.get_correspondences()
    assert (np.diff(cor[:, 0]) > 0).all()
    # The sets are equal except where the two final transforms (equal to ~1e-7: the engine applies
    # the composed T to the pristine source, the reference transforms its copy incrementally) put a
    # source point within rounding of a decision boundary -- and that is PROVEN pair by pair:
    # a differing pair must be a near-tie between two target points, or sit on the radius.
    a = dict(cor.tolist())
    b = dict(ref.correspondence_set.tolist())
    src64 = d["src"].astype(np.float64) @ T[:3, :3].astype(np.float64).T + T[:3, 3].astype(np.float64)
    tgt64 = d["tgt"].astype(np.float64)
    r2 = float(d["max_dist"]) ** 2
    for i in set(a) | set(b):
        ja, jb = a.get(i), b.get(i)
        if ja == jb:
            continue
        da = ((src64[i] - tgt64[ja]) ** 2).sum() if ja is not None else r2
        db = ((src64[i] - tgt64[jb]) ** 2).sum() if jb is not None else r2
        assert abs(da - db) <= 1e-5 * max(da, db), "source %d: %s vs %s is not a near-tie" % (i, ja, jb)


def test_point_to_point_on_an_exactly_planar_cloud_returns_a_rotation(eng):
    """A source whose points all share one coordinate: the Kabsch cross-covariance has a zero row and its smallest
    singular value is rounding noise.  Eigen's JacobiSVD (kabsch.cu:108, full U and V) still yields a proper rotation;
    so must the loop's step (host_solver.h svd3: the column of a vanishing singular value is completed, not divided out)
    -- and the transform equals the oracle's, whose Kabsch is pinned against numpy's fp64 SVD on such clouds."""
    rng = np.random.default_rng(5)
    n = 30000
    tgt = rng.random((n, 3), dtype=np.float32)
    tgt[:, 2] = np.float32(0.25)
    a = 0.01
    Rz = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    src = ((tgt.astype(np.float64) - [0.5, 0.5, 0.25]) @ Rz.T + [0.5, 0.5, 0.25] + [0.004, -0.003, 0.0]).astype(np.float32)
    src[:, 2] = np.float32(0.25)
    src = np.ascontiguousarray(src[rng.permutation(n)])
    r = 0.02
    eng.set_target(tgt)
    eng.set_source(src)
    res = eng.registration_icp(P2P, r, None, 0.0, 0.0, 12, -1.0)
    T = np.array(res.transformation, np.float32).reshape(4, 4).T
    ref = orc.registration_icp(src, tgt, r, est=P2P, det_thresh=-1.0, relative_fitness=0.0, relative_rmse=0.0, max_iteration=12)
    R = T[:3, :3].astype(np.float64)
    assert abs(np.linalg.det(R) - 1.0) <= 1e-5 and np.abs(R @ R.T - np.eye(3)).max() <= 1e-5
    assert np.linalg.norm(T - ref.transformation) <= 1e-5
    assert res.fitness == pytest.approx(ref.fitness, abs=2e-5) and res.fitness > 0.99
    moved = src.astype(np.float64) @ R.T + T[:3, 3]
    assert np.abs(moved[:, 2] - 0.25).max() <= 1e-5          # (the plane stays the plane)


def test_icp_default_criteria_init_and_convergence(eng):
    d = make_pair(50000, seed=77)
    init = rigid(0.01, [0, 0, 1], [0.001, 0.0, -0.001])
    eng.set_target(d["tgt"], d["tgt_nrm"])
    eng.set_source(d["src"])
    res = eng.registration_icp(PT2PL, d["max_dist"], init, 1e-6, 1e-6, 30, -1.0)
    ref = orc.registration_icp(d["src"], d["tgt"], d["max_dist"], init=init, est=orc.EST_PT2PL,
                               tgt_nrm=d["tgt_nrm"], det_thresh=-1.0)
    T = np.array(res.transformation, np.float32).reshape(4, 4).T
    assert np.linalg.norm(T - ref.transformation) <= 1e-5
    assert np.linalg.norm(T - d["T_gt"]) <= 2e-5
    assert res.iterations < 30 and res.iterations == ref.iterations            # converged at the same iteration
    ev = eng.evaluate_registration(d["max_dist"], T)
    oe = orc.evaluate_registration(d["src"], d["tgt"], d["max_dist"], T)
    assert ev.fitness == pytest.approx(oe.fitness, abs=1e-5) and ev.fitness > 0.999


def test_icp_reference_error_paths(eng):
    d = make_pair(3000, seed=4)
    eng.set_target(d["tgt"])                               # no normals
    eng.set_source(d["src"])
    res = eng.registration_icp(PT2PL, d["max_dist"], None, 1e-6, 1e-6, 5, 1e-6)
    np.testing.assert_array_equal(np.array(res.transformation).reshape(4, 4), np.eye(4))  # identity updates
    assert res.fitness > 0.9
    res = eng.registration_icp(P2P, 0.0, None, 1e-6, 1e-6, 5, 1e-6)   # invalid distance: empty result
    assert res.fitness == 0 and res.n_correspondences == 0
    # det_thresh = 1e-6 with a big cloud: fp32 determinant overflows -> identity updates (quirk 6)
    big = make_pair(400000, seed=8)
    eng.set_target(cuda(big["tgt"]), cuda(big["tgt_nrm"]))
    eng.set_source(cuda(big["src"]))
    sys = eng.compute_system(PT2PL) if eng.search_radius_1nn(big["max_dist"])[2][0] else None
    from cupoch_amd.engine import solve_system
    ok_e, _ = solve_system(sys, 1e-6)
    ok_o, _ = orc.solve_system(sys, 1e-6)
    assert ok_e == ok_o


# --------------------------------------------------------------------------- geometry
def test_transform_roundtrip_golden_and_oracle(eng, golden):
    g = golden["pointcloud_transform"]                # src/tests/geometry/pointcloud.cpp:143-174
    T = np.asarray(g["transformation"], np.float32)
    Tinv = np.eye(4, dtype=np.float32)
    Tinv[:3, :3] = T[:3, :3].T
    Tinv[:3, 3] = -T[:3, :3].T @ T[:3, 3]
    p = np.asarray(g["points"], np.float32)
    n = np.asarray(g["normals"], np.float32)
    p1, n1, _ = eng.transform(T, p, n)
    np.testing.assert_array_equal(p1, orc.transform_points(T, p))      # same fp32 expression: bit-exact
    np.testing.assert_array_equal(n1, orc.transform_normals(T, n))
    p2, n2, _ = eng.transform(Tinv, p1, n1)
    np.testing.assert_allclose(p2, p, atol=g["tol"])
    np.testing.assert_allclose(n2, n, atol=g["tol"])
    rng = np.random.default_rng(1)
    cov = rng.standard_normal((1000, 3, 3)).astype(np.float32)
    pts = cuda(rng.standard_normal((1000, 3)).astype(np.float32))
    ref_pts = orc.transform_points(T, pts.cpu().numpy())
    _, _, c1 = eng.transform(T, pts, None, cuda(cov))                   # device tensors: in place
    np.testing.assert_array_equal(pts.cpu().numpy(), ref_pts)
    np.testing.assert_array_equal(c1.cpu().numpy(), orc.rotate_covariances(T, cov))


def _rows(a):
    a = np.asarray(a, np.float64)
    return a[np.lexsort((a[:, 2], a[:, 1], a[:, 0]))]


def test_voxel_downsample_golden(eng, golden):
    g = golden["voxel_down_sample"]                   # src/tests/geometry/pointcloud.cpp:371-469
    p, n, c = eng.voxel_downsample(np.asarray(g["points"], np.float32), g["voxel_size"],
                                   np.asarray(g["normals"], np.float32),
                                   np.asarray(g["colors"], np.float32))
    assert len(p) == len(g["ref_points"])
    np.testing.assert_allclose(_rows(p), _rows(g["ref_points"]), atol=g["tol"])
    np.testing.assert_allclose(_rows(n), _rows(g["ref_normals"]), atol=g["tol"])
    np.testing.assert_allclose(_rows(c), _rows(g["ref_colors"]), atol=g["tol"])


# (the grid's packed key: 12 / 18 / 42 / 3 bits -- one pass with 4 unsorted low bits, two with 2, the 64-bit fallback,
# no pass at all -- then 21 bits, 24, 30, 15 and a grid that is long in one axis only; the last one is the 10M bench's
# shape with runs long enough for the run-wise means: 21 bits, two passes, 5 low bits left to the means kernel.  Where a
# grid has more possible runs than an eighth of the points the key is sorted whole instead)
@pytest.mark.parametrize("n,voxel", [(1000, 0.1), (200000, 0.02), (200000, 1e-4), (5000, 10.0), (300000, 0.01),
                                     (300000, 0.004), (100000, 0.001), (50000, 0.04), (70001, 0.3), (800000, 0.01)])
def test_voxel_downsample_matches_oracle(eng, n, voxel):
    rng = np.random.default_rng(n)
    pts = rng.random((n, 3), dtype=np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    col = rng.random((n, 3), dtype=np.float32)
    p, nn, c = eng.voxel_downsample(cuda(pts), voxel, cuda(nrm), cuda(col))
    rp, rn, rc = orc.voxel_downsample(pts, voxel, nrm, col)
    assert len(p) == len(rp)                                  # same voxels, same (lexicographic) order
    np.testing.assert_allclose(p.cpu().numpy(), rp, atol=1e-6)
    np.testing.assert_allclose(nn.cpu().numpy(), rn, atol=2e-5)
    np.testing.assert_allclose(c.cpu().numpy(), rc, atol=1e-6)
    p0, _, _ = eng.voxel_downsample(pts, 0.0)                 # down_sample.cu:173-176 -> empty cloud
    assert len(p0) == 0
    p1, n1, c1 = eng.voxel_downsample(pts, voxel)             # no normals / colors path
    np.testing.assert_allclose(p1, rp, atol=1e-6)
    assert n1 is None and c1 is None
    if n == 70001:                                            # a slab: 12 bits along x, 1 along y and z
        slab = pts * np.array([50.0, 0.2, 0.2], np.float32)
        ps, _, cs = eng.voxel_downsample(cuda(slab), 0.02, None, cuda(col))
        rs, _, rcs = orc.voxel_downsample(slab, 0.02, None, col)
        assert len(ps) == len(rs)
        np.testing.assert_allclose(ps.cpu().numpy(), rs, atol=4e-6)
        np.testing.assert_allclose(cs.cpu().numpy(), rcs, atol=1e-6)


def test_voxel_downsample_edge_shapes(eng):
    """The run-wise mean kernel's corners: one point; a voxel that holds 50k copies of one point next to sparse ones (a
    run of hundreds of 64-element chunks); colours without normals; every point in ONE voxel; a cloud smaller than a
    wave; a grid whose key needs more than 64 bits (three stable sorts, one per axis) -- each against the oracle (same
    voxels, same lexicographic order)."""
    rng = np.random.default_rng(77)
    one = np.array([[0.3, -0.2, 0.9]], np.float32)
    p, _, _ = eng.voxel_downsample(one, 0.05)
    np.testing.assert_array_equal(p, one)
    heavy = np.concatenate([np.repeat(np.array([[0.5, 0.5, 0.5]], np.float32), 50000, 0),
                            rng.random((3000, 3), dtype=np.float32)])[rng.permutation(53000)]
    col = rng.random((53000, 3), dtype=np.float32)
    for voxel in (0.01, 0.11):
        p, nn, c = eng.voxel_downsample(cuda(heavy), voxel, None, cuda(col))
        rp, _, rc = orc.voxel_downsample(heavy, voxel, None, col)
        assert nn is None and len(p) == len(rp)
        np.testing.assert_allclose(p.cpu().numpy(), rp, atol=1e-6)
        np.testing.assert_allclose(c.cpu().numpy(), rc, atol=2e-6)
    small = rng.random((37, 3), dtype=np.float32)
    nrm = rng.standard_normal((37, 3)).astype(np.float32)
    for voxel in (0.2, 5.0):                                   # 5.0: every point in one voxel
        p, nn, _ = eng.voxel_downsample(small, voxel, nrm)
        rp, rn, _ = orc.voxel_downsample(small, voxel, nrm)
        assert len(p) == len(rp) and (voxel < 1.0 or len(p) == 1)
        np.testing.assert_allclose(p, rp, atol=1e-6)
        np.testing.assert_allclose(nn, rn, atol=2e-5)
    wide = (rng.random((4000, 3)) * 3000.0).astype(np.float32)    # 3 x 22 key bits at voxel 0.001
    wn = rng.standard_normal((4000, 3)).astype(np.float32)
    p, nn, c = eng.voxel_downsample(cuda(wide), 0.001, cuda(wn), cuda(col[:4000]))
    rp, rn, rc = orc.voxel_downsample(wide, 0.001, wn, col[:4000])
    assert len(p) == len(rp)
    np.testing.assert_allclose(p.cpu().numpy(), rp, rtol=1e-6, atol=1e-6)
    np.testing.assert_allclose(nn.cpu().numpy(), rn, atol=2e-5)
    np.testing.assert_allclose(c.cpu().numpy(), rc, atol=2e-6)


def test_voxel_downsample_both_forms_agree_to_the_last_bit_or_two(eng):
    """The 32-bit-key path with the payload carried through the radix passes against the first form (64-bit keys,
    indices, one gather), which now serves only grids whose packed key needs more than 32 bits: ONE far point at
    large positive coordinates leaves the grid's origin where it was (the minimum bound) but stretches the grid to
    3 x 21 bits -- every other voxel must come out in the same place with values that differ at most in the last bit
    or two (both add a voxel's points in fp64, but deal them to their lanes differently)."""
    rng = np.random.default_rng(9)
    n = 400000
    pts = rng.random((n, 3), dtype=np.float32)
    nrm = rng.standard_normal((n, 3)).astype(np.float32)
    col = rng.random((n, 3), dtype=np.float32)
    far = np.full((1, 3), 3000.0, np.float32)
    for v in (0.5, 0.05, 0.011, 0.003):
        a = [np.asarray(x) for x in eng.voxel_downsample(pts, v, nrm, col)]
        b = [np.asarray(x) for x in eng.voxel_downsample(np.vstack([pts, far]), v, np.vstack([nrm, nrm[:1]]),
                                                         np.vstack([col, col[:1]]))]
        for x, y in zip(a, b):
            assert y.shape[0] == x.shape[0] + 1, v          # (the far point's voxel: the largest key, last)
            np.testing.assert_array_max_ulp(x, y[:-1], maxulp=2)
        np.testing.assert_array_equal(b[0][-1], far[0])


def test_covariances_from_normals_matches_oracle(eng):
    rng = np.random.default_rng(0)
    nrm = rng.standard_normal((10000, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[0] = [-1, 0, 0]                                       # c < -0.99 shortcut (generalized_icp.cu:23-26)
    nrm[1] = [1, 0, 0]
    got = eng.covariances_from_normals(nrm, 1e-3)
    np.testing.assert_allclose(got, orc.covariances_from_normals(nrm, 1e-3), atol=1e-7)


def test_estimate_normals_golden_and_oracle(eng, golden):
    g = golden["estimate_normals"]                    # src/tests/geometry/pointcloud.cpp:535-597
    got = eng.estimate_normals_knn(np.asarray(g["points"], np.float32), g["knn"])
    ref = np.asarray(g["ref_normals"], np.float32)
    flip = np.sign(ref[:, 0]) * np.sign(got[:, 0]) < 0
    got[flip] *= -1
    np.testing.assert_allclose(got, ref, atol=g["tol"])
    rng = np.random.default_rng(12)
    pts = rng.random((30000, 3), dtype=np.float32)
    pts[:, 2] = 0.2 * np.sin(3 * pts[:, 0]) + 0.0005 * rng.standard_normal(30000).astype(np.float32)
    for k in (20, 30):
        got = eng.estimate_normals_knn(cuda(pts), k).cpu().numpy()
        ref = orc.estimate_normals_knn(pts, k)
        dots = np.abs((got * ref).sum(1))
        # fp32 raw-moment covariances (the reference's formulation) leave ~1e-3 rad of
        # summation-order noise; a different k-th neighbour on an exact tie moves a few more
        assert (dots > 1 - 1e-4).mean() > 0.995, "normals differ: %g" % (dots > 1 - 1e-4).mean()
        assert np.median(1 - dots) < 1e-6
    # KDTreeSearchParamRadius(radius, max_nn): sparse neighbourhoods fall back to (0,0,1)
    # (with 3-6 neighbours the fp32 raw-moment covariance is nearly singular: its smallest
    # eigenvector amplifies summation-order noise, so the sparse case is held to a looser bar)
    for radius, max_nn, agree in ((0.02, 30, 0.99), (0.004, 16, 0.9)):
        got = eng.estimate_normals_radius(cuda(pts), radius, max_nn).cpu().numpy()
        ref = orc.estimate_normals_radius(pts, radius, max_nn)
        fallback = (ref == np.float32([0, 0, 1])).all(1)
        assert ((got == np.float32([0, 0, 1])).all(1) == fallback).mean() > 0.999
        dots = np.abs((got * ref).sum(1))
        assert (dots > 1 - 1e-3).mean() > agree, (radius, (dots > 1 - 1e-3).mean())
    assert fallback.any() and not fallback.all()


def test_estimate_normals_disagreements_are_explained(eng):
    """the normals agree with the oracle's only statistically (fp32 raw-moment
    covariances, estimate_normals.cu:38-64).  This pins WHY: the neighbour sets themselves are
    identical (bit-exact distances; indices up to ties at the k-th distance), every normal --
    the engine's and the oracle's -- matches the fp64 normal of its own neighbour set wherever the
    covariance's smallest eigenvalue is well separated, and every engine/oracle disagreement sits
    on a differing set or a near-degenerate covariance."""
    rng = np.random.default_rng(12)
    n, k = 30000, 30
    pts = rng.random((n, 3), dtype=np.float32)
    pts[:, 2] = 0.2 * np.sin(3 * pts[:, 0]) + 0.0005 * rng.standard_normal(n).astype(np.float32)
    got = eng.estimate_normals_knn(cuda(pts), k).cpu().numpy()
    ref = orc.estimate_normals_knn(pts, k)
    eng.set_target(pts)
    found, idx, d2 = eng.search_knn(pts, k)
    _, oi, od = orc.search_knn(pts, pts, k)
    assert found == n * k and np.array_equal(d2, od)                       # distances bit for bit
    sets_equal = (np.sort(idx, 1) == np.sort(oi, 1)).all(1)
    assert sets_equal.mean() > 0.999                                        # (ties at the k-th distance only)
    P = pts[idx].astype(np.float64)
    C = np.einsum("nki,nkj->nij", P, P) / k - np.einsum("ni,nj->nij", P.mean(1), P.mean(1))
    w, v = np.linalg.eigh(C)
    n64 = v[:, :, 0]
    sep = (w[:, 1] - w[:, 0]) / np.maximum(w[:, 2], 1e-300)                # separation of the smallest eigenvalue
    well = sep > 0.02
    assert well.mean() > 0.9
    dg, dr = np.abs((got * n64).sum(1)), np.abs((ref * n64).sum(1))
    assert (dg[well & sets_equal] > 1 - 1e-4).all() and (dr[well & sets_equal] > 1 - 1e-4).all()
    bad = np.abs((got * ref).sum(1)) < 1 - 1e-4
    assert not (bad & well & sets_equal).any(), int((bad & well & sets_equal).sum())
    # up to NUM_MAX_NN = 100 neighbours (the big candidate lists): same statement of agreement
    for kk in (64, 100):
        g2 = eng.estimate_normals_knn(cuda(pts), kk).cpu().numpy()
        r2 = orc.estimate_normals_knn(pts, kk)
        dots = np.abs((g2 * r2).sum(1))
        assert (dots > 1 - 1e-4).mean() > 0.995 and np.median(1 - dots) < 1e-6
