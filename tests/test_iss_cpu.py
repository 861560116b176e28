"""The CPU restatement of ComputeISSKeypoints (tests/iss_exact.py) against properties that need no GPU: the deviation
table of DESIGN.md (raw against centred coordinates, fp64 against fp32), invariance of the centred detector under a
translation of the cloud, the scaled-eigenvalue quirk of FastEigen3x3Val, and its eigenvalues against LAPACK."""
import os

import numpy as np

import iss_exact as ix

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fragment():
    return np.load(os.path.join(GOLDEN, "fragment_every3rd.npz"))["points"].astype(F32)


def test_the_deviation_table_of_the_design_document():
    pts = _fragment()
    res, rs, rn = ix.resolution(pts)
    assert abs(float(res) - 0.00807) < 1e-5 and abs(float(rs) - 0.0484) < 1e-4 and abs(float(rn) - 0.0323) < 1e-4
    raw64 = ix.iss(pts, dtype=np.float64, centred=False)      # the reference's formula, exact enough
    cen64 = ix.iss(pts, dtype=np.float64, centred=True)
    raw32 = ix.iss(pts, dtype=F32, centred=False)             # the reference's arithmetic
    cen32 = ix.iss(pts, dtype=F32, centred=True)              # the engine's contract
    assert [int(r["mask"].sum()) for r in (raw64, cen64, raw32, cen32)] == [786, 766, 1141, 763]
    assert [int((r["mask"] != raw64["mask"]).sum()) for r in (cen64, raw32, cen32)] == [20, 1315, 23]
    # fp32 on raw coordinates: the cancellation error is of the order of the smallest eigenvalue
    both = (raw32["eig"] != -1).any(1) & (raw64["eig"] != -1).any(1)
    ratio = raw32["eig"][both, 0].astype(np.float64) / raw64["eig"][both, 0]
    assert np.nanmax(np.abs(ratio)) > 100.0
    # centred: fp32 stays within 1e-5 of fp64 on eigenvalues of order 1, and differs only where a rounding may decide
    dev = np.abs(cen32["eig"][both].astype(np.float64) - cen64["eig"][both]).max()
    assert dev < 2e-5, dev
    und = ix.undecided(cen64)
    assert 0.03 < und.mean() <= 0.10
    assert not ((cen32["mask"] != cen64["mask"]) & ~und).any()
    assert ix.undecided(cen64, ratio_tol=1e-3, tie_tol=1e-3).mean() > 0.10      # (a wider band would be no test)


def test_the_centred_detector_does_not_depend_on_the_origin():
    """the cloud moved by (100, 100, 100) -- exactly, in fp64 -- over the rows of the cloud where it was"""
    pts = _fragment()
    a = ix.iss(pts, dtype=np.float64, centred=True)
    moved = pts.astype(np.float64) + 100.0
    assert np.array_equal(moved - 100.0, pts.astype(np.float64))
    pad, cnt = ix.padded(*a["salient_rows"], 100)

    def mask_of(cloud, dtype, centred):
        eig = ix.eig_of_rows(cloud, pad, cnt, 5, dtype, centred)
        return ix.suppress(ix.gates(eig, cnt, 5, 0.975, 0.975), *a["non_max_rows"])
    und = ix.undecided(a)
    assert not ((mask_of(moved, np.float64, True) != a["mask"]) & ~und).any()
    # in fp32 the moved coordinates are another cloud (6 bits fewer); its centred form still finds a comparable set,
    # the raw form -- the reference's arithmetic -- is noise at that distance from the origin
    cen32, raw32 = mask_of(moved, F32, True), mask_of(moved, F32, False)
    assert 0.5 * a["mask"].sum() < cen32.sum() < 2.0 * a["mask"].sum()
    assert (raw32 != a["mask"]).sum() > 10 * (cen32 != a["mask"]).sum()


def test_general_branch_is_scaled_diagonal_branch_is_not():
    for dt in (F32, np.float64):
        D = np.diag([4.0, 1.0, 2.0]).astype(dt)[None]
        assert np.array_equal(ix.eigenvalues(D)[0], np.array([1, 2, 4], dt))            # C's own diagonal, sorted
        G = D.copy()
        G[0, 0, 1] = G[0, 1, 0] = 0.5
        want = np.linalg.eigvalsh(G[0].astype(np.float64)) / 4.0                         # of C / C.max(): not scaled back
        np.testing.assert_allclose(ix.eigenvalues(G)[0], want, rtol=0, atol=2e-6 if dt is F32 else 1e-14)
        # the largest entry may sit off the diagonal
        H = np.array([[1.0, 3.0, 0.0], [3.0, 1.0, 0.0], [0.0, 0.0, 2.0]], dt)[None]
        np.testing.assert_allclose(ix.eigenvalues(H)[0], np.linalg.eigvalsh(H[0].astype(np.float64)) / 3.0, rtol=0,
                                   atol=2e-6 if dt is F32 else 1e-14)
        Z = np.zeros((1, 3, 3), dt)
        Z[0, 0, 0] = -1.0                                                                # C.max() == 0
        assert np.array_equal(ix.eigenvalues(Z)[0], np.zeros(3, dt))
    assert ix.is_zero(np.full((1, 3, 3), 1e-5, F32))[0] and not ix.is_zero(np.full((1, 3, 3), 1.1e-5, F32))[0]


def test_eigenvalues_against_lapack():
    rng = np.random.default_rng(4)
    q = rng.standard_normal((5000, 40, 3)) * rng.uniform(0.01, 1.0, (5000, 1, 3))
    q -= q.mean(1, keepdims=True)
    C = np.einsum("nki,nkj->nij", q, q) / 40.0
    want = np.linalg.eigvalsh(C) / C.reshape(len(C), 9).max(1)[:, None]
    # The closed form takes acos of det(B) / 2: a rounding error d of some 10 eps in that argument becomes an angle
    # error of up to sqrt(2 d) where the argument is +-1 (two equal eigenvalues), a third of it after the division, and
    # 2 p sin(2 pi / 3) times that in the two eigenvalues off the extreme one: 1.7 p sqrt(20 eps) / 3 with p <= 0.6
    # for a matrix whose largest entry is 1.  That is 4e-4 in fp32 and 2e-8 in fp64.
    np.testing.assert_allclose(ix.eigenvalues(C), want, rtol=0, atol=2e-8)
    np.testing.assert_allclose(ix.eigenvalues(C.astype(F32)), want, rtol=0, atol=4e-4)


def test_gates_and_suppression_on_a_hand_built_case():
    eig = np.array([[0.1, 0.5, 1.0], [0.49, 0.5, 1.0], [0.1, 0.99, 1.0], [0.0, 0.0, 1.0], [-1e-8, 0.5, 1.0],
                    [-1, -1, -1], [0.1, 0.5, 1.0], [0.2, 0.5, 1.0]], F32)
    cnt = np.array([9, 9, 9, 9, 9, 9, 4, 9], np.int32)
    sal = ix.gates(eig, cnt, 5, 0.975, 0.975)
    assert sal.dtype == F32
    assert np.array_equal(sal, np.array([0.1, -1, -1, -1, -1e-8, -1, -1, 0.2], F32))
    # rows: 0 sees 7 (beaten), 7 sees 0, 4 alone (negative: never a keypoint), two tied points both stay
    sal = np.array([0.1, 0.2, 0.2, -1e-8, 0.0], F32)
    indptr = np.array([0, 2, 4, 6, 7, 8])
    idx = np.array([0, 1, 1, 2, 2, 1, 3, 4])
    assert ix.suppress(sal, indptr, idx).tolist() == [False, True, True, False, True]
