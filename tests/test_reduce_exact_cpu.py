"""The construction of tests/reduce_exact.py, held on the CPU so that a failure of tests/test_gpu_reduce_exact.py can
only mean the kernel: the constructed matches are the nearest neighbours and unique, every per-row term is exact in
float32 at the largest size, the integer references are what the oracle computes, and an eighth of the source misses."""
import numpy as np
import pytest

import reduce_exact as rx
from oracle import oracle as orc

LARGEST = rx.BIG_SIZES[-1]


def transformed(n, tname):
    T = rx.TRANSFORMS[tname].astype(np.float64)
    return rx.stored(n, tname)["pts"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]


@pytest.mark.parametrize("tname", list(rx.TRANSFORMS))
@pytest.mark.parametrize("n", [257, 65537])
def test_the_constructed_matches_are_the_unique_nearest_neighbours(n, tname):
    c, tgt = rx.case(n), rx.target()["pts"].astype(np.float64)
    src = transformed(n, tname)
    hit = ~c["miss"]
    assert np.array_equal(src[hit] * rx.Q, c["q_i"][hit])                   # the transformed frame is the same for both
    t2 = (tgt * tgt).sum(1)
    for lo in range(0, n, 4096):
        s = src[lo:lo + 4096]
        # |s|^2 - 2 s.t + |t|^2, exact in fp64: coordinates are multiples of 2^-8 below 8
        d2 = (s * s).sum(1)[:, None] - 2.0 * (s @ tgt.T) + t2[None, :]
        order = np.argmin(d2, axis=1)[:, None]
        first = np.take_along_axis(d2, order, 1)[:, 0]
        np.put_along_axis(d2, order, np.inf, 1)
        second = d2.min(1)
        near = first < rx.MAX_DIST ** 2                                     # the engine's strict rule
        want = c["nn"][lo:lo + 4096]
        assert np.array_equal(near, want >= 0)
        assert np.array_equal(order[near, 0], want[near])
        assert (second[near] > first[near]).all()                           # no second target at the same distance
        assert np.array_equal(first[near].astype(np.float32), c["d2"][lo:lo + 4096][near])
        assert (first[~near] >= 4.0 ** 2).all()                             # a miss is nowhere near the radius


@pytest.mark.parametrize("tname", list(rx.TRANSFORMS))
@pytest.mark.parametrize("est", [rx.P2P, rx.PT2PL, rx.SYM, rx.COLORED, rx.GICP], ids=lambda e: rx.EST_NAMES[e])
def test_every_term_is_exact_in_float32_at_the_largest_size(est, tname):
    rx.self_check(LARGEST, tname, est, rx.eigen3_host)


def test_gicp_weight_returns_a_dyadic_diagonal_matrix_unchanged():
    """what makes GICP's words exact: eigen3.h gicp_weight, on the host, takes a diagonal (Ct + Cs)^-1 as it is"""
    A = np.zeros((27, 3, 3), np.float32)
    vals = np.array([1.0, 0.5, 0.25], np.float32)
    for k in range(27):
        A[k, 0, 0], A[k, 1, 1], A[k, 2, 2] = vals[k // 9], vals[k // 3 % 3], vals[k % 3]
    assert np.array_equal(rx.eigen3_host(A), A)


def test_the_integer_references_are_the_oracles():
    n = 65537
    o = rx.oracle_inputs(n)
    args = (o["src"], o["tgt"], o["cor"], o["src_nrm"], o["tgt_nrm"], o["src_cov"], o["tgt_cov"])
    assert len(o["cor"]) == rx.case(n)["count"]
    for est in (rx.P2P, rx.PT2PL, rx.SYM):
        ref, got = rx.reference(n, est), orc.compute_system(est, *args)[:30]
        np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max(), err_msg=rx.EST_NAMES[est])
        assert orc.compute_rmse(est, *args) == pytest.approx(rx.reference_rmse(n, est), rel=1e-6)   # (a float32)
        got_sum = orc.compute_rmse(est, *args) ** 2 * len(o["cor"])
        assert got_sum == pytest.approx(rx.reference_error_sum(n, est), rel=1e-6)
    # GICP: the oracle takes W = sqrt((Ct + Cs)^-1) through the eigen-solver and multiplies it out again (1e-7 in
    # float32 per entry); the statistics do not go through the weights
    ref, got = rx.reference(n, rx.GICP), orc.compute_system(rx.GICP, *args)[:30]
    np.testing.assert_allclose(got, ref, rtol=2e-5, atol=2e-5 * np.abs(ref).max())
    np.testing.assert_allclose(got[28:30], ref[28:30], rtol=1e-12)
    # colored ICP at lambda_geometric = 1: the geometric row alone, whatever the gradients
    tg, c = rx.target(), rx.case(n)
    grad = orc.color_gradients(tg["pts"], tg["nrm"], tg["colors"], rx.GRADIENT_RADIUS, 30)
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0
    orc.set_colored_context(c["colors"], tg["colors"], grad, 1.0)
    got = orc.compute_system(rx.COLORED, o["src"], o["tgt"], o["cor"], tgt_nrm=o["tgt_nrm"])[:30]
    ref = rx.reference(n, rx.COLORED)
    np.testing.assert_allclose(got, ref, rtol=1e-12, atol=1e-12 * np.abs(ref).max())
    assert np.array_equal(ref, rx.reference(n, rx.PT2PL))


@pytest.mark.parametrize("n", rx.SIZES + rx.BIG_SIZES)
def test_an_eighth_of_the_source_misses(n):
    """outside 5 % .. 25 % a case would not exercise the masking; below 255 points a share says nothing (n = 1 has its
    one point matched by construction), there the ends are checked alone"""
    c = rx.case(n)
    assert not c["miss"][c["ends"]].any() and c["count"] == n - int(c["miss"].sum())
    assert c["off_i"].any(1).all() and np.abs(c["off_i"]).max() <= 7
    if n >= 255:
        assert 0.05 <= c["miss"].mean() <= 0.25, c["miss"].mean()
    st = rx.stored(n, "rot90z")["p_i"]
    if c["miss"].any():                                                     # every miss lies beyond every matched point
        assert st[c["miss"]].max(1).min() >= 3 * rx.Q and np.abs(st[~c["miss"]]).max() < 2 * rx.Q


def test_the_grid_formula_puts_the_sizes_where_the_table_says():
    g = rx.grid_of
    assert [g(n) for n in (1, 256, 257, 32512, 32768, 32769, 65536, 65537)] == [1, 1, 2, 127, 128, 129, 256, 256]
    assert [g(n) for n in (1048576, 1048577, 2097153, 4194303, 4194304, 4194305)] == [256, 257, 513, 1024, 1024, 1024]
    assert g(2097153, True) == 512 and g(4194305, True) == 512 and g(262145, True) == 256
