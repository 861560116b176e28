"""GPU: the ICP reduction (csrc/reduce.h, launched by launch_reduce in csrc/mi_icp.hip) against integer arithmetic, bit
for bit, at every grid regime (tests/reduce_exact.py builds the clouds and lists the sizes; tests/test_reduce_exact_cpu.py
holds the construction, so a failure here can only mean the kernel).

Every term the kernels add on these clouds is exactly representable and every sum fits 53 bits, so the fp64 sums are
exact in ANY order and compute_system must return the reference's words.  No tolerance: one dropped, duplicated or
leaked element changes word [29] by one and the others by a non-zero row.

  1. point-to-plane, point-to-point, symmetric: the search returns exactly the constructed matches and misses,
     compute_system(est, T)[:30] equals the reference, compute_rmse(est, T) equals the float32 predicted from the exact
     MODE 1 sum -- at every size and under both transforms (identity; a quarter turn about z with a dyadic translation).
     Point-to-plane takes reduce_pt2pl_kernel here: that is decided by pt2pl_reduction() from state the test sets up
     itself and checks -- a target staged WITH normals (its 24-byte records exist), a search that has just run on these
     clouds (last_search_kind() >= 0), no explicit pairs since the clouds were staged.  Every other estimator, every
     MODE 1 sum and every explicit-pairs call takes reduce_kernel.
  2. colored ICP: at lambda_geometric = 1 the photometric row is multiplied by 0 and the geometric row is the
     point-to-plane row, so [0..29] are the point-to-plane reference bit for bit (the engine's gradients on the lattice
     are finite: asserted); at the default 0.968 [0..27] agree with the oracle on the constructed pairs to the 1e-9 of
     tests/test_gpu_colored.py and [28], [29] are exact.
  3. GICP on dyadic diagonal covariances (Cs = Ct, entries 0.5, 1, 2): (Ct + Cs)^-1 is a dyadic diagonal, gicp_weight
     returns it unchanged (held on the host in the CPU file), and all 30 words are exact; [0..27] also agree with the
     oracle to the existing 2e-5 (sizes up to 1,048,577: at 4,194,305 the oracle's eigen-solver would take longer than
     the rest of the test, and the exact words say more).  At 4,194,305 GICP runs under the quarter turn only (its
     covariances alone are a 150-MB upload per case).
  4. explicit pairs (set_correspondences; reduce_kernel's a.pairs path): 65,537 and 1,048,577 pairs over a 20,000-point
     source, sources repeating, one pair in 16 with an index out of range on either side (the kernel skips those).
  5. one engine serves 4,194,305, then 257, 1,048,577, 129 and 4,194,305 again, point-to-plane: every answer exact
     (stale rows of `partial`, the ticket's reset, a 1024-row buffer read by a smaller grid).
  6. the loop's own sums: icp_begin reports the constructed count, the float32 fitness and inlier_rmse of the exact
     sums, bit for bit; after icp_iterate(1) the transform is solve(reference sums) * T -- the host solver
     (mi_icp_solve_system; oracle.kabsch_from_sums for point-to-point), composed in float32 the way loop.h composes.
     The sizes sit on both sides of the one-launch iteration's limits (170,000 point-to-plane, 135,000 point-to-point);
     the evaluation after the step is that kernel's below the limit and search + reduction above, and its count and
     fitness must be the constructed ones again (the step moves the source by a small fraction of the 1/64 that
     separates the matches from the radius).
     The device composes dT * T in float32 and its wave solver is only known to equal the serial one, so the
     difference to the host's result is measured, not derived: ONE_STEP_MEASURED below, bound 8 x that.

Which size catches which fault (reasoned from the kernel source):
  - reduce_pt2pl_kernel without the `have[u]` mask: lanes past the end add element 0's row and unmatched lanes add
    slot 0's -- every point-to-plane size, from n = 1 (three of the four in-flight elements are past the end) on;
    [29] becomes a multiple of the lanes run.
  - reduce_kernel's loop with `k + stride < a.count` for `k < a.count`: every thread drops its last trip -- every size
    for point-to-point, symmetric, colored and GICP, and every MODE 1 sum (n = 1 already returns zeros); what only a
    second trip can show, a prefetched element used, starts at 65,537.
  - the finishing block's partial round started at `b + kParts`: the eight rows of the round's first slot are skipped --
    every grid that is not a multiple of 128 rows, from n = 1 (one row, skipped: zeros) through 257 points (2 rows),
    32,512 (127), 32,769 (129), 1,048,577 (257) to 2,097,153 (513); 32,768, 65,536 and 4,194,304 (128, 256 and 1024
    rows: full rounds only) pass, which tells this fault from the two above.
"""
import functools

import numpy as np
import pytest

import reduce_exact as rx
from oracle import oracle as orc
from reduce_exact import COLORED, GICP, P2P, PT2PL, SYM

pytestmark = pytest.mark.gpu

# the largest |T - solve(reference sums) * T| (Frobenius) over every case of test 6, MI355X, 2026-10-17
ONE_STEP_MEASURED = 0.0
ONE_STEP_BOUND = 8 * ONE_STEP_MEASURED

SMALL = [n for n in rx.SIZES if n <= 1048577]
EVERY = [pytest.param(n, t, id="%d-%s" % (n, t)) for n in rx.SIZES + rx.BIG_SIZES for t in rx.TRANSFORMS]
SMALL_T = [pytest.param(n, t, id="%d-%s" % (n, t)) for n in SMALL for t in rx.TRANSFORMS]
LOOP_SIZES = {PT2PL: [257, 65537, 170000, 170001, 262145, 1048577],
              P2P: [257, 65537, 135000, 135001, 170000, 170001, 262145, 1048577]}


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@functools.lru_cache(maxsize=64)
def ref(n, est):
    return rx.reference(n, est)


def same_words(got, want, what):
    bad = np.flatnonzero(got[:len(want)] != want)
    assert not len(bad), "%s: words %s differ: got %s, exact %s" % (what, bad.tolist(), got[bad].tolist(), want[bad].tolist())


def stage(e, n, tname, covs=False):
    """the clouds of case n under transform tname, the way test_compute_system_matches_oracle stages its own: the target
    with normals (so its records exist), the source with normals; then the search, which must return the construction"""
    tg, st, c = rx.target(), rx.stored(n, tname), rx.case(n)
    e.set_target(tg["pts"], tg["nrm"], tg["cov"] if covs else None)
    e.set_source(st["pts"], st["nrm"], st["cov"] if covs else None)
    return tg, st, c


def search(e, n, tname):
    c = rx.case(n)
    idx, d2, stats = e.search_radius_1nn(rx.MAX_DIST, rx.TRANSFORMS[tname])
    assert e.last_search_kind() >= 0                                        # nearest-neighbour state is valid from here
    assert np.array_equal(idx, c["nn"]), "the search does not return the constructed matches"
    assert np.array_equal(d2, c["d2"])
    assert stats[0] == c["count"] and stats[1] == ref(n, P2P)[28] and stats[2] == n, stats


# --------------------------------------------------------------------------- 1
@pytest.mark.parametrize("n,tname", EVERY)
def test_exact_systems_and_rmse(eng, n, tname):
    T = rx.TRANSFORMS[tname]
    stage(eng, n, tname)
    search(eng, n, tname)
    for est in (PT2PL, P2P, SYM):
        what = "%s n=%d %s" % (rx.EST_NAMES[est], n, tname)
        same_words(eng.compute_system(est, T), ref(n, est), what)
        got, want = eng.compute_rmse(est, T), rx.reference_rmse(n, est)
        assert got == want, "%s: rmse %r, predicted %r" % (what, got, want)
    same_words(eng.compute_system(PT2PL, T), ref(n, PT2PL), "point-to-plane again (ticket re-armed)")


# --------------------------------------------------------------------------- 2
@pytest.mark.parametrize("n,tname", SMALL_T)
def test_colored_geometric_row_is_exact_and_the_default_matches_the_oracle(eng, n, tname):
    T = rx.TRANSFORMS[tname]
    tg, st, c = stage(eng, n, tname)
    eng.set_target_colors(tg["colors"])
    eng.set_source_colors(c["colors"])
    grad = eng.compute_color_gradients(rx.GRADIENT_RADIUS, 30)
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0, "the lattice's colour gradients must be finite"
    search(eng, n, tname)
    try:
        eng.set_lambda_geometric(1.0)
        what = "colored lambda=1 n=%d %s" % (n, tname)
        same_words(eng.compute_system(COLORED, T), ref(n, PT2PL), what)
        got, want = eng.compute_rmse(COLORED, T), rx.reference_rmse(n, COLORED)
        assert got == want, "%s: error sum %r, predicted %r" % (what, got, want)
    finally:
        eng.set_lambda_geometric(0.968)
    got = eng.compute_system(COLORED, T)
    o = rx.oracle_inputs(n)
    orc.set_colored_context(c["colors"], tg["colors"], grad, 0.968)
    want = orc.compute_system(COLORED, o["src"], o["tgt"], o["cor"], tgt_nrm=o["tgt_nrm"])
    scale = np.abs(want[:27]).max()
    assert np.abs(got[:28] - want[:28]).max() <= 1e-9 * max(scale, 1.0), np.abs(got[:28] - want[:28]).max()
    same_words(got[28:30], ref(n, PT2PL)[28:30], "colored n=%d %s statistics" % (n, tname))


# --------------------------------------------------------------------------- 3
GICP_CASES = SMALL_T + [pytest.param(rx.BIG_SIZES[-1], "rot90z", id="%d-rot90z" % rx.BIG_SIZES[-1])]


@pytest.mark.parametrize("n,tname", GICP_CASES)
def test_gicp_on_dyadic_covariances_is_exact(eng, n, tname):
    T = rx.TRANSFORMS[tname]
    stage(eng, n, tname, covs=True)
    search(eng, n, tname)
    got = eng.compute_system(GICP, T)
    want = ref(n, GICP)
    same_words(got[28:30], want[28:30], "gicp n=%d %s statistics" % (n, tname))
    if n <= 1048577:
        o = rx.oracle_inputs(n)
        args = (o["src"], o["tgt"], o["cor"], o["src_nrm"], o["tgt_nrm"], o["src_cov"], o["tgt_cov"])
        sys_o = orc.compute_system(GICP, *args)
        np.testing.assert_allclose(got[:28], sys_o[:28], rtol=2e-5, atol=2e-5 * np.abs(sys_o).max())
        if n <= 65537:
            assert eng.compute_rmse(GICP, T) == pytest.approx(orc.compute_rmse(GICP, *args), rel=1e-5)
    same_words(got, want, "gicp n=%d %s" % (n, tname))


# --------------------------------------------------------------------------- 4
@pytest.mark.parametrize("m", [65537, 1048577])
@pytest.mark.parametrize("tname", list(rx.TRANSFORMS))
def test_explicit_pairs_are_exact(eng, tname, m):
    n = 20000
    T = rx.TRANSFORMS[tname]
    tg, st, c = stage(eng, n, tname)
    rng = np.random.default_rng(m)
    src = rng.choice(np.flatnonzero(~c["miss"]), m)                         # sources repeat
    pairs = np.stack([src, c["tix"][src]], 1).astype(np.int32)
    k = np.arange(m)
    out = k % 16 == 5                                                       # one pair in 16 is out of range: skipped
    pairs[out & (k % 64 == 5), 0] = -1
    pairs[out & (k % 64 == 21), 1] = -1
    pairs[out & (k % 64 == 37), 0] = n
    pairs[out & (k % 64 == 53), 1] = rx.NT
    out[-1] = False                                                         # (the last pair is a real one)
    pairs[-1] = [src[-1], c["tix"][src[-1]]]
    rows = rx.rows_for(n, src[~out])
    eng.set_correspondences(pairs)
    for est in (PT2PL, P2P, SYM):
        what = "%s %d pairs %s" % (rx.EST_NAMES[est], m, tname)
        same_words(eng.compute_system(est, T), rx.reference(n, est, rows), what)
        got, want = eng.compute_rmse(est, T), rx.reference_rmse(n, est, rows)
        assert got == want, "%s: rmse %r, predicted %r" % (what, got, want)


# --------------------------------------------------------------------------- 5
def test_one_engine_across_sizes_stays_exact():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    try:
        for n in (rx.BIG_SIZES[-1], 257, 1048577, 129, rx.BIG_SIZES[-1]):
            stage(e, n, "rot90z")
            search(e, n, "rot90z")
            same_words(e.compute_system(PT2PL, rx.T_ROT90Z), ref(n, PT2PL), "pt2pl n=%d on a reused engine" % n)
    finally:
        e.close()


# --------------------------------------------------------------------------- 6
def compose(dT, T):
    """loop.h: sum = (((0 + u_r0 B_0c) + u_r1 B_1c) + u_r2 B_2c) + u_r3 B_3c in float32, no contraction"""
    out = np.zeros((4, 4), np.float32)
    for k in range(4):
        out = out + np.outer(dT[:, k], T[k, :]).astype(np.float32)
    return out


@pytest.mark.parametrize("est,n", [pytest.param(est, n, id="%s-%d" % (rx.EST_NAMES[est], n))
                                   for est in (PT2PL, P2P) for n in LOOP_SIZES[est]])
def test_the_loops_own_sums_and_first_step(eng, est, n):
    from cupoch_amd import engine as engine_mod
    c = rx.case(n)
    count, fitness, rmse = rx.reference_stats(n)
    sys32 = np.zeros(32, np.float64)
    sys32[:30] = ref(n, est)
    if est == P2P:
        dT = orc.kabsch_from_sums(sys32, n)
    else:
        ok, dT = engine_mod.solve_system(sys32, -1.0)
        assert ok
    for tname, T in rx.TRANSFORMS.items():
        stage(eng, n, tname)
        res = eng.icp_begin(est, rx.MAX_DIST, T, -1.0)
        what = "%s n=%d %s" % (rx.EST_NAMES[est], n, tname)
        assert res.n_correspondences == count, what
        assert float(res.fitness) == fitness and float(res.inlier_rmse) == rmse, \
            "%s: fitness %r (%r), rmse %r (%r)" % (what, res.fitness, fitness, res.inlier_rmse, rmse)
        res = eng.icp_iterate(1)
        T1 = np.array(res.transformation, np.float32).reshape(4, 4).T
        err = float(np.linalg.norm(T1.astype(np.float64) - compose(dT, T).astype(np.float64)))
        print("one step %s: |T - solve(reference sums) T| = %.3e" % (what, err))
        assert err <= ONE_STEP_BOUND, "%s: %.3e (1e-5 or more is a wrong sum, not rounding)" % (what, err)
        # the evaluation behind the step (below the limits: the one-launch iteration's own sums)
        assert res.n_correspondences == count and float(res.fitness) == fitness, what
