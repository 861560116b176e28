"""GPU: feature matching, the reciprocal pairs and tuple list, one optimiser step and the whole FastGlobalRegistration
call through the C ABI, against the numpy restatement (tests/fgr_exact.py).  tests/test_fgr_cpu.py asserts, without a
GPU, that no scene used here has a row whose two best distances the fp32 chain could order either way; so an index
must equal the fp64 neighbour exactly."""
import ctypes as C

import numpy as np
import pytest

import fgr_exact as fx

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -24


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def scenes():
    """name -> (scene, option, fp64 restatement, fp32-step restatement), computed once"""
    out = {}
    for name, (sc, opt) in fx.fgr_scenes().items():
        out[name] = (sc, opt, fx.fgr(sc["src"], sc["tgt"], sc["sfeat"], sc["tfeat"], opt, 0, fp32=False),
                     fx.fgr(sc["src"], sc["tgt"], sc["sfeat"], sc["tfeat"], opt, 0, fp32=True))
    return out


def _host(*ts):
    return [t.cpu().numpy() for t in ts]


def _check_match(eng, Q, R, sample):
    dim = Q.shape[1]
    qi, qd, ri, rd = _host(*eng.feature_match(Q, R))
    D = fx.dist64(Q, R)
    rng = np.random.default_rng(len(Q) * 7 + len(R))
    for idx, d, M, A, B in ((qi, qd, D, Q, R), (ri, rd, D.T, R, Q)):
        want = fx.neighbours(M)
        assert np.array_equal(idx, want)               # (np.argmin: the smallest index among equals)
        best = M[np.arange(len(M)), want]
        assert (np.abs(d.astype(np.float64) - best) <= (dim + 2) * U * best).all()
        for i in rng.choice(len(A), min(sample, len(A)), replace=False):
            assert d[i].tobytes() == fx.chain_exact(A[i], B[idx[i]]).tobytes(), (i, d[i])
    # both directions of the call are consistent: what one list calls a reciprocal pair, the other does too
    recip = [(i, j) for i, j in enumerate(qi) if ri[j] == i]
    for i, j in recip:
        assert qd[i].tobytes() == rd[j].tobytes()
    return qi, ri


@pytest.mark.parametrize("nq,nr,dim", fx.match_cases(), ids=lambda v: str(v))
def test_match_equals_fp64_neighbours(eng, nq, nr, dim):
    Q, R = fx.match_case(nq, nr, dim)
    _check_match(eng, Q, R, 32 if max(nq, nr) >= 257 else 4)      # (64 pairs of every large case, 8 of the others)


def test_match_duplicated_rows_take_the_smallest_index(eng):
    Q, R = fx.duplicate_case()
    qi, ri = _check_match(eng, Q, R, 32)
    D = fx.dist64(Q, R)
    assert (np.sort(D, axis=1)[:, 0] == np.sort(D, axis=1)[:, 1]).sum() >= 20      # (ties there are)
    assert (D[np.arange(len(Q)), qi] == 0).sum() >= 40


def test_match_nan_never_wins(eng):
    Q, R = fx.match_case(65, 129, 33)
    Q, R = Q.copy(), R.copy()
    Q[7] = np.nan                       # a row of NaNs: no neighbour
    Q[9, 3] = np.nan                    # one NaN poisons the row's every distance
    R[11, 0] = np.nan                   # a column that can never win
    qi, qd, ri, rd = _host(*eng.feature_match(Q, R))
    assert qi[7] == -1 and qi[9] == -1 and np.isnan(qd[7]) and np.isnan(qd[9])
    assert ri[11] == -1 and np.isnan(rd[11]) and not (qi == 11).any()
    D = fx.dist64(Q, R)
    keep = np.ones(65, bool)
    keep[[7, 9]] = False
    assert np.array_equal(qi[keep], fx.neighbours(D)[keep])
    assert np.array_equal(ri, fx.neighbours(D.T))
    R[:] = np.nan
    qi, qd, ri, rd = _host(*eng.feature_match(Q, R))
    assert (qi == -1).all() and (ri == -1).all() and np.isnan(qd).all()
    Q[:] = np.inf                       # inf - finite = inf: a distance like any other, the smallest index wins
    R = fx.match_case(65, 129, 33)[1]
    qi, qd, ri, rd = _host(*eng.feature_match(Q, R))
    assert (qi == 0).all() and np.isinf(qd).all() and (ri == 0).all()


def test_invalid_arguments_are_refused_before_any_launch(eng):
    from cupoch_amd import MiIcpError
    L, ctx = eng._L, eng._ctx
    Q, R = fx.match_case(8, 8, 33)
    import torch
    q, r = torch.from_numpy(Q).cuda(), torch.from_numpy(R).cuda()
    out = torch.zeros(64, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    for nq, nr, dim, qq, rr in ((8, 8, 0, q, r), (8, 8, 513, q, r), (0, 8, 33, q, r), (8, 0, 33, q, r), (8, 2 ** 31, 33, q, r),
                                (-1, 8, 33, q, r)):
        assert L.mi_icp_feature_match(ctx, p(qq), nq, p(rr), nr, dim, p(out), None, None, None) == -1
    assert L.mi_icp_feature_match(ctx, None, 8, p(r), 8, 33, p(out), None, None, None) == -1
    assert L.mi_icp_feature_match(ctx, p(q), 8, None, 8, 33, p(out), None, None, None) == -1
    assert (out == 0).all()
    with pytest.raises(MiIcpError) as e:
        eng.feature_match(np.zeros((0, 33), F), R)
    assert e.value.code == -1
    opt = eng.fgr_option()
    from cupoch_amd._lib import Result
    rs = Result()
    pts = torch.zeros((8, 3), device="cuda")
    for args in ((None, p(q), 8, p(pts), p(r), 8, 33), (p(pts), None, 8, p(pts), p(r), 8, 33), (p(pts), p(q), 0, p(pts), p(r), 8, 33),
                 (p(pts), p(q), 8, p(pts), p(r), 8, 600), (p(pts), p(q), 8, p(pts), None, 8, 33)):
        assert L.mi_icp_fast_global_registration(ctx, *args, C.byref(opt), 0, C.byref(rs)) == -1
    assert L.mi_icp_fast_global_registration(ctx, p(pts), p(q), 8, p(pts), p(r), 8, 33, None, 0, C.byref(rs)) == -1
    n = C.c_int64(5)
    assert L.mi_icp_correspondences_from_features(ctx, p(q), 8, p(r), 8, 0, 0, 0.1, p(out), C.byref(n)) == -1 and n.value == 0
    assert L.mi_icp_fgr_optimize(ctx, p(pts), 8, p(pts), 8, None, 12, 1.0, C.byref(opt), p(pts), None, None) == -1
    assert L.mi_icp_fgr_correspondences(ctx, None, 8, p(out), 8, p(pts), p(pts), 0.95, 10, 0, p(out), C.byref(n), p(out), C.byref(n)) == -1


# ---- pairs and tuples ---------------------------------------------------------------------------------------------------
def test_pairs_and_tuples_equal_the_restatement(eng, scenes):
    for name, (sc, opt, r64, _) in scenes.items():
        qi, _, ri, _ = _host(*eng.feature_match(sc["sfeat"], sc["tfeat"]))
        pairs, corr = _host(*eng.fgr_correspondences(qi, ri, sc["src"], sc["tgt"], opt.tuple_scale, opt.maximum_tuple_count, 0))
        want_pairs = fx.reciprocal_pairs(qi, ri)
        want_corr, passing = fx.tuples(want_pairs, sc["src"], sc["tgt"], opt.tuple_scale, opt.maximum_tuple_count, 0)
        assert np.array_equal(pairs, want_pairs) and np.array_equal(corr, want_corr), name      # ... fed the engine's lists
        assert np.array_equal(qi, r64.s_idx) and np.array_equal(ri, r64.t_idx), name
        assert np.array_equal(pairs, r64.pairs) and np.array_equal(corr, r64.corr), name          # ... and end to end
        assert len(corr) == 1000 and 3 * passing > 1000


def test_tuple_list_is_cut_at_exactly_the_count(eng, scenes):
    sc, opt, r64, _ = scenes["d33_rel"]
    for maxc in (1, 3, 10, 1000, 10 ** 6):
        pairs, corr = _host(*eng.fgr_correspondences(r64.s_idx, r64.t_idx, sc["src"], sc["tgt"], 0.95, maxc, 5))
        want, passing = fx.tuples(r64.pairs, sc["src"], sc["tgt"], 0.95, maxc, 5)
        assert len(corr) == min(maxc, 3 * passing) and np.array_equal(corr, want), maxc
    assert len(_host(*eng.fgr_correspondences(r64.s_idx, r64.t_idx, sc["src"], sc["tgt"], 0.95, 0, 5))[1]) == 0
    for ncorr in (0, 1, 9, 10):
        # neighbour lists that make exactly the first ncorr true pairs reciprocal
        s_idx = np.full(360, -1, np.int32)
        s_idx[r64.pairs[:ncorr, 0]] = r64.pairs[:ncorr, 1]
        pairs, corr = _host(*eng.fgr_correspondences(s_idx, r64.t_idx, sc["src"], sc["tgt"], 0.95, 10 ** 6, 5))
        want, passing = fx.tuples(r64.pairs[:ncorr], sc["src"], sc["tgt"], 0.95, 10 ** 6, 5)
        assert np.array_equal(pairs, r64.pairs[:ncorr]) and np.array_equal(corr, want) and len(corr) == 3 * passing, ncorr
        assert passing > 0 or ncorr <= 2


def test_seeds_and_contexts(eng, scenes):
    from cupoch_amd.engine import Engine
    sc, opt, r64, _ = scenes["d33_rel"]
    a = _host(*eng.fgr_correspondences(r64.s_idx, r64.t_idx, sc["src"], sc["tgt"], 0.95, 1000, 5))[1]
    b = _host(*eng.fgr_correspondences(r64.s_idx, r64.t_idx, sc["src"], sc["tgt"], 0.95, 1000, 6))[1]
    assert not np.array_equal(a, b)
    other = Engine(0)
    try:
        c = _host(*other.fgr_correspondences(r64.s_idx, r64.t_idx, sc["src"], sc["tgt"], 0.95, 1000, 5))[1]
        assert a.tobytes() == c.tobytes()
        r1 = eng.fast_global_registration(sc["src"], sc["tgt"], sc["sfeat"], sc["tfeat"], None, 3)
        r2 = other.fast_global_registration(sc["src"], sc["tgt"], sc["sfeat"], sc["tfeat"], None, 3)
        r3 = eng.fast_global_registration(sc["src"], sc["tgt"], sc["sfeat"], sc["tfeat"], None, 3)
        assert bytes(r1) == bytes(r2) == bytes(r3)
        assert np.array_equal(eng.get_correspondences(), other.get_correspondences())
    finally:
        other.close()


# ---- the optimiser ------------------------------------------------------------------------------------------------------
def test_one_step_sums_and_par_schedule(eng, scenes):
    """the 27 sums of one step against fp64 numpy on the same fp32 points and par.  Bound per entry c * 2^-24 * sum
    |term| with c = 16, the fp32 roundings behind one term of the kernel (feature_kernels.h counts them: the residual 1;
    its square 2, the sum of three squares 5, + par 6, the division 7, squared 15; times the residual 16); the fp64
    accumulation itself adds n * 2^-53, far below."""
    for name in ("d33_rel", "d352_abs"):
        sc, opt, r64, r32 = scenes[name]
        ns_, nt_, _, sg, _ = fx.normalize(sc["src"], sc["tgt"], opt.use_absolute_scale, fp32=True)
        one = eng.fgr_option(use_absolute_scale=opt.use_absolute_scale, iteration_number=1)
        T, sums, par = eng.fgr_optimize(ns_, nt_, r32.corr, float(sg), one)
        p, q = ns_[r32.corr[:, 0]], nt_[r32.corr[:, 1]]
        want, mags = fx.step_sums(p, q, sg, fp32=False)
        assert (np.abs(sums - want) <= 16 * U * mags + 1e-300).all(), name
        assert (mags[[3, 9, 14, 16, 17, 19]] == 0).all() and (sums[[3, 9, 14, 16, 17, 19]] == 0).all()
        tr, _, _ = fx.optimize(ns_, nt_, r32.corr, sg, opt, fp32=True, iterations=1)
        assert np.linalg.norm(T - tr) < 1e-5, name
        sched = fx.par_schedule(sg, 9, opt)
        for k in range(9):
            step = eng.fgr_option(use_absolute_scale=opt.use_absolute_scale, iteration_number=k + 1)
            assert F(eng.fgr_optimize(ns_, nt_, r32.corr, float(sg), step)[2]).tobytes() == sched[k].tobytes(), (name, k)
        # fewer than ten correspondences, or no iteration: identity, zero sums, par untouched
        T, sums, par = eng.fgr_optimize(ns_, nt_, r32.corr[:9], 0.75, one)
        assert np.array_equal(T, np.eye(4, dtype=F)) and not sums.any() and par == 0.75
        T, sums, par = eng.fgr_optimize(ns_, nt_, r32.corr, 0.75, eng.fgr_option(iteration_number=0))
        assert np.array_equal(T, np.eye(4, dtype=F)) and not sums.any() and par == 0.75


def test_whole_call_against_the_restatement_and_ground_truth(eng, scenes):
    """T against the restatement with the stated fp32 steps: the bound is 8 G, G the largest Frobenius gap over the
    scenes between that restatement and the one in fp64 throughout -- the fp64 sums of an iteration do not compound,
    the fp32 point updates do, and numpy rounds them in another order than the kernel.  Against ground truth: the fp64
    restatement's own error on the scene, plus its gap G to the fp32 one, plus the 8 G above (the triangle inequality)."""
    from cupoch_amd import registration as reg
    from cupoch_amd.geometry import PointCloud
    G = max(np.linalg.norm(r32.T.astype(np.float64) - r64.T) for _, _, r64, r32 in scenes.values())
    assert 1e-8 < G < 1e-5
    for name, (sc, opt, r64, r32) in scenes.items():
        copt = eng.fgr_option(**vars(opt))
        res = eng.fast_global_registration(sc["src"], sc["tgt"], sc["sfeat"], sc["tfeat"], copt, 0)
        T = np.array(res.transformation, F).reshape(4, 4).T
        gap, err = np.linalg.norm(T - r32.T), np.linalg.norm(T - sc["T_gt"])
        print("%s: |T - T_restated|_F = %.3g (bound %.3g), |T - T_gt|_F = %.3g, G = %.3g" % (name, gap, 8 * G, err, G))
        assert gap <= 8 * G, name
        assert err <= np.linalg.norm(r64.T - sc["T_gt"]) + 9 * G, name
        cor = eng.get_correspondences()
        src, tgt = PointCloud(sc["src"]), PointCloud(sc["tgt"])
        ev = reg.evaluate_registration(src, tgt, opt.maximum_correspondence_distance, T)
        assert res.fitness == F(ev.fitness) and res.inlier_rmse == F(ev.inlier_rmse), name
        assert np.array_equal(cor, ev.correspondence_set) and res.n_correspondences == len(cor), name
        if name != "noisy":
            assert res.n_correspondences >= 300 and res.inlier_rmse < 1e-3, name
        # the ctypes mirror: the same call, the same bytes
        fs, ft = reg.Feature(sc["sfeat"].shape[1], sc["sfeat"]), reg.Feature(sc["tfeat"].shape[1], sc["tfeat"])
        out = reg.registration_fast_based_on_feature_matching(src, tgt, fs, ft, reg.FastGlobalRegistrationOption(**vars(opt)), seed=0)
        assert out.transformation.tobytes() == T.tobytes() and out.fitness == res.fitness, name
        assert np.array_equal(out.correspondence_set, cor), name


def test_degenerate_inputs(eng, scenes):
    sc, opt, r64, _ = scenes["d33_rel"]
    means = np.array([sc["src"].astype(np.float64).mean(0), sc["tgt"].astype(np.float64).mean(0)])

    def run(src, tgt, fs, ft):
        res = eng.fast_global_registration(src, tgt, fs, ft, None, 0)
        return res, np.array(res.transformation, F).reshape(4, 4).T

    # all descriptors equal: every neighbour is index 0, one reciprocal pair, fewer than ten correspondences: the
    # optimiser returns identity, which maps back to the shift between the means
    res, T = run(sc["src"], sc["tgt"], np.ones((360, 33), F), np.ones((380, 33), F))
    assert np.array_equal(T[:3, :3], np.eye(3, dtype=F)) and np.allclose(T[:3, 3], means[1] - means[0], atol=1e-5)
    want = fx.fgr(sc["src"], sc["tgt"], None, None, nn=(np.zeros(360, np.int32), np.zeros(380, np.int32)))
    assert len(want.corr) == 0 and np.linalg.norm(T - want.T) < 1e-5
    # one point per side
    res, T = run(sc["src"][:1], sc["tgt"][:1], sc["sfeat"][:1], sc["tfeat"][:1])
    assert np.array_equal(T[:3, :3], np.eye(3, dtype=F)) and np.allclose(T[:3, 3], sc["tgt"][0] - sc["src"][0], atol=1e-6)
    assert res.fitness == 1.0 and res.n_correspondences == 1
    # two true pairs: every trial repeats one of them and fails, no correspondence, the identity again
    i = r64.pairs[:2]
    res, T = run(sc["src"][i[:, 0]], sc["tgt"][i[:, 1]], sc["sfeat"][i[:, 0]], sc["tfeat"][i[:, 1]])
    assert np.array_equal(T[:3, :3], np.eye(3, dtype=F))


def test_correspondences_from_features(eng, scenes):
    from cupoch_amd import registration as reg
    sc, opt, r64, _ = scenes["d33_rel"]
    fs, ft = reg.FeatureFPFH(data=sc["sfeat"]), reg.FeatureFPFH(data=sc["tfeat"])
    rows = np.stack([np.arange(360, dtype=np.int32), r64.s_idx], 1)
    assert np.array_equal(reg.correspondences_from_features(fs, ft), rows)
    assert np.array_equal(reg.correspondences_from_features(fs, ft, True), r64.pairs)
    assert np.array_equal(reg.correspondences_from_features(fs, ft, True, 0.9), rows)        # too few remain: unfiltered
    assert len(reg.correspondences_from_features(reg.FeatureFPFH(), ft)) == 0
