"""Feature matching and FastGlobalRegistration without a GPU: the numpy restatement (tests/fgr_exact.py) recovers the
scene's transform in both scale modes; none of the scenes the GPU tests use has a row the fp32 distance chain could
order otherwise than fp64 does; csrc/fgr_rules.h (sampler, tuple test, par schedule) equals the restatement in a
stand-alone sanitized program; the Python surface has the reference's names and defaults; the ABI family is declared,
exported and bound and takes no mem_kind."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fgr_exact as fx
from conftest import ROOT

F = np.float32


@pytest.fixture(scope="module")
def scenes():
    return fx.fgr_scenes()


def test_restatement_recovers_the_scene_in_both_scale_modes(scenes):
    for name, (sc, opt) in scenes.items():
        r64 = fx.fgr(sc["src"], sc["tgt"], sc["sfeat"], sc["tfeat"], opt, seed=0, fp32=False)
        r32 = fx.fgr(sc["src"], sc["tgt"], sc["sfeat"], sc["tfeat"], opt, seed=0, fp32=True)
        assert len(r64.corr) == 1000 and r64.passing * 3 > 1000, name
        if name == "noisy":
            assert 150 <= len(r64.pairs) <= 300 and np.linalg.norm(r64.T - sc["T_gt"]) < 2e-3, name
        else:
            assert 300 <= len(r64.pairs) <= 306 and 28000 <= r64.passing <= 30000, name
            assert np.linalg.norm(r64.T - sc["T_gt"]) < 1e-7, name
        assert np.array_equal(r32.corr, r64.corr)
        assert np.linalg.norm(r32.T.astype(np.float64) - r64.T) < 1e-5, name      # (the stated fp32 steps cost this much)
        # the 300 shared points pair up truly (a few of the 60 + 80 unshared ones pair among themselves)
        if name != "noisy":
            assert (sc["src_base"][r64.pairs[:, 0]] == sc["tgt_base"][r64.pairs[:, 1]]).sum() == 300


def test_no_scene_of_the_gpu_tests_has_an_undecided_row(scenes):
    """the condition the GPU tests rest on: wherever they demand the fp64 neighbour, best and second best are further
    apart than the derived band of the fp32 chain"""
    for name, (sc, _) in scenes.items():
        D = fx.dist64(sc["sfeat"], sc["tfeat"])
        dim = sc["sfeat"].shape[1]
        assert not fx.undecided(D, dim).any() and not fx.undecided(D.T, dim).any(), name
    for nq, nr, dim in fx.match_cases():
        Q, R = fx.match_case(nq, nr, dim)
        D = fx.dist64(Q, R)
        assert not fx.undecided(D, dim).any() and not fx.undecided(D.T, dim).any(), (nq, nr, dim)
    # the duplicate case: undecided rows exist, and each is a tie of bit-equal distances
    Q, R = fx.duplicate_case()
    D = fx.dist64(Q, R)
    for M in (D, D.T):
        und = fx.undecided(M, 33)
        assert und.sum() >= 20
        two = np.partition(M, 1, axis=1)[:, :2]
        assert (two[und, 0] == two[und, 1]).all()


def test_exact_chain_is_within_its_bound_of_fp64():
    rng = np.random.default_rng(4)
    for dim in (1, 33, 352):
        Q, R = fx.match_case(8, 8, dim)
        D = fx.dist64(Q, R)
        for _ in range(8):
            i, j = rng.integers(0, 8, 2)
            d = float(fx.chain_exact(Q[i], R[j]))
            assert abs(d - D[i, j]) <= (dim + 2) * 2.0 ** -24 * D[i, j]


def test_tuple_list_edges():
    sc = fx.scene(33, seed=1)
    D = fx.dist64(sc["sfeat"], sc["tfeat"])
    pairs = fx.reciprocal_pairs(fx.neighbours(D), fx.neighbours(D.T))
    for maxc in (1, 3, 10, 1000, 10 ** 6):
        corr, passing = fx.tuples(pairs, sc["src"], sc["tgt"], 0.95, maxc, 5)
        assert len(corr) == min(maxc, 3 * passing)
    for ncorr in (0, 1, 9, 10):
        corr, passing = fx.tuples(pairs[:ncorr], sc["src"], sc["tgt"], 0.95, 10 ** 6, 5)
        assert len(corr) == 3 * passing and (ncorr > 2 or passing == 0)      # (one or two pairs: every draw repeats one)
    a, _ = fx.tuples(pairs, sc["src"], sc["tgt"], 0.95, 1000, 5)
    b, _ = fx.tuples(pairs, sc["src"], sc["tgt"], 0.95, 1000, 6)
    assert not np.array_equal(a, b)


def _bits(v):
    return int(np.array(v, F).view(np.uint32))


def test_header_rules_equal_the_restatement_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "test_fgr_rules")
    src = os.path.join(ROOT, "tests", "cpp", "test_fgr_rules.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "cupoch_amd", "csrc"), src, "-o", exe])
    assert re.findall(r'#include\s+"([^"]+)"', open(src).read()) == ["fgr_rules.h"]
    rng = np.random.default_rng(3)
    text, want = [], []
    for seed, ncorr in ((0, 1), (0, 304), (5, 10), (2 ** 64 - 1, 2 ** 31 - 1), (12345678901234567, 9)):
        for t in (0, 1, 7, 30399, 2 ** 33):
            text.append("B %d %d %d" % (seed, t, ncorr))
            want.append([fx.below(fx.u(seed, 3 * t + m), ncorr) for m in range(3)])
    # the tuple test: triangles near the scale's edge, congruent ones, degenerate ones
    s2 = F(0.95) * F(0.95)
    accepts = []
    for k in range(400):
        p = rng.uniform(-3, 3, (3, 3)).astype(F)
        kind = k % 4
        if kind == 0:
            q = (p * F(rng.uniform(0.9, 1.1))).astype(F)                      # a scaled copy: near the edge
        elif kind == 1:
            q = (p[:, ::-1] + F(1.5)).astype(F)                               # congruent
        elif kind == 2:
            q = rng.uniform(-3, 3, (3, 3)).astype(F)
        else:
            p[1] = p[0]                                                       # a repeated pair
            q = p.copy()
        ok = True
        for m in range(3):
            li = fx.side2(p[m][None], p[(m + 1) % 3][None])[0]
            lj = fx.side2(q[m][None], q[(m + 1) % 3][None])[0]
            ok = ok and bool(li * s2 < lj) and bool(lj * s2 < li)
        text.append("A %08x " % _bits(s2) + " ".join("%08x" % _bits(v) for v in np.concatenate([p.ravel(), q.ravel()])))
        want.append([int(ok)])
        accepts.append(ok)
    assert 50 < sum(accepts) < 350
    for opt in (fx.Option(), fx.Option(decrease_mu=False), fx.Option(division_factor=2.0, maximum_correspondence_distance=0.3)):
        for par0 in (1.0, 4.7, 0.01):
            par = F(par0)
            for itr in range(12):
                nxt = fx.par_next(par, itr, opt)
                text.append("P %08x %d %d %08x %08x" % (_bits(par), itr, int(opt.decrease_mu), _bits(opt.maximum_correspondence_distance),
                                                        _bits(opt.division_factor)))
                want.append([_bits(nxt)])
                par = nxt
    for passing, maxc in ((0, 1000), (1, 1), (1, 3), (333, 1000), (334, 1000), (5, 10 ** 6), (7, 0)):
        text.append("C %d %d" % (passing, maxc))
        want.append([min(3 * passing, maxc)])
    out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    got = [[int(t, 16) if len(t) == 8 and line_op == "P" else int(t) for t in line.split()]
           for line, line_op in zip([l for l in out if l.strip()], [t[0] for t in text])]
    assert got == want


def test_par_schedule_of_the_defaults():
    par = fx.par_schedule(1.0, 9, fx.Option())
    want, p = [], F(1.0)
    for itr in range(9):
        if itr % 4 == 0 and p > F(0.025):
            p = F(p / F(1.4))
        want.append(p)
    assert par.tobytes() == np.array(want, F).tobytes()
    assert par[0] == par[3] and par[4] == par[7] and par[8] < par[4] < par[0] < 1.0
    assert (fx.par_schedule(1.0, 9, fx.Option(decrease_mu=False)) == 1.0).all()


def test_python_surface_names_and_defaults():
    import copy
    import inspect
    from cupoch_amd import registration as reg
    o = reg.FastGlobalRegistrationOption()
    assert (o.division_factor, o.use_absolute_scale, o.decrease_mu, o.maximum_correspondence_distance, o.iteration_number,
            o.tuple_scale, o.maximum_tuple_count) == (1.4, False, True, 0.025, 64, 0.95, 1000)
    ref = fx.Option()
    assert vars(ref) == {k: getattr(o, k) for k in vars(ref)}
    assert "division_factor=1.4" in repr(o) and "maximum_tuple_count=1000" in repr(o)
    o2 = reg.FastGlobalRegistrationOption(maximum_tuple_count=7, use_absolute_scale=True)
    assert o2.maximum_tuple_count == 7 and o2.use_absolute_scale is True
    c = o2._c()
    assert (c.use_absolute_scale, c.decrease_mu, c.iteration_number, c.maximum_tuple_count) == (1, 1, 64, 7)
    assert abs(c.division_factor - 1.4) < 1e-6 and abs(c.tuple_scale - 0.95) < 1e-6
    for cls, dim in ((reg.FeatureFPFH, 33), (reg.FeatureSHOT, 352)):
        f = cls()
        assert f.dimension() == dim and f.num() == 0 and f.is_empty()
        f.resize(5)
        assert f.num() == 5 and f.data.shape == (5, dim) and not f.is_empty()
        f.data = np.arange(3 * dim, dtype=np.float64).reshape(3, dim)
        assert f.num() == 3 and f.data.dtype == np.float32
        g = copy.deepcopy(f)
        g.data[0, 0] = -1
        assert f.data[0, 0] == 0 and "dimension = %d and num = 3" % dim in repr(f)
        with pytest.raises(ValueError):
            f.data = np.zeros((3, dim + 1))
    assert reg.Feature(32).dimension() == 32
    sig = inspect.signature(reg.registration_fast_based_on_feature_matching).parameters
    assert list(sig) == ["source", "target", "source_feature", "target_feature", "option", "seed"] and sig["seed"].default == 0
    sig = inspect.signature(reg.correspondences_from_features).parameters
    assert sig["mutual_filter"].default is False and sig["mutual_consistency_ratio"].default == 0.1


FGR_NAMES = ["mi_icp_feature_match", "mi_icp_fgr_correspondences", "mi_icp_fgr_optimize", "mi_icp_correspondences_from_features",
             "mi_icp_fast_global_registration"]


def test_abi_family_is_declared_exported_and_bound_and_takes_no_mem_kind():
    from cupoch_amd import _lib
    src = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    code = re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    for n in FGR_NAMES:
        m = re.search(r"MI_ICP_API\s+int\s+%s\s*\(([^;]*?)\)\s*;" % n, code, flags=re.S)
        assert m, n
        assert "mem_kind" not in m.group(1), n
        assert n in _lib.SIGNATURES
    assert "mi_feature" in _lib.UNITS
    for f in ("mi_feature.hip", "feature_kernels.h", "fgr_rules.h"):
        assert os.path.exists(os.path.join(_lib.CSRC, f)), f
    _lib.build()
    L = _lib.load()
    assert all(hasattr(L, n) for n in FGR_NAMES)
    assert "feature matching and FastGlobalRegistration" in src
    assert C.sizeof(_lib.FgrOption) == 28
    # no context: refused before anything else
    assert L.mi_icp_feature_match(None, None, 1, None, 1, 33, None, None, None, None) == -1
    assert L.mi_icp_fast_global_registration(None, None, None, 1, None, None, 1, 33, None, 0, None) == -1
