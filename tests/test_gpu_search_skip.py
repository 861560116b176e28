"""GPU: the SEARCH SKIP (csrc/nn_search.h "the skip", csrc/loop.h odometer).  A seeded search of the
registration loop leaves, per packet of 64 source points, a limit on the loop's odometer; while the odometer stays below
it the packet is not searched again.  Whatever is skipped, the matches must be exactly what an unskipped search finds.

The oracle is the engine's own pass FROM THE ROOT (which never skips) at the same transform -- run on a second engine
holding the same clouds, so that the loop under test keeps its limits from one check to the next.  Sources have
200,003 points: above the one-launch iteration's size (170,000), not a multiple of 64 (pad lanes)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402

pytestmark = pytest.mark.gpu
PT2PL = 2
N = 200_003


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


class Pair:
    """the loop under test (`a`) and the unskipped oracle (`b`) on the same clouds"""

    def __init__(self, src, tgt, nrm):
        from cupoch_amd.engine import Engine
        self.a, self.b = Engine(0), Engine(0)
        self.d_src, self.d_tgt, self.d_nrm = cuda(src), cuda(tgt), cuda(nrm)
        for e in (self.a, self.b):
            e.set_target(self.d_tgt, self.d_nrm)
            e.set_source(self.d_src)

    def close(self):
        self.a.close()
        self.b.close()

    def check(self, res, max_dist, what):
        """a's matches against a pass from the root at a's transform"""
        T = np.array(res.transformation, np.float32).reshape(4, 4).T
        got = self.a.get_correspondences()
        self.b.drop_seeds()
        ref = self.b.evaluate_registration(max_dist, T)
        assert self.b.last_search_kind() == 0, "the oracle pass did not start at the root"
        want = self.b.get_correspondences()
        assert got.shape == want.shape and np.array_equal(got, want), "%s: matches differ from the unskipped search" % what
        assert res.n_correspondences == ref.n_correspondences
        return T


@pytest.fixture(scope="module")
def exact():
    src, tgt, nrm, _, max_dist = bench.synth(N)
    p = Pair(src, tgt, nrm)
    yield p, max_dist
    p.close()


def test_exact_clouds_skip_most_packets_and_keep_every_match(exact):
    p, max_dist = exact
    p.a.icp_begin(PT2PL, max_dist, None, -1.0)
    p.a.icp_iterate(10)
    st = p.a.search_skip_state()
    share = float(st["will_skip"].mean())
    print("exact clouds: %.1f %% of %d packets unexpired after 10 iterations (travel %.3g, fuzz %.3g)"
          % (100 * share, len(st["limits"]), st["travel"], st["fuzz"]))
    assert st["armed"] and share >= 0.5
    for k in range(5):
        before = int(p.a.search_skip_state()["will_skip"].sum())
        res = p.a.icp_iterate(1)
        assert before > 0, "iteration %d skipped nothing: the check would be vacuous" % k
        p.check(res, max_dist, "iteration %d (%d packets skipped)" % (k, before))


def test_noisy_transient_matches_and_statistics_equal_an_engine_that_never_skips():
    src, tgt, nrm, _, max_dist = bench.synth(N)
    s = float(N) ** (-1.0 / 3.0)
    rng = np.random.default_rng(5)
    keep = rng.random(N) < 0.6
    noisy = (src[keep] + rng.normal(0.0, 0.15 * s, (int(keep.sum()), 3))).astype(np.float32)
    init = np.eye(4, dtype=np.float32)
    init[:3, 3] = (1.5 * s / np.sqrt(3.0)) * np.array([1.0, -1.0, 1.0], np.float32)
    p = Pair(noisy, tgt, nrm)
    from cupoch_amd.engine import Engine
    c = Engine(0)   # the same loop, its limits dropped in front of every iteration (a search outside the loop does that)
    try:
        c.set_target(p.d_tgt, p.d_nrm)
        c.set_source(p.d_src)
        ra = p.a.icp_begin(PT2PL, max_dist, init, -1.0)
        rc = c.icp_begin(PT2PL, max_dist, init, -1.0)
        skipped = []
        for k in range(30):
            st = p.a.search_skip_state()
            skipped.append(float(st["will_skip"].mean()))
            ra = p.a.icp_iterate(1)
            c.evaluate_registration(max_dist, np.array(rc.transformation, np.float32).reshape(4, 4).T)
            assert not c.search_skip_state()["armed"]
            rc = c.icp_iterate(1)
            p.check(ra, max_dist, "iteration %d" % k)
            assert np.array_equal(np.array(ra.transformation), np.array(rc.transformation))
            assert np.float32(ra.fitness).tobytes() == np.float32(rc.fitness).tobytes()
            assert np.float32(ra.inlier_rmse).tobytes() == np.float32(rc.inlier_rmse).tobytes()
        print("noisy transient: share of packets skipped per iteration:", " ".join("%.3f" % x for x in skipped))
        # (documented, DESIGN 4.1: with this noise some lane of every packet needs a halo line, no packet holds a limit --
        # what the case checks is that the searches which record nothing change nothing either)
        assert max(skipped) == 0.0
    finally:
        c.close()
        p.close()


def test_limits_that_are_crossed_expire_and_the_matches_that_change_are_found():
    """Clean clouds a twentieth of a spacing off: the loop's steps shrink through 1e-3 ... 1e-6 spacings while most
    packets hold limits.  6000 source points lie within 1e-5 ... 1e-2 spacings of the bisector of two target points a
    fifth of a spacing apart: a step of that size changes their match.  A packet that skipped by an odometer reading too
    small, or by a margin too wide, would keep the old one."""
    s = float(N) ** (-1.0 / 3.0)
    rng = np.random.default_rng(17)
    n_tw = 6000
    base = rng.random((N - n_tw, 3))
    v = rng.standard_normal((n_tw, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    tgt = np.concatenate([base, base[:n_tw] + 0.2 * s * v]).astype(np.float32)
    eta = 10.0 ** rng.uniform(-5.0, -2.0, n_tw) * s * rng.choice([-1.0, 1.0], n_tw)
    mid = tgt[:n_tw].astype(np.float64) * 0.5 + tgt[N - n_tw:].astype(np.float64) * 0.5 + eta[:, None] * v
    src = np.concatenate([tgt[:N - n_tw], mid.astype(np.float32)])
    src = src[rng.permutation(N)]
    nrm = rng.standard_normal((N, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    init = np.eye(4, dtype=np.float32)
    init[:3, 3] = (0.05 * s / np.sqrt(3.0)) * np.array([1.0, -1.0, 1.0], np.float32)
    max_dist = 2.0 * s
    p = Pair(src, tgt, nrm)

    def matches():
        c = p.a.get_correspondences()
        m = np.full(N, -1, np.int64)
        m[c[:, 0]] = c[:, 1]
        return m

    try:
        res = p.a.icp_begin(PT2PL, max_dist, init, -1.0)
        p.check(res, max_dist, "first pass")
        prev = matches()
        skipped = expired = changed = 0
        for k in range(8):
            before = p.a.search_skip_state()
            res = p.a.icp_iterate(1)
            p.check(res, max_dist, "iteration %d" % k)
            after = p.a.search_skip_state()     # (the odometer as the search of this iteration read it)
            cur = matches()
            moved = after["travel"] - before["travel"]
            if before["armed"]:
                held = np.isfinite(before["limits"])
                with np.errstate(invalid="ignore"):
                    kept = held & (after["travel"] + after["fuzz"] < before["limits"])
                skipped += int(kept.sum())
                expired += int((held & ~kept).sum())
                changed += int((cur != prev).sum())
                print("iteration %d: odometer +%.3g spacings, %d packets skipped, %d limits crossed, %d matches changed"
                      % (k, moved / s, kept.sum(), (held & ~kept).sum(), (cur != prev).sum()))
            prev = cur
        assert skipped > 0 and expired > 0 and changed > 0, (skipped, expired, changed)
    finally:
        p.close()


def test_ties_never_skip():
    """every target point twice, every source point midway between eight lattice points (exact in fp32): each lane's
    match has an equal in its leaf -- margin 0, no limit, no skip"""
    h = 1.0 / 64.0
    g = np.arange(60, dtype=np.float32) * np.float32(h)
    lat = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    tgt = np.concatenate([lat, lat])
    rng = np.random.default_rng(7)
    tgt = tgt[rng.permutation(len(tgt))]
    nrm = rng.standard_normal(tgt.shape).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    gm = (np.arange(59, dtype=np.float32) + np.float32(0.5)) * np.float32(h)
    mid = np.stack(np.meshgrid(gm, gm, gm, indexing="ij"), -1).reshape(-1, 3)
    src = mid[rng.permutation(len(mid))[:N]]
    max_dist = 1.5 * h
    p = Pair(src, tgt, nrm)
    try:
        res = p.a.icp_begin(PT2PL, max_dist, None, -1.0)
        assert res.n_correspondences == N
        for k in range(5):
            res = p.a.icp_iterate(1)
            p.check(res, max_dist, "iteration %d" % k)
            st = p.a.search_skip_state()
            assert not np.isfinite(st["limits"]).any() and not st["will_skip"].any(), "a packet of tied lanes holds a limit"
    finally:
        p.close()


def test_matches_at_the_radius_edge():
    """every source point exactly L beside its target point (coordinates on a 2^-20 grid), max_dist = L (1 + 5e-7):
    most matches sit within 1e-6 of the radius; normals a little off the z axis keep the transform creeping, so
    matches cross the radius in both directions"""
    rng = np.random.default_rng(11)
    q = np.float32(2.0 ** -20)
    tgt = (np.round(rng.random((N, 3)) * 2.0 ** 20) * q).astype(np.float32)
    L = np.float32(5347.0) * q                      # 0.3 spacings
    src = (tgt + np.array([L, 0, 0], np.float32)).astype(np.float32)
    assert np.array_equal((src - tgt)[:, 0], np.full(N, L, np.float32))
    nrm = np.concatenate([1e-3 * rng.standard_normal((N, 2)), np.ones((N, 1))], 1).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    max_dist = float(L) * (1.0 + 5e-7)
    p = Pair(src[rng.permutation(N)], tgt, nrm)
    try:
        res = p.a.icp_begin(PT2PL, max_dist, None, -1.0)
        print("radius edge: %d of %d matched at the start" % (res.n_correspondences, N))
        assert res.n_correspondences > N // 2
        for k in range(10):
            res = p.a.icp_iterate(1)
            p.check(res, max_dist, "iteration %d" % k)
    finally:
        p.close()


def test_whatever_voids_the_limits_is_followed_by_a_whole_search(exact):
    p, max_dist = exact
    s = float(N) ** (-1.0 / 3.0)
    p.a.icp_begin(PT2PL, max_dist, None, -1.0)
    res = p.a.icp_iterate(10)
    T = np.array(res.transformation, np.float32).reshape(4, 4).T
    other = T.copy()
    other[:3, 3] += np.float32(0.4 * s)

    def again(what, armed_before):
        if armed_before is not None:
            assert p.a.search_skip_state()["armed"] == armed_before, what
        r = p.a.icp_iterate(1)
        p.check(r, max_dist, what)
        return r

    assert p.a.search_skip_state()["will_skip"].mean() >= 0.5
    p.a.evaluate_registration(max_dist, other)
    again("after evaluate_registration with another T", False)
    # (that iteration started from the other transform's matches: some lane of most packets had to walk, few packets got
    # a limit, and the host's sample may keep the next search ungated; the one after it is gated again)
    again("the iteration after that", None)
    again("the second iteration after that", True)
    p.a.evaluate_registration(0.8 * max_dist, T)
    again("after a search with another max_dist", False)
    p.a.drop_seeds()
    again("after drop_seeds", False)
    # (new clouds end a stepping loop: it is begun again, from where it stood)
    p.a.set_source(p.d_src)
    res = p.a.icp_begin(PT2PL, max_dist, T, -1.0)
    assert not p.a.search_skip_state()["will_skip"].any(), "limits survived set_source / icp_begin"
    p.check(res, max_dist, "first pass after set_source")
    for k in range(3):
        res = p.a.icp_iterate(1)
        p.check(res, max_dist, "iteration %d after set_source" % k)
    st = p.a.search_skip_state()
    assert st["armed"] and st["will_skip"].mean() >= 0.5


def test_a_loop_whose_first_step_relocates_keeps_every_match():
    """a thin sheet, the source 12 in-sheet spacings above it: the first update moves it by more than a leaf's width"""
    n = N
    rng = np.random.default_rng(13)
    uv = rng.random((n, 2))
    z = 0.15 * np.sin(5 * uv[:, 0]) * np.cos(4 * uv[:, 1])
    tgt = np.stack([uv[:, 0], uv[:, 1], z], 1).astype(np.float32)
    gx = 0.75 * np.cos(5 * uv[:, 0]) * np.cos(4 * uv[:, 1])
    gy = -0.6 * np.sin(5 * uv[:, 0]) * np.sin(4 * uv[:, 1])
    nrm = np.stack([-gx, -gy, np.ones(n)], 1).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    sp = float(n) ** -0.5
    src = (tgt + np.array([0, 0, 12 * sp], np.float32)).astype(np.float32)[rng.permutation(n)]
    max_dist = 16 * sp
    p = Pair(src, tgt, nrm)
    try:
        res = p.a.icp_begin(PT2PL, max_dist, None, -1.0)
        for k in range(6):
            res = p.a.icp_iterate(1)
            p.check(res, max_dist, "iteration %d" % k)
        counters = p.a.loop_counters()
        print("relocating loop: %d re-locations in %d iterations" % (counters[2], counters[0]))
        assert counters[2] >= 1, "no step of this loop set `relocate`: the data do not test what they should"
    finally:
        p.close()
