"""GPU: the PAIR STREAM of the point-to-plane reduction (csrc/reduce.h PairArgs).  Once the matches of a packet
of 64 source points have stood still through a whole search, the reduction keeps the packet's 64 matched {point, normal}
records next to the source and reads those instead of the index and the gather.  Whatever it reads, the 30 sums -- hence
every transformation, fitness and rmse -- must be the gather path's, bit for bit.

The oracle is the engine's own gather path: engine `b` holds the same clouds and runs the same loop, but drops every
pair state in front of every iteration (mi_icp_debug_drop_pairs), so its reductions never read a record.  All sources
are above the one-launch iteration's size (170,000 points): below it the loop never takes this kernel.

Seeds of the noisy cases, checked beforehand on the CPU with the oracle port (kd-tree search, point-to-plane system and
solve per iteration; sigma = 0.15 spacings; scripts/dev/pair_stream_seed_check.py, its output in
profiles/pair_stream_seed_check.txt):
  converged (seed 5, 60 % of bench.synth(300,007): 179,960 points -- 60 % of 200,003 points would be 120,061, which the
      loop takes in one launch per iteration, never through this kernel): 100.0000 % of the points keep their match over
      the last three of twelve iterations (changes per iteration: 13196 2550 377 57 6 0 1 0 0 0 0 0);
  transient (seed 6, all of bench.synth(200,003), init 1.5 spacings + 0.5 s rad off): 11,559 times after iteration 10 a point changes
      its match having kept it for two iterations (iterations 11..18: 9004 2119 383 43 7 1 0 1; seed 7: 16,013) -- in
      iterations 13 and 14, with half the packets already still, a record that is valid and is then voided by the search
      is reachable from the reference alone."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import reduce_exact as rx  # noqa: E402

pytestmark = pytest.mark.gpu
PT2PL = 2
N = 200_003


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def popcount(masks):
    return int(np.unpackbits(np.ascontiguousarray(masks).view(np.uint8)).sum())


def same_result(ra, rb, what):
    assert np.array_equal(np.array(ra.transformation, np.float32), np.array(rb.transformation, np.float32)), what + ": T differs"
    assert np.float32(ra.fitness).tobytes() == np.float32(rb.fitness).tobytes(), what + ": fitness differs"
    assert np.float32(ra.inlier_rmse).tobytes() == np.float32(rb.inlier_rmse).tobytes(), what + ": rmse differs"
    assert ra.n_correspondences == rb.n_correspondences, what + ": count differs"


class Pair:
    """the loop under test (`a`) and the same loop that never reads a pair record (`b`)"""

    def __init__(self):
        from cupoch_amd.engine import Engine
        self.a, self.b = Engine(0), Engine(0)

    def load(self, src, tgt, nrm):
        self.d_src, self.d_tgt, self.d_nrm = cuda(src), cuda(tgt), cuda(nrm)
        for e in (self.a, self.b):
            e.set_target(self.d_tgt, self.d_nrm)
            e.set_source(self.d_src)
        return self

    def close(self):
        self.a.close()
        self.b.close()

    def begin(self, max_dist, init):
        ra = self.a.icp_begin(PT2PL, max_dist, init, -1.0)
        rb = self.b.icp_begin(PT2PL, max_dist, init, -1.0)
        same_result(ra, rb, "first pass")

    def step(self, what):
        """one iteration of both; b's pair states are dropped first and must still be unread after it"""
        self.b.drop_pairs()
        ra, rb = self.a.icp_iterate(1), self.b.icp_iterate(1)
        same_result(ra, rb, what)
        assert int(self.b.pair_state()["state"].max()) <= 1, "the oracle engine reached a pair record"
        return ra

    def same_matches(self):
        ca, cb = self.a.get_correspondences(), self.b.get_correspondences()
        assert ca.shape == cb.shape and np.array_equal(ca, cb), "correspondences differ"
        return ca


def run_lattice(p, n, tname, iters=6):
    tg, st = rx.target(), rx.stored(n, tname)
    p.load(st["pts"], tg["pts"], tg["nrm"])
    p.begin(rx.MAX_DIST, rx.TRANSFORMS[tname])
    for k in range(1, iters + 1):
        p.step("n = %d, %s, iteration %d" % (n, tname, k))
        s = p.a.pair_state()
        if k >= 3:
            assert (s["state"] == 2).all(), "iteration %d: %d packets not in state 2" % (k, int((s["state"] != 2).sum()))
    cor = p.same_matches()
    nn = rx.case(n)["nn"]
    assert len(s["state"]) == (n + 63) // 64
    # the masks against the constructed misses: as many lanes as matches, none past the end, and the matched sources exactly
    assert popcount(s["mask"]) == int((nn >= 0).sum()) == len(cor)
    assert np.array_equal(np.sort(cor[:, 0]), np.flatnonzero(nn >= 0))
    live = n - 64 * (len(s["mask"]) - 1)
    assert live == 64 or int(s["mask"][-1]) >> live == 0, "the last packet's mask covers lanes past the end"
    assert int((nn < 0).sum()) > 0


@pytest.fixture(scope="module")
def pair():
    p = Pair()
    yield p
    p.close()


# 170,001: the first size with search + reduction, 17 live lanes in the last packet; 262,145: kU = 4, a second outer trip
# with one live lane; 4,194,305: kU = 2 and the 1024-row grid's size (reduce_exact.py SIZES)
@pytest.mark.parametrize("tname", ["identity", "rot90z"])
@pytest.mark.parametrize("n", [170_001, 262_145, 4_194_305])
def test_lattice_with_constructed_misses_pairs_every_packet_and_sums_as_the_gather(pair, n, tname):
    run_lattice(pair, n, tname)


def test_one_context_reused_across_sizes_reads_no_stale_record(pair):
    for n in (4_194_305, 170_001, 4_194_305):
        run_lattice(pair, n, "rot90z", iters=4)


def noisy_clouds(seed, share, n=N):
    src, tgt, nrm, _, max_dist = bench.synth(n)
    s = float(n) ** (-1.0 / 3.0)
    rng = np.random.default_rng(seed)
    if share < 1.0:
        keep = rng.random(n) < share
        noisy = (src[keep] + rng.normal(0.0, 0.15 * s, (int(keep.sum()), 3))).astype(np.float32)
    else:
        noisy = (src + rng.normal(0.0, 0.15 * s, src.shape)).astype(np.float32)
    return noisy, tgt, nrm, max_dist, s


def test_converged_noisy_partial_overlap_is_read_from_the_pairs(pair):
    noisy, tgt, nrm, max_dist, _ = noisy_clouds(5, 0.6, 300_007)
    assert len(noisy) > 170_000
    pair.load(noisy, tgt, nrm)
    pair.begin(max_dist, None)
    shares = []
    for k in range(1, 13):
        pair.step("noisy converged, iteration %d" % k)
        shares.append(float((pair.a.pair_state()["state"] == 2).mean()))
    pair.same_matches()
    print("noisy converged: share of packets in state 2 per iteration:", " ".join("%.3f" % x for x in shares))
    assert shares[-1] >= 0.9


def test_transient_voids_records_where_the_search_changes_a_match(pair):
    noisy, tgt, nrm, max_dist, s = noisy_clouds(6, 1.0)
    init = np.eye(4, dtype=np.float32)
    init[:3, 3] = (1.5 * s / np.sqrt(3.0)) * np.array([1.0, -1.0, 1.0], np.float32)
    ang = 0.5 * s
    init[:3, :3] = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]], np.float32)
    pair.load(noisy, tgt, nrm)
    pair.begin(max_dist, init)
    was_valid = np.zeros((len(noisy) + 63) // 64, bool)
    voided, counts = 0, []
    for k in range(1, 31):
        pair.step("transient, iteration %d" % k)
        st = pair.a.pair_state()["state"]
        # (read after the iteration's reduction, which has raised every 0 to 1 already: a record the search voided shows as 1)
        voided += int((was_valid & (st < 2)).sum())
        was_valid |= st == 2
        counts.append((int((st == 0).sum()), int((st == 1).sum()), int((st == 2).sum())))
    pair.same_matches()
    print("transient: packets in state 0 / 1 / 2 after each iteration:", " ".join("%d/%d/%d" % c for c in counts))
    print("transient: %d times a packet seen in state 2 was seen below it after a later iteration" % voided)
    assert voided > 0


@pytest.fixture(scope="module")
def exact_clouds():
    return bench.synth(N)


def test_gate_and_pairs_together(pair, exact_clouds):
    src, tgt, nrm, _, max_dist = exact_clouds
    pair.load(src, tgt, nrm)
    pair.begin(max_dist, None)
    skipped = []
    for k in range(1, 25):
        sa, sk = pair.a.pair_state()["state"], pair.a.search_skip_state()["will_skip"]
        pair.step("exact clouds, iteration %d" % k)
        after = pair.a.pair_state()["state"]
        skipped.append(float(sk.mean()))
        assert (after[sk & (sa == 2)] == 2).all(), "iteration %d: a packet the gate skipped lost its record" % k
    pair.same_matches()
    print("exact clouds: share of packets the gate skips per iteration:", " ".join("%.3f" % x for x in skipped))
    print("exact clouds: will_skip.mean() = %.3f at the end, %.3f of the packets in state 2"
          % (float(pair.a.search_skip_state()["will_skip"].mean()), float((after == 2).mean())))
    assert skipped[-1] > 0.0 and (after == 2).mean() >= 0.9


def test_source_of_a_multiple_of_64_points(pair):
    src, tgt, nrm, _, max_dist = bench.synth(200_064)
    pair.load(src, tgt, nrm)
    pair.begin(max_dist, None)
    for k in range(1, 7):
        pair.step("200,064 points, iteration %d" % k)
    pair.same_matches()
    s = pair.a.pair_state()
    assert len(s["state"]) == 200_064 // 64 and (s["state"] == 2).mean() >= 0.9


def test_the_host_voids_every_record_where_matches_packets_or_target_change(exact_clouds):
    src, tgt, nrm, _, max_dist = exact_clouds
    p = Pair().load(src, tgt, nrm)
    e = p.a
    try:
        def paired():
            e.icp_begin(PT2PL, max_dist, None, -1.0)
            r = e.icp_iterate(4)
            assert (e.pair_state()["state"] == 2).mean() >= 0.9, "the loop has not paired: the check would be vacuous"
            return r

        for what, act in (("set_source", lambda r: e.set_source(p.d_src)),
                          ("set_target", lambda r: e.set_target(p.d_tgt, p.d_nrm)),
                          ("drop_seeds", lambda r: e.drop_seeds()),
                          ("a second icp_begin", lambda r: e.icp_begin(PT2PL, max_dist, None, -1.0)),
                          ("evaluate_registration", lambda r: e.evaluate_registration(
                              max_dist, np.array(r.transformation, np.float32).reshape(4, 4).T))):
            r = paired()
            act(r)
            assert int(e.pair_state()["state"].max()) == 0, "%s left a pair state standing" % what
    finally:
        p.close()


def test_both_pair_instantiations_keep_two_workgroups_per_cu():
    """the reduction is launched on 512 blocks, two per CU: <2,1,pairs> (4 Mi points and more) and <4,1,pairs> (below;
    181 registers, the one nearest the edge) must both be granted them"""
    from cupoch_amd import _lib
    L = _lib.load()
    assert L.mi_icp_debug_occupancy(3) >= 2 and L.mi_icp_debug_occupancy(9) >= 2
