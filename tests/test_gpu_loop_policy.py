"""GPU: the observable decisions of the registration loop's host policy (csrc/loop_policy.h, wired in by loop_run,
loop_begin, launch_nn and mi_icp_set_target) on four seeded synthetic pairs.  tests/test_loop_policy.py pins the rules on
a CPU; this pins what the callers hand them and in which order, through what already exists: the profile's halo builds
started by loops, the result's iterations and nn_passes, Engine.loop_counters() and Engine.last_search_kind()."""
import os

import pytest

from conftest import make_pair

pytestmark = pytest.mark.gpu

# (halo builds started by loops, iterations, nn_passes, loop counters: iterations, passes, re-locations, armed, last search
# kind).  MEASURED on an MI355X at the commit before loop_policy.h existed, by measure() below as it stands: integers that
# deterministic rules produce from fixed inputs, so the comparison is exact.
EXPECTED = {
    "a": (0, 12, 13, 12, 13, 0, 0, 1),
    "b": (1, 12, 13, 12, 13, 0, 0, 1),
    "c": (1, 30, 31, 30, 31, 0, 0, 1),
    "d": (1, 12, 13, 12, 13, 0, 0, 1),   # (the one build is the first registration's: the second target's started ahead, behind its tree)
}


def _register(eng, d, iters):
    import torch
    from cupoch_amd import _lib
    eng.set_target(torch.from_numpy(d["tgt"]).cuda(), torch.from_numpy(d["tgt_nrm"]).cuda())
    eng.set_source(torch.from_numpy(d["src"]).cuda())
    r = eng.registration_icp(_lib.EST_POINT_TO_PLANE, d["max_dist"], None, 0.0, 0.0, max_iteration=iters, det_thresh=-1.0)
    return (eng.get_profile()["halo_builds_by_loops"], int(r.iterations), int(r.nn_passes),
            *(int(v) for v in eng.loop_counters()), eng.last_search_kind())


def measure(case):
    """a  60,000 points, clean, point-to-plane: small, and never asks
    b  60,000 points with the noise of test_gpu_threads kind 0: small, builds on demand at the first look
    c  600,000 noisy points: above kLarge -- single-iteration chunks, the decision at the second look
    d  case b, then a new 60,000-point target on the same context: the build starts ahead"""
    from cupoch_amd.engine import Engine
    eng = Engine(0)
    try:
        if case == "a":
            return _register(eng, make_pair(60000, seed=23), 12)
        if case == "b":
            return _register(eng, make_pair(60000, seed=21, noise=0.1), 12)
        if case == "c":
            return _register(eng, make_pair(600000, seed=25, noise=0.1), 30)
        _register(eng, make_pair(60000, seed=21, noise=0.1), 12)
        return _register(eng, make_pair(60000, seed=27, noise=0.1), 12)
    finally:
        eng.close()


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_loop_decisions_equal_those_measured_before_the_policy_header(case):
    if case == "c" and os.environ.get("MI_ICP_WAIT_LINKS") is not None:
        pytest.skip("MI_ICP_WAIT_LINKS builds every halo up front: the two-look decision does not run")
    got = measure(case)
    print("case %s: %r" % (case, got))
    assert got == EXPECTED[case]
