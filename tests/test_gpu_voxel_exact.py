"""VoxelDownSample held EXACTLY on every path of mi_icp_voxel_downsample (csrc/mi_voxel.hip), and the path asserted.

Every general-path kernel adds in fp64 and rounds once, (float)(sum / count).  The lattice clouds of
tests/voxel_exact.py have fp64 sums that are exact in any order, so each output float has ONE right value -- the numpy
restatement's, which tests/test_voxel_exact_cpu.py holds against the CPU oracle bit for bit -- whatever kernel ran and
however it grouped the additions.  A point dropped from a crowded voxel, added twice or credited to a sibling voxel of
its run changes an exact sum (colour channel 0 is 1.0 in every point: its mean is exactly 1), where an absolute
tolerance of 1e-6 lets it pass once the voxel is fine enough or full enough.

Every case declares the plan it was written for as literals -- (path, key bits, L, sort passes, sort kind, means
kernel) -- and asserts that mi_icp_debug_last_voxel_plan reports it: a case that no longer runs what it names fails
instead of silently testing something else.  The rows are the smallest clouds that reach each path (voxel_exact.LATTICE
lists them with what each pins).

Not covered: voxel_means_runs is only ever launched with L == 0 (mi_voxel.hip gives L > 0 to voxel_means_wave), so its
L > 0 branch -- the search of the run, the walk of the mask -- cannot be reached from the entry point.

Bounds.
 * Lattice clouds: points and colours bit for bit.  Normals within 4 ulp of w / |w| computed in fp64 from the float32
   means w: w is exact.  With u = 2^-24, l * l = w0^2 + w1^2 + w2^2 is off by at most 3 u relatively (the three
   products together u of the sum, the terms being positive; the two additions u each; fewer with FMA contraction),
   the square root halves that and is correctly rounded (1.5 u + u), the division is correctly rounded (u more):
   3.5 u relative, which is 1.75 ... 3.5 ulp of the result by where it sits in its binade -- typically under 3, and 4
   leaves slack over the worst.  NaN exactly where the reference has NaN (w = 0: 0 / 0).
 * The random family, against the oracle: both sides round an fp64 quotient to float; the two quotients differ by at
   most 2 * count * 2^-53 relatively (fp64 sums of non-negative terms in two orders: no cancellation), so the two floats
   are equal or adjacent: 1 ulp.  Normals: unit vectors, the same three roundings on either side, 4 * 2^-24 absolute;
   the fp64 order noise, 1e-13 / |w|, is negligible while |w| >= 1e-3, which is asserted on the reference."""
import ctypes as C
import functools
import math
import os

import numpy as np
import pytest
import torch

import voxel_exact as vx
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

SUBSETS = {"points": (False, False), "normals": (True, False), "colors": (False, True), "both": (True, True)}


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def cuda(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def host(a):
    return None if a is None else np.array(a)


def plan_of(eng):
    out = (C.c_int32 * 8)()
    assert eng._L.mi_icp_debug_last_voxel_plan(eng._ctx, out) == 0
    assert out[0] == eng._L.mi_icp_debug_last_voxel_path(eng._ctx)
    return list(out)


def downsample(eng, case, pts, nrm, col, put=cuda):
    """one call, the dense path switched off where the case says so (the switch is read at every call); numpy
    results and the plan word"""
    if case.get("no_dense"):
        os.environ["MI_ICP_NO_DENSE_VOXEL"] = "1"
    else:
        os.environ.pop("MI_ICP_NO_DENSE_VOXEL", None)
    try:
        p, n, c = eng.voxel_downsample(put(pts), float(case["voxel"]), put(nrm), put(col))
    finally:
        os.environ.pop("MI_ICP_NO_DENSE_VOXEL", None)
    back = lambda a: None if a is None else (a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a))
    return back(p), back(n), back(c), plan_of(eng)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def check_plan(plan, case, nvox):
    print("%s: plan %s, %d voxels" % (case["id"], plan, nvox))
    assert tuple(plan[:6]) == case["plan"], "the case was written for another plan"
    assert plan[6] == nvox and plan[7] == 0


def check_lattice(eng, case_id, with_nrm, with_col, put):
    c, pts, nrm, col, ref = vx.lattice(case_id)
    nrm = nrm if with_nrm else None
    col = col if with_col else None
    p, n, k, plan = downsample(eng, c, pts, nrm, col, put)
    check_plan(plan, c, len(ref["points"]))
    assert len(p) == len(ref["points"])
    assert same_bits(p, ref["points"])
    assert (n is None) == (nrm is None) and (k is None) == (col is None)
    if col is not None:
        assert (k[:, 0] == 1.0).all()
        assert same_bits(k, ref["colors"])
    if nrm is not None:
        assert np.array_equal(np.isnan(n), np.isnan(ref["normals"]))
        worst = vx.ulps(n, ref["normals"]).max()
        print("normals: %.3g ulp" % worst)
        assert worst <= 4
    p2, n2, k2, plan2 = downsample(eng, c, pts, nrm, col, put)            # the same bits from call to call
    assert plan2 == plan and same_bits(p2, p)
    assert n is None or same_bits(n2, n)
    assert k is None or same_bits(k2, k)


@pytest.mark.parametrize("subset", list(SUBSETS))
@pytest.mark.parametrize("case_id", vx.LATTICE_IDS)
def test_lattice_cloud_is_the_restatement_bit_for_bit_on_the_declared_plan(eng, case_id, subset):
    check_lattice(eng, case_id, *SUBSETS[subset], put=cuda)


@pytest.mark.parametrize("case_id", [c["id"] for c in vx.LATTICE if c["host"]])
def test_lattice_cloud_from_host_arrays(eng, case_id):
    check_lattice(eng, case_id, True, True, put=host)


@functools.lru_cache(maxsize=None)
def oracle_of(case_id):
    c, pts, nrm, col = vx.random_case(case_id)
    return orc.voxel_downsample(pts, c["voxel"], nrm, col)


@pytest.mark.parametrize("case_id", vx.RANDOM_IDS + ["faces"])
def test_random_cloud_is_within_an_ulp_of_the_oracle_on_the_declared_plan(eng, case_id):
    """faces: half of the points on or one ulp beside the cell faces of a non-dyadic voxel, on the general path --
    voxel_cell puts them where the IEEE division does (same voxels, same count)"""
    c, pts, nrm, col = vx.random_case(case_id)
    rp, rn, rc = oracle_of(case_id)
    p, n, k, plan = downsample(eng, c, pts, nrm, col)
    check_plan(plan, c, len(rp))
    assert len(p) == len(rp)
    up, uc, dn = vx.ulps(p, rp).max(), vx.ulps(k, rc).max(), np.abs(n.astype(np.float64) - rn).max()
    print("points %.3g ulp, colours %.3g ulp, normals %.3g" % (up, uc, dn))
    assert up <= 1 and uc <= 1
    assert dn <= 4 * 2.0 ** -24


# ---- the bounds and the centre that place the grid: mi_icp_compute_bounds -------------------------------------------
def bounds_cloud(n):
    """coordinates k / 8, k = 0 .. 511: every fp64 sum of them (and of the planted extremes) is exact"""
    rng = np.random.default_rng(n)
    return (rng.integers(0, 512, size=(n, 3)).astype(np.float64) / 8.0).astype(np.float32)


def check_bounds(eng, pts_host, pts_dev, centre="exact"):
    mn, mx, ce = eng.compute_bounds(pts_dev)
    # values, not bits: fminf does not say which zero the minimum of -0 and +0 is
    assert np.array_equal(mn, np.fmin.reduce(pts_host, axis=0)) and np.array_equal(mx, np.fmax.reduce(pts_host, axis=0))
    if centre == "exact":
        S = pts_host.astype(np.float64).sum(axis=0)                         # (exact: see bounds_cloud)
        assert same_bits(ce, (S / len(pts_host)).astype(np.float32))
    return ce


@pytest.mark.parametrize("n", vx.BOUNDS_SIZES)
def test_bounds_and_centre_at_every_place_of_the_reduction(eng, n):
    """A unique minimum and a unique maximum per axis, planted in turn at every place bounds_partial (csrc/lbvh.h) reads
    from (voxel_exact.bounds_slots): the first and the last point, the four slots of the unrolled loop and the tail
    where the size has them.  The centre of the lattice cloud is (S / n) rounded once, S exact, bit for bit; the centre
    of a non-negative random cloud is within 1 ulp of math.fsum's (two fp64 sums of non-negative terms differ by at most
    n * 2^-53 relatively; both quotients are rounded to float: equal or adjacent)."""
    pts = bounds_cloud(n)
    dev = cuda(pts)
    check_bounds(eng, pts, dev)
    lo, hi = np.float32([-1.0, -2.0, -3.0]), np.float32([100.0, 101.0, 102.0])
    for place, idx in vx.bounds_slots(n).items():
        for extreme in (lo, hi):
            keep = pts[idx].copy()
            pts[idx] = extreme
            dev[idx] = torch.from_numpy(extreme).cuda()
            mn, mx, _ = eng.compute_bounds(dev)
            assert np.array_equal(mn if extreme is lo else mx, extreme), place
            check_bounds(eng, pts, dev)
            pts[idx] = keep
            dev[idx] = torch.from_numpy(keep).cuda()
    check_bounds(eng, pts, pts)                                             # host arrays
    rnd = np.random.default_rng(n + 1).random((n, 3), dtype=np.float32)
    ce = check_bounds(eng, rnd, cuda(rnd), centre=None)
    want = np.array([math.fsum(rnd[:, d].tolist()) / n for d in range(3)])
    worst = vx.ulps(ce, want).max()
    print("centre: %.3g ulp" % worst)
    assert worst <= 1


def test_nan_coordinates_do_not_reach_the_bounds(eng):
    n = 786433                                                              # the unrolled loop and a tail
    pts = bounds_cloud(n)
    rng = np.random.default_rng(9)
    pts[rng.integers(0, n, size=n // 100), rng.integers(0, 3, size=n // 100)] = np.nan
    for idx in vx.bounds_slots(n).values():
        pts[idx, idx % 3] = np.nan
    assert np.isnan(pts).any(axis=0).all()
    mn, mx, _ = eng.compute_bounds(cuda(pts))
    assert np.array_equal(mn, np.fmin.reduce(pts, axis=0)) and np.array_equal(mx, np.fmax.reduce(pts, axis=0))
    assert np.isfinite(mn).all() and np.isfinite(mx).all()


def test_an_empty_cloud_has_zero_bounds(eng):
    mn, mx, ce = eng.compute_bounds(np.empty((0, 3), np.float32))
    assert not mn.any() and not mx.any() and not ce.any()
    mn, mx, ce = eng.compute_bounds(torch.empty((0, 3), dtype=torch.float32, device="cuda"))
    assert not mn.any() and not mx.any() and not ce.any()
