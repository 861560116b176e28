"""The construction of tests/voxel_exact.py, held on the CPU so that a failure of tests/test_gpu_voxel_exact.py can only
mean the kernels: the numpy restatement is the oracle bit for bit on every lattice cloud, the clouds' fp64 sums do not
depend on the order of addition, every case has the key bits it declares, and the bounds that the GPU tests assert on
the random family hold for the oracle against the restatement."""
import numpy as np
import pytest

import voxel_exact as vx
from oracle import oracle as orc


@pytest.mark.parametrize("case_id", vx.LATTICE_IDS)
def test_restated_is_the_oracle_bit_for_bit_on_the_lattice(case_id):
    c, pts, nrm, col, ref = vx.lattice(case_id)
    rp, rn, rc = orc.voxel_downsample(pts, c["voxel"], nrm, col)
    assert len(rp) == len(ref["points"]) == len(ref["count"]) and ref["count"].sum() == c["n"]
    np.testing.assert_array_equal(ref["points"], rp)
    np.testing.assert_array_equal(ref["colors"], rc)
    assert (rc[:, 0] == 1.0).all()
    nan = np.isnan(ref["normals"])
    assert np.array_equal(nan, np.isnan(rn))
    assert nan[ref["inverse"][0]].all() or not c["cancel"]                   # the voxel whose normals cancel
    assert vx.ulps(rn, ref["normals"]).max() <= 4                            # (the bound of the GPU test, on the oracle)
    # every voxel stays inside its cell: the restated cells are the builder's
    assert ref["bits"] == c["bits"] and sum(c["bits"]) == c["plan"][1]


@pytest.mark.parametrize("case_id", vx.LATTICE_IDS)
def test_lattice_sums_do_not_depend_on_the_order_of_addition(case_id):
    """the premise: forward and backward fp64 summation of every voxel agree bitwise (and so does pairwise summation)"""
    c, pts, nrm, col, ref = vx.lattice(case_id)
    inv, m = ref["inverse"], len(ref["count"])
    for a in (pts, nrm, col):
        a64 = a.astype(np.float64)
        fwd, bwd = np.zeros((m, 3)), np.zeros((m, 3))
        np.add.at(fwd, inv, a64)
        np.add.at(bwd, inv[::-1], a64[::-1])
        assert np.array_equal(fwd, bwd)
        order = np.argsort(inv, kind="stable")
        starts = np.concatenate([[0], np.cumsum(ref["count"])[:-1]])
        assert np.array_equal(np.add.reduceat(a64[order], starts, axis=0), fwd)


def test_the_cases_hold_the_shapes_their_rows_name():
    def counts(case_id):
        return vx.lattice(case_id)[4]["count"]
    for cid in ("a-n1", "a-n7", "b-n9", "b-n64", "b-n65", "b-n200"):
        assert len(counts(cid)) == 1                                         # one voxel, one run
    # row c: every voxel the grid can hold / the lowest and the highest alone
    assert len(counts("c-4bits-all")) == 3 and len(counts("c-5bits-all")) == 7
    assert len(counts("c-4bits-ends")) == 2 and len(counts("c-5bits-ends")) == 2
    # row d at 12 and 13 bits: a run with a full mask, a run with its two end voxels alone
    for cid, L in (("d-12bits", 4), ("d-13bits", 5)):
        c, pts, _, _, ref = vx.lattice(cid)
        z = np.floor((ref["points"][:, 2] - c["base"]) / c["voxel"] + 0.5).astype(int)   # (the mean lies within its cell)
        w = 1 << L
        assert set(z[(z >> L) == 1]) == set(range(w, 2 * w)) and set(z[(z >> L) == 2]) == {2 * w, 3 * w - 1}
    # rows d / e: 2^(bits - L) against n / 8
    assert 2048 // 8 == 256 and 2047 // 8 < 256
    # row f: more than 16 points per voxel; a voxel's run spans the scan tile's edge at 2048; n % 8 != 0
    for cid in ("f-n200", "f-n2049"):
        cnt = counts(cid)
        assert cnt.sum() > 16 * len(cnt)
    assert 2048 not in np.cumsum(counts("f-n2049")) and 2049 % 8 != 0
    # rows a, e, g, j, k: at most 16 points per voxel (a thread each)
    for cid in ("a-n1", "a-n7", "e-n2047", "g-16bits", "g-24bits", "g-32bits", "j-21bits", "k-24bits"):
        cnt = counts(cid)
        assert cnt.sum() <= 16 * len(cnt) and (cid.startswith("a") or cnt.max() >= 2)
    # row g: run heads on both sides of the tile's edge
    for cid in ("g-16bits", "g-24bits", "g-32bits"):
        heads = np.concatenate([[0], np.cumsum(counts(cid))])
        assert ((heads >= 2040) & (heads < 2048)).any() and ((heads >= 2048) & (heads < 2056)).any()
    # row m: n / 8 is exactly the number of possible runs
    assert 524288 // 8 == 1 << 16


@pytest.mark.parametrize("case_id", vx.RANDOM_IDS + ["faces"])
def test_the_random_family_bounds_hold_for_the_oracle(case_id):
    """1 ulp on points and colours, 4 * 2^-24 on normals (tests/test_gpu_voxel_exact.py derives them), the oracle
    against the restatement -- were the reference itself outside a bound, the derivation would be wrong"""
    c, pts, nrm, col = vx.random_case(case_id)
    ref = vx.restated(pts, c["voxel"], nrm, col)
    rp, rn, rc = orc.voxel_downsample(pts, c["voxel"], nrm, col)
    assert len(rp) == len(ref["points"])
    assert ref["bits"] == c["bits"] and sum(c["bits"]) == c["plan"][1]
    assert vx.ulps(rp, ref["points"]).max() <= 1
    assert vx.ulps(rc, ref["colors"]).max() <= 1
    assert ref["normal_length"].min() >= 1e-3                                # (else: another seed, not another bound)
    assert np.abs(rn - ref["normals"]).max() <= 4 * 2.0 ** -24
    assert (pts >= 0).all() and (col >= 0).all()                             # no cancellation in the sums


@pytest.mark.parametrize("n,places", [(1, ""), (255, ""), (256, ""), (257, ""), (262144, ""), (262145, "tail"), (786432, "tail"),
                                      (786433, "u0 u1 u2 u3 tail"), (1048577, "u0 u1 u2 u3 tail")])
def test_bounds_slots_name_every_place_of_the_reduction(n, places):
    """the sizes of the bounds test: one block; the 1024-block cap; the first size with a second point per thread; the
    largest without and the first with the four-way loop; a size with that loop and a tail"""
    assert n in vx.BOUNDS_SIZES
    s = vx.bounds_slots(n)
    stride = min(1024, (n + 255) // 256) * 256
    assert set(s) == {"first", "last"} | set(places.split())
    assert all(0 <= i < n for i in s.values()) and s["first"] == 0 and s["last"] == n - 1
    if "u0" in s:
        assert [s["u%d" % k] - s["u0"] for k in range(4)] == [0, stride, 2 * stride, 3 * stride] and s["u3"] < n
    if "tail" in s:
        i = s["tail"] % stride                                                # the thread's walk reaches it one at a time
        while i + 3 * stride < n:
            i += 4 * stride
        assert i <= s["tail"] and (s["tail"] - i) % stride == 0
