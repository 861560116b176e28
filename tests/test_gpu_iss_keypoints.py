"""GPU: geometry::keypoint::ComputeISSKeypoints and PointCloud::SelectByMask (include/mi_icp.h mi_icp_iss_keypoints /
mi_icp_select_by_mask, csrc/iss.h) held to the CPU restatement of tests/iss_exact.py.

The mask is a discontinuous function of fp32 arithmetic, so everything discrete is held exactly and only the eigenvalues
get a tolerance:
  rows and suppression   from the engine's own saliency, the restated step 5 over restated rows gives mask_out, everywhere
  counts and gates       the restated rows' lengths are counts_out; from the engine's own eigenvalues and counts the
                         restated step 4 in numpy float32 gives saliency_out bit for bit
  eigenvalues            against the fp64 restatement, at most 4x the deviation of the fp32 CPU restatement
                         (fragment_every3rd: CPU fp32 9.3e-6 measured; the test prints the engine's figure and the ratio)
  end to end             mask_out equals the fp64 restatement's outside the undecided set (at most 10 % of the points)"""
import os

import numpy as np
import pytest
import torch

import iss_exact as ix
import knn_exact as kx

pytestmark = pytest.mark.gpu

F32 = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULTS = dict(salient_radius=0.0, non_max_radius=0.0, gamma_21=0.975, gamma_32=0.975, min_neighbors=5, max_neighbors=100)
CAPACITY_EDGES = [1, 5, 32, 33, 64, 65, 100]


@pytest.fixture(scope="module")
def eng():
    from cupoch_amd.engine import Engine
    e = Engine(0)
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _fixture(name):
    return np.load(os.path.join(GOLDEN, name))["points"].astype(F32)


def _run(eng, pts, device=True, **kw):
    a = dict(DEFAULTS, **kw)
    mask, m, radii, sal, eig, cnt = eng.iss_keypoints(_dev(pts) if device else pts, want_response=True, **a)
    return dict(mask=_np(mask), m=m, radii=radii, saliency=_np(sal), eig=_np(eig), counts=_np(cnt), args=a)


def _check_discrete(pts, out, case):
    """checks 1 and 2 of the module's list, at every point"""
    a = out["args"]
    rs, rn = F32(out["radii"][0]), F32(out["radii"][1])
    indptr, idx = ix.rows(pts, rs, a["max_neighbors"])
    cnt = np.diff(indptr).astype(np.int32)
    bad = np.flatnonzero(out["counts"] != cnt)
    assert not len(bad), "%s: %d counts differ, first at %d (%d vs %d)" % (case, len(bad), bad[0], out["counts"][bad[0]], cnt[bad[0]])
    sal = ix.gates(out["eig"], out["counts"], a["min_neighbors"], a["gamma_21"], a["gamma_32"])
    assert out["saliency"].dtype == F32 and sal.dtype == F32
    bad = np.flatnonzero(sal.view(np.uint32) != out["saliency"].view(np.uint32))
    assert not len(bad), "%s: %d saliencies differ from the gates of the engine's eigenvalues, first at %d" % (case, len(bad), bad[0])
    few = out["counts"] < a["min_neighbors"]
    assert (out["eig"][few] == -1).all(), "%s: eigenvalues where there are too few neighbours" % case
    mask = ix.suppress(out["saliency"], *ix.rows(pts, rn, a["max_neighbors"]))
    bad = np.flatnonzero(mask != (out["mask"] != 0))
    assert not len(bad), "%s: %d mask entries differ, first at %d" % (case, len(bad), bad[0])
    assert set(np.unique(out["mask"]).tolist()) <= {0, 1} and out["m"] == int(mask.sum()), case


# ---- rows, counts, gates and suppression, exact ---------------------------------------------------------------------
def _anisotropic_lattice(seed):
    """every site of a 30 x 20 x 12 block with steps of 1, 2 and 3 lattice units, shuffled: interior points have one
    and the same neighbourhood -- saliencies tie exactly -- and whole shells of points lie at one distance"""
    g = np.stack(np.meshgrid(np.arange(30), 2 * np.arange(20), 3 * np.arange(12), indexing="ij"), -1).reshape(-1, 3)
    g = g - g.max(0) // 2
    return (g[np.random.default_rng(seed).permutation(len(g))] * kx.SCALE).astype(F32)


@pytest.mark.parametrize("max_neighbors", CAPACITY_EDGES)
def test_lattice_with_ties_at_the_radius_and_in_saliency(eng, max_neighbors):
    pts = _anisotropic_lattice(max_neighbors)
    # radii of whole lattice steps: points at exactly r (d2 == r*r, exact in fp32) are outside, whole shells tie inside
    for steps_s, steps_n in [(5, 3), (6, 4), (10, 5)]:
        out = _run(eng, pts, salient_radius=steps_s * kx.SCALE, non_max_radius=steps_n * kx.SCALE, min_neighbors=3,
                   max_neighbors=max_neighbors)
        _check_discrete(pts, out, "lattice r=%d/%d max_neighbors=%d" % (steps_s, steps_n, max_neighbors))
        if max_neighbors == 100 and steps_s == 6:
            sal = out["saliency"]
            top = sal[sal >= 0]
            assert len(top) and (top == top.max()).sum() > 100, "the lattice lost its tied saliencies"
            assert out["m"] > 100, "tied neighbours must both stay"


@pytest.mark.parametrize("max_neighbors", CAPACITY_EDGES)
@pytest.mark.parametrize("cloud", ["graded", "duplicates", "sheet"])
def test_dyadic_clouds_at_every_capacity(eng, cloud, max_neighbors):
    pts = {"graded": kx.cloud_graded, "duplicates": kx.cloud_duplicates, "sheet": kx.cloud_sheet}[cloud](20_000, seed=max_neighbors + 3)
    # whole steps: ties at the radius; a density at which some rows are truncated and some are not
    from scipy.spatial import cKDTree
    tree = cKDTree(pts.astype(np.float64))
    q = pts[:400].astype(np.float64)
    steps = next((s for s in range(2, 200) if tree.query_ball_point(q, s * kx.SCALE, return_length=True).mean() >= max(6, 0.8 * max_neighbors)), 200)
    out = _run(eng, pts, salient_radius=steps * kx.SCALE, non_max_radius=max(1, (2 * steps) // 3) * kx.SCALE,
               max_neighbors=max_neighbors, min_neighbors=min(5, max_neighbors))
    _check_discrete(pts, out, "%s steps=%d max_neighbors=%d" % (cloud, steps, max_neighbors))
    assert out["counts"].max() == max_neighbors            # some rows are truncated ...
    if max_neighbors > 1:                                  # ... and some are not (a row of one holds the point itself)
        assert (out["counts"] < max_neighbors).any()


@pytest.mark.parametrize("name", ["fragment_every3rd.npz", "fragment_points.npz"])
def test_fragment_scans_with_default_arguments(eng, name):
    pts = _fixture(name)
    out = _run(eng, pts)
    _check_discrete(pts, out, name)
    assert 0 < out["m"] < len(pts) // 10


def test_two_million_points(eng):
    rng = np.random.default_rng(7)
    centres = rng.uniform(-40, 40, (300, 3))
    pts = np.concatenate([centres[rng.integers(0, 300, 1_900_000)] + rng.normal(0, 0.8, (1_900_000, 3)) * [1.0, 0.6, 0.3],
                          rng.uniform(-45, 45, (100_000, 3))]).astype(F32)
    pts = pts[rng.permutation(len(pts))]
    out = _run(eng, pts, salient_radius=0.2, non_max_radius=0.14)
    _check_discrete(pts, out, "2M blobs")
    assert out["m"] > 0


# ---- eigenvalues within the CPU's own fp32 error, the mask against fp64 -----------------------------------------------
def test_eigenvalues_and_mask_against_fp64_on_the_fragment(eng):
    pts = _fixture("fragment_every3rd.npz")
    out = _run(eng, pts)
    ref = ix.iss(pts, dtype=np.float64, centred=True)
    cpu = ix.iss(pts, dtype=F32, centred=True)
    # the radii: an fp64 sum of fp32 terms, the order is the only freedom
    np.testing.assert_allclose(out["radii"], ref["radii"], rtol=1e-6)
    np.testing.assert_allclose(out["radii"][0] / out["radii"][1], 1.5, rtol=1e-6)
    assert np.array_equal(out["counts"], ref["counts"])
    have = (ref["eig"] != -1).any(1)
    assert np.array_equal(have, (out["eig"] != -1).any(1)) and np.array_equal(have, (cpu["eig"] != -1).any(1))
    dev_gpu = float(np.abs(out["eig"][have].astype(np.float64) - ref["eig"][have]).max())
    dev_cpu = float(np.abs(cpu["eig"][have].astype(np.float64) - ref["eig"][have]).max())
    print("eigenvalues: largest deviation from fp64  engine %.3g  CPU fp32 %.3g  ratio %.2f" % (dev_gpu, dev_cpu, dev_gpu / dev_cpu))
    assert dev_gpu <= 4.0 * dev_cpu, (dev_gpu, dev_cpu)
    # end to end: the mask outside the undecided set
    und = ix.undecided(ref)
    print("undecided: %.2f %% of the points; engine differs from fp64 at %d points, %d of them outside"
          % (100.0 * und.mean(), int(((out["mask"] != 0) != ref["mask"]).sum()), int((((out["mask"] != 0) != ref["mask"]) & ~und).sum())))
    assert und.mean() <= 0.10
    assert not (((out["mask"] != 0) != ref["mask"]) & ~und).any()
    assert not ((cpu["mask"] != ref["mask"]) & ~und).any()
    # the deviation from the reference's arithmetic, as DESIGN.md records it
    raw64 = ix.iss(pts, dtype=np.float64, centred=False)
    raw32 = ix.iss(pts, dtype=F32, centred=False)
    assert [int(r["mask"].sum()) for r in (raw64, ref, raw32, cpu)] == [786, 766, 1141, 763]
    assert [int((r["mask"] != raw64["mask"]).sum()) for r in (ref, raw32, cpu)] == [20, 1315, 23]


# ---- edges ----------------------------------------------------------------------------------------------------------
def test_empty_tiny_and_degenerate_clouds(eng):
    mask, m, radii = eng.iss_keypoints(np.zeros((0, 3), F32))
    assert len(mask) == 0 and m == 0
    out = _run(eng, np.random.default_rng(0).random((4, 3), dtype=F32), salient_radius=2.0, non_max_radius=1.0)
    assert out["m"] == 0 and (out["saliency"] == -1).all() and (out["counts"] == 4).all()      # n < min_neighbors
    same = np.full((5000, 3), 0.25, F32)
    out = _run(eng, same, salient_radius=0.1, non_max_radius=0.1)
    assert out["m"] == 0 and (out["counts"] == 100).all() and (out["eig"] == -1).all()           # zero covariance
    out = _run(eng, same)                                                                         # resolution 0: radii 0
    assert out["radii"] == (0.0, 0.0) and out["m"] == 0 and (out["counts"] == 0).all()


def test_collinear_and_coplanar_clouds(eng):
    """exact lines and planes on the lattice: e0 is 0 or a rounding error of either sign; the gates let it through when
    e1 > 0, saliency = e0, and only e0 >= 0 with nothing positive in the row is a keypoint"""
    t = np.arange(-300, 301)
    line = (np.stack([t, t * 0 + 7, t * 0 - 5], 1) * kx.SCALE).astype(F32)
    out = _run(eng, line, salient_radius=20.5 * kx.SCALE, non_max_radius=10.5 * kx.SCALE)
    _check_discrete(line, out, "line")
    inner = out["counts"] == 41
    assert inner.any() and (out["eig"][inner, 0] == 0).all() and (out["eig"][inner, 1] == 0).all()
    assert (out["saliency"][inner] == -1).all()          # e0 / e1 = 0 / 0: NaN compares false
    g = np.stack(np.meshgrid(np.arange(-40, 41), np.arange(-40, 41), indexing="ij"), -1).reshape(-1, 2)
    plane = (np.column_stack([g[:, 0], 2 * g[:, 1], g[:, 0] + g[:, 1]]) * kx.SCALE).astype(F32)
    out = _run(eng, plane, salient_radius=10.5 * kx.SCALE, non_max_radius=5.5 * kx.SCALE)
    _check_discrete(plane, out, "plane")
    passed = out["saliency"] != -1
    assert passed.any() and (np.abs(out["saliency"][passed]) < 1e-5).all()
    assert not (out["mask"][out["saliency"] < 0]).any()


def test_explicit_radii_equal_computed_ones_and_one_zero_replaces_both(eng):
    pts = _fixture("fragment_every3rd.npz")
    auto = _run(eng, pts)
    rs, rn = auto["radii"]
    expl = _run(eng, pts, salient_radius=rs, non_max_radius=rn)
    assert expl["radii"] == (rs, rn) and expl["mask"].tobytes() == auto["mask"].tobytes()
    assert expl["saliency"].tobytes() == auto["saliency"].tobytes()
    for kw in (dict(salient_radius=0.1), dict(non_max_radius=0.1)):
        one = _run(eng, pts, **kw)
        assert one["radii"] == (rs, rn) and one["mask"].tobytes() == auto["mask"].tobytes()


def test_errors_leave_the_context_usable(eng):
    from cupoch_amd._lib import MiIcpError
    pts = _dev(np.random.default_rng(1).random((2000, 3), dtype=F32))
    for kw in (dict(max_neighbors=0), dict(max_neighbors=101), dict(max_neighbors=-3), dict(salient_radius=-1.0),
               dict(non_max_radius=float("nan")), dict(salient_radius=float("inf"))):
        with pytest.raises(MiIcpError):
            eng.iss_keypoints(pts, **dict(DEFAULTS, **kw))
    with pytest.raises(MiIcpError):
        eng.select_by_mask(pts, np.ones(1999, bool))
    with pytest.raises(MiIcpError):
        eng.select_by_mask(pts, np.ones(2001, bool))
    mask, m, _ = eng.iss_keypoints(pts)
    assert len(mask) == 2000 and int(_np(mask).sum()) == m
    p2, _, _ = eng.select_by_mask(pts, mask)
    assert len(p2) == m


def test_memory_kinds_determinism_and_the_callers_target(eng):
    from cupoch_amd.engine import Engine
    pts = _fixture("fragment_every3rd.npz")
    rng = np.random.default_rng(9)
    tgt, q = rng.random((20_000, 3), dtype=F32), rng.random((3000, 3), dtype=F32)
    eng.set_target(_dev(tgt))
    before = eng.search_knn(_dev(q), 8)
    d = _run(eng, pts)
    h = _run(eng, pts, device=False)
    after = eng.search_knn(_dev(q), 8)
    for x, y in zip(before, after):
        assert np.array_equal(_np(x), _np(y))
    d2 = _run(eng, pts)
    e2 = Engine(0)
    try:
        d3 = _run(e2, pts)
    finally:
        e2.close()
    for key in ("mask", "saliency", "eig", "counts"):
        assert d[key].tobytes() == h[key].tobytes() == d2[key].tobytes() == d3[key].tobytes(), key
    assert d["radii"] == h["radii"] == d3["radii"] and d["m"] == h["m"]
    mask, _, _ = eng.iss_keypoints(pts)
    assert isinstance(mask, np.ndarray) and mask.dtype == np.uint8
    mask, _, _ = eng.iss_keypoints(_dev(pts))
    assert mask.is_cuda and mask.dtype == torch.uint8


# ---- SelectByMask ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device", [True, False])
def test_select_by_mask_against_boolean_indexing(eng, device):
    rng = np.random.default_rng(5)
    n = 100_003
    pts, nrm, col = (rng.random((n, 3), dtype=F32) for _ in range(3))
    mask = rng.random(n) < 0.3
    put = _dev if device else (lambda a: a)
    for invert in (False, True):
        want = mask != invert
        p, nn, c = eng.select_by_mask(put(pts), put(mask), invert, put(nrm), put(col))
        assert np.array_equal(_np(p), pts[want]) and np.array_equal(_np(nn), nrm[want]) and np.array_equal(_np(c), col[want])
        p, nn, c = eng.select_by_mask(put(pts), put(mask.astype(np.uint8) * 7), invert)
        assert np.array_equal(_np(p), pts[want]) and nn is None and c is None
    for m in (np.zeros(n, bool), np.ones(n, bool)):
        p, _, _ = eng.select_by_mask(put(pts), put(m))
        assert np.array_equal(_np(p), pts[m])
    p, _, _ = eng.select_by_mask(np.zeros((0, 3), F32), np.zeros(0, bool))
    assert len(p) == 0


# ---- both front ends ------------------------------------------------------------------------------------------------
def test_both_front_ends_return_the_abis_mask(eng):
    from cupoch_amd import geometry, pybind, utility
    pts = _fixture("fragment_every3rd.npz")
    rng = np.random.default_rng(2)
    nrm, col = rng.random(pts.shape, dtype=F32), rng.random(pts.shape, dtype=F32)
    abi = _run(eng, pts)["mask"] != 0
    abi5 = _run(eng, pts, salient_radius=0.05, non_max_radius=0.03, gamma_21=0.9, gamma_32=0.8, min_neighbors=7, max_neighbors=40)["mask"] != 0
    for mod, util in ((geometry, utility), (pybind.geometry, pybind.utility)):
        pcl = mod.PointCloud()
        pcl.points = util.Vector3fVector(pts)
        pcl.normals = util.Vector3fVector(nrm)
        pcl.colors = util.Vector3fVector(col)
        kp, mask = mod.keypoint.compute_iss_keypoints(pcl)
        assert type(mask).__name__ == "BoolVector"
        got = np.asarray(mask.cpu()).astype(bool)
        assert np.array_equal(got, abi)
        assert np.array_equal(np.asarray(kp.points.cpu()), pts[abi]) and np.array_equal(np.asarray(kp.normals.cpu()), nrm[abi])
        assert np.array_equal(np.asarray(kp.colors.cpu()), col[abi])
        kp5, mask5 = mod.keypoint.compute_iss_keypoints(pcl, salient_radius=0.05, non_max_radius=0.03, gamma_21=0.9,
                                                        gamma_32=0.8, min_neighbors=7, max_neighbors=40)
        assert np.array_equal(np.asarray(mask5.cpu()).astype(bool), abi5) and len(kp5.points) == int(abi5.sum())
        rest = pcl.select_by_mask(mask, invert=True)
        assert np.array_equal(np.asarray(rest.points.cpu()), pts[~abi])
        assert np.array_equal(np.asarray(pcl.select_by_mask(util.BoolVector(abi)).colors.cpu()), col[abi])
        assert len(pcl.select_by_mask(util.BoolVector(abi[:-1])).points) == 0          # another size: logged, empty
        kp0, mask0 = mod.keypoint.compute_iss_keypoints(mod.PointCloud())
        assert len(kp0.points) == 0 and len(mask0) == 0


def test_cpp_surface(eng, tmp_path):
    import json
    import subprocess
    from cupoch_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _lib.build()
    cpp = os.path.join(root, "cupoch_amd", "cpp")
    subprocess.check_call(["make", "-s", "-C", cpp])
    exe = str(tmp_path / "test_iss_keypoints")
    libdir = os.path.join(root, "cupoch_amd", "lib")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(cpp, "include"), "-I" + os.path.join(root, "include"),
                           "-I/opt/rocm/include", os.path.join(root, "tests", "cpp", "test_iss_keypoints.cpp"),
                           "-o", exe, "-L" + libdir, "-lcupoch_amd", "-lmi_icp", "-L/opt/rocm/lib",
                           "-lamdhip64", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    pts = _fixture("fragment_every3rd.npz")
    src, dst = str(tmp_path / "points.f32"), str(tmp_path / "mask.u8")
    pts.tofile(src)
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    r = json.loads(out.stdout.strip().splitlines()[-1])
    abi = _run(eng, pts)
    assert np.array_equal(np.fromfile(dst, np.uint8), abi["mask"])
    assert r["points"] == len(pts) and r["keypoints"] == abi["m"] and r["rest"] == len(pts) - abi["m"]
    assert r["gathered_in_order"] and r["same_twice"] and r["empty_cloud_empty"] and r["max_neighbors_101_throws"]
    assert r["wrong_size_points"] == 0
    assert "[SelectByMask] The point size should be equal to the mask size." in out.stderr
    assert "[ComputeISSKeypoints] Input PointCloud is empty!" in out.stderr
