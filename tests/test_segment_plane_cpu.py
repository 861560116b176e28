"""PointCloud::SegmentPlane without a GPU: the restatement of tests/segment_plane_exact.py on the reference's own test,
the sampler's known answers and properties, and the surface under the reference's names."""
import ctypes
import inspect
import os
import re
from fractions import Fraction

import numpy as np

import segment_plane_exact as sx

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# tests/geometry/pointcloud.cpp:659-674 of the reference (SegmentPlaneKnownPlane)
FIVE = np.array([[1, 1, -1], [2, 2, -5], [-1, -1, 1], [-2, -2, 3], [10, 10, -21]], F32)


def test_the_references_five_points_come_back_for_every_seed():
    # all five have x = y; 1..4 are collinear (z = -2x - 1), so the four triples without point 0 are invalid and the
    # six with it span x = y: every hypothesis is either invalid or holds all five, and if all ten iterations are
    # invalid the zero plane holds all five as well
    saw_invalid = False
    for seed in range(100):
        r = sx.run(FIVE, 0.01, 3, 10, seed)
        assert r.inliers.tolist() == [0, 1, 2, 3, 4], seed
        assert set(r.counts[r.valid].tolist()) <= {5} and (r.counts[~r.valid] == 0).all()
        saw_invalid |= bool((~r.valid).any())
        if r.best < 0:
            assert not r.valid.any() and not r.ransac.any()
        else:
            assert r.best == int(np.flatnonzero(r.valid)[0]) or len(r.tied) > 1
            n = r.ransac[:3].astype(np.float64)
            assert abs(abs(n[0]) - np.sqrt(0.5)) < 1e-7 and n[0] == -n[1] and n[2] == 0 and r.ransac[3] == 0
        p = r.plane          # the refit spans x = y as well; its largest determinant is det_x or det_y
        assert abs(abs(p[0]) - np.sqrt(0.5)) < 1e-12 and abs(p[0] + p[1]) < 1e-12 and abs(p[2]) < 1e-12 and abs(p[3]) < 1e-12
    assert saw_invalid
    # with a single iteration the four invalid triples (4 of 10 equally likely) do turn up: the degenerate rule
    assert any(sx.run(FIVE, 0.01, 3, 1, s).best < 0 and len(sx.run(FIVE, 0.01, 3, 1, s).inliers) == 5 for s in range(40))


def test_arguments_as_the_reference_treats_them():
    for ransac_n, pts in [(2, FIVE), (0, FIVE), (3, FIVE[:2]), (6, FIVE), (3, FIVE[:0])]:
        r = sx.run(pts, 0.01, ransac_n, 10, 1)
        assert len(r.inliers) == 0 and not r.plane.any() and r.best == -1
    r = sx.run(FIVE, 0.01, 5, 10, 1)         # ransac_n > 3 still samples three
    assert r.inliers.tolist() == [0, 1, 2, 3, 4]
    r = sx.run(FIVE, 0.01, 3, 0, 1)          # no iterations: the zero plane, everything within a positive threshold
    assert r.best == -1 and r.inliers.tolist() == [0, 1, 2, 3, 4]
    r = sx.run(FIVE, 0.0, 3, 10, 1)          # strict <
    assert len(r.inliers) == 0 and not r.plane.any()


def test_sampler_known_answers():
    # splitmix64's published first outputs for seed 0
    assert [sx.u(0, j) for j in range(3)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    known = {(0, 0, 3): (2, 0, 1), (0, 0, 5): (4, 1, 0), (0, 1, 5): (4, 0, 1), (7, 3, 4): (1, 0, 3),
             (1, 0, 1000): (566, 746, 971), (42, 7, 113662): (8303, 68176, 70450),
             (12345, 4096, 10_000_000): (8839670, 1703258, 948242),
             (2 ** 64 - 1, 99, 2 ** 31): (2060665127, 2006489669, 1711170005)}
    for (seed, t, n), tri in known.items():
        assert sx.triple(seed, t, n) == tri, (seed, t, n)
    # by hand for (0, 0, 3): u0 / 2^64 = 0.883.. -> i0 = 2; u1 / 2^64 = 0.431.. -> below(u1, 2) = 0 < 2 stays 0;
    # below(u2, 1) = 0 >= min = 0 -> 1, 1 < max = 2 stays 1
    assert sx.below(sx.u(0, 0), 3) == 2 and sx.below(sx.u(0, 1), 2) == 0 and sx.below(sx.u(0, 2), 1) == 0


def test_sampler_indices_are_distinct_and_cover():
    for n in (3, 4, 2 ** 31):
        for seed in (0, 1, 2 ** 63 + 5):
            for t in range(2000):
                tri = sx.triple(seed, t, n)
                assert len(set(tri)) == 3 and min(tri) >= 0 and max(tri) < n, (n, seed, t, tri)
    for n in (3, 4, 7, 50):
        seen = [set(), set(), set()]
        for t in range(3000):
            for k, i in enumerate(sx.triple(9, t, n)):
                seen[k].add(i)
        assert all(s == set(range(n)) for s in seen), n       # every index, in every position
    # no state: iteration t alone determines the triple
    assert tuple(sx.triples(5, 18, 1000)[17]) == sx.triple(5, 17, 1000)


def test_distance_is_the_fma_chain_rounded_once_per_step():
    rng = np.random.default_rng(0)
    pts = rng.uniform(-3, 3, (400, 3)).astype(F32)
    planes, valid = sx.triangle_planes(pts, sx.triples(3, 8, len(pts)))
    assert valid.all()
    for pl in planes:
        quick, exact = sx.distances(pl, pts), sx.distances(pl, pts, exact=True)
        assert (quick == exact).mean() > 0.99          # the fp64 shortcut rounds twice: rarely a last place apart
        assert np.abs(quick.astype(np.float64) - exact).max() <= 2.0 ** -21
        n64 = np.abs(pts.astype(np.float64) @ pl[:3].astype(np.float64) + float(pl[3]))
        assert np.abs(exact - n64).max() < 2e-6
    # the rounding helper: halves go to even, subnormals keep their spacing
    assert sx._round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == 1
    assert sx._round_f32(Fraction(1) + Fraction(3, 2 ** 24)) == Fraction(1) + Fraction(1, 2 ** 22)
    assert sx._round_f32(Fraction(3, 2 ** 150)) == Fraction(1, 2 ** 148)
    for v in rng.standard_normal(200):
        assert float(sx._round_f32(Fraction(float(v)))) == float(F32(v))


def test_selection_prefers_count_then_error_sum_then_iteration():
    # a slab and clutter: the winner holds the most inliers of any valid hypothesis, and the list is its own
    rng = np.random.default_rng(4)
    slab = np.column_stack([rng.uniform(-2, 2, (600, 2)), rng.normal(0, 0.004, 600)])
    pts = np.concatenate([slab, rng.uniform(-2, 2, (300, 3))]).astype(F32)
    r = sx.run(pts, 0.02, 3, 60, 11)
    assert r.best >= 0 and r.count == r.counts[r.valid].max() == len(r.inliers)
    assert r.best == int(np.flatnonzero(r.valid & (r.counts == r.count))[0]) or len(r.tied) > 1
    assert abs(abs(r.plane[2]) - 1) < 1e-3 and r.plane[np.argmax(np.abs(r.plane[:3]))] > 0


# ---- the surface ------------------------------------------------------------------------------------------------------
def test_library_exports_the_entry_point_and_lib_binds_it():
    from cupoch_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    assert re.search(r"MI_ICP_API int mi_icp_segment_plane\(", hdr)
    res, args = _lib.SIGNATURES["mi_icp_segment_plane"]
    assert len(args) == 14 and args[6] is ctypes.c_uint64
    _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "mi_icp_segment_plane")


def test_python_surface_has_the_references_names():
    from cupoch_amd import geometry
    from cupoch_amd.engine import Engine
    ps = inspect.signature(geometry.PointCloud.segment_plane).parameters
    assert list(ps)[1:] == ["distance_threshold", "ransac_n", "num_iterations", "seed"]
    assert ps["distance_threshold"].default == 0.01 and ps["ransac_n"].default == 3 and ps["num_iterations"].default == 100
    assert ps["seed"].default is None
    assert list(inspect.signature(Engine.segment_plane).parameters)[1:] == [
        "points", "distance_threshold", "ransac_n", "num_iterations", "seed"]


def test_cpp_surface_declares_the_reference_signature():
    h = open(os.path.join(ROOT, "cupoch_amd", "cpp", "include", "cupoch", "geometry", "pointcloud.h")).read()
    assert re.search(r"std::tuple<Eigen::Vector4f, utility::device_vector<size_t>> SegmentPlane\(float distance_threshold = 0.01,"
                     r"\s+size_t ransac_n = 3,\s+size_t num_iterations = 100\) const;", h)
    py = open(os.path.join(ROOT, "cupoch_amd", "cpp", "src", "pybind_module.cpp")).read()
    assert '"segment_plane"' in py and '"distance_threshold"_a = 0.01f, "ransac_n"_a = 3, "num_iterations"_a = 100' in py
