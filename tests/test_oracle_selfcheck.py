"""Oracle self-checks: exact kd-tree vs brute force vs the reference's own
FLANN CPU index (oracle/_ref), and ICP self-consistency (recover a known
T_gt) -- the part of the path the reference's tests leave unpinned."""
import numpy as np
import pytest

from conftest import make_pair
from oracle import oracle as orc


def test_kdtree_equals_bruteforce():
    rng = np.random.default_rng(0)
    tgt = rng.random((3000, 3), dtype=np.float32)
    qry = rng.random((500, 3), dtype=np.float32)
    r1, i1, d1 = orc.search_knn(tgt, qry, 7)
    r2, i2, d2 = orc.search_bruteforce(tgt, qry, 7)
    assert r1 == r2
    np.testing.assert_array_equal(i1, i2)
    np.testing.assert_array_equal(d1, d2)
    r1, i1, d1 = orc.search_radius(tgt, qry, 0.05, 1)
    r2, i2, d2 = orc.search_bruteforce(tgt, qry, 1, radius=0.05)
    assert r1 == r2
    np.testing.assert_array_equal(i1, i2)
    np.testing.assert_array_equal(d1, d2)
    assert (i1 < 0).any() and (i1 >= 0).any()      # both outcomes exercised
    assert np.isinf(d1[i1 < 0]).all()


def test_radius_is_strict_and_ties_take_lowest_index():
    tgt = np.array([[1, 0, 0], [0, 1, 0], [1, 0, 0]], np.float32)
    qry = np.zeros((1, 3), np.float32)
    r, idx, d2 = orc.search_radius(tgt, qry, 1.0, 1)      # d2 == r2 -> rejected
    assert r == 0 and idx[0, 0] == -1 and np.isinf(d2[0, 0])
    r, idx, d2 = orc.search_radius(tgt, qry, 1.0001, 1)
    assert r == 1 and idx[0, 0] == 0 and d2[0, 0] == 1.0
    assert orc.search_radius(np.zeros((0, 3)), qry, 1.0, 1)[0] == -1   # kdtree_flann.cu:72-73


def _flann_answers(g, tgt, qry):
    """What the reference's FLANN CPU kd-tree answers on the test's inputs: as recorded in
    tests/golden/ref_flann_search.npz (oracle/make_ref_vectors.py) and, where oracle/_ref is built, asked again."""
    from oracle.make_ref_vectors import FLANN_MAX_NN, FLANN_RADIUS, FLANN_VECTORS
    v = np.load(FLANN_VECTORS)
    yield (v["golden_knn_idx"], v["knn_idx"], v["knn_d2"], int(v["radius_count"][0]), v["radius_idx"], v["radius_d2"])
    if orc.ref_flann_available():
        gi, _ = orc.ref_flann_knn(g["points"], [g["query"]], g["knn"])
        yield (gi[0],) + orc.ref_flann_knn(tgt, qry, 5) + orc.ref_flann_radius(tgt, qry, FLANN_RADIUS, FLANN_MAX_NN)


def test_kdtree_equals_reference_flann_cpu(golden):
    from oracle.make_ref_vectors import FLANN_MAX_NN, FLANN_RADIUS, flann_inputs
    g = golden["kdtree_search_knn"]
    tgt, qry = flann_inputs()
    _, oi, od = orc.search_knn(tgt, qry, 5)
    r2, roi, rod = orc.search_radius(tgt, qry, FLANN_RADIUS, FLANN_MAX_NN)
    for gidx, fi, fd, r, ri, rd in _flann_answers(g, tgt, qry):
        assert gidx.tolist() == g["ref_indices"]
        # FLANN's randomized-kd-tree "exact" mode accumulates its lower bound per
        # split instead of per dimension and so misses a true neighbour in ~0.5% of
        # the slots (never the other way round): the oracle must never be beaten
        # and must agree on the overwhelming majority.
        assert (od <= fd * (1 + 2e-6)).all()
        assert (fi == oi).mean() > 0.98
        same = fi == oi
        np.testing.assert_allclose(fd[same], od[same], rtol=2e-6)
        assert (rod <= rd * (1 + 2e-6)).all()
        assert (ri == roi).mean() > 0.98 and abs(r - r2) <= 0.02 * r2


def test_rodrigues_and_solve():
    T = orc.vector6_to_matrix4([0, 0, 0, 1, 2, 3])
    np.testing.assert_array_equal(T[:3, :3], np.eye(3))
    T = orc.vector6_to_matrix4([0.1, -0.2, 0.3, 0, 0, 0])
    np.testing.assert_allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-6)
    np.testing.assert_allclose(np.linalg.det(T[:3, :3]), 1.0, atol=1e-6)
    rng = np.random.default_rng(2)
    J = rng.standard_normal((200, 6))
    r = rng.standard_normal(200) * 1e-2
    sys = np.zeros(32)
    A = J.T @ J
    sys[:21] = A[np.triu_indices(6)]
    sys[21:27] = J.T @ r
    ok, T = orc.solve_system(sys, 1e-6)
    x = np.linalg.solve(A, -J.T @ r)
    assert ok
    np.testing.assert_allclose(T, orc.vector6_to_matrix4(x), atol=2e-6)
    ok, T = orc.solve_system(np.zeros(32), 1e-6)       # singular -> det check fails
    assert not ok
    np.testing.assert_array_equal(T, np.eye(4))
    big = sys.copy()
    big[:21] *= 1e7                                    # det overflows fp32 -> failure (quirk 6)
    ok, _ = orc.solve_system(big, 1e-6)
    assert not ok
    ok, _ = orc.solve_system(big, -1.0)
    assert ok


@pytest.mark.parametrize("est", [orc.EST_P2P, orc.EST_PT2PL, orc.EST_SYM, orc.EST_GICP])
def test_icp_recovers_ground_truth(est):
    d = make_pair(20000, seed=7)
    kw = {}
    if est in (orc.EST_PT2PL, orc.EST_SYM):
        kw = dict(src_nrm=d["src_nrm"], tgt_nrm=d["tgt_nrm"], det_thresh=-1.0)
    if est == orc.EST_GICP:
        kw = dict(src_cov=orc.covariances_from_normals(d["src_nrm"]),
                  tgt_cov=orc.covariances_from_normals(d["tgt_nrm"]))
    res = orc.registration_icp(d["src"], d["tgt"], d["max_dist"], est=est, **kw)
    assert res.fitness > 0.99
    assert np.linalg.norm(res.transformation - d["T_gt"]) < 2e-5
    # correspondences ascend in source index and are stable-compacted
    assert (np.diff(res.correspondence_set[:, 0]) > 0).all()


def test_icp_edge_cases():
    d = make_pair(2000, seed=3)
    res = orc.registration_icp(d["src"], d["tgt"], 0.0)           # registration.cu:40-42
    assert res.fitness == 0 and len(res.correspondence_set) == 0
    np.testing.assert_array_equal(res.transformation, np.eye(4))
    # point-to-plane without target normals -> identity updates (:199-200)
    res = orc.registration_icp(d["src"], d["tgt"], d["max_dist"], est=orc.EST_PT2PL)
    np.testing.assert_array_equal(res.transformation, np.eye(4))
    # default det_thresh 1e-6 with a large cloud overflows fp32 det: documented quirk 6
    ev = orc.evaluate_registration(d["src"], d["tgt"], d["max_dist"], d["T_gt"])
    assert ev.fitness == 1.0 and ev.inlier_rmse < 1e-5


# ---- colored ICP (no reference golden vectors exist for it: parity unpinned, see oracle/README.md)
def _colored_case(planar):
    from conftest import make_colored
    tgt, col, T = make_colored(12000, seed=3, planar=planar)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (len(tgt), 1)) if planar else None
    if nrm is None:
        nrm = orc.estimate_normals_knn(tgt, 20)
        nrm[nrm[:, 2] < 0] *= -1
    src = orc.transform_points(np.linalg.inv(T).astype(np.float32), tgt)
    return src, tgt, col, nrm, T


def test_colour_gradient_matches_the_analytic_texture_gradient():
    src, tgt, col, nrm, T = _colored_case(planar=True)
    g = orc.color_gradients(tgt, nrm, col, 6.0, 30)
    q = tgt / 100.0
    mean_w = (1.0 + 0.9 + 1.1) / 3.0
    gx = 0.4 * 9 * np.cos(9 * q[:, 0]) * np.cos(7 * q[:, 1]) / 100.0 * mean_w
    gy = -0.4 * 7 * np.sin(9 * q[:, 0]) * np.sin(7 * q[:, 1]) / 100.0 * mean_w
    inner = (q[:, 0] > 0.1) & (q[:, 0] < 0.9) & (q[:, 1] > 0.1) & (q[:, 1] < 0.9)
    clipped = col[:, 2] >= 1.0   # the blue channel saturates there
    ok = inner & ~clipped
    err = np.hypot(g[ok, 0] - gx[ok], g[ok, 1] - gy[ok])
    assert np.median(err) < 2e-3 and np.abs(g[ok, 2]).max() < 1e-4, (np.median(err), np.abs(g[ok, 2]).max())


def test_colored_icp_recovers_in_plane_motion_that_point_to_plane_cannot_see():
    src, tgt, col, nrm, T = _colored_case(planar=True)
    res_c = orc.registration_colored_icp(src, tgt, 3.0, col, col, nrm, det_thresh=-1.0)
    res_p = orc.registration_icp(src, tgt, 3.0, est=orc.EST_PT2PL, tgt_nrm=nrm, det_thresh=-1.0)
    err_c = np.linalg.norm(res_c.transformation - T)
    err_p = np.linalg.norm(res_p.transformation - T)
    assert err_c < 0.05 * np.linalg.norm(T - np.eye(4)), (err_c, err_p)
    assert err_p > 10 * err_c, (err_c, err_p)


def test_colored_rmse_is_the_plain_sum_of_squared_residuals():
    src, tgt, col, nrm, T = _colored_case(planar=False)
    g = orc.color_gradients(tgt, nrm, col, 6.0, 30)
    orc.set_colored_context(col, col, g, 0.968)
    _, idx, _ = orc.search_radius(tgt, src, 3.0, 1)
    idx = idx[:, 0]
    cor = np.stack([np.arange(len(src)), idx], 1)[idx >= 0].astype(np.int32)
    whole = orc.compute_rmse(orc.EST_COLORED, src, tgt, cor, tgt_nrm=nrm)
    half = orc.compute_rmse(orc.EST_COLORED, src, tgt, cor[: len(cor) // 2], tgt_nrm=nrm) + \
        orc.compute_rmse(orc.EST_COLORED, src, tgt, cor[len(cor) // 2:], tgt_nrm=nrm)
    assert whole > 0 and abs(whole - half) <= 1e-4 * whole   # additive: a sum, not a root-mean


# --- depth image -> point cloud (pointcloud_factory.cu) and the KinFu pose estimation -------------
def test_depth_restatement_obeys_the_pinhole_model_and_the_reference_rules():
    from conftest import render_depth, small_pose
    K = [525.0, 525.0, 319.5, 239.5]
    d = render_depth(640, 480, K, np.eye(4), holes=0.1, seed=2)
    p, _, _ = orc.create_from_depth(d, K, stride=1)
    assert len(p) == int((d > 0).sum())                      # d <= 0 dropped, pixel order kept
    v, u = np.nonzero(d > 0)
    np.testing.assert_allclose(p[:, 2], d[v, u], rtol=1e-6)
    np.testing.assert_allclose(p[:, 0] / p[:, 2] * K[0] + K[2], u, atol=2e-3)     # projects back onto its pixel
    np.testing.assert_allclose(p[:, 1] / p[:, 2] * K[1] + K[3], v, atol=2e-3)
    # extrinsic: points are mapped by its inverse
    E = np.linalg.inv(small_pose(0.4, 0.3))
    q, _, _ = orc.create_from_depth(d, K, E)
    np.testing.assert_allclose(q, orc.transform_points(np.linalg.inv(E).astype(np.float32), p), atol=2e-6)
    # stride: pixel (row*stride, col*stride) of a (w/stride) x (h/stride) grid
    s3, _, _ = orc.create_from_depth(d, K, stride=3)
    sub = d[: (480 // 3) * 3: 3, : (640 // 3) * 3: 3]
    assert len(s3) == int((sub > 0).sum())
    # uint16 depth: * the correctly rounded reciprocal of (int)scale, >= (int)trunc dropped
    d16 = (np.clip(d, 0, 60) * 1000).astype(np.uint16)
    a, _, _ = orc.create_from_depth(d16, K, depth_scale=1000.9, depth_trunc=2.9)
    assert len(a) == int(((d16 > 0) & (d16.astype(np.float32) * np.float32(1.0 / np.float64(np.float32(1000))) < 2)).sum())
    # RGB-D form: cutoff, colours scaled by 1/255, rejected pixels +inf when not compacted
    col = np.random.default_rng(0).integers(0, 256, (480, 640, 3), dtype=np.uint8)
    p2, n2, c2 = orc.create_from_depth(d, K, color=col, depth_cutoff=2.5, rgbd=True, compute_normals=True,
                                       valid_only=False)
    keep = (d > 0) & (d < 2.5)
    assert len(p2) == 640 * 480 and (np.isfinite(p2[:, 0]) == keep.ravel()).all()
    assert np.isinf(c2[~keep.ravel()]).all()
    np.testing.assert_allclose(c2[keep.ravel()], col[keep] / 255.0, atol=1e-7)
    # normals of the back wall (z = 4, seen head-on) point at the camera: (0, 0, -1)
    clean = render_depth(640, 480, K, np.eye(4))
    _, n3, _ = orc.create_from_depth(clean, K, rgbd=True, compute_normals=True, valid_only=False)
    n3 = n3.reshape(480, 640, 3)
    assert np.abs(clean[84:131, 479:526] - 4.0).max() < 1e-5
    np.testing.assert_allclose(n3[85:130, 480:525].reshape(-1, 3), np.tile([0, 0, -1.0], (45 * 45, 1)), atol=1e-4)
    assert (n2[:, 2] <= 0).all()


def test_pyramid_intrinsics_follow_the_half_pixel_convention():
    w, h, fx, fy, cx, cy = orc.pyramid_level_intrinsic(640, 480, 525.0, 525.0, 319.5, 239.5, 1)
    assert (w, h) == (320, 240) and fx == 262.5 and cx == 159.5 and cy == 119.5
    assert orc.pyramid_level_intrinsic(640, 480, 525.0, 525.0, 319.5, 239.5, 0)[2] == 525.0


def test_kinfu_pose_estimation_recovers_the_camera_motion():
    from conftest import render_depth, small_pose
    K0 = (640, 480, 525.0, 525.0, 319.5, 239.5)
    pose_b = small_pose(0.02, 0.03)
    frames, models = [], []
    for level in range(3):       # every level rendered with its own intrinsics (half-pixel convention)
        w, h, fx, fy, cx, cy = orc.pyramid_level_intrinsic(*K0, level)
        k = [fx, fy, cx, cy]
        for pose, dst in ((np.eye(4), models), (pose_b, frames)):
            p, n, _ = orc.create_from_depth(render_depth(w, h, k, pose), k, rgbd=True, compute_normals=True,
                                            depth_cutoff=6.0)
            dst.append(dict(points=p, normals=n))
    # a threshold above the occlusion shadows' width lets their wrong matches bias the result
    # (7e-3 at 0.1); 0.03 keeps them out
    T = orc.kinfu_pose_estimation(np.eye(4, dtype=np.float32), frames, models, distance_threshold=0.03,
                                  icp_iterations=(10, 10, 10))
    assert np.linalg.norm(T - pose_b) < 2e-3, np.linalg.norm(T - pose_b)


# --- RGB-D odometry (odometry/odometry.cu) -------------------------------------------------------
def test_odometry_filters_and_correspondence_rule():
    rng = np.random.default_rng(0)
    img = rng.random((17, 23), dtype=np.float32)
    g = orc.od_filter(img, 0)
    pad = np.pad(img.astype(np.float64), 1, mode="edge")                       # clamp-to-edge
    k = np.array([0.25, 0.5, 0.25])
    ref = sum(k[j] * sum(k[i] * pad[j:j + 17, i:i + 23] for i in range(3)) for j in range(3))
    np.testing.assert_allclose(g, ref, rtol=1e-6)
    ramp = np.tile(np.arange(23, dtype=np.float32), (17, 1))                    # d/dx = 1: Sobel * 1/8
    np.testing.assert_allclose(orc.od_filter(ramp, 1)[:, 1:-1] * 0.125, 1.0, rtol=1e-6)
    assert np.abs(orc.od_filter(ramp, 2)).max() == 0.0
    np.testing.assert_allclose(orc.od_downsample(img)[3, 4], img[6:8, 8:10].mean(), rtol=1e-6)
    assert orc.od_downsample(img).shape == (8, 11)
    # identity extrinsic: every valid pixel corresponds to itself; a NaN or a depth jump does not
    d = np.full((12, 16), 2.0, np.float32)
    d[3, 4] = np.nan
    dt = d.copy()
    dt[5, 6] = 2.5
    dt[3, 4] = 2.0
    c = orc.od_correspondence([[20, 0, 7.5], [0, 20, 5.5], [0, 0, 1]], np.eye(4), d, dt, 0.03)
    assert len(c) == 12 * 16 - 2 and (c[:, 0] == c[:, 2]).all() and (c[:, 1] == c[:, 3]).all()
    assert not ((c[:, 0] == 4) & (c[:, 1] == 3)).any() and not ((c[:, 0] == 6) & (c[:, 1] == 5)).any()


@pytest.mark.parametrize("jac", [orc.OD_COLOR_TERM, orc.OD_HYBRID_TERM])
def test_odometry_recovers_the_camera_motion(jac):
    from conftest import render_rgbd, small_pose
    K = [262.5, 262.5, 159.5, 119.5]
    pose_b = small_pose(0.02, 0.03)
    ca, da = render_rgbd(320, 240, K, np.eye(4))
    cb, db = render_rgbd(320, 240, K, pose_b)
    ok, T, info = orc.compute_rgbd_odometry(cb, db, ca, da, K, jacobian=jac, max_depth=6.0)
    assert ok
    motion = np.linalg.norm(np.eye(4) - pose_b)
    assert np.linalg.norm(T - pose_b) < (0.1 if jac == orc.OD_HYBRID_TERM else 0.5) * motion
    assert np.allclose(info, info.T) and (np.diag(info) > 1e4).all()
    # no overlap in depth range: nothing corresponds, the "solution" of a zero system
    ok2, T2, _ = orc.compute_rgbd_odometry(cb, db, ca, da, K, jacobian=jac, max_depth=0.1)
    assert not np.isfinite(T2).all() or np.allclose(T2, np.eye(4))


def test_weighted_odometry_and_twist_conversion():
    from conftest import render_rgbd, small_pose
    x = np.array([0.1, -0.2, 0.05, 1, 2, 3], np.float32)
    T = np.empty(16, np.float32)
    orc.lib().oracle_vector6_to_matrix4(orc._p(x), orc._p(T))
    np.testing.assert_allclose(orc.matrix4_to_vector6(T.reshape(4, 4).T), x, atol=1e-6)     # log(exp(x)) = x
    np.testing.assert_array_equal(orc.matrix4_to_vector6(np.eye(4)), np.zeros(6, np.float32))
    K = [262.5, 262.5, 159.5, 119.5]
    pose_b = small_pose(0.02, 0.03)
    ca, da = render_rgbd(320, 240, K, np.eye(4))
    cb, db = render_rgbd(320, 240, K, pose_b)
    ok, T, tw, info = orc.compute_weighted_rgbd_odometry(cb, db, ca, da, K, max_depth=6.0)
    assert ok and np.linalg.norm(T - pose_b) < 0.1 * np.linalg.norm(np.eye(4) - pose_b)
    np.testing.assert_allclose(tw, orc.matrix4_to_vector6(T), atol=1e-5)
    # a strong prior on a wrong velocity pulls the result away from the data's optimum
    ok, T2, _, _ = orc.compute_weighted_rgbd_odometry(cb, db, ca, da, K, max_depth=6.0, prev_twist=np.zeros(6),
                                                      inv_sigma_mat_diag=[1e7] * 6)
    assert np.linalg.norm(T2 - np.eye(4)) < np.linalg.norm(T - np.eye(4))


@pytest.mark.parametrize("c", [(7, 5, 1), (16, 16, 3), (193, 128, 2), (323, 243, 3)], ids=lambda c: "%dx%d_L%d" % c)
@pytest.mark.parametrize("init", ["identity", "small"])
def test_od_images_is_the_composition_of_the_public_pieces(c, init):
    """od_core's front half (oracle_od_images) = PreprocessDepth in numpy, od_filter, the mean scaling of NormalizeIntensity in
    numpy over od_correspondence's list, od_filter + od_downsample per level, od_filter 1 / 2 of the target: bit for bit"""
    import odometry_exact as oe
    w, h, L = c
    ref = oe.case(w, h, L, init)
    cs, ds, ct, dt = ref["frames"]
    K, T0 = ref["K"], ref["T0"]

    def preprocess(d):
        d = d.copy()
        with np.errstate(invalid="ignore"):
            d[(d < np.float32(oe.MIN_DEPTH)) | (d > np.float32(oe.MAX_DEPTH)) | (d <= 0)] = np.nan
        return d

    col = [orc.od_filter(cs, 0), orc.od_filter(ct, 0)]
    dep = [orc.od_filter(preprocess(ds), 0), orc.od_filter(preprocess(dt), 0)]
    corr = orc.od_correspondence([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1]], T0, dep[0], dep[1], oe.MAX_DEPTH_DIFF)
    assert len(corr) == ref["count"] > 0
    for s, (x, y) in enumerate(((corr[:, 0], corr[:, 1]), (corr[:, 2], corr[:, 3]))):
        total = np.cumsum(col[s][y, x].astype(np.float64))[-1]                    # one after the other, in list order
        mean = np.float32(total) / np.float32(len(corr))
        scale = np.float32(0.5 / np.float64(mean))
        col[s] = scale * col[s] + np.float32(0.0)
        assert col[s].dtype == np.float32
    for level in range(L):
        if level:
            col = [orc.od_downsample(orc.od_filter(a, 0)) for a in col]
            dep = [orc.od_downsample(a) for a in dep]
        mine = {0: col[0], 1: dep[0], 2: col[1], 3: dep[1], 4: orc.od_filter(col[1], 1), 5: orc.od_filter(col[1], 2),
                6: orc.od_filter(dep[1], 1), 7: orc.od_filter(dep[1], 2)}
        for which in range(8):
            assert mine[which].shape == (h >> level, w >> level)
            diff = oe.same_bits(ref["images"][level][which], mine[which])
            assert diff is None, (level, orc.OD_IMAGES[which], diff)
        assert np.isnan(dep[0]).any() and not np.isnan(col[0]).any()


def test_od_filters_against_an_fp64_restatement():
    """Gaussian3 on random floats (all terms positive: fp32 loses a few ulps); both Sobels on an image of small integers,
    where fp32 is exact and a difference of neighbours cannot cancel into its own rounding error -- and on which a swap
    of the two axes shows (the image is not symmetric)"""
    rng = np.random.default_rng(3)
    h, w = 19, 26

    def sep(img, kx, ky):
        pad = np.pad(img.astype(np.float64), 1, mode="edge")
        return sum(ky[j] * sum(kx[i] * pad[j:j + h, i:i + w] for i in range(3)) for j in range(3))

    g3, s1, s2 = [0.25, 0.5, 0.25], [-1.0, 0.0, 1.0], [1.0, 2.0, 1.0]
    img = rng.random((h, w), dtype=np.float32)
    np.testing.assert_allclose(orc.od_filter(img, 0), sep(img, g3, g3), rtol=1e-6)
    ints = rng.integers(0, 256, (h, w)).astype(np.float32)
    dx, dy = sep(ints, s1, s2), sep(ints, s2, s1)
    assert np.abs(dx - dy).max() > 100
    np.testing.assert_allclose(orc.od_filter(ints, 1), dx, rtol=1e-6)
    np.testing.assert_allclose(orc.od_filter(ints, 2), dy, rtol=1e-6)


def test_odometry_results_are_those_recorded_before_od_images_was_split_off():
    """tests/golden/odometry_oracle_parent.npz: what compute_rgbd_odometry / compute_weighted_rgbd_odometry returned for these
    two calls before od_core's front half became a function of its own.  Bit for bit."""
    import os
    from conftest import ROOT, render_rgbd, small_pose
    g = np.load(os.path.join(ROOT, "tests", "golden", "odometry_oracle_parent.npz"))
    pose = small_pose(0.02, 0.03)
    with np.errstate(invalid="ignore"):
        K = [65.6, 65.6, 39.5, 29.5]
        ca, da = render_rgbd(80, 60, K, np.eye(4), holes=0.02, seed=1)
        cb, db = render_rgbd(80, 60, K, pose, holes=0.02, seed=2)
        for jac in (0, 1):
            ok, T, info = orc.compute_rgbd_odometry(cb, db, ca, da, K, jacobian=jac, iterations=(3, 2, 1), max_depth=6.0)
            assert ok and T.tobytes() == g["plain_T_%d" % jac].tobytes() and info.tobytes() == g["plain_info_%d" % jac].tobytes()
        K = [66.4, 66.4, 40.0, 30.0]
        ca, da = render_rgbd(81, 61, K, np.eye(4), holes=0.02, seed=3)
        cb, db = render_rgbd(81, 61, K, pose, holes=0.02, seed=4)
    ok, T, tw, info = orc.compute_weighted_rgbd_odometry(
        cb, db, ca, da, K, odo_init=small_pose(0.01, 0.01), prev_twist=orc.matrix4_to_vector6(pose), iterations=(2, 2),
        max_depth=6.0, nu=3.0, sigma2_init=0.5, inv_sigma_mat_diag=[500.0] * 6)
    assert ok and T.tobytes() == g["weighted_T"].tobytes() and tw.tobytes() == g["weighted_twist"].tobytes()
    assert info.tobytes() == g["weighted_info"].tobytes()


def _kabsch_numpy_fp64(src32, tgt32):
    """registration/kabsch.cu:74-118 in fp64 with numpy's SVD: R = V diag(1, 1, det(U V)) U^T, t = ct - R cs"""
    S, G = src32.astype(np.float64), tgt32.astype(np.float64)
    cs, ct = S.mean(0), G.mean(0)
    H = (S - cs).T @ (G - ct) / len(S)
    U, s, Vt = np.linalg.svd(H)
    R = Vt.T @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt.T)]) @ U.T
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = ct - R @ cs
    return T, s


def test_kabsch_matches_numpy_fp64_svd_also_on_planar_sources():
    """The oracle's and the engine's Kabsch (their own restatements of a 3x3 SVD: third_party/eigen is not vendored)
    against numpy's fp64 SVD on 200 random clouds -- general, nearly planar, and EXACTLY planar, where a row of the
    cross-covariance is zero: Eigen's two-sided JacobiSVD returns full orthogonal factors there, i.e. a proper
    rotation (until late in round 5 both restatements divided a column of noise by a singular value of ~1e-17 and
    returned a 'rotation' of rank 2)."""
    from cupoch_amd import engine
    rng = np.random.default_rng(11)
    for case in range(200):
        n = int(rng.integers(3, 300))
        scale = 10 ** rng.uniform(-2, 1)
        src = rng.standard_normal((n, 3)) * scale
        if case % 4 == 1:
            src[:, 2] *= 1e-3
        if case % 4 == 2:
            src[:, 2] = 0.25 * scale                       # exactly planar
        a = rng.standard_normal(3)
        a /= np.linalg.norm(a)
        th = rng.uniform(0, np.pi)
        K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
        R = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
        tgt = src @ R.T + rng.standard_normal(3) * scale + rng.standard_normal((n, 3)) * scale * 1e-3
        s32, t32 = src.astype(np.float32), tgt.astype(np.float32)
        cor = np.stack([np.arange(n), np.arange(n)], 1).astype(np.int32)
        sys = orc.compute_system(orc.EST_P2P, s32, t32, cor)
        ref, sv = _kabsch_numpy_fp64(s32, t32)
        if sv[1] < 1e-6 * sv[0]:
            continue                                        # (collinear: the rotation about the line is free)
        unit = max(1.0, float(np.abs(ref[:3, 3]).max()))
        for name, T in (("oracle", orc.kabsch_from_sums(sys, n)), ("engine", engine.kabsch_from_sums(sys, n))):
            assert abs(np.linalg.det(T[:3, :3].astype(np.float64)) - 1.0) <= 1e-5, (name, case)
            assert np.abs(T - ref).max() <= 2e-6 * unit, (name, case, float(np.abs(T - ref).max()))
