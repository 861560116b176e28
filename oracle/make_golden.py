#!/usr/bin/env python3
"""Regenerate tests/golden/reference_tests.json from the reference checkout.

Run HERE (the container that has /root/reference); the GPU box only sees the
committed JSON.  Inputs are produced by the reference's own deterministic
generator (unit_test::Raw, compiled into oracle/_ref/libref_raw.so); expected
values are the literal golden vectors of the reference's googletest files,
parsed out of the .cpp sources (cited per entry).
"""
import json
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle as orc  # noqa: E402

REF = os.environ.get("CUPOCH_REFERENCE", "/root/reference")
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "golden",
                   "reference_tests.json")


def test_body(path, suite, case):
    src = open(os.path.join(REF, path)).read()
    m = re.search(r"TEST\(\s*%s\s*,\s*%s\s*\)\s*\{" % (suite, case), src)
    assert m, (path, suite, case)
    i, depth = m.end(), 1
    while depth:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
    return src[m.end():i - 1]


def case_span(path, suite, case):
    """(body, "path:first-last line") of one TEST"""
    src = open(os.path.join(REF, path)).read()
    body = test_body(path, suite, case)
    start = re.search(r"TEST\(\s*%s\s*,\s*%s\s*\)\s*\{" % (suite, case), src).start()
    first = src.count("\n", 0, start) + 1
    last = first + src[start:src.index(body, start) + len(body)].count("\n")
    return body, "%s:%d-%d" % (path, first, last)


def all_reference_cases():
    """every "Suite.Case" under the reference's src/tests, in file and line order"""
    names = []
    for root, _, files in sorted(os.walk(os.path.join(REF, "src", "tests"))):
        for f in sorted(files):
            if f.endswith((".cpp", ".cu")):
                names += ["%s.%s" % m for m in re.findall(r"^TEST\(\s*(\w+)\s*,\s*(\w+)\s*\)", open(os.path.join(root, f)).read(), re.M)]
    return names


def brace_list(body, name):
    m = re.search(r"%s\s*\[\s*\]\s*=\s*\{([^}]*)\}" % name, body)
    return [float(x) for x in m.group(1).replace("\n", " ").split(",") if x.strip()]


def vec3_pushes(body, var):
    pat = r"%s\.push_back\(Vector3f\(([^)]*)\)\)" % var
    return [[float(v) for v in m.split(",")] for m in re.findall(pat, body)]


IMAGE_CPP = "src/tests/geometry/image.cpp"
POINTCLOUD_CPP = "src/tests/geometry/pointcloud.cpp"
LINESET_CPP = "src/tests/geometry/lineset.cpp"


def image_vectors(g):
    """src/tests/geometry/image.cpp: every case whose operation is built.  Inputs are unit_test::Rand(host_vector<uint8_t>&,
    0, 255, 0) or the test's own literal; `ref_bytes` are the literal bytes the test compares with EXPECT_EQ per byte
    (`ref_floats`: the one case that compares floats, under THRESHOLD_1E_4)."""
    def entry(case, width, height, channels, bpc, data, call, ref_shape, **more):
        body, cite = case_span(IMAGE_CPP, "Image", case)
        e = {"cite": cite, "width": width, "height": height, "channels": channels, "bytes_per_channel": bpc,
             "input": [int(v) for v in data], "call": call,
             "ref_width": ref_shape[0], "ref_height": ref_shape[1], "ref_channels": ref_shape[2], "ref_bytes_per_channel": ref_shape[3]}
        e.update(more)
        g["image_" + case] = e
        return body, e

    ints = lambda body, name: [int(v) for v in brace_list(body, name)]
    rand = lambda n: orc.ref_rand_u8(n, 0, 255, 0)

    # TEST_CreateFloatImage (image.cpp:200-226) calls CreateFloatImage() with the default type whatever `type` it was given,
    # so the _Equal cases hold the Weighted vectors: recorded as written
    for channels, bpc, suffixes in ((1, 1, ("",)), (1, 2, ("",)), (1, 4, ("",)), (3, 1, ("_Weighted", "_Equal")),
                                    (3, 2, ("_Weighted", "_Equal")), (3, 4, ("_Weighted", "_Equal"))):
        for suffix in suffixes:
            case = "CreateFloatImage_%d_%d%s" % (channels, bpc, suffix)
            body, e = entry(case, 5, 5, channels, bpc, rand(25 * channels * bpc), "create_float_image", (5, 5, 1, 4),
                            args={"type": "default (Weighted)"}, helper_cite=IMAGE_CPP + ":200-226")
            e["ref_bytes"] = ints(body, "raw_ref")
    body, e = entry("ConvertDepthToFloatImage", 5, 5, 1, 1, rand(25), "convert_depth_to_float_image", (5, 5, 1, 4),
                    args={"depth_scale": 1000.0, "depth_trunc": 3.0})
    e["ref_bytes"] = ints(body, "raw_ref")

    body, e = entry("TransposeUint8", 6, 3, 1, 1, ints(test_body(IMAGE_CPP, "Image", "TransposeUint8"), "raw_input"), "transpose", (3, 6, 1, 1))
    e["ref_bytes"] = ints(body, "raw_transposed_ref")
    fin = np.array(brace_list(test_body(IMAGE_CPP, "Image", "TransposeFloat"), "raw_input"), np.float32)
    body, e = entry("TransposeFloat", 6, 3, 1, 4, fin.tobytes(), "transpose", (3, 6, 1, 4))
    e["ref_floats"], e["tol"] = brace_list(body, "raw_transposed_ref"), 1e-4     # unit_test.cpp:83-87
    for case, call in (("FlipVerticalImage", "flip_vertical"), ("FlipHorizontalImage", "flip_horizontal")):
        body, e = entry(case, 6, 3, 1, 1, ints(test_body(IMAGE_CPP, "Image", case), "raw_input"), call, (6, 3, 1, 1))
        e["ref_bytes"] = ints(body, "raw_flipped")

    # TEST_Filter (image.cpp:588-614): 100 random bytes as 5 x 5 floats, CreateFloatImage (a copy), then the filter
    for kind in ("Gaussian3", "Gaussian5", "Gaussian7", "Sobel3Dx", "Sobel3Dy"):
        body, e = entry("Filter_" + kind, 5, 5, 1, 4, rand(100), "filter", (5, 5, 1, 4), pre="create_float_image",
                        args={"filter_type": kind}, helper_cite=IMAGE_CPP + ":588-614")
        e["ref_bytes"] = ints(body, "raw_ref")
    body, e = entry("FilterHorizontal", 5, 5, 1, 4, rand(100), "filter_horizontal", (5, 5, 1, 4), pre="create_float_image",
                    args={"kernel": [0.25, 0.5, 0.25]})
    e["ref_bytes"] = ints(body, "raw_ref")
    body, e = entry("Downsample", 5, 5, 1, 4, rand(100), "downsample", (2, 2, 1, 4), pre="create_float_image")
    e["ref_bytes"] = ints(body, "raw_ref")

    # the shape-only cases: what the test prepares and every value it expects
    empty = {"width": 0, "height": 0, "num_of_channels": 0, "bytes_per_channel": 0, "data_size": 0, "is_empty": True,
             "min_bound": [0.0, 0.0], "max_bound": [0.0, 0.0], "test_image_boundary_0_0": False, "bytes_per_line": 0}
    prepared = {"width": 1920, "height": 1080, "num_of_channels": 3, "bytes_per_channel": 1, "data_size": 1920 * 1080 * 3,
                "is_empty": False, "min_bound": [0.0, 0.0], "max_bound": [1920.0, 1080.0], "test_image_boundary_0_0": True,
                "bytes_per_line": 1920 * 3}
    g["image_DefaultConstructor"] = {"cite": case_span(IMAGE_CPP, "Image", "DefaultConstructor")[1], "prepare": None, "clear": False,
                                     "dimension": 2, "expect": empty, "tol": 1e-4}
    g["image_CreateImage"] = {"cite": case_span(IMAGE_CPP, "Image", "CreateImage")[1], "prepare": [1920, 1080, 3, 1], "clear": False,
                              "expect": prepared, "tol": 1e-4}
    g["image_Clear"] = {"cite": case_span(IMAGE_CPP, "Image", "Clear")[1], "prepare": [1920, 1080, 3, 1], "clear": True,
                        "expect": empty, "tol": 1e-4}


def cloud_vectors(g):
    """src/tests/geometry/pointcloud.cpp and lineset.cpp: the cases on 100 points of Rand(points, 0, 1000, 0).  tol is
    ExpectEQ's default threshold THRESHOLD_1E_4 (unit_test.h:40,53-65)."""
    pts = orc.ref_rand_vec3f(100, [0, 0, 0], [1000, 1000, 1000], 0)
    lo, hi = [19.607843, 0.0, 0.0], [996.078431, 996.078431, 996.078431]
    for case, key, ref in (("GetMinBound", "pointcloud_get_min_bound", lo), ("GetMaxBound", "pointcloud_get_max_bound", hi)):
        body, cite = case_span(POINTCLOUD_CPP, "PointCloud", case)
        got = [float(v) for v in re.search(r"ExpectEQ\(Vector3f\(([^)]*)\)", body).group(1).split(",")]
        assert got == ref, (case, got)
        g[key] = {"cite": cite, "points": pts.tolist(), "ref": got, "tol": 1e-4}
    for case, key in (("SelectByIndex", "pointcloud_select_by_index"), ("SelectByMask", "pointcloud_select_by_mask")):
        body, cite = case_span(POINTCLOUD_CPP, "PointCloud", case)
        idx = [int(v) for v in re.findall(r"ref_idx\.push_back\((\d+)\)", body)]
        assert len(idx) == 10
        # the test forms its expectation from its own input (points[i] for i in ref_idx) and sorts both sides (sort::Do)
        g[key] = {"cite": cite, "points": pts.tolist(), "indices": idx, "ref_points": pts[idx].tolist(), "sorted": True, "tol": 1e-4}
    body, cite = case_span(POINTCLOUD_CPP, "PointCloud", "UniformDownSample")
    g["pointcloud_uniform_down_sample"] = {"cite": cite, "points": pts.tolist(), "every_k_points": 4,
                                           "ref_points": vec3_pushes(body, "ref"), "tol": 1e-4}
    assert len(g["pointcloud_uniform_down_sample"]["ref_points"]) == 25
    body, cite = case_span(POINTCLOUD_CPP, "PointCloud", "CropPointCloud")
    mn = [float(v) for v in re.search(r"minBound\(([^)]*)\)", body).group(1).split(",")]
    mx = [float(v) for v in re.search(r"maxBound\(([^)]*)\)", body).group(1).split(",")]
    g["pointcloud_crop"] = {"cite": cite, "points": pts.tolist(), "min_bound": mn, "max_bound": mx,
                            "expect": "every output coordinate >= min_bound and <= max_bound (ExpectLE / ExpectGE)"}

    # the container cases: what is set and the flags the test expects before and after
    zero = [0.0, 0.0, 0.0]
    none = {"is_empty": True, "has_points": False, "has_normals": False, "has_colors": False, "min_bound": zero, "max_bound": zero}
    full = {"is_empty": False, "has_points": True, "has_normals": True, "has_colors": True, "min_bound": lo, "max_bound": hi}
    cs = lambda case: case_span(POINTCLOUD_CPP, "PointCloud", case)[1]
    g["pointcloud_constuctor"] = {"cite": cs("Constuctor"), "dimension": 3, "expect": none, "tol": 1e-4}
    g["pointcloud_clear"] = {"cite": cs("Clear"), "points": pts.tolist(), "normals": pts.tolist(), "colors": pts.tolist(),
                             "expect_set": full, "expect_cleared": none, "tol": 1e-4}
    g["pointcloud_is_empty"] = {"cite": cs("IsEmpty"), "points": pts.tolist(), "expect_before": True, "expect_after": False}
    for what in ("points", "normals", "colors"):
        g["pointcloud_has_" + what] = {"cite": cs("Has" + what.capitalize()), "size": 100, "set": sorted({"points", what}),
                                       "flag": "has_" + what, "expect_before": False, "expect_after": True}

    ls_none = {"is_empty": True, "has_points": False, "has_lines": False, "has_colors": False, "min_bound": zero, "max_bound": zero}
    ls_full = {"is_empty": False, "has_points": True, "has_lines": True, "has_colors": True, "min_bound": lo, "max_bound": hi}
    g["lineset_constructor"] = {"cite": case_span(LINESET_CPP, "LineSet", "Constructor")[1], "dimension": 3, "expect": ls_none, "tol": 1e-4}
    # Rand(host_vector<Vector2i>&, (0, 0), (1000, 1000), 0) (rand.cpp:73-87): the factor is a float quotient held in a double
    raw = orc.ref_rand_vec4i(50, 0, 255, 0).reshape(-1).astype(np.float64)          # factor 1: Raw::Next<int>() itself
    lines = (raw * np.float64(np.float32(1000) / np.float32(255))).astype(np.int64).reshape(100, 2)
    body, cite = case_span(LINESET_CPP, "LineSet", "Clear")
    got = [[float(v) for v in m.split(",")] for m in re.findall(r"ExpectEQ\(Vector3f\(([^)]*)\)", body)]
    assert got == [lo, hi], got
    g["lineset_clear"] = {"cite": cite, "points": pts.tolist(), "lines": lines.tolist(), "colors": pts.tolist(),
                          "expect_set": ls_full, "expect_cleared": ls_none, "tol": 1e-4}


# suites of the reference that this repository ports by hand (each file cites the reference file it ports)
PORTED = {
    "Collision": "tests/cpp/test_collision.cpp", "Graph": "tests/cpp/test_graph.cpp", "SimplePlanner": "tests/cpp/test_graph.cpp",
    "VoxelGrid": "tests/cpp/test_voxelgrid.cpp", "OccupancyGrid": "tests/cpp/test_occupancygrid.cpp",
    "DistanceTransform": "tests/cpp/test_distancetransform.cpp", "LaserScanBuffer": "tests/cpp/test_laserscanbuffer.cpp",
    "UniformTSDFVolume.Constructor": "tests/cpp/test_uniform_tsdfvolume.cpp", "UniformTSDFVolume.RealData": "tests/test_tsdf_cpu.py",
    "PointCloud.SegmentPlaneKnownPlane": "tests/cpp/test_segment_plane.cpp",
    "PointCloud.RemoveRadiusOutliers": "tests/test_outlier_removal_cpu.py",
    "PointCloud.CreatePointCloudFromFile": "tests/test_io_and_real_data.py",
}
NOT_BUILT = {
    "TriangleMesh": "geometry::TriangleMesh", "Feature.ComputeFPFHFeature": "registration::ComputeFPFHFeature",
    "PointCloud.GetOrientedBoundingBox": "PointCloud::GetOrientedBoundingBox", "PointCloud.NormalizeNormals": "PointCloud::NormalizeNormals",
    "PointCloud.OrientNormalsToAlignWithDirection": "PointCloud::OrientNormalsToAlignWithDirection",
    "Image.FloatValueAt": "geometry::FloatValueAt",
    "Image.CreateDepthToCameraDistanceMultiplierFloatImage": "Image::CreateDepthToCameraDistanceMultiplierFloatImage as an Image factory",
}
GOLDEN = {
    "KDTreeFlann.SearchKNN": "kdtree_search_knn", "KDTreeFlann.SearchRadius": "kdtree_search_radius",
    "LinearBoundingVolumeHierarchyKNN.SearchKNN": "lbvh_search_nn", "Kabsch.Kabsch": "kabsch",
    "PointCloud.Transform": "pointcloud_transform", "PointCloud.VoxelDownSample": "voxel_down_sample",
    "PointCloud.EstimateNormals": "estimate_normals",
    "RGBDOdometryJacobianFromColorTerm.ComputeJacobianAndResidual": "odometry_jacobian_color",
    "RGBDOdometryJacobianFromHybridTerm.ComputeJacobianAndResidual": "odometry_jacobian_hybrid",
    "PointCloud.GetMinBound": "pointcloud_get_min_bound", "PointCloud.GetMaxBound": "pointcloud_get_max_bound",
    "PointCloud.SelectByIndex": "pointcloud_select_by_index", "PointCloud.SelectByMask": "pointcloud_select_by_mask",
    "PointCloud.UniformDownSample": "pointcloud_uniform_down_sample", "PointCloud.CropPointCloud": "pointcloud_crop",
    "PointCloud.Constuctor": "pointcloud_constuctor", "PointCloud.Clear": "pointcloud_clear", "PointCloud.IsEmpty": "pointcloud_is_empty",
    "PointCloud.HasPoints": "pointcloud_has_points", "PointCloud.HasNormals": "pointcloud_has_normals",
    "PointCloud.HasColors": "pointcloud_has_colors",
    "LineSet.Constructor": "lineset_constructor", "LineSet.Clear": "lineset_clear",
}


def ledger(g):
    """one status per TEST(suite, case) of the reference: golden:<key of this file>, ported:<test file of this
    repository>, or not built: <operation>.  The names are found in the reference's sources and must be the ones listed."""
    out = {}
    for name in all_reference_cases():
        suite = name.split(".")[0]
        if name in GOLDEN or (suite == "Image" and "image_" + name.split(".")[1] in g):
            out[name] = "golden:" + GOLDEN.get(name, "image_" + name.split(".")[1])
        elif name in PORTED or suite in PORTED:
            out[name] = "ported:" + PORTED.get(name, PORTED.get(suite))
        elif name in NOT_BUILT or suite in NOT_BUILT:
            out[name] = "not built: " + NOT_BUILT.get(name, NOT_BUILT.get(suite))
        else:
            raise AssertionError("reference case without a status: " + name)
        assert name not in PORTED or name not in NOT_BUILT
    listed = set(GOLDEN) | {n for n in out if n.startswith("Image.")} | {n for n in out if n in PORTED or n.split(".")[0] in PORTED} \
        | {n for n in out if n in NOT_BUILT or n.split(".")[0] in NOT_BUILT}
    assert listed == set(out), sorted(listed ^ set(out))
    for table in (GOLDEN, PORTED, NOT_BUILT):      # nothing listed that the reference does not hold
        for k in table:
            assert k in out or any(n.startswith(k + ".") for n in out), k
    for name, st in out.items():
        if st.startswith("golden:"):
            assert st[7:] in g, (name, st)
        if st.startswith("ported:"):
            assert os.path.exists(os.path.join(os.path.dirname(OUT), "..", "..", st[7:])), st
    return out


def main():
    orc.build()
    g = {}
    pts100 = orc.ref_rand_vec3f(100, [0, 0, 0], [10, 10, 10], 0)

    b = test_body("src/tests/knn/kdtree_flann.cpp", "KDTreeFlann", "SearchKNN")
    g["kdtree_search_knn"] = {
        "cite": "src/tests/knn/kdtree_flann.cpp:47-91",
        "points": pts100.tolist(), "query": [1.647059, 4.392157, 8.784314], "knn": 30,
        "ref_indices": [int(x) for x in brace_list(b, "indices0")],
        "ref_distance2": brace_list(b, "distances0"), "ref_return": 30, "tol": 1e-4}

    b = test_body("src/tests/knn/kdtree_flann.cpp", "KDTreeFlann", "SearchRadius")
    g["kdtree_search_radius"] = {
        "cite": "src/tests/knn/kdtree_flann.cpp:93-135",
        "points": pts100.tolist(), "query": [1.647059, 4.392157, 8.784314],
        "radius": 5.0, "max_nn": 15,
        "ref_indices": [int(x) for x in brace_list(b, "indices0")],
        "ref_distance2": brace_list(b, "distances0"), "ref_return": 15, "tol": 1e-4}

    b = test_body("src/tests/knn/lbvh_knn.cpp", "LinearBoundingVolumeHierarchyKNN", "SearchKNN")
    g["lbvh_search_nn"] = {
        "cite": "src/tests/knn/lbvh_knn.cpp:47-86",
        "points": pts100.tolist(), "query": [1.647059, 4.392157, 8.784314],
        "ref_index": int(brace_list(b, "indices0")[0]),
        "ref_distance2": brace_list(b, "distances0")[0], "ref_return": 1, "tol": 1e-9}

    rad = np.float32(30.0) / np.float32(180.0) * np.pi
    c, s = float(np.cos(np.float32(rad))), float(np.sin(np.float32(rad)))
    g["kabsch"] = {
        "cite": "src/tests/registration/kabsch.cpp:35-55",
        "points": orc.ref_rand_vec3f(20, [0, 0, 0], [1000, 1000, 1000], 0).tolist(),
        "ref_tf": [[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]],
        "tol_rel": 1e-3}

    c4, s4 = float(np.cos(np.pi / 4)), float(np.sin(np.pi / 4))
    g["pointcloud_transform"] = {
        "cite": "src/tests/geometry/pointcloud.cpp:143-174",
        "points": orc.ref_rand_vec3f(10, [0, 0, 0], [1000, 1000, 1000], 0).tolist(),
        "normals": orc.ref_rand_vec3f(10, [0, 0, 0], [1000, 1000, 1000], 0).tolist(),
        "transformation": [[1, 0, 0, 1], [0, c4, -s4, 2], [0, s4, c4, 3], [0, 0, 0, 1]],
        "tol": 5e-4}

    b = test_body("src/tests/geometry/pointcloud.cpp", "PointCloud", "VoxelDownSample")
    g["voxel_down_sample"] = {
        "cite": "src/tests/geometry/pointcloud.cpp:371-469",
        "points": orc.ref_rand_vec3f(20, [0, 0, 0], [1000, 1000, 1000], 0).tolist(),
        "normals": orc.ref_rand_vec3f(20, [0, 0, 0], [10, 10, 10], 0).tolist(),
        "colors": orc.ref_rand_vec3f(20, [0, 0, 0], [255, 255, 255], 0).tolist(),
        "voxel_size": 0.5,
        "ref_points": vec3_pushes(b, "ref_points"),
        "ref_normals": vec3_pushes(b, "ref_normals"),
        "ref_colors": vec3_pushes(b, "ref_colors"), "tol": 1e-4}

    b = test_body("src/tests/geometry/pointcloud.cpp", "PointCloud", "EstimateNormals")
    g["estimate_normals"] = {
        "cite": "src/tests/geometry/pointcloud.cpp:535-597",
        "points": orc.ref_rand_vec3f(40, [0, 0, 0], [1000, 1000, 1000], 0).tolist(),
        "knn": 30, "ref_normals": vec3_pushes(b, "ref"), "tol": 1e-4}

    def vec6_rows(body, var):
        pat = r"%s\[\d+\]\s*<<([^;]*);" % var
        return [[float(v) for v in m.replace("\n", " ").split(",")] for m in re.findall(pat, body)]

    # the two Jacobian functors of the RGB-D odometry: inputs as the tests build them
    # (odometry_tools.cpp GenerateImage / ShiftLeft / ShiftUp over unit_test::Rand)
    img = lambda vmin, vmax, seed: orc.ref_rand_floats(100, vmin, vmax, seed).reshape(10, 10)
    shift_left = lambda a, s: np.stack([[a[h, (w + s) % 10] for w in range(10)] for h in range(10)]).astype(np.float32)
    shift_up = lambda a, s: np.stack([[a[(h + s) % 10, w] for w in range(10)] for h in range(10)]).astype(np.float32)
    for name, case, hybrid in (("odometry_jacobian_color", "RGBDOdometryJacobianFromColorTerm", 0),
                               ("odometry_jacobian_hybrid", "RGBDOdometryJacobianFromHybridTerm", 1)):
        path = "src/tests/odometry/rgbdodometry_jacobian_from_%s_term.cpp" % ("hybrid" if hybrid else "color")
        b = test_body(path, case, "ComputeJacobianAndResidual")
        tgt_color = shift_up(shift_left(img(0.0, 1.0, 1), 10), 5)
        dx_color, dy_color = shift_left(img(0.0, 1.0, 1), 10), shift_up(img(0.0, 1.0, 1), 5)
        tgt_depth = img(1.0, 2.0, 0)
        # (both tests pass the target depth image as the depth-gradient images)
        g[name] = {
            "cite": path + ":31-" + ("134" if hybrid else "112"), "hybrid": hybrid,
            "source_color": img(0.0, 1.0, 1).tolist(), "source_depth": img(0.0, 1.0, 0).tolist(),
            "target_color": tgt_color.tolist(), "target_depth": tgt_depth.tolist(),
            "dx_color": dx_color.tolist(), "dy_color": dy_color.tolist(),
            "source_xyz": orc.ref_rand_floats(300, 0.0, 1.0, 0).reshape(10, 10, 3).tolist(),
            "intrinsic": [[0.5, 0, 0.75], [0, 0.65, 0.35], [0, 0, 0]],
            "extrinsic": [[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]],
            "corresps": orc.ref_rand_vec4i(10, 0, 3, 0).tolist(),
            "ref_J_r": vec6_rows(b, "ref_J_r"), "ref_r": brace_list(b, "ref_r_raw"), "tol": 1e-4}

    image_vectors(g)
    cloud_vectors(g)
    g["reference_cases"] = ledger(g)

    for k, v in g.items():
        for name in ("ref_points", "ref_normals", "ref_colors", "ref_indices"):
            if name in v:
                assert len(v[name]) > 0, (k, name)
    with open(OUT, "w") as f:
        json.dump(g, f, indent=0)
    print("wrote", os.path.normpath(OUT), {k: len(json.dumps(v)) for k, v in g.items()})


if __name__ == "__main__":
    main()
