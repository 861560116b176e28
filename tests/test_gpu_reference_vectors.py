"""GPU: every recorded case of the reference's image.cpp, pointcloud.cpp and lineset.cpp (tests/golden/reference_tests.json,
tests/test_reference_vectors_cpu.py) replayed through the Python mirror, once from a numpy array and once from a device
tensor, and compared as the reference's test compares: image.cpp on the bytes (EXPECT_EQ per byte), the clouds under
ExpectEQ's threshold 1e-4.  These are 5 x 5 and 6 x 3 images and 100-point clouds; the larger shapes are in
test_gpu_image.py, test_gpu_depth.py and test_gpu_laserscan.py, against the restatements these vectors pin."""
import numpy as np
import pytest

import test_reference_vectors_cpu as rv

pytestmark = pytest.mark.gpu

F = np.float32
SIDES = ["numpy", "cuda"]
GOLDEN_KEYS = rv.IMAGE_VALUE_KEYS + rv.IMAGE_SHAPE_KEYS + rv.CLOUD_KEYS      # the keys this module consumes


def put(a, side):
    import torch
    a = np.ascontiguousarray(a)
    return a if side == "numpy" else torch.from_numpy(a).cuda()


def image_replayed(e, side):
    from cupoch_amd import geometry as g
    im = g.Image(put(rv.image_input(e), side))
    assert (im.width, im.height, im.num_of_channels, im.bytes_per_channel) == (e["width"], e["height"], e["channels"], e["bytes_per_channel"])
    if e.get("pre") == "create_float_image":
        im = im.create_float_image()
    call = e["call"]
    if call == "create_float_image":
        return im.create_float_image()              # the reference's helper passes no type
    if call == "convert_depth_to_float_image":
        return im.convert_depth_to_float_image(e["args"]["depth_scale"], e["args"]["depth_trunc"])
    if call == "filter":
        T = g.ImageFilterType
        return im.filter({"Gaussian3": T.Gaussian3, "Gaussian5": T.Gaussian5, "Gaussian7": T.Gaussian7, "Sobel3Dx": T.Sobel3dx,
                          "Sobel3Dy": T.Sobel3dy}[e["args"]["filter_type"]])
    if call == "filter_horizontal":
        return im.filter_horizontal(e["args"]["kernel"])
    return getattr(im, call)()                      # downsample, transpose, flip_vertical, flip_horizontal


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("key", rv.IMAGE_VALUE_KEYS)
def test_image_cases_give_the_reference_bytes(golden, key, side):
    e = golden[key]
    out = image_replayed(e, side)
    assert not out.is_empty()
    rv.image_compare(e, np.ascontiguousarray(np.asarray(out)))


def image_state(im):
    data_size = 0 if im.data is None else int(np.asarray(im).size) * im.bytes_per_channel
    return {"width": im.width, "height": im.height, "num_of_channels": im.num_of_channels, "bytes_per_channel": im.bytes_per_channel,
            "data_size": data_size, "is_empty": im.is_empty(), "min_bound": im.get_min_bound().tolist(),
            "max_bound": im.get_max_bound().tolist(), "test_image_boundary_0_0": im.test_image_boundary(0, 0),
            "bytes_per_line": im.bytes_per_line()}


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("key", rv.IMAGE_SHAPE_KEYS)
def test_image_shape_cases(golden, key, side):
    from cupoch_amd import geometry as g
    e = golden[key]
    if e["prepare"] is None:
        im = g.Image()
    else:
        w, h, c, b = e["prepare"]
        im = g.Image(put(np.zeros((h, w, c), rv._DTYPES[b]), side))     # Prepare: a zeroed buffer of these dimensions
    if e["clear"]:
        im.clear()
    assert image_state(im) == e["expect"]


def cloud(points, side, normals=None, colors=None):
    from cupoch_amd import geometry as g
    pc = g.PointCloud(put(np.array(points, F), side))
    if normals is not None:
        pc.normals = put(np.array(normals, F), side)
    if colors is not None:
        pc.colors = put(np.array(colors, F), side)
    return pc


def xyz(pc):
    return np.asarray(pc.points.cpu() if hasattr(pc.points, "cpu") else pc.points, F).reshape(-1, 3)


def flags(x, names):
    out = {n: getattr(x, n)() for n in names if n not in ("min_bound", "max_bound")}
    out["min_bound"], out["max_bound"] = x.get_min_bound(), x.get_max_bound()
    return out


def same_flags(got, want, tol):
    for k, v in want.items():
        if k in ("min_bound", "max_bound"):
            assert rv._near(got[k], v, tol), k              # ExpectEQ(Vector3f, Vector3f), THRESHOLD_1E_4
        else:
            assert got[k] is v, k


@pytest.mark.parametrize("side", SIDES)
def test_pointcloud_bounds(golden, side):
    for key, get in (("pointcloud_get_min_bound", "get_min_bound"), ("pointcloud_get_max_bound", "get_max_bound")):
        g = golden[key]
        pc = cloud(g["points"], side)
        for _ in range(2):                                   # the reference asks twice
            assert rv._near(getattr(pc, get)(), g["ref"], g["tol"])


@pytest.mark.parametrize("side", SIDES)
def test_pointcloud_selections(golden, side):
    g = golden["pointcloud_select_by_index"]
    out = cloud(g["points"], side).select_by_index(put(np.array(g["indices"], np.int64), side))
    assert rv._near(rv._lex(xyz(out)), rv._lex(g["ref_points"]), g["tol"])
    g = golden["pointcloud_select_by_mask"]
    mask = np.zeros(len(g["points"]), bool)
    mask[g["indices"]] = True
    out = cloud(g["points"], side).select_by_mask(put(mask, side))
    assert rv._near(rv._lex(xyz(out)), rv._lex(g["ref_points"]), g["tol"])
    g = golden["pointcloud_uniform_down_sample"]
    out = cloud(g["points"], side).uniform_down_sample(g["every_k_points"])
    assert rv._near(xyz(out), g["ref_points"], g["tol"])    # in order: ExpectEQ without a sort
    g = golden["pointcloud_crop"]
    from cupoch_amd import geometry as geo
    out = xyz(cloud(g["points"], side).crop(geo.AxisAlignedBoundingBox(g["min_bound"], g["max_bound"])))
    pts, lo, hi = np.array(g["points"], F), np.array(g["min_bound"], F), np.array(g["max_bound"], F)
    assert (out >= lo).all() and (out <= hi).all()          # ExpectLE / ExpectGE: all the reference asks
    assert out.tobytes() == pts[((pts >= lo) & (pts <= hi)).all(1)].tobytes()


@pytest.mark.parametrize("side", SIDES)
def test_pointcloud_container_cases(golden, side):
    from cupoch_amd import geometry as geo
    names = ("is_empty", "has_points", "has_normals", "has_colors", "min_bound", "max_bound")
    g = golden["pointcloud_constuctor"]
    same_flags(flags(geo.PointCloud(), names), g["expect"], g["tol"])
    g = golden["pointcloud_clear"]
    pc = cloud(g["points"], side, g["normals"], g["colors"])
    same_flags(flags(pc, names), g["expect_set"], g["tol"])
    pc.clear()
    same_flags(flags(pc, names), g["expect_cleared"], g["tol"])
    g = golden["pointcloud_is_empty"]
    pc = geo.PointCloud()
    assert pc.is_empty() is g["expect_before"]
    pc.points = put(np.array(g["points"], F), side)
    assert pc.is_empty() is g["expect_after"]
    for what in ("points", "normals", "colors"):
        g = golden["pointcloud_has_" + what]
        pc = geo.PointCloud()
        assert getattr(pc, g["flag"])() is g["expect_before"]
        for attribute in g["set"]:                           # value-initialised vectors of `size`, points first
            setattr(pc, attribute, put(np.zeros((g["size"], 3), F), side))
        assert getattr(pc, g["flag"])() is g["expect_after"]


@pytest.mark.parametrize("side", SIDES)
def test_lineset_cases(golden, side):
    from cupoch_amd import geometry as geo
    names = ("is_empty", "has_points", "has_lines", "has_colors", "min_bound", "max_bound")
    g = golden["lineset_constructor"]
    same_flags(flags(geo.LineSet(), names), g["expect"], g["tol"])
    g = golden["lineset_clear"]
    ls = geo.LineSet(put(np.array(g["points"], F), side), put(np.array(g["lines"], np.int32), side))
    ls.colors = put(np.array(g["colors"], F), side)
    same_flags(flags(ls, names), g["expect_set"], g["tol"])
    ls.clear()
    same_flags(flags(ls, names), g["expect_cleared"], g["tol"])
