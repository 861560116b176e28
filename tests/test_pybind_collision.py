"""The collision rows of the reference's pybind11 module (cupoch_amd/cpp/src/pybind_module.cpp) with the reference's
Python names (src/python/cupoch_pybind/collision): names on the CPU, and on the GPU the reference's two unit tests and
one scene per side kind with the same pairs as the numpy restatement (tests/collision_exact.py).  Skips only where there
is nothing to build the module with."""
import numpy as np
import pytest

import collision_exact as ex

F = np.float32


def module():
    import importlib.util
    import shutil
    missing = [n for n in ("make", "g++") if shutil.which(n) is None] + ([] if importlib.util.find_spec("pybind11") else ["pybind11"])
    if missing:                 # nothing to build the module with: the only reason to skip
        pytest.skip("cupoch_pybind cannot be built here: no %s" % ", ".join(missing))
    from cupoch_amd import pybind as cph        # (a build or an import that breaks is a failure)
    return cph


def test_collision_rows_have_the_references_names():
    cph = module()
    c = cph.collision
    assert c.CollitionResult is c.CollisionResult                           # the reference's spelling, and the right one
    for name in ("is_collided", "get_collision_index_pairs", "get_first_collision_indices", "get_second_collision_indices", "first",
                 "second", "collision_index_pairs"):
        assert hasattr(c.CollitionResult, name), name
    assert [n for n in ("Unspecified", "Primitives", "VoxelGrid", "OccupancyGrid", "LineSet") if hasattr(c.CollitionResult.Type, n)] == \
        ["Unspecified", "Primitives", "VoxelGrid", "OccupancyGrid", "LineSet"]
    assert int(c.Primitive.Type.Box) == 1 and int(c.Primitive.Type.Sphere) == 2 and int(c.Primitive.Type.Capsule) == 3
    for name in ("Primitive", "Box", "Sphere", "Capsule", "Cylinder", "PrimitiveArray", "compute_intersection", "create_voxel_grid"):
        assert hasattr(c, name), name
    assert not hasattr(c, "create_voxel_grid_with_sweeping") and not hasattr(c, "create_triangle_mesh")
    doc = c.compute_intersection.__doc__
    assert doc.count("margin:") == 11 and doc.count("= 0.0") == 11 and "lineset" in doc and "occgrid" in doc and "primitives" in doc
    b = c.Box(np.array([1, 2, 3], F))
    assert list(b.lengths) == [1, 2, 3] and np.array_equal(b.transform, np.eye(4, dtype=F)) and b.type == c.Primitive.Type.Box
    s = c.Sphere(0.5, np.array([1, 2, 3], F))
    assert s.radius == 0.5 and list(s.transform[:3, 3]) == [1, 2, 3]
    cap = c.Capsule(0.25, 2.0)
    assert (cap.radius, cap.height) == (0.25, 2.0)
    box = cap.get_axis_aligned_bounding_box()                                 # host arithmetic: no GPU needed
    assert list(box.get_min_bound()) == [-0.25, -0.25, -1.25] and list(box.get_max_bound()) == [0.25, 0.25, 1.25]
    arr = c.PrimitiveArray()
    arr.append(b), arr.append(s)
    assert len(arr) == 2
    for name in ("points", "lines", "colors", "has_points", "has_lines", "has_colors", "get_line_coordinate", "paint_uniform_color",
                 "create_from_axis_aligned_bounding_box", "translate", "scale", "rotate", "transform", "get_axis_aligned_bounding_box"):
        assert hasattr(cph.geometry.LineSet, name), name


def _grid(g, keys, vs, origin, as_given=False):
    out = g.VoxelGrid()
    out.voxel_size, out.origin = float(vs), np.asarray(origin, F)
    if as_given:
        out.voxels = g.DeviceVoxelMap(np.ascontiguousarray(keys, np.int32), np.ones((len(keys), 3), F))
    else:
        out.add_voxels([g.Voxel(np.asarray(k, np.int32)) for k in keys])
    return out


@pytest.mark.gpu
def test_reference_unit_tests_through_the_pybind_module():
    cph = module()
    g, c = cph.geometry, cph.collision
    assert not c.compute_intersection(g.VoxelGrid(), g.VoxelGrid()).is_collided()
    v1, v2 = _grid(g, [[0, 0, 0], [5, 0, 0]], 1.0, (0, 0, 0)), _grid(g, [[0, 0, 0], [10, 0, 0]], 1.0, (0, 0, 0))
    r = c.compute_intersection(v1, v2)
    assert r.is_collided() and r.get_collision_index_pairs().tolist() == [[0, 0]] and repr(r) == "collision::CollisionResult with 1 collisions."
    assert r.first == c.CollitionResult.Type.VoxelGrid and list(r.get_first_collision_indices().cpu()) == [0]
    assert not c.compute_intersection(g.VoxelGrid(), g.LineSet()).is_collided()
    ls = g.LineSet(np.array([[-0.1, -0.1, -0.1], [-0.1, -0.1, 1.1], [1.1, 1.1, 1.1]], F), np.array([[0, 1], [0, 2]], np.int32))
    assert c.compute_intersection(v1, ls).get_collision_index_pairs().tolist() == [[0, 1]]
    assert c.compute_intersection(ls, v1, margin=0.0).get_collision_index_pairs().tolist() == [[1, 0]]
    a, b = ls.get_line_coordinate(1)
    assert list(a) == [F(-0.1)] * 3 and list(b) == [F(1.1)] * 3 and repr(ls) == "geometry::LineSet with 2 lines."
    a, b = ls.get_line_coordinate(2)                                           # out of range: zeros
    assert not np.asarray(a).any() and not np.asarray(b).any()
    R = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F)                         # a quarter turn about z, about the origin
    assert ls.rotate(R, center=False) is ls
    assert np.array_equal(np.asarray(ls.points.cpu()), np.array([[0.1, -0.1, -0.1], [0.1, -0.1, 1.1], [-1.1, 1.1, 1.1]], F))


@pytest.mark.gpu
def test_scene_through_the_pybind_module_equals_the_restatement():
    cph = module()
    g, c = cph.geometry, cph.collision
    a_keys, b_keys, pts, lines, prims, cloud, cap = ex.scene_inputs()
    a = _grid(g, a_keys, ex.SCENE_VS, ex.SCENE_ORIGIN)
    b = _grid(g, b_keys, ex.SCENE_VS_B, ex.SCENE_ORIGIN + F(0.037), as_given=True)
    rev = _grid(g, a_keys[::-1], ex.SCENE_VS, ex.SCENE_ORIGIN, as_given=True)
    ls = g.LineSet(pts, lines)
    occ = g.OccupancyGrid(ex.SCENE_VS, ex.SCENE_RES, ex.SCENE_ORIGIN)
    occ.insert(g.PointCloud(cloud), ex.SCENE_ORIGIN + F(0.01))
    occ_index = np.array([v.grid_index for v in occ.extract_occupied_voxels()], np.int32).reshape(-1, 3)
    assert len(occ_index) > 50

    def make(P):
        if P.type == ex.BOX:
            return c.Box(P.param, P.transform)
        if P.type == ex.SPHERE:
            s = c.Sphere(float(P.param[0]))
            s.transform = P.transform
            return s
        return (c.Capsule if P.type == ex.CAPSULE else c.Cylinder)(float(P.param[0]), float(P.param[1]), P.transform)

    arr = c.PrimitiveArray()
    for P in prims:
        arr.append(make(P))
    want = ex.scene_expected(occ_index)
    m = ex.SCENE_MARGIN
    sides = {"v": a, "l": ls, "o": occ, "p": arr, "r": rev}
    for name, pairs in want.items():
        if name == "capsule":
            continue
        x, y = sides[name[0]], (b if name in ("vv", "rv") else sides[name[1]])
        got = c.compute_intersection(x, y, m).get_collision_index_pairs()
        assert np.array_equal(got, pairs), name
    vg = c.create_voxel_grid(make(cap), 0.05)
    assert np.array_equal(vg.voxels.cpu()[0], want["capsule"]) and np.array_equal(vg.origin, cap.transform[:3, 3])
    assert len(c.create_voxel_grid(make(cap), 0.0).voxels) == 0
    mn, mx = ex.primitive_aabb(cap)
    box = make(cap).get_axis_aligned_bounding_box()
    assert np.array_equal(box.get_min_bound(), mn) and np.array_equal(box.get_max_bound(), mx)
    edges = g.LineSet.create_from_axis_aligned_bounding_box(box)
    assert len(edges.points) == 8 and len(edges.lines) == 12 and np.array_equal(edges.get_min_bound(), mn)
    assert edges.paint_uniform_color(np.array([1, 0, 0], F)).has_colors() and np.array_equal(edges.colors.cpu(), np.tile([1, 0, 0], (12, 1)))
    edges.translate(np.array([1, 2, 3], F))
    assert np.allclose(edges.get_min_bound(), mn + np.array([1, 2, 3], F), atol=1e-6)
