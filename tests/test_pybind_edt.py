"""The DistanceTransform rows of the reference's pybind11 module (cupoch_amd/cpp/src/pybind_module.cpp) with the
reference's Python names (src/python/cupoch_pybind/geometry/distancetransform.cpp): names, defaults and reprs on the CPU,
and on the GPU the reference's unit test and the 65^3 scene with the same bytes as the numpy restatement
(tests/edt_exact.py).  Skips only where the module cannot be imported."""
import numpy as np
import pytest

import edt_exact as ex

F = np.float32


def module():
    try:
        from cupoch_amd import pybind as cph
    except Exception as e:      # not built and not buildable here
        pytest.skip("cupoch_pybind cannot be imported: %s" % e)
    return cph


def test_distancetransform_rows_have_the_references_names_and_defaults():
    g = module().geometry
    v = g.DistanceVoxel()
    assert list(v.nearest_index) == [0, 0, 0] and v.distance == 0.0
    assert repr(v) == "geometry::DistanceVoxel with nearest_index: (0, 0, 0), distance: 0)"
    v.nearest_index, v.distance = np.array([261, 261, 261]), 1.5
    assert repr(v) == "geometry::DistanceVoxel with nearest_index: (261, 261, 261), distance: 1.5)"
    d = g.DistanceTransform()
    assert F(d.voxel_size) == F(0.05) and d.resolution == 512 and list(d.origin) == [0, 0, 0]
    assert repr(d) == "geometry::DistanceTransform with 512 resolution."
    d = g.DistanceTransform(0.1, 65)                                        # origin defaults to zero
    assert list(d.origin) == [0, 0, 0] and repr(d) == "geometry::DistanceTransform with 65 resolution."
    d = g.DistanceTransform(voxel_size=0.2, resolution=33, origin=np.array([1, 2, 3], F))
    assert F(d.voxel_size) == F(0.2) and d.resolution == 33 and list(d.origin) == [1, 2, 3]
    d.voxel_size, d.resolution, d.origin = 0.5, 16, np.array([0, 1, 0], F)  # read-write attributes
    assert (F(d.voxel_size), d.resolution, list(d.origin)) == (F(0.5), 16, [0, 1, 0])
    doc = g.DistanceTransform.__init__.__doc__
    assert "voxel_size:" in doc and "resolution:" in doc and "origin:" in doc and "= array([0., 0., 0.]" in doc
    for name in ("reconstruct", "compute_edt", "get_distance", "get_distances", "create_from_occupancy_grid", "voxel_size",
                 "resolution", "origin", "compute_voronoi_diagram", "get_voxel"):
        assert hasattr(g.DistanceTransform, name), name
    assert "voxel_size:" in g.DistanceTransform.reconstruct.__doc__ and "resolution:" in g.DistanceTransform.reconstruct.__doc__
    assert "VoxelGrid" in g.DistanceTransform.compute_edt.__doc__


@pytest.mark.gpu
def test_reference_unit_test_through_the_pybind_module():
    g = module().geometry
    grid = g.VoxelGrid()
    grid.voxel_size = 1.0
    grid.add_voxel(g.Voxel(np.array([5, 5, 5])))
    d = g.DistanceTransform(1.0, 512)
    d.compute_voronoi_diagram(grid)
    inside, v = d.get_voxel(np.zeros(3, F))
    assert inside and list(v.nearest_index) == [261, 261, 261] and F(v.distance) == np.sqrt(F(75))
    assert d.get_distance(np.full(3, 5.5, F)) == 0.0 and np.isnan(d.get_distance(np.array([256.5, 0, 0], F)))


@pytest.mark.gpu
def test_scene_through_the_pybind_module_equals_the_restatement():
    cph = module()
    g = cph.geometry
    pts = ex.scene_points()
    grid = g.VoxelGrid.create_from_point_cloud_within_bounds(g.PointCloud(pts), ex.SCENE_VS, ex.SCENE_LO, -ex.SCENE_LO)
    keys = grid.voxels.cpu()[0]
    d = g.DistanceTransform(ex.SCENE_VS, ex.SCENE_RES, ex.SCENE_ORIGIN)
    assert np.isposinf(d.get_distance(ex.SCENE_ORIGIN))                    # no sites yet
    d.compute_edt(grid)
    near, dist = d.get_voxels()
    ex.scene_check(keys, near, dist)
    c = ex.cells_of_points(pts, ex.SCENE_VS, ex.SCENE_ORIGIN, ex.SCENE_RES)
    ins = ex.inside(c, ex.SCENE_RES)
    lin = (c[ins, 0] * ex.SCENE_RES + c[ins, 1]) * ex.SCENE_RES + c[ins, 2]
    for q in (d.get_distances(pts), d.get_distances(cph.utility.Vector3fVector(pts))):
        assert (q[ins].view(np.uint32) == dist[lin].view(np.uint32)).all() and np.isnan(q[~ins]).all()
    # create_from_occupancy_grid computes
    occ = g.OccupancyGrid(0.1, 32)
    occ.add_voxel(np.array([3, 4, 5]), True)
    t = g.DistanceTransform.create_from_occupancy_grid(occ)
    assert t.resolution == 32 and F(t.voxel_size) == F(0.1)
    inside, v = t.get_voxel((np.array([3, 4, 8], F) - 16 + F(0.5)) * F(0.1))
    assert inside and list(v.nearest_index) == [3, 4, 5] and F(v.distance) == F(3.0) * F(0.1)
