"""The OccupancyGrid rows of the reference's pybind11 module (cupoch_amd/cpp/src/pybind_module.cpp) with the reference's
Python names (src/python/cupoch_pybind/geometry/occupancygrid.cpp): names and defaults on the CPU, and on the GPU the
same bytes as the numpy restatement (tests/occgrid_exact.py).  Skips only where the module cannot be imported."""
import numpy as np
import pytest

import occgrid_exact as ox

F = np.float32


def module():
    try:
        from cupoch_amd import pybind as cph
    except Exception as e:      # not built and not buildable here
        pytest.skip("cupoch_pybind cannot be imported: %s" % e)
    return cph


def test_occupancy_rows_have_the_references_names_and_defaults():
    g = module().geometry
    o = g.OccupancyGrid()
    assert F(o.voxel_size) == F(0.05) and o.resolution == 512 and np.array_equal(o.origin, np.zeros(3, F))
    assert (F(o.clamping_thres_min), F(o.clamping_thres_max), F(o.prob_hit_log), F(o.prob_miss_log),
            F(o.occ_prob_thres_log)) == (F(-2.0), F(3.5), F(0.85), F(-0.4), F(0.0))
    assert o.visualize_free_area is True
    for name in ("voxel_size", "resolution", "clamping_thres_min", "clamping_thres_max", "prob_hit_log",
                 "prob_miss_log", "occ_prob_thres_log"):
        setattr(o, name, 2)
        assert getattr(o, name) == 2
    o.visualize_free_area = False
    o.origin = np.array([1, 2, 3], F)
    assert o.visualize_free_area is False and np.array_equal(o.origin, np.array([1, 2, 3], F))
    o = g.OccupancyGrid(0.1, 33)
    assert F(o.voxel_size) == F(0.1) and o.resolution == 33
    o = g.OccupancyGrid(voxel_size=0.1, resolution=33, origin=np.array([0.5, 0, 0], F))
    assert np.array_equal(o.origin, np.array([0.5, 0, 0], F))
    for name in ("voxels", "reconstruct", "insert", "set_free_area"):
        assert hasattr(g.OccupancyGrid, name), name
    assert not hasattr(g.OccupancyGrid, "create_from_voxel_grid")     # not built, and not pretended
    assert hasattr(g.PointCloud, "create_from_occupancy_grid")
    V = g.OccupancyVoxel
    v = V()
    assert list(v.grid_index) == [0, 0, 0] and np.isnan(v.prob_log) and list(v.color) == [0.0, 0.0, 1.0]
    assert list(V(np.array([1, 2, 3])).grid_index) == [1, 2, 3] and V(np.array([1, 2, 3]), 0.5).prob_log == 0.5
    v = V(grid_index=np.array([1, 2, 3]), prob_log=0.5, color=np.array([0.25, 0.5, 0.75], F))
    assert repr(v) == "geometry::OccupancyVoxel with grid_index: (1, 2, 3), prob_log: 0.5, color: (0.25, 0.5, 0.75)"
    v.prob_log, v.grid_index, v.color = 1.5, np.array([4, 5, 6]), np.array([1, 0, 0], F)
    assert v.prob_log == 1.5 and list(v.grid_index) == [4, 5, 6] and list(v.color) == [1.0, 0.0, 0.0]


@pytest.mark.gpu
def test_grid_through_the_pybind_module_equals_the_restatement():
    g = module().geometry
    res = 33
    free, ins = ox.scene("g", res, 5000)
    grid, ref = g.OccupancyGrid(ox.VOXEL, res, np.asarray(ox.ORIGINS[res], F)), ox.new_grid(res)
    grid.prob_hit_log, grid.occ_prob_thres_log = 0.7, 0.3
    ref.prob_hit_log, ref.occ_prob_thres_log = F(0.7), F(0.3)
    grid.set_free_area(free[1], free[2])
    ox.set_free_area(ref, free[1], free[2])
    cloud = g.PointCloud(ins[1])
    for max_range in (-1.0, 0.9):
        grid.insert(cloud, ins[2], max_range)
        ox.insert(ref, ins[1], ins[2], max_range)
    grid.insert(cloud, ins[2])                                        # max_range defaults to -1
    ox.insert(ref, ins[1], ins[2])

    def same(a, b):
        a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
        return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())

    assert same(grid.get_voxels(), ref.prob)
    ijk, p, _ = ox.extract(ref, ox.KNOWN)
    vox = grid.voxels
    assert len(p) > 1000 and len(vox) == len(p) and repr(grid) == "geometry::OccupancyGrid with %d voxels." % len(p)
    assert np.array_equal(np.array([v.grid_index for v in vox]), ijk) and same(np.array([v.prob_log for v in vox], F), p)
    assert all(list(v.color) == [0.0, 0.0, 1.0] for v in vox[:50])
    _, po, pts = ox.extract(ref, ox.OCCUPIED)
    pc = g.PointCloud.create_from_occupancy_grid(grid)
    assert len(po) > 100 and same(pc.points.cpu(), pts) and (pc.colors.cpu() == np.array([0, 0, 1], F)).all()
    assert same(grid.get_min_bound(), ox.get_min_bound(ref)) and same(grid.get_max_bound(), ox.get_max_bound(ref))
    known, v = grid.get_voxel(pts[0])
    assert known and F(v.prob_log) == po[0] and grid.is_occupied(pts[0]) and grid.is_unknown(np.array([99.0, 0, 0], F))
    grid.reconstruct(0.2, 16)
    assert len(grid.voxels) == 0 and grid.resolution == 16 and F(grid.voxel_size) == F(0.2)
