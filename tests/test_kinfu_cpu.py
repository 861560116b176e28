"""kinfu.KinfuPipeline without a GPU: the mirror's option defaults and names, the pybind11 module's `kinfu` rows with the
reference's names (src/python/cupoch_pybind/kinfu/kinfu.cpp), and the C ABI's one-pass model pyramid declared, exported
and bound."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT

FIELDS = ("num_pyramid_levels", "diameter", "sigma_depth", "sigma_space", "depth_cutoff", "tsdf_length", "tsdf_resolution",
          "sdf_trunc", "tsdf_color_type", "tsdf_origin", "distance_threshold", "icp_iterations", "tf_type")


def test_mirror_option_defaults_are_the_references():
    from cupoch_amd import integration, kinfu, registration
    o = kinfu.KinfuOption()
    assert (o.num_pyramid_levels, o.diameter, o.sigma_depth, o.sigma_space, o.depth_cutoff) == (4, 1, 1.0, 10.0, 3.0)
    assert (o.tsdf_length, o.tsdf_resolution, o.sdf_trunc) == (8.0, 512, pytest.approx(0.05))
    assert o.tsdf_color_type == integration.TSDFVolumeColorType.RGB8 and np.array_equal(o.tsdf_origin, np.zeros(3, np.float32))
    assert (o.distance_threshold, o.icp_iterations) == (0.5, [20, 20, 20, 20])
    assert o.tf_type == registration.TransformationEstimationType.PointToPlane
    for name in FIELDS:
        assert hasattr(o, name), name
    # the new keywords come after the ones the constructor had
    import inspect
    names = list(inspect.signature(kinfu.KinfuOption.__init__).parameters)
    assert names[-3:] == ["diameter", "sigma_depth", "sigma_space"] and names[1] == "num_pyramid_levels"
    assert kinfu.KinfuOption(2, 1.0, 0.1, (5, 5)).icp_iterations == [5, 5]


def test_mirror_pipeline_names():
    from cupoch_amd import integration, kinfu
    for name in ("reset", "process_frame", "extract_point_cloud"):
        assert callable(getattr(kinfu.KinfuPipeline, name)), name
    assert not hasattr(kinfu.KinfuPipeline, "extract_triangle_mesh")     # no TriangleMesh type, and not pretended
    assert callable(integration.UniformTSDFVolume.raycast_levels)
    for name in ("create_volume", "integrate_and_raycast", "point_cloud_pyramid", "pose_estimation"):
        assert callable(getattr(kinfu, name)), name                      # the free functions stay
    src = open(os.path.join(ROOT, "cupoch_amd", "kinfu.py")).read()
    for attr in ("cur_pose", "frame_id", "volume", "model_pyramid", "option", "intrinsic"):
        assert re.search(r"self\.%s = " % attr, src), attr


def test_pybind_kinfu_rows_have_the_references_names():
    try:
        from cupoch_amd import pybind as cph
    except Exception as e:      # not built and not buildable here
        pytest.skip("cupoch_pybind cannot be imported: %s" % e)
    k = cph.kinfu
    o = k.KinfuOption()
    for name in FIELDS:
        assert hasattr(o, name), name
    assert (o.num_pyramid_levels, o.diameter, o.sigma_depth, o.sigma_space, o.depth_cutoff) == (4, 1, 1.0, 10.0, 3.0)
    assert (o.tsdf_length, o.tsdf_resolution, o.sdf_trunc) == (8.0, 512, np.float32(0.05))
    assert o.tsdf_color_type == cph.integration.TSDFVolumeColorType.RGB8
    assert np.array_equal(o.tsdf_origin, np.zeros(3, np.float32))
    assert (o.distance_threshold, o.icp_iterations) == (0.5, [20, 20, 20, 20])
    assert o.tf_type == cph.registration.TransformationEstimationType.PointToPlane
    o.num_pyramid_levels, o.icp_iterations, o.tsdf_origin = 2, [3, 4], np.array([1, 2, 3], np.float32)
    import copy
    c = copy.deepcopy(o)
    assert (c.num_pyramid_levels, c.icp_iterations) == (2, [3, 4]) and np.array_equal(c.tsdf_origin, [1, 2, 3])
    assert copy.copy(o).icp_iterations == [3, 4] and k.KinfuOption(o).num_pyramid_levels == 2
    with pytest.raises(TypeError):
        k.KinfuOption(4, 1)                                              # a default constructor plus fields, as the reference
    for name in ("reset", "process_frame", "extract_point_cloud", "cur_pose", "model_pyramid"):
        assert hasattr(k.KinfuPipeline, name), name
    for name in ("extract_triangle_mesh", "__copy__", "__deepcopy__"):
        assert not hasattr(k.KinfuPipeline, name), name


def test_raycast_levels_is_declared_exported_and_bound():
    import ctypes as C
    from cupoch_amd import _lib
    _lib.build()
    src = open(os.path.join(ROOT, "include", "mi_icp.h")).read()
    m = re.search(r"MI_ICP_API\s+int\s+mi_icp_tsdf_raycast_levels\s*\(([^;]*?)\)\s*;", src, flags=re.S)
    assert m and "mem_kind" not in m.group(1) and re.search(r"int64_t\s*\*\s*m\b", m.group(1))
    assert re.search(r"#define\s+MI_ICP_TSDF_MAX_LEVELS\s+16\b", src)
    assert "CreatePyramidLevel" in src and "raycast_levels" in src       # the contract block names the levels' cameras
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert re.search(r" T mi_icp_tsdf_raycast_levels\b", out)
    res, args = _lib.SIGNATURES["mi_icp_tsdf_raycast_levels"]
    assert res is C.c_int and len(args) == 14 and args[-1] == C.POINTER(C.c_int64)
    assert len(_lib.SIGNATURES["mi_icp_tsdf_raycast"][1]) == 14          # (that one ends in mem_kind)
