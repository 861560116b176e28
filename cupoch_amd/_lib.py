"""Loader for libmi_icp.so (the HIP engine behind this package).

There is no CPU fallback: if the shared library is missing or cannot be
loaded, importing a compute entry point raises.  `build()` compiles it in-tree
with hipcc for gfx950 (it cross-compiles on a box without a GPU).
"""
import ctypes as C
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libmi_icp.so")
INCLUDE = os.path.join(ROOT, "include")

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-I/opt/rocm/include"]
# the library's translation units (csrc/ctx.h says what each holds); compiled side by side, then linked
UNITS = ["mi_icp", "mi_build", "mi_geometry", "mi_voxel", "mi_rgbd", "mi_tsdf", "mi_stsdf", "mi_occgrid", "mi_voxelgrid", "mi_collision", "mi_graph", "mi_laserscan", "mi_image", "mi_sgm", "mi_feature", "mi_edt", "mi_knn", "mi_comm", "mi_debug"]
OBJ_DIR = os.path.join(LIB_DIR, "obj")

MI_ICP_HOST, MI_ICP_DEVICE = 0, 1
EST_POINT_TO_POINT, EST_POINT_TO_PLANE, EST_SYMMETRIC, EST_GENERALIZED = 1, 2, 3, 5
EST_COLORED = 4


MI_ICP_ERR_INVALID, MI_ICP_ERR_STATE, MI_ICP_ERR_HIP, MI_ICP_ERR_COMM, MI_ICP_ERR_NO_DEVICE = -1, -2, -3, -4, -5


class MiIcpError(RuntimeError):
    code = None     # the C ABI's status where the error came from a call (engine.Engine._chk)


def _sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC)
                  if f.endswith((".hip", ".h"))) + [os.path.join(INCLUDE, "mi_icp.h"),
                                                 os.path.join(INCLUDE, "mi_icp_debug.h")]


def needs_build():
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    return any(os.path.getmtime(s) > t for s in _sources())


def build(force=False, verbose=False, variant=None, defines=()):
    """hipcc --offload-arch=gfx950 -c csrc/<unit>.hip for every unit (in parallel; a unit whose object is newer than
    every source is kept), then hipcc -shared ... -o cupoch_amd/lib/libmi_icp.so
    variant / defines: a second build for same-box A/B runs (MI_ICP_LIB_PATH), e.g. variant="ab",
    defines=("-DNAME=1",) -> cupoch_amd/lib/libmi_icp_ab.so
    Safe against several processes building at once (every rank of a multi-process test imports the package): one
    file lock around the whole build, objects and the library written under a temporary name and renamed; objects
    compiled with other flags / defines are never reused (a stamp in the object directory holds their hash)."""
    lib_path = LIB_PATH if not variant else os.path.join(LIB_DIR, "libmi_icp_%s.so" % variant)
    obj_dir = OBJ_DIR if not variant else OBJ_DIR + "_" + variant
    if not force and not variant and not needs_build():
        return LIB_PATH
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise MiIcpError("hipcc not found; cannot build libmi_icp.so")
    os.makedirs(obj_dir, exist_ok=True)
    import fcntl
    import hashlib
    with open(os.path.join(LIB_DIR, ".build.lock"), "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            if not force and not variant and not needs_build():
                return LIB_PATH          # (another process built it while this one waited)
            return _build_locked(hipcc, lib_path, obj_dir, force, verbose, tuple(defines), hashlib)
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)


def _build_locked(hipcc, lib_path, obj_dir, force, verbose, defines, hashlib):
    headers = [s for s in _sources() if s.endswith(".h")]
    newest_header = max(os.path.getmtime(h) for h in headers)
    flags_hash = hashlib.sha1(" ".join(HIPCC_FLAGS + list(defines)).encode()).hexdigest()
    stamp = os.path.join(obj_dir, "flags.stamp")
    if not (os.path.exists(stamp) and open(stamp).read().strip() == flags_hash):
        force = True                     # objects of another flag set: none may be reused

    def compile_unit(u):
        src, obj = os.path.join(CSRC, u + ".hip"), os.path.join(obj_dir, u + ".o")
        if not force and os.path.exists(obj) and os.path.getmtime(obj) > max(newest_header, os.path.getmtime(src)):
            return obj
        tmp = "%s.tmp.%d" % (obj, os.getpid())
        cmd = [hipcc] + HIPCC_FLAGS + list(defines) + ["-c", src, "-o", tmp]
        if verbose:
            print(" ".join(cmd[:-1] + [obj]), flush=True)
        subprocess.check_call(cmd)
        os.replace(tmp, obj)
        return obj

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=len(UNITS)) as pool:
        objs = list(pool.map(compile_unit, UNITS))
    with open(stamp + ".tmp", "w") as f:
        f.write(flags_hash + "\n")
    os.replace(stamp + ".tmp", stamp)
    tmp = "%s.tmp.%d" % (lib_path, os.getpid())
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", tmp]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    os.replace(tmp, lib_path)
    return lib_path


ITERATION_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_float, C.c_float)   # mi_icp_iteration_fn


class Params(C.Structure):
    _fields_ = [("relative_fitness", C.c_float), ("relative_rmse", C.c_float),
                ("max_iteration", C.c_int32), ("det_thresh", C.c_float)]


class Result(C.Structure):
    _fields_ = [("transformation", C.c_float * 16), ("fitness", C.c_float),
                ("inlier_rmse", C.c_float), ("n_correspondences", C.c_int64),
                ("iterations", C.c_int32), ("nn_passes", C.c_int32)]


class OdometryOption(C.Structure):
    _fields_ = [("num_levels", C.c_int32), ("iterations", C.c_int32 * 8), ("max_depth_diff", C.c_float),
                ("min_depth", C.c_float), ("max_depth", C.c_float), ("nu", C.c_float), ("sigma2_init", C.c_float),
                ("inv_sigma_mat_diag", C.c_float * 6)]


class OccGridParams(C.Structure):                      # mi_icp_occgrid_params
    _fields_ = [("voxel_size", C.c_float), ("origin", C.c_float * 3), ("clamping_thres_min", C.c_float),
                ("clamping_thres_max", C.c_float), ("prob_hit_log", C.c_float), ("prob_miss_log", C.c_float),
                ("occ_prob_thres_log", C.c_float)]


class Primitive(C.Structure):                          # mi_icp_primitive (80 bytes)
    _fields_ = [("type", C.c_int32), ("transform", C.c_float * 16), ("param", C.c_float * 3)]


class CollisionSide(C.Structure):                      # mi_icp_collision_side
    _fields_ = [("kind", C.c_int32), ("keys_sorted", C.c_int32), ("keys", C.c_void_p), ("keys_index", C.c_void_p),
                ("m", C.c_int64),
                ("voxel_size", C.c_float), ("origin", C.c_float * 3), ("grid", C.c_void_p),
                ("grid_params", OccGridParams), ("points", C.c_void_p), ("n_points", C.c_int64),
                ("lines", C.c_void_p), ("n_lines", C.c_int64), ("primitives", C.c_void_p),
                ("n_primitives", C.c_int64)]


class FgrOption(C.Structure):                          # mi_icp_fgr_option (the reference's seven defaults)
    _fields_ = [("division_factor", C.c_float), ("use_absolute_scale", C.c_int32), ("decrease_mu", C.c_int32),
                ("maximum_correspondence_distance", C.c_float), ("iteration_number", C.c_int32),
                ("tuple_scale", C.c_float), ("maximum_tuple_count", C.c_int32)]


COLLISION_VOXELGRID, COLLISION_OCCGRID, COLLISION_LINESET, COLLISION_PRIMITIVES = 1, 2, 3, 4

# name -> (restype, argtypes); must list every MI_ICP_API symbol of include/mi_icp.h
_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGNATURES = {
    "mi_icp_create": (_I, [_I, C.POINTER(_P)]),
    "mi_icp_destroy": (None, [_P]),
    "mi_icp_last_error": (C.c_char_p, [_P]),
    "mi_icp_version": (C.c_char_p, []),
    "mi_icp_set_stream": (_I, [_P, _P]),
    "mi_icp_synchronize": (_I, [_P]),
    "mi_icp_set_target": (_I, [_P, _P, _P, _P, _L, _I]),
    "mi_icp_set_source": (_I, [_P, _P, _P, _P, _L, _I]),
    "mi_icp_search_radius_1nn": (_I, [_P, _P, _F, _P, _P, _I, _P]),
    "mi_icp_get_correspondences": (_I, [_P, _P, _L, C.POINTER(_L), _I]),
    "mi_icp_set_correspondences": (_I, [_P, _P, _L, _I]),
    "mi_icp_compute_system": (_I, [_P, _I, _P, _P]),
    "mi_icp_compute_transformation": (_I, [_P, _I, _P, _F, _P]),
    "mi_icp_compute_rmse": (_I, [_P, _I, _P, C.POINTER(_F)]),
    "mi_icp_solve_system": (_I, [_P, _F, _P]),
    "mi_icp_kabsch_from_sums": (_I, [_P, _L, _P]),
    "mi_icp_vector6_to_matrix4": (None, [_P, _P]),
    "mi_icp_lzf_decompress": (_L, [_P, _L, _P, _L]),
    "mi_icp_lzf_compress": (_L, [_P, _L, _P, _L]),
    "mi_icp_evaluate_registration": (_I, [_P, _F, _P, C.POINTER(Result)]),
    "mi_icp_registration_icp": (_I, [_P, _I, _F, _P, C.POINTER(Params), C.POINTER(Result)]),
    "mi_icp_icp_begin": (_I, [_P, _I, _F, _P, _F, C.POINTER(Result)]),
    "mi_icp_icp_iterate": (_I, [_P, _I, C.POINTER(Result)]),
    "mi_icp_transform": (_I, [_P, _P, _P, _P, _P, _L, _I]),
    "mi_icp_compute_bounds": (_I, [_P, _P, _L, _I, _P, _P, _P]),
    "mi_icp_affine": (_I, [_P, _P, _F, _I, _P, _P, _P, _P, _P, _L, _I]),
    "mi_icp_voxel_downsample": (_I, [_P, _P, _P, _P, _L, _F, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_select_by_index": (_I, [_P, _P, _P, _P, _L, _P, _L, _I, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_select_by_mask": (_I, [_P, _P, _P, _P, _L, _P, _L, _I, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_uniform_downsample": (_I, [_P, _P, _P, _P, _L, _L, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_remove_statistical_outliers": (_I, [_P, _P, _P, _P, _L, _I, _F, _P, _P, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_remove_radius_outliers": (_I, [_P, _P, _P, _P, _L, _I, _F, _P, _P, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_cluster_dbscan": (_I, [_P, _P, _L, _F, _L, _I, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_segment_plane": (_I, [_P, _P, _L, _F, _L, _L, C.c_uint64, _P, _P, _P, C.POINTER(_L), C.POINTER(_L), C.POINTER(_L), _I]),
    "mi_icp_iss_keypoints": (_I, [_P, _P, _L, _F, _F, _F, _F, _I, _I, _P, _P, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_farthest_point_downsample": (_I, [_P, _P, _P, _P, _L, _L, _P, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_pass_through_filter": (_I, [_P, _P, _P, _P, _L, _I, _F, _F, _P, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_crop_aabb": (_I, [_P, _P, _P, _P, _L, _P, _P, _P, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_remove_none_finite": (_I, [_P, _P, _P, _P, _L, _I, _I, _P, _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_gaussian_filter": (_I, [_P, _P, _P, _P, _L, _F, _F, _I, _P, _P, _P, _I]),
    "mi_icp_create_from_depth": (_I, [_P, _P, _I, _P, _I, _I, _I, _P, _P, _F, _F, _F, _I, _I, _I, _I,
                                      _P, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_compute_rgbd_odometry": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _I, _P, C.POINTER(_I), _P, _P, _I]),
    "mi_icp_compute_weighted_rgbd_odometry": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, C.POINTER(_I), _P, _P, _P, _I]),
    "mi_icp_tsdf_create": (_I, [_P, _F, _I, _F, _I, _P, C.POINTER(_P)]),
    "mi_icp_tsdf_destroy": (_I, [_P, _P]),
    "mi_icp_tsdf_reset": (_I, [_P, _P]),
    "mi_icp_tsdf_integrate": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P, _I]),
    "mi_icp_tsdf_extract_point_cloud": (_I, [_P, _P, _P, _P, _P, _L, C.POINTER(_L), _I]),
    "mi_icp_tsdf_extract_voxel_point_cloud": (_I, [_P, _P, _P, _P, _L, C.POINTER(_L), _I]),
    "mi_icp_tsdf_raycast": (_I, [_P, _P, _I, _I, _P, _P, _F, _I, _P, _P, _P, _L, C.POINTER(_L), _I]),
    "mi_icp_tsdf_raycast_levels": (_I, [_P, _P, _I, _I, _I, _P, _P, _F, _I, _P, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_tsdf_get_voxels": (_I, [_P, _P, _P, _P, _P, _I]),
    "mi_icp_stsdf_create": (_I, [_P, _F, _F, _I, _I, _I, C.POINTER(_P)]),
    "mi_icp_stsdf_destroy": (_I, [_P, _P]),
    "mi_icp_stsdf_reset": (_I, [_P, _P]),
    "mi_icp_stsdf_integrate": (_I, [_P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _P]),
    "mi_icp_stsdf_extract_point_cloud": (_I, [_P, _P, _P, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_stsdf_extract_voxel_point_cloud": (_I, [_P, _P, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_stsdf_get_units": (_I, [_P, _P, _P, _P, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_stsdf_num_units": (_I, [_P, _P, C.POINTER(_L), C.POINTER(_L)]),
    "mi_icp_occgrid_create": (_I, [_P, _I, C.POINTER(_P)]),
    "mi_icp_occgrid_destroy": (_I, [_P, _P]),
    "mi_icp_occgrid_reset": (_I, [_P, _P]),
    "mi_icp_occgrid_reconstruct": (_I, [_P, _P, _I]),
    "mi_icp_occgrid_insert": (_I, [_P, _P, C.POINTER(OccGridParams), _P, _L, _P, _F]),
    "mi_icp_occgrid_add_voxels": (_I, [_P, _P, C.POINTER(OccGridParams), _P, _L, _I]),
    "mi_icp_occgrid_set_free_area": (_I, [_P, _P, C.POINTER(OccGridParams), _P, _P]),
    "mi_icp_occgrid_query": (_I, [_P, _P, C.POINTER(OccGridParams), _P, _L, _P, _P]),
    "mi_icp_occgrid_extract": (_I, [_P, _P, C.POINTER(OccGridParams), _I, _P, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_occgrid_get_bounds": (_I, [_P, _P, _P, _P]),
    "mi_icp_occgrid_get_voxels": (_I, [_P, _P, _P]),
    "mi_icp_dt_create": (_I, [_P, _I, C.POINTER(_P)]),
    "mi_icp_dt_destroy": (_I, [_P, _P]),
    "mi_icp_dt_reconstruct": (_I, [_P, _P, _I]),
    "mi_icp_dt_compute_cells": (_I, [_P, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_dt_compute_voxelgrid": (_I, [_P, _P, _F, _P, _P, _L, _F, _P, C.POINTER(_L)]),
    "mi_icp_dt_compute_occgrid": (_I, [_P, _P, _P, _F]),
    "mi_icp_dt_query": (_I, [_P, _P, _F, _P, _P, _L, _P, _P]),
    "mi_icp_dt_get_voxels": (_I, [_P, _P, _F, _P, _P]),
    "mi_icp_voxelgrid_from_points": (_I, [_P, _P, _P, _L, _F, _P, _P, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_voxelgrid_dense": (_I, [_P, _I, _I, _I, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_voxelgrid_merge": (_I, [_P, _P, _P, _L, _P, _P, _L, _I, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_voxelgrid_carve": (_I, [_P, _P, _P, _L, _F, _P, _P, _I, _I, _I, _I, _P, _P, _I, _P, _P, C.POINTER(_L)]),
    "mi_icp_voxelgrid_query": (_I, [_P, _P, _L, _I, _F, _P, _P, _L, _P, _P]),
    "mi_icp_voxelgrid_bounds": (_I, [_P, _P, _L, _F, _P, _P, _P, _P]),
    "mi_icp_voxelgrid_select_by_index": (_I, [_P, _P, _P, _L, _P, _L, _I, _P, _P, C.POINTER(_L)]),
    "mi_icp_voxelgrid_paint": (_I, [_P, _P, _L, _P, _L, _P]),
    "mi_icp_collision_compute": (_I, [_P, C.POINTER(CollisionSide), C.POINTER(CollisionSide), _F, _P, _L, C.POINTER(_L)]),
    "mi_icp_collision_voxelize_primitive": (_I, [_P, C.POINTER(Primitive), _F, _P, _P, _L, C.POINTER(_L), _P]),
    "mi_icp_collision_sort_keys": (_I, [_P, _P, _L, _P, _P, C.POINTER(_L)]),
    "mi_icp_primitive_aabb": (_I, [C.POINTER(Primitive), _P, _P]),
    "mi_icp_graph_construct": (_I, [_P, _P, _P, _P, _L, _L, _P]),
    "mi_icp_graph_weights_from_distance": (_I, [_P, _P, _L, _P, _L, _P]),
    "mi_icp_graph_node_distances": (_I, [_P, _P, _L, _P, _P]),
    "mi_icp_graph_lattice": (_I, [_P, _P, _P, _P, _P, _L, _P, _P, _L, _P, C.POINTER(_L), C.POINTER(_L)]),
    "mi_icp_graph_set_edge_weights": (_I, [_P, _P, _P, _L, _P, _L, _I, _F]),
    "mi_icp_graph_remove_edges": (_I, [_P, _P, _P, _P, _L, _L, _P, _L, _I, _P, C.POINTER(_L)]),
    "mi_icp_graph_sssp": (_I, [_P, _P, _P, _P, _L, _L, _L, _L, _P, _P, _P]),
    "mi_icp_graph_sssp_limits": (_I, [C.POINTER(_L), C.POINTER(_L), C.POINTER(C.c_int32)]),
    "mi_icp_laserscan_to_points": (_I, [_P, _P, _P, _P, C.c_int32, C.c_int32, C.c_int32, C.c_int32, _F, _F, _F, _F, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_laserscan_from_points": (_I, [_P, _P, _L, _F, _F, _F, C.c_int32, _F, _F, _F, _F, C.c_int32, _P, C.POINTER(C.c_int32)]),
    "mi_icp_laserscan_from_depth": (_I, [_P, _P, _I, _I, _I, _P, _F, _F, _I, _F, _F, _F, C.c_int32, _F, _F, _F, _F, C.c_int32, _P,
                                         C.POINTER(C.c_int32)]),
    "mi_icp_laserscan_range_filter": (_I, [_P, _P, _L, _F, _F, _P]),
    "mi_icp_laserscan_shadow_filter": (_I, [_P, _P, C.c_int32, C.c_int32, _F, _F, _F, _F, C.c_int32, C.c_int32, _I, _P]),
    "mi_icp_laserscan_scale": (_I, [_P, _P, _L, _F]),
    "mi_icp_laserscan_limits": (_I, [C.POINTER(_L), C.POINTER(_L)]),
    "mi_icp_image_filter": (_I, [_P, _P, _I, _I, _P, _I, _P, _I, _P]),
    "mi_icp_image_downsample": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "mi_icp_image_pyramid_level": (_I, [_P, _P, _I, _I, _P]),
    "mi_icp_image_bilateral_table": (_I, [_I, _F, _P]),
    "mi_icp_image_bilateral": (_I, [_P, _P, _I, _I, _I, _F, _P, _P]),
    "mi_icp_image_create_float": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "mi_icp_image_depth_to_float": (_I, [_P, _P, _I, _I, _I, _I, _F, _F, _P]),
    "mi_icp_image_create_gray": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "mi_icp_image_from_float": (_I, [_P, _P, _I, _I, _I, _P]),
    "mi_icp_image_linear_transform": (_I, [_P, _P, _I, _I, _I, _I, _F, _F]),
    "mi_icp_image_clip": (_I, [_P, _P, _I, _I, _F, _F]),
    "mi_icp_image_move": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "mi_icp_image_depth_format": (_I, [_P, _P, _I, _I, _I, _P]),
    "mi_icp_image_limits": (_I, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mi_icp_sgm_create": (_I, [_P, _I, _I, _I, _I, _F, _I, _I, _I, _I, C.POINTER(_P)]),
    "mi_icp_sgm_destroy": (_I, [_P, _P]),
    "mi_icp_sgm_process": (_I, [_P, _P, _P, _P, _P]),
    "mi_icp_sgm_census": (_I, [_P, _P, _I, _I, _P]),
    "mi_icp_sgm_get_sums": (_I, [_P, _P, _P]),
    "mi_icp_sgm_limits": (_I, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mi_icp_create_from_disparity": (_I, [_P, _P, _P, _I, _I, _I, _P, _P, _P]),
    "mi_icp_feature_match": (_I, [_P, _P, _L, _P, _L, _I, _P, _P, _P, _P]),
    "mi_icp_fgr_correspondences": (_I, [_P, _P, _L, _P, _L, _P, _P, _F, _L, C.c_uint64, _P, C.POINTER(_L), _P, C.POINTER(_L)]),
    "mi_icp_fgr_optimize": (_I, [_P, _P, _L, _P, _L, _P, _L, _F, C.POINTER(FgrOption), _P, _P, _P]),
    "mi_icp_correspondences_from_features": (_I, [_P, _P, _L, _P, _L, _I, _I, _F, _P, C.POINTER(_L)]),
    "mi_icp_fast_global_registration": (_I, [_P, _P, _P, _L, _P, _P, _L, _I, C.POINTER(FgrOption), C.c_uint64, C.POINTER(Result)]),
    "mi_icp_covariances_from_normals": (_I, [_P, _P, _L, _F, _P, _I]),
    "mi_icp_estimate_normals_knn": (_I, [_P, _P, _L, _I, _P, _I]),
    "mi_icp_estimate_normals_radius": (_I, [_P, _P, _L, _F, _I, _P, _I]),
    "mi_icp_search_knn": (_I, [_P, _P, _L, _I, _F, _P, _P, C.POINTER(_L), _I]),
    "mi_icp_set_target_colors": (_I, [_P, _P, _I]),
    "mi_icp_set_source_colors": (_I, [_P, _P, _I]),
    "mi_icp_set_lambda_geometric": (_I, [_P, _F]),
    "mi_icp_compute_color_gradients": (_I, [_P, _F, _I, _P, _I]),
    "mi_icp_registration_colored_icp": (_I, [_P, _F, _P, C.POINTER(Params), _F, C.POINTER(Result)]),
    "mi_icp_comm_unique_id": (_I, [_P]),
    "mi_icp_comm_init": (_I, [_P, _P, _I, _I]),
    "mi_icp_comm_init_local": (_I, [_P, C.c_char_p, _I, _I]),
    "mi_icp_comm_kind": (_I, [_P]),
    "mi_icp_comm_autotune": (_I, [_P, _I, _P, _P]),
    "mi_icp_comm_destroy": (_I, [_P]),
    "mi_icp_set_global_source_count": (_I, [_P, _L]),
    "mi_icp_spatial_order": (_I, [_P, _P, _L, _P, _I]),
    "mi_icp_set_iteration_callback": (_I, [_P, _P, _P]),
    "mi_icp_set_profiling": (_I, [_P, _I]),
    "mi_icp_get_profile": (_I, [_P, _P]),
    # include/mi_icp_debug.h (test-only)
    "mi_icp_debug_sort_pairs": (_I, [_P, _P, _P, _L, _I]),
    "mi_icp_debug_sort_pairs32": (_I, [_P, _P, _P, _L, _I]),
    "mi_icp_debug_sort_payload32": (_I, [_P, _P, _P, _P, _P, _L, _I, _I]),
    "mi_icp_debug_sort_plan": (_I, [_L, _P]),
    "mi_icp_debug_exclusive_scan": (_I, [_P, _P, _P, _L, _P]),
    "mi_icp_debug_morton_order": (_I, [_P, _P, _L, _P]),
    "mi_icp_debug_morton_order_bits": (_I, [_P, _P, _L, _I, _P]),
    "mi_icp_debug_nn_stats": (_I, [_P, _P, _F, _I, _P]),
    "mi_icp_debug_nn_stats8": (_I, [_P, _P, _F, _I, _P]),
    "mi_icp_debug_get_tree": (_I, [_P, C.POINTER(_L), _P, _P]),
    "mi_icp_debug_drop_seeds": (_I, [_P]),
    "mi_icp_debug_last_search_kind": (_I, [_P]),
    "mi_icp_debug_last_voxel_path": (_I, [_P]),
    "mi_icp_debug_last_voxel_plan": (_I, [_P, _P]),
    "mi_icp_debug_occupancy": (_I, [_I]),
    "mi_icp_debug_loop_counters": (_I, [_P, _P]),
    "mi_icp_debug_search_skip": (_I, [_P, _P, _P, _L, C.POINTER(_L), C.POINTER(_I)]),
    "mi_icp_debug_pair_state": (_I, [_P, _P, _P, _L, C.POINTER(_L)]),
    "mi_icp_debug_drop_pairs": (_I, [_P]),
    "mi_icp_debug_locate": (_I, [_P, _P, _P]),
    "mi_icp_debug_set_step_stamps": (_I, [_P, _I]),
    "mi_icp_debug_get_step_stamps": (_I, [_P, _P, C.POINTER(C.c_double)]),
    "mi_icp_debug_solve_both": (_I, [_I, _P, _I, C.c_float, _P, _P, _P, _P]),
    "mi_icp_debug_get_leaf_regions": (_I, [_P, _P]),
    "mi_icp_debug_get_leaf_halos": (_I, [_P, _P]),
    "mi_icp_debug_eigen3": (_I, [_I, _P, _L, _P, _P, _P]),
    "mi_icp_debug_odometry_image": (_I, [_P, _I, _I, _P, C.POINTER(_I), C.POINTER(_I)]),
    "mi_icp_debug_image_bilateral": (_I, [_P, _P, _I, _I, _I, _F, _P, _P, _I]),
}

_lib = None


def load():
    """Load libmi_icp.so and bind every entry point; raises if it is absent."""
    global _lib
    if _lib is not None:
        return _lib
    override = os.environ.get("MI_ICP_LIB_PATH")   # A/B runs of two builds on one box (scripts/gpu_ab_libs.sh)
    path = override or LIB_PATH
    if not os.path.exists(path):
        raise MiIcpError(
            "libmi_icp.so is not built (%s). Run `python -c 'import __graft_entry__ as g; "
            "g.build()'` or cupoch_amd._lib.build(); there is no CPU fallback." % LIB_PATH)
    try:
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
    except OSError as e:  # e.g. libamdhip64 missing
        raise MiIcpError("cannot load %s: %s" % (path, e))
    for name, (res, args) in SIGNATURES.items():
        if override and name.startswith("mi_icp_debug_") and not hasattr(lib, name):
            continue     # (an older build under comparison may lack a test-only entry point)
        fn = getattr(lib, name)  # AttributeError if the library lacks a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
