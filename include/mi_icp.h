/*
 * mi_icp.h -- C ABI of libmi_icp.so, the MI355X (gfx950) ICP registration
 * engine that sits behind cupoch's registration / geometry C++ surface.
 *
 * Every entry point names the reference interface it replaces
 * (paths relative to the cupoch tree, v0.2.11.0).  The reference-side
 * bindings (C++ classes in namespace cupoch, Python ctypes) are shown in
 * INTEGRATION.md; cupoch_amd/cpp and the Python modules under cupoch_amd implement them.
 *
 * Conventions
 *   - every function returns an int status: 0 = MI_ICP_OK, negative = error;
 *     nothing throws or exit()s across this boundary (the reference prints and
 *     exit(0)s on device errors, utility/platform.cu:60-67);
 *     mi_icp_last_error() returns the text of the last failure on a context.
 *   - points / normals / colors are AoS float[n][3] with a 12-byte stride
 *     (the memory layout of device_vector<Eigen::Vector3f>,
 *     geometry/pointcloud.h:259-262); covariances are float[n][9],
 *     column-major 3x3 (Eigen::Matrix3f); 4x4 transforms are float[16]
 *     column-major, i.e. exactly Eigen::Matrix4f::data();
 *     correspondences are int32 pairs (source_idx, target_idx) =
 *     device_vector<Eigen::Vector2i> (registration/transformation_estimation.h:36).
 *   - every buffer argument carries a mem_kind: MI_ICP_HOST (pageable or
 *     pinned host memory, copied by the engine) or MI_ICP_DEVICE (a HIP device
 *     pointer on the context's GPU, read in place).  Any other value returns
 *     MI_ICP_ERR_INVALID before any buffer is read or written.  The caller owns all
 *     buffers it passes; the context owns its internal SoA copies, LBVH and
 *     scratch arena.
 *     THE ONE EXCEPTION is the mi_icp_occgrid_* family and the mi_icp_voxelgrid_* and
 *     mi_icp_dt_* families beside it: their arrays (points, voxel
 *     indices, outputs) are HIP device pointers only and they have no memory-kind
 *     argument; their small fixed-size arguments (the parameter block, viewpoint3,
 *     corners, bounds, counts) are host pointers or values.
 *   - one context per GPU; a context is not thread-safe, independent contexts
 *     may be driven from different host threads.
 *   - all work is enqueued on the context's stream (mi_icp_set_stream; the
 *     default is the null stream).  Functions that return scalars or host
 *     buffers synchronise that stream before returning.
 */
#ifndef MI_ICP_H_
#define MI_ICP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_ICP_API __attribute__((visibility("default")))

enum {
    MI_ICP_OK = 0,
    MI_ICP_ERR_INVALID = -1,   /* bad argument (null, negative size, bad enum) */
    MI_ICP_ERR_STATE = -2,     /* call order: no target / source / normals set */
    MI_ICP_ERR_HIP = -3,       /* a HIP runtime call failed */
    MI_ICP_ERR_COMM = -4,      /* RCCL unavailable or failed */
    MI_ICP_ERR_NO_DEVICE = -5  /* no usable gfx950 device */
};

enum { MI_ICP_HOST = 0, MI_ICP_DEVICE = 1 };

/* registration::TransformationEstimationType
 * (registration/transformation_estimation.h:38-45), same values */
enum {
    MI_ICP_EST_POINT_TO_POINT = 1,
    MI_ICP_EST_POINT_TO_PLANE = 2,
    MI_ICP_EST_SYMMETRIC = 3,
    MI_ICP_EST_COLORED = 4, /* TransformationEstimationType::ColoredICP */
    MI_ICP_EST_GENERALIZED = 5
};

typedef struct mi_icp_ctx mi_icp_ctx;

/* registration::ICPConvergenceCriteria (registration/registration.h:35-49)
 * + the estimator's scalar parameter. */
typedef struct {
    float relative_fitness; /* default 1e-6; compared as an ABSOLUTE difference */
    float relative_rmse;    /* default 1e-6; ditto (registration.cu:165-170) */
    int32_t max_iteration;  /* default 30 */
    float det_thresh;       /* PointToPlane / Symmetric det check, default 1e-6;
                               <= 0 disables it (utility/eigen.cu:114) */
} mi_icp_params;

/* registration::RegistrationResult (registration/registration.h:51-67);
 * the correspondence set itself is fetched with mi_icp_get_correspondences. */
typedef struct {
    float transformation[16]; /* column-major */
    float fitness;
    float inlier_rmse;
    int64_t n_correspondences;
    int32_t iterations;   /* solves executed */
    int32_t nn_passes;    /* nearest-neighbour passes executed (iterations+1) */
} mi_icp_result;

/* ---- context / errors  (replaces utility::InitializeAllocator + GetStream,
 *      utility/device_vector.h:78-106, utility/platform.cu:38-67) ---------- */
MI_ICP_API int mi_icp_create(int device, mi_icp_ctx** out);
MI_ICP_API void mi_icp_destroy(mi_icp_ctx* ctx);
MI_ICP_API const char* mi_icp_last_error(const mi_icp_ctx* ctx);
MI_ICP_API const char* mi_icp_version(void);
/* hip_stream: a hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) */
MI_ICP_API int mi_icp_set_stream(mi_icp_ctx* ctx, void* hip_stream);
MI_ICP_API int mi_icp_synchronize(mi_icp_ctx* ctx);

/* ---- clouds -----------------------------------------------------------
 * mi_icp_set_target replaces knn::KDTreeFlann::KDTreeFlann(target.points_) /
 * SetRawData (knn/kdtree_flann.inl:124-144) and FLANN's
 * CudaKdTreeBuilder::buildTree (third_party/flann/algorithms/
 * kdtree_cuda_builder.h:401-700): partitions the target into kd cells and
 * builds the implicit 8-ary tree over them.  normals / covs may be NULL.
 * Synchronous (the tree's size is read back once); at most ~3e8 points.
 * The leaves' HALOS (what a loop's seeded searches use once the matches are no
 * longer exact; csrc/leaf_halo.h) are built on demand, on a private low-priority
 * stream: when a registration loop's searches ask for them (ahead of the loop's first
 * pass, on the loop's own stream, on a context whose loops have asked before), and --
 * for a target below 2M points on a context that has registered before -- right behind
 * the tree, next to whatever the caller enqueues next.
 * Device memory a context keeps per target point: ~75 B of tree (leaf lines, regions,
 * records; 1.67 slots per point at 10M), + 40 B with normals, + 60 B with covariances;
 * the halos add 1 KB per LEAF (~215 B per point) once built, and their build 0.5 KB per
 * leaf of candidate scratch that is released at the end of the registration call that
 * built them (targets whose scratch is below 64 MB keep it: frame-to-frame callers).
 * mi_icp_set_source replaces `geometry::PointCloud pcd = source`
 * (registration/registration.cu:147): the engine keeps a Morton-sorted SoA
 * copy and never mutates the caller's cloud.  Stream-ordered. */
MI_ICP_API int mi_icp_set_target(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                 const float* covs, int64_t n, int mem_kind);
MI_ICP_API int mi_icp_set_source(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                 const float* covs, int64_t n, int mem_kind);

/* ---- nearest neighbours -------------------------------------------------
 * knn::KDTreeFlann::SearchRadius(source.points_, r, max_nn = 1, indices,
 * dists) as used by GetRegistrationResultAndCorrespondences
 * (registration/registration.cu:33-80, knn/kdtree_flann.inl:96-122):
 * for every source point transformed by T, the target point with the
 * smallest d2 subject to the strict test d2 < float(r*r); no match ->
 * idx -1, d2 +inf.  idx_out / d2_out are in ORIGINAL source order and hold
 * ORIGINAL target indices; either may be NULL.  stats[3] (optional) receives
 * {count, sum d2, n_source}.  T == NULL means identity.
 * The result also becomes the context's current correspondence set.  Among
 * target points at exactly the same distance the one with the lowest position
 * in the tree's order is returned (FLANN returns the first one it visits).  A
 * search on the same pair of clouds as the previous one starts from its matches;
 * that only makes it faster. */
MI_ICP_API int mi_icp_search_radius_1nn(mi_icp_ctx* ctx, const float* T, float radius,
                                        int32_t* idx_out, float* d2_out, int mem_kind,
                                        double* stats);

/* ---- correspondences ----------------------------------------------------
 * get: RegistrationResult::correspondence_set_ (registration.cu:54-69):
 * pairs (i, j), ascending in source index i (stable compaction).
 * `capacity` is in pairs; *count receives the number of pairs available.
 * set: supplies an explicit CorrespondenceSet for the
 * TransformationEstimation::ComputeTransformation / ComputeRMSE entry points
 * below (registration/transformation_estimation.h:50-65). */
MI_ICP_API int mi_icp_get_correspondences(mi_icp_ctx* ctx, int32_t* pairs, int64_t capacity,
                                          int64_t* count, int mem_kind);
MI_ICP_API int mi_icp_set_correspondences(mi_icp_ctx* ctx, const int32_t* pairs,
                                          int64_t count, int mem_kind);

/* ---- estimation ---------------------------------------------------------
 * mi_icp_compute_system replaces utility::ComputeJTJandJTr
 * (utility/eigen.inl:84-145) over the estimator's Jacobian functor
 * (registration/transformation_estimation.cu:34-90,
 *  registration/generalized_icp.cu:63-105) or, for point-to-point, the three
 * reductions of registration/kabsch.cu:42-104.  The source is taken under T
 * (points R*p+t, normals R*n, covariances R*C*R^T).  out[32] (fp64):
 *   [0..20] upper triangle of JtJ row-major, [21..26] Jtr, [27] sum r^2,
 *   [28] sum d2, [29] count;
 *   point-to-point: [0..2] sum ps, [3..5] sum pt, [6..14] sum ps*pt^T
 *   (row-major), [27] sum |ps-pt|^2, [28] sum d2, [29] count.
 * mi_icp_compute_transformation = TransformationEstimation*::
 * ComputeTransformation (transformation_estimation.cu:137-142,195-222,
 * 289-350; generalized_icp.cu:152-183) incl. SolveJacobianSystemAndObtain-
 * ExtrinsicMatrix (utility/eigen.cu:107-122) / Kabsch (kabsch.cu:105-118);
 * solver failure -> identity.  mi_icp_compute_rmse = ::ComputeRMSE. */
MI_ICP_API int mi_icp_compute_system(mi_icp_ctx* ctx, int est_type, const float* T,
                                     double* out32);
MI_ICP_API int mi_icp_compute_transformation(mi_icp_ctx* ctx, int est_type, const float* T,
                                             float det_thresh, float* update16);
MI_ICP_API int mi_icp_compute_rmse(mi_icp_ctx* ctx, int est_type, const float* T,
                                   float* rmse);
/* host-only helpers, exposed for parity tests:
 * utility::SolveJacobianSystemAndObtainExtrinsicMatrix (utility/eigen.cu:107-122),
 * utility::TransformVector6fToMatrix4f (utility/eigen.cu:28-50). */
MI_ICP_API int mi_icp_solve_system(const double* sys32, float det_thresh, float* T16);
MI_ICP_API int mi_icp_kabsch_from_sums(const double* sys32, int64_t n_model, float* T16);
MI_ICP_API void mi_icp_vector6_to_matrix4(const float* x6, float* T16);

/* host-only: the LZF byte format of PCD's "DATA binary_compressed" (io/file_format/file_pcd.cu:218,461,690
 * call liblzf's lzf_decompress / lzf_compress).  Return the number of bytes produced, 0 on a
 * corrupt stream or when out_capacity is too small (compress: 2 x in_len always suffices). */
MI_ICP_API int64_t mi_icp_lzf_decompress(const void* in, int64_t in_len, void* out, int64_t out_capacity);
MI_ICP_API int64_t mi_icp_lzf_compress(const void* in, int64_t in_len, void* out, int64_t out_capacity);

/* ---- the registration loop ---------------------------------------------
 * registration::EvaluateRegistration (registration.cu:106-119) and
 * registration::RegistrationICP (registration.cu:121-172) with the built-in
 * estimators.  init == NULL means identity.  GICP expects covariances on both
 * clouds (RegistrationGeneralizedICP's InitializePointCloudForGeneralizedICP,
 * generalized_icp.cu:37-61, is mi_icp_covariances_from_normals). */
MI_ICP_API int mi_icp_evaluate_registration(mi_icp_ctx* ctx, float max_distance,
                                            const float* T, mi_icp_result* out);
MI_ICP_API int mi_icp_registration_icp(mi_icp_ctx* ctx, int est_type, float max_distance,
                                       const float* init, const mi_icp_params* params,
                                       mi_icp_result* out);

/* Stepping form of the same loop (no reference counterpart: the reference only
 * offers the whole call).  begin = the setup + first correspondence pass
 * (registration.cu:144-152); iterate(n) = n executions of the loop body
 * (registration.cu:155-163) without the convergence test.  Used by per-frame
 * callers that budget iterations themselves and by bench.py, which times
 * exactly K iterations. */
MI_ICP_API int mi_icp_icp_begin(mi_icp_ctx* ctx, int est_type, float max_distance,
                                const float* init, float det_thresh, mi_icp_result* out);
MI_ICP_API int mi_icp_icp_iterate(mi_icp_ctx* ctx, int n_iterations, mi_icp_result* out);

/* ---- geometry -----------------------------------------------------------
 * PointCloud::Transform (geometry/pointcloud.cu:293-299): in place on the
 * caller's arrays; any of the three may be NULL. */
MI_ICP_API int mi_icp_transform(mi_icp_ctx* ctx, const float* T, float* xyz, float* normals,
                                float* covs, int64_t n, int mem_kind);
/* GeometryBase3D::GetMinBound / GetMaxBound / GetCenter of a cloud (geometry/geometry_base.h:47-52,
 * geometry/pointcloud.cu:205-215; utility::ComputeMinBound / ComputeMaxBound / ComputeCenter,
 * utility/eigen.inl:208-232).  Any of the outputs (host float[3]) may be NULL; an empty cloud
 * gives zero vectors.  The centre is the fp64 sum divided by n, rounded once (the reference
 * sums in fp32). */
MI_ICP_API int mi_icp_compute_bounds(mi_icp_ctx* ctx, const float* xyz, int64_t n, int mem_kind,
                                     float* min3, float* max3, float* center3);
/* GeometryBase3D::Translate / Scale / Rotate (geometry/geometry_base.h:58-90,
 * geometry/pointcloud.cu:225-242, geometry_utils.cu:150-270), in place:
 *   points  <- (R (p - center)) * scale + center + translate
 *   normals <- R n          covariances <- R C R^T           (only when R9 is given)
 * with exactly the reference functors' operations for the terms present: R9 (column-major 3x3,
 * Eigen::Matrix3f::data()), center3, translate3 may be NULL, use_scale = 0 skips the scaling.
 *   Translate(t, relative)  = affine(NULL, 0, 0, NULL, relative ? t : t - GetCenter(), points)
 *   Scale(s, center)        = affine(NULL, s, 1, center ? GetCenter() : NULL, NULL, points)
 *   Rotate(R, center)       = affine(R, 0, 0, center ? GetCenter() : NULL, NULL, points, normals, covs) */
MI_ICP_API int mi_icp_affine(mi_icp_ctx* ctx, const float* R9, float scale, int use_scale,
                             const float* center3, const float* translate3, float* xyz, float* normals,
                             float* covs, int64_t n, int mem_kind);
/* PointCloud::VoxelDownSample (geometry/down_sample.cu:170-273): outputs in
 * lexicographic voxel order; out arrays must hold n entries; *m receives the
 * voxel count (0 for voxel_size <= 0 or a too-small voxel, as the reference
 * returns an empty cloud).  normals / colors and their outputs may be NULL.
 * A voxel's values are added in fp64 in a fixed order -- the same result on
 * every run; in the input's order on dense grids (csrc/voxel_dense.h) and on
 * fine ones (a point or two per voxel), where the means equal the CPU oracle's
 * bit for bit (the reference's thrust::reduce_by_key adds in fp32 in an order
 * of its own choosing).  The entry point synchronises the context's stream. */
MI_ICP_API int mi_icp_voxel_downsample(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                       const float* colors, int64_t n, float voxel_size,
                                       float* out_xyz, float* out_normals, float* out_colors,
                                       int64_t* m, int mem_kind);
/* PointCloud::SelectByIndex (geometry/down_sample.cu:40-62,110-129).  indices: int64 [n_indices]
 * (device_vector<size_t>), in the same memory kind as the points.
 *   invert = 0  a gather in the order given: out entry j = point indices[j]; repeated indices repeat
 *               points; *m = n_indices.  Outputs hold n_indices entries.
 *   invert = 1  the points NOT named, ascending in index; a repeated index counts once (the
 *               reference sizes its output n - n_indices and would misbehave on repeats).  Outputs
 *               hold n entries.
 * An index outside [0, n) is MI_ICP_ERR_INVALID (checked on the device; the status comes back with
 * the count, no extra wait).  normals / colors and their outputs may be NULL.  The entry point
 * synchronises the context's stream. */
MI_ICP_API int mi_icp_select_by_index(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                      const float* colors, int64_t n, const int64_t* indices,
                                      int64_t n_indices, int invert, float* out_xyz, float* out_normals,
                                      float* out_colors, int64_t* m, int mem_kind);
/* PointCloud::SelectByMask (geometry/down_sample.cu:131-168).  mask: one byte per point (uint8
 * [n_mask], device_vector<bool>), in the same memory kind as the points.  The points, and normals /
 * colours where given, of the entries whose byte is non-zero (invert != 0: zero), ascending in
 * index; *m = their number.  Outputs hold n entries.  n_mask != n is MI_ICP_ERR_INVALID, as the
 * reference refuses a mask of another size.  The entry point synchronises the context's stream. */
MI_ICP_API int mi_icp_select_by_mask(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                     const float* colors, int64_t n, const uint8_t* mask, int64_t n_mask,
                                     int invert, float* out_xyz, float* out_normals, float* out_colors,
                                     int64_t* m, int mem_kind);
/* PointCloud::UniformDownSample (geometry/down_sample.cu:275-316): the points at indices 0, k, 2k, ...
 * -- *m = n / every_k_points of them (the size the reference allocates; 0 when k > n) -- with their
 * normals / colours (either may be NULL).  every_k_points < 1 is MI_ICP_ERR_INVALID.  Outputs hold
 * n / every_k_points entries.  A strided copy per attribute; synchronises the context's stream. */
MI_ICP_API int mi_icp_uniform_downsample(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                         const float* colors, int64_t n, int64_t every_k_points,
                                         float* out_xyz, float* out_normals, float* out_colors,
                                         int64_t* m, int mem_kind);
/* PointCloud::FarthestPointDownSample(num_samples) (geometry/pointcloud.cu:122-139, 301-338).  Its
 * contract, which the selection sel[0 .. num_samples) meets exactly:
 *   sel[0] = 0; dist[i] = +inf for every point.
 *   After choosing s = sel[t]:  dist[i] = min(dist[i], d2(i, s)) for every point, d2 = fma(dz, dz,
 *   fma(dy, dy, dx*dx)) of the fp32 differences p_i - p_s, as everywhere in this header.
 *   sel[t+1] = the index of the largest dist; TIES GO TO THE LOWEST INDEX.
 * Deviation (deliberate): the reference reduces with "a > b ? a : b" under a thrust tree, which leaves
 * ties to the order of the reduction -- its result is not a function of its input.  Lowest-first is
 * the rule of Open3D's FarthestPointDownSample, from which the reference's descends.  A consequence:
 * once every remaining dist is 0 (the cloud has fewer distinct points than samples asked for), the
 * largest is 0 at index 0 and index 0 repeats, as a repeated index would in the reference.
 * Outputs: the selected points, with normals / colours where given (either may be NULL), in selection
 * order; out_idx (int64 [num_samples], may be NULL) = sel; *m = num_samples.  Outputs hold
 * num_samples entries.  num_samples == 0 gives *m = 0; num_samples == n gives the cloud itself in
 * input order (sel = 0, 1, ..., n-1), as the reference's early return does; num_samples > n (the
 * reference logs an error) or < 0 is MI_ICP_ERR_INVALID.
 * Non-finite coordinates are outside the contract (mi_icp_remove_none_finite comes first).  What
 * happens: min is IEEE minNum, so a NaN d2 leaves dist as it is; a point with a non-finite coordinate
 * keeps dist = +inf, and the lowest such index is chosen at every step after the first.  The call
 * terminates and every index lies in [0, n).
 * One launch per sample, all enqueued before the call's one wait on the context's stream: the chosen
 * index and its coordinates never leave the device in between.  A maximum of integers has no
 * summation order: the same input gives the same bytes on every run and context.  No tree is built;
 * the caller's target / source / loop state are not touched.  Memory: 4 bytes per point. */
MI_ICP_API int mi_icp_farthest_point_downsample(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                                const float* colors, int64_t n, int64_t num_samples,
                                                float* out_xyz, float* out_normals, float* out_colors,
                                                int64_t* out_idx, int64_t* m, int mem_kind);
/* The predicate filters of geometry::PointCloud.  Each gives the kept points, with normals / colours
 * where given (either may be NULL), ascending in index; out_idx (int64, may be NULL) their original
 * indices; *m their number.  Outputs hold n entries.  n = 0 gives *m = 0.  Each synchronises the
 * context's stream.
 *   PassThroughFilter(axis_no, min_bound, max_bound) (pointcloud.cu:108-120, 436-466): a point is kept
 *     iff !(v < min_bound || max_bound < v), v = p[axis_no] -- so a NaN coordinate is kept, as the
 *     reference's comparison keeps it, and so is every point when a bound is NaN.  axis_no outside
 *     {0, 1, 2} is MI_ICP_ERR_INVALID.
 *   Crop(AxisAlignedBoundingBox<3>) (pointcloud.cu:340-348, boundingvolume.cu:81-101): a point is kept
 *     iff on all three axes !(p < min || p > max): the bounds are inclusive and a NaN coordinate is
 *     kept, as in the reference.  An empty box -- Volume() = ((max0 - min0) * (max1 - min1)) *
 *     (max2 - min2) in fp32 not > 0 -- is MI_ICP_ERR_INVALID (the reference logs an error).
 *   RemoveNoneFinitePoints(remove_nan, remove_infinite) (pointcloud.cu:40-54, 360-385): a point is
 *     DROPPED iff (remove_nan and a coordinate is NaN) or (remove_infinite and a coordinate is +-inf).
 *     The reference works in place; this entry writes to outputs like its siblings, the C++ and
 *     Python methods replace the cloud's own arrays. */
MI_ICP_API int mi_icp_pass_through_filter(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                          const float* colors, int64_t n, int axis_no, float min_bound,
                                          float max_bound, float* out_xyz, float* out_normals,
                                          float* out_colors, int64_t* out_idx, int64_t* m, int mem_kind);
MI_ICP_API int mi_icp_crop_aabb(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                const float* colors, int64_t n, const float* min_bound3,
                                const float* max_bound3, float* out_xyz, float* out_normals,
                                float* out_colors, int64_t* out_idx, int64_t* m, int mem_kind);
MI_ICP_API int mi_icp_remove_none_finite(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                         const float* colors, int64_t n, int remove_nan,
                                         int remove_infinite, float* out_xyz, float* out_normals,
                                         float* out_colors, int64_t* out_idx, int64_t* m, int mem_kind);
/* PointCloud::CreateFromDepthImage and PointCloud::CreateFromRGBDImage
 * (geometry/pointcloud_factory.cu:43-110,117-220,286-376) incl. the
 * RemoveNoneFinitePoints pass that follows (geometry/pointcloud.cu:40-54,360-385):
 * the depth-image side of the path's tracker callers (kinfu/kinfu.cpp:87-104).
 *   depth       [height][width], MI_ICP_DEPTH_F32 or MI_ICP_DEPTH_U16 (then value * the
 *               reciprocal of (int)depth_scale, values >= (int)depth_trunc dropped,
 *               image.cu:339-348 as the reference is built -- "depth_to_float" under
 *               "image" below; both are truncated to int as the reference does)
 *   color       NULL, MI_ICP_COLOR_U8X3 [h][w][3] (scaled by 1/255) or
 *               MI_ICP_COLOR_F32X1 [h][w] (replicated to 3 channels)
 *   intrinsic4  fx, fy, cx, cy;   extrinsic: 4x4 column-major or NULL (identity);
 *               points are mapped by extrinsic^-1
 *   rgbd = 0    CreateFromDepthImage: pixel (row*stride, col*stride) of a
 *               (width/stride) x (height/stride) grid, depth <= 0 dropped, no
 *               colours or normals; non-finite points always removed
 *   rgbd = 1    CreateFromRGBDImage: stride must be 1; a pixel is kept when
 *               depth > 0 and (depth_cutoff <= 0 or depth < depth_cutoff);
 *               compute_normals: cross product of the 4-neighbourhood differences,
 *               flipped to z <= 0 (:161-199); valid_only = 0 keeps one point per
 *               pixel, rejected ones +inf.
 * Outputs must hold (width/stride)*(height/stride) points; *m = points written, in
 * pixel order.
 *
 * THE NUMERIC CONTRACT (fp32, products never fused, division and sqrtf correctly rounded, in exactly the
 * order written; tests/depth_exact.py restates it in numpy).
 *  pose     the extrinsic's inverse (the identity's for NULL), computed IN DOUBLE by Gauss-Jordan elimination
 *           with partial pivoting (the pivot of a column is the first row of the largest magnitude at or below
 *           the diagonal; the pivot row is divided by the pivot, then taken times the entry from every other
 *           row whose entry in that column is not zero), every entry rounded to float at the end.  A column
 *           whose pivot is 0: MI_ICP_ERR_INVALID.  Only its rows 0..2 are used.
 *  pixels   output element idx stands for row = (idx / (width/stride)) * stride, col = (idx % (width/stride))
 *           * stride (integer divisions), pix = row*width + col.
 *  d        the depth of the pixel; for MI_ICP_DEPTH_U16 (float)v * r, r = (float)(1.0 / (double)(float)(int)
 *           depth_scale), set to 0 when >= (float)(int)depth_trunc: the one rule of "depth_to_float" under "image"
 *           below, which the reference's vector TEST(Image, ConvertDepthToFloatImage) pins.  LaserScanBuffer's depth
 *           entry and Image::ConvertDepthToFloatImage give the same words.
 *  accepted rgbd = 0: !(d <= 0) -- NaN and +inf are accepted.  rgbd = 1: d > 0 && (depth_cutoff <= 0 ||
 *           depth_cutoff > d).
 *  point    x = ((float)col - cx) * d / fx,  y = ((float)row - cy) * d / fy,
 *           p[r] = ((pose[r][0]*x + pose[r][1]*y) + pose[r][2]*d) + pose[r][3]  for r = 0, 1, 2.
 *           A rejected pixel's point is (+inf, +inf, +inf).
 *  colour   MI_ICP_COLOR_U8X3: (float)u8 / 255.0f per channel; MI_ICP_COLOR_F32X1: the value, three times.
 *           A rejected pixel's colour is (+inf, +inf, +inf); an accepted pixel keeps its colour even where
 *           its point is not finite.
 *  normal   (rgbd = 1, stride 1) of pixel pix: zero when row < 1 || col < 1.  Otherwise, with the points of
 *           l = pixel pix-1, r = pixel pix+1, u = pixel pix-width, d = pixel pix+width -- so the right
 *           neighbour of the last column is the next row's first pixel; r and d count as (0,0,0) when their
 *           index is >= width*height; any neighbour with a coordinate that is not finite counts as (0,0,0):
 *           h = l - r,  v = u - d,  c = (h1*v2 - h2*v1, h2*v0 - h0*v2, h0*v1 - h1*v0),
 *           norm = sqrtf((c0*c0 + c1*c1) + c2*c2).  norm == 0: the normal is (0,0,0).  Otherwise n = c / norm,
 *           and if n2 > 0 every component is multiplied by -1.0f (a zero component becomes -0).  The pixel's
 *           own point plays no part: a pixel without a point has a normal (seen with valid_only = 0).
 *  valid_only  keeps the pixels whose three coordinates are finite, in pixel order, with their normals and
 *           colours; 0 writes every sampled pixel.  rgbd = 0 always compacts.
 *  A comparison may rely on every word written, the sign of zeros and infinities included; only the sign and
 *  payload of a NaN are not defined (a NaN arises from 0 * inf and inf - inf: col == cx under an infinite
 *  depth, overflowing products). */
#define MI_ICP_DEPTH_F32 0
#define MI_ICP_DEPTH_U16 1
#define MI_ICP_COLOR_NONE 0
#define MI_ICP_COLOR_U8X3 1
#define MI_ICP_COLOR_F32X1 2
MI_ICP_API int mi_icp_create_from_depth(mi_icp_ctx* ctx, const void* depth, int depth_type,
                                        const void* color, int color_type, int width, int height,
                                        const float* intrinsic4, const float* extrinsic,
                                        float depth_scale, float depth_trunc, float depth_cutoff,
                                        int stride, int rgbd, int compute_normals, int valid_only,
                                        float* out_xyz, float* out_normals, float* out_colors,
                                        int64_t* m, int mem_kind);
/* odometry::ComputeRGBDOdometry (odometry/odometry.cu:833-943, odometry.h:43-53): the
 * transformation that maps the source RGB-D frame onto the target frame, and the 6x6
 * information matrix of the result.  The other in-repo caller of ComputeJTJandJTr /
 * SolveJacobianSystemAndObtainExtrinsicMatrix (utility/eigen.h:79-115) besides the ICP
 * estimators.
 *   colors / depths  [height][width] float32 (intensity in [0,1], depth in the scene's unit);
 *   intrinsic4       fx, fy, cx, cy;   odo_init: 4x4 column-major or NULL (identity);
 *   jacobian         MI_ICP_ODOMETRY_COLOR_TERM (rgbdodometry_jacobian.inl:41-94) or
 *                    MI_ICP_ODOMETRY_HYBRID_TERM (:96-172, the reference's default);
 *   option           OdometryOption (odometry_option.h:30-62); iterations[] coarsest level
 *                    first, as iteration_number_per_pyramid_level_.
 * Outputs: *success (0: the reference's failure result -- identity transformation and
 * identity information), transformation16 column-major, information36 row-major. */
#define MI_ICP_ODOMETRY_COLOR_TERM 0
#define MI_ICP_ODOMETRY_HYBRID_TERM 1
#define MI_ICP_ODOMETRY_MAX_LEVELS 8
typedef struct mi_icp_odometry_option {
    int32_t num_levels;                               /* 3 */
    int32_t iterations[MI_ICP_ODOMETRY_MAX_LEVELS];   /* {20, 10, 5} */
    float max_depth_diff;                             /* 0.03 */
    float min_depth;                                  /* 0.0 */
    float max_depth;                                  /* 4.0 */
    /* ComputeWeightedRGBDOdometry only */
    float nu;                                         /* 5.0 */
    float sigma2_init;                                /* 1.0 */
    float inv_sigma_mat_diag[6];                      /* 0 */
} mi_icp_odometry_option;
MI_ICP_API int mi_icp_compute_rgbd_odometry(mi_icp_ctx* ctx, const float* source_color,
                                            const float* source_depth, const float* target_color,
                                            const float* target_depth, int width, int height,
                                            const float* intrinsic4, const float* odo_init,
                                            int jacobian, const mi_icp_odometry_option* option,
                                            int* success, float* transformation16,
                                            double* information36, int mem_kind);
/* odometry::ComputeWeightedRGBDOdometry (odometry/odometry.cu:633-706,766-831,927-941): the same
 * with t-distribution weights on the correspondences (always the hybrid term) and a motion prior
 * inv_sigma_mat_diag . (prev_twist - velocity so far); twist6 receives the velocity of this call
 * (angle * axis, translation: utility::TransformMatrix4fToVector6f).  prev_twist6 may be NULL (0). */
MI_ICP_API int mi_icp_compute_weighted_rgbd_odometry(mi_icp_ctx* ctx, const float* source_color,
                                                     const float* source_depth, const float* target_color,
                                                     const float* target_depth, int width, int height,
                                                     const float* intrinsic4, const float* odo_init,
                                                     const float* prev_twist6,
                                                     const mi_icp_odometry_option* option, int* success,
                                                     float* transformation16, float* twist6,
                                                     double* information36, int mem_kind);
/* InitializePointCloudForGeneralizedICP's normals -> covariances
 * (registration/generalized_icp.cu:18-30,52-59). */
MI_ICP_API int mi_icp_covariances_from_normals(mi_icp_ctx* ctx, const float* normals,
                                               int64_t n, float epsilon, float* covs,
                                               int mem_kind);
/* PointCloud::EstimateNormals(KDTreeSearchParamKNN(knn))
 * (geometry/estimate_normals.cu:82-127), knn <= 100 (knn::NUM_MAX_NN,
 * knn/kdtree_search_param.h:26; lists of up to 32 neighbours take the faster kernel).
 * Workspace: the k-NN kernels (this call, mi_icp_search_knn, the colour gradients) keep
 * their candidates' INDICES in a device slab sized by the waves the GPU can hold at once,
 * not by the queries: ~50 MB at any list length and any number of points (a wave claims a
 * row of its XCD's pool when it starts and returns it when it ends), allocated by the first
 * such call of a context and reused by the later ones; EstimateNormals builds the cloud's
 * tree in a private scratch context of its own (the caller's target / source / loop
 * state survive the call). */
MI_ICP_API int mi_icp_estimate_normals_knn(mi_icp_ctx* ctx, const float* xyz, int64_t n,
                                           int knn, float* normals, int mem_kind);
/* PointCloud::EstimateNormals(KDTreeSearchParamRadius(radius, max_nn)): the max_nn
 * (<= 100) nearest points with d2 < radius^2, as KDTreeFlann::SearchRadius
 * feeds it (geometry/estimate_normals.cu:93-101, knn/kdtree_flann.inl:96-122);
 * fewer than 3 neighbours -> (0,0,1). */
MI_ICP_API int mi_icp_estimate_normals_radius(mi_icp_ctx* ctx, const float* xyz, int64_t n,
                                              float radius, int max_nn, float* normals,
                                              int mem_kind);

/* PointCloud::RemoveStatisticalOutliers(nb_neighbors, std_ratio) (geometry/down_sample.cu:354-438).
 * Per point, avg = the mean of the SQUARED distances of its nb_neighbors nearest points, itself
 * included (fewer when the cloud has fewer points); mean = sum(avg) / n; std = sqrt(sum over the
 * points with avg > 0 of (avg - mean)^2 / (n - 1)); a point is kept iff avg > 0 and
 * avg < mean + std_ratio * std -- so a point whose neighbours all coincide with it is removed, and
 * fewer than 2 points give an empty result, as in the reference.
 * Outputs: the kept points with their normals / colours (either may be NULL; covariances are not
 * carried, as in the reference), out_indices (int64, may be NULL) their original indices ascending,
 * *m their count; all arrays hold n entries.  avg_d2 (float[n] or NULL): avg of every point in the
 * cloud's order.
 * Deviations (deliberate): a point's k fp32 squared distances are added in fp64 -- in any order the
 * same sum -- divided in fp64 and rounded once to fp32; mean, the sum of squares and the threshold
 * are fp64 sums in a fixed order (per block, then over the blocks; no float atomics), the
 * comparison is (double)avg < threshold: the same input gives the same output on every run and
 * every context (the reference sums in fp32 in thrust's order).
 * Limits: nb_neighbors in [1, 100] (knn::NUM_MAX_NN), std_ratio > 0; else MI_ICP_ERR_INVALID.
 * The cloud's tree is built in the private scratch context, as for EstimateNormals: the caller's
 * target / source / loop state survive the call.  Synchronises the context's stream. */
MI_ICP_API int mi_icp_remove_statistical_outliers(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                                  const float* colors, int64_t n, int nb_neighbors,
                                                  float std_ratio, float* out_xyz, float* out_normals,
                                                  float* out_colors, int64_t* out_indices, float* avg_d2,
                                                  int64_t* m, int mem_kind);
/* PointCloud::RemoveRadiusOutliers(nb_points, search_radius) (geometry/down_sample.cu:317-352): a
 * point is kept iff SearchRadius(search_radius, max_nn = nb_points + 1) -- d2 < radius^2 in fp32,
 * the point itself included -- finds nb_points + 1 points.  Outputs as for the statistical filter;
 * counts (int32[n] or NULL): the number found per point in the cloud's order, capped at
 * nb_points + 1.  Limits: nb_points >= 1 with nb_points + 1 <= 100 (knn::NUM_MAX_NN), radius > 0;
 * else MI_ICP_ERR_INVALID.  Scratch context and synchronisation as above. */
MI_ICP_API int mi_icp_remove_radius_outliers(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                             const float* colors, int64_t n, int nb_points, float radius,
                                             float* out_xyz, float* out_normals, float* out_colors,
                                             int64_t* out_indices, int32_t* counts, int64_t* m, int mem_kind);

/* PointCloud::ClusterDBSCAN(eps, min_points, print_progress, max_edges)
 * (geometry/pointcloud_cluster.cu:109-179).  Its contract, which the labels meet exactly:
 *   row(i)  SearchRadius(p_i, eps, max_nn = max_edges + 1): the nearest max_edges + 1 points with
 *           fp32 d2 < eps*eps, ascending in distance, ties ascending in index, the point itself
 *           among them (pointcloud_cluster.cu:124-125).
 *   N(i)    row(i) without i; deg(i) = |N(i)|; i is CORE iff deg(i) >= min_points.  A non-core
 *           point keeps no edges (pointcloud_cluster.cu:41-53).
 *   edges   i -> j for every core i and j in N(i); reach(i) = i and all it reaches along edges.
 *   roots   the loop at pointcloud_cluster.cu:147-178 visits the points in order and starts a BFS
 *           from every point no earlier BFS reached: r is a ROOT iff no j < r has r in reach(j).
 *           A root starts a cluster iff |reach(r)| >= min_points (every core root does); the
 *           clusters are numbered 0, 1, ... in ascending order of their roots.
 *   labels  label(x) = the number of the LARGEST root whose reach holds x (each BFS overwrites
 *           the labels of all it reaches), or -1 when that root started no cluster.
 * Hence, as in the reference: a border point reachable from several clusters takes the highest
 * number; with min_points <= 1 an isolated point is a cluster of its own; with max_edges = 0
 * every row holds one point; a truncated row can make an edge one-way (j in N(i), i not in
 * N(j)), and a later root can then reach into an earlier cluster and relabel all of it, so a
 * cluster number may appear on no point; and when more than max_edges points coincide with p_i
 * at lower indices, i is not in its own row and deg(i) counts all max_edges + 1.
 * Outputs: labels int32[n]; degrees int32[n] or NULL: deg(i), before the core test (the
 * reference keeps 0 for non-core points); *n_clusters = the cluster numbers handed out.
 * Limits: eps > 0 with eps*eps finite (the reference would square a negative eps: a deviation),
 * min_points >= 0, max_edges in [0, 100] (knn::NUM_MAX_NN), n < 2^31; else MI_ICP_ERR_INVALID.
 * n = 0 gives zero clusters.  Labels are integers fixed by the contract: every run and every
 * context gives the same bytes.  The cloud's tree is built in the private scratch context, as for
 * EstimateNormals: the caller's target / source / loop state survive the call.  Memory on top of
 * the tree: n * (max_edges + 1) int32 rows and 48 bytes per point (4.5 GB at n = 10M, max_edges
 * = 100).  Synchronises the context's stream once; truncated rows that chain one-way edges
 * through more than a few pieces add one wait per 16 further rounds. */
MI_ICP_API int mi_icp_cluster_dbscan(mi_icp_ctx* ctx, const float* xyz, int64_t n, float eps,
                                     int64_t min_points, int max_edges, int32_t* labels,
                                     int32_t* degrees, int64_t* n_clusters, int mem_kind);

/* PointCloud::SegmentPlane(distance_threshold, ransac_n, num_iterations) (geometry/segmentation.cu:
 * 187-268): RANSAC over planes through three points.  All hypotheses are drawn up front and scored
 * in one pass over the points; the contract, which the outputs meet exactly (the refit apart):
 *   sampler   u(j), j = 0, 1, ...: output j of splitmix64 seeded with `seed`, all in uint64:
 *               z = seed + (j + 1) * 0x9E3779B97F4A7C15;  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;
 *               z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  u = z ^ (z >> 31).
 *             below(u, k) = floor(u * k / 2^64) (the high word of the 128-bit product).
 *   triple    iteration t = 0 .. num_iterations - 1 draws  i0 = below(u(3t), n);
 *               i1 = below(u(3t + 1), n - 1), plus 1 if i1 >= i0;
 *               i2 = below(u(3t + 2), n - 2), plus 1 if i2 >= min(i0, i1), then plus 1 if
 *               i2 >= max(i0, i1)  (the comparisons use the updated values).
 *             Three distinct indices, a pure function of (seed, t, n): the head of a uniform
 *             permutation, as the reference's three are.
 *   plane     ComputeTrianglePlane (segmentation.cu:60-74) of p0 = xyz[i0], p1, p2 in fp32, every
 *             operation rounded, none fused:  e0 = p1 - p0, e1 = p2 - p0,
 *               a = e0y*e1z - e0z*e1y,  b = e0z*e1x - e0x*e1z,  c = e0x*e1y - e0y*e1x,
 *               norm = sqrt((a*a + b*b) + c*c);  the hypothesis is VALID iff 0 < norm < inf; then
 *               (a, b, c) /= norm (IEEE division),  d = -((a*x0 + b*y0) + c*z0).
 *   distance  dist(p) = |fma(c, z, fma(b, y, fma(a, x, d)))| in fp32: three fused multiply-adds, d
 *             first.  p is an INLIER iff dist(p) < distance_threshold, strictly (a NaN never is).
 *             The scoring pass and the pass that lists the inliers evaluate this one expression.
 *   winner    count(t) = the inliers of hypothesis t, an integer.  Among the valid hypotheses
 *             with count >= 1: the largest count; among equal counts the smallest error sum, the
 *             fp64 sum of the inliers' fp32 distances in a fixed order (per thread, wave, block,
 *             then the blocks in order -- computed only when counts tie); among equal sums the
 *             lowest t.  (At equal count the reference's inlier_rmse_ = sum / sqrt(count) orders
 *             as the sum does, and it keeps the first of equals, segmentation.cu:237-242.)
 *   none      no valid hypothesis with an inlier (all triples collinear, num_iterations <= 0,
 *             threshold <= 0 or NaN): the best plane stays (0, 0, 0, 0) as in the reference, every
 *             finite point's distance is 0, so every such point is an inlier when
 *             distance_threshold > 0 and none otherwise.  *best_iteration = -1, *best_count = 0.
 *   outputs   inliers (int64[n] on the side mem_kind names): the *m indices of the winning RANSAC
 *             plane's inliers, ascending.  ransac_plane4 (host float[4] or NULL): that plane.
 *             plane4 (host float[4]): GetPlaneFromPoints of those inliers (segmentation.cu:135-185):
 *             centroid; the six centred second moments xx xy xz yy yz zz; det_x = yy*zz - yz*yz,
 *             det_y = xx*zz - xz*xz, det_z = xx*yy - xy*xy; the branch of the strictly largest
 *             (x before y before z, as written there) gives abc; abc /= |abc|; d = -abc . centroid;
 *             no inliers or a zero norm: the zero plane.  All sums (fixed order: per block, then
 *             the blocks in order), the centring, determinants and the normalisation in fp64,
 *             rounded to fp32 once.  *best_iteration / *best_count (host, may be NULL): the
 *             winner's t and count(t).
 *   arguments ransac_n < 3 or n < ransac_n: MI_ICP_OK with the zero planes and *m = 0 (the reference
 *             logs an error and returns exactly that).  ransac_n > 3 still samples three points,
 *             as in the reference.
 * Deviations (deliberate): the random stream is not the reference's (rand() seeding
 * thrust::default_random_engine, then a sort of n keys per iteration): same distribution of triples,
 * other triples.  Counts are compared as integers (the reference compares (float)count / (float)n,
 * which ties distinct counts once n exceeds 2^24).  The distance is the fma chain above (the
 * reference: Eigen's 4-vector dot in fp32, order unspecified).  The refit is fp64 (the reference sums
 * in fp32 in thrust's order and is not reproducible bit for bit even by itself).
 * Limits: n < 2^31, num_iterations <= 65536; else MI_ICP_ERR_INVALID.  Integers apart from the refit,
 * whose sums have a fixed order: every run and every context gives the same bytes.  Runs in the
 * private scratch context, as the outlier filters do: the caller's target / source / loop state
 * survive.  The number of kernel launches does not depend on num_iterations, the points are read
 * once for scoring per 2048 hypotheses, once for the flags, twice for the refit (and once per
 * block row of the tie pass when counts tie).  Synchronises the context's stream once (twice with
 * MI_ICP_HOST, for the copy of the list). */
MI_ICP_API int mi_icp_segment_plane(mi_icp_ctx* ctx, const float* xyz, int64_t n, float distance_threshold,
                                    int64_t ransac_n, int64_t num_iterations, uint64_t seed, float* plane4,
                                    float* ransac_plane4, int64_t* inliers, int64_t* m,
                                    int64_t* best_iteration, int64_t* best_count, int mem_kind);

/* geometry::keypoint::ComputeISSKeypoints(input, salient_radius, non_max_radius, gamma_21, gamma_32,
 * min_neighbors, max_neighbors) (geometry/iss_keypoints.cu:37-172): Intrinsic Shape Signatures.  Its
 * contract, which mask, counts and saliency meet exactly given the eigenvalues (these carry fp32
 * rounding in an order the contract leaves open):
 *   radii     salient_radius == 0 or non_max_radius == 0: BOTH are replaced (iss_keypoints.cu:124-127)
 *             by 6 * resolution and 4 * resolution (fp32 products), resolution =
 *             (float)sqrt(S / n) in fp64, S = the fp64 sum, in a fixed order, over all points of the
 *             fp32 squared distance to the nearest other entry of a k = 2 search (the point itself
 *             being the first; a duplicate counts with 0) -- an RMS, as the reference computes it.
 *             radii_out (host float[2] or NULL): the radii used.
 *   row(i,r)  the points j with fp32 d2(i, j) < r*r (r*r one fp32 product; d2 = fma(dz, dz,
 *             fma(dy, dy, dx*dx)) of the fp32 differences p_i - p_j, as everywhere in this header), the
 *             point itself among them; when more than max_neighbors, the max_neighbors smallest by
 *             (d2, index) -- SearchRadius(r, max_neighbors), ClusterDBSCAN's row convention.
 *   eig(i)    count = |row(i, salient_radius)|.  count < min_neighbors: eig = (-1, -1, -1).  Otherwise
 *             the nine cumulants (x, y, z, xx, xy, xz, yy, yz, zz) of q = p_j - p_i over the row in
 *             fp32 (the subtraction first, products unfused, the sums in an order the contract leaves
 *             open), each divided by (float)count, C = E[qq^T] - E[q]E[q]^T entry by entry as the
 *             reference forms it.  ZERO TEST: Eigen's isZero() at its fp32 default, i.e. every
 *             |C_ij| <= 1e-5 ABSOLUTE (a cloud whose salient neighbourhoods are smaller than a few
 *             millimetres in its own unit has no keypoints, in the reference as here): eig =
 *             (-1, -1, -1).  Otherwise FastEigen3x3Val (utility/eigenvalue.inl:93-170): with
 *             mc = the largest of the nine entries (signed), mc == 0 gives zeros; off-diagonal
 *             entries of C / mc all zero gives the diagonal of C itself; otherwise the closed form
 *             gives the eigenvalues of C / mc, NOT scaled back.  Sorted as the reference sorts
 *             them: e0 = min, e2 = max, e1 = ((v0 + v1) + v2) - e0 - e2.  These values are compared
 *             across points as they are -- scaled in one point, unscaled in the next -- in the
 *             reference and here.
 *   saliency  e0 if e2 > 0 && e1 / e2 < gamma_21 && e0 / e1 < gamma_32 (IEEE fp32 divisions; a NaN
 *             compares false), else -1.  A flat or straight neighbourhood has e0 = 0 or a rounding
 *             error of either sign: it passes the gates when e1 > 0, and its saliency is that e0.
 *   mask(i)   saliency(i) >= 0 and no l in row(i, non_max_radius) has saliency(i) < saliency(l)
 *             (strict: tied neighbours both stay).  So a negative e0 is never a keypoint and
 *             suppresses nobody; e0 = 0 is one when nothing in its row is positive.
 * Outputs, n entries each on the side mem_kind names: mask_out (uint8, 0 / 1); saliency_out (float),
 * eig_out (float[n][3]), counts_out (int32: count above) -- each may be NULL; *m = the number of
 * mask bytes set.  The keypoints themselves: mi_icp_select_by_mask.
 * Deviation (deliberate): the reference accumulates raw coordinates; the covariance is the same
 * quantity, but E[xx] - E[x]E[x] in fp32 then cancels to the order of the smallest eigenvalue for
 * coordinates of order 1 (DESIGN.md has the measurement).  Negative radii are turned away (the
 * reference would square them).
 * Limits: radii >= 0 with finite squares, max_neighbors in [1, 100] (knn::NUM_MAX_NN), n < 2^31; else
 * MI_ICP_ERR_INVALID.  n = 0 gives *m = 0.  The same input gives the same bytes on every run and
 * context.  The cloud's tree is built once, in the private scratch context: the caller's target /
 * source / loop state survive.  Memory on top of the tree: 13 bytes per point plus the outputs;
 * no row is written out.  Synchronises the context's stream once, twice when the radii are computed. */
MI_ICP_API int mi_icp_iss_keypoints(mi_icp_ctx* ctx, const float* xyz, int64_t n, float salient_radius,
                                    float non_max_radius, float gamma_21, float gamma_32, int min_neighbors,
                                    int max_neighbors, uint8_t* mask_out, float* saliency_out, float* eig_out,
                                    int32_t* counts_out, float* radii_out, int64_t* m, int mem_kind);

/* PointCloud::GaussianFilter(search_radius, sigma2, num_max_search_points) (geometry/pointcloud.cu:
 * 56-106, 387-434).  Its contract:
 *   row(i)  row(i, search_radius) of mi_icp_iss_keypoints above with max_neighbors =
 *           num_max_search_points: fp32 d2 < r*r, the smallest by (d2, index) when more, the point
 *           itself among them.
 *   w_j     exp(-0.5 * d2(i, j) / sigma2) in fp32, d2 the value the row was chosen by.
 *   out(i)  sum over row(i) of w_j * p_j, divided by the sum of the w_j; likewise the normals and
 *           colours where given (either may be NULL).  Normals are NOT re-normalised, as in the
 *           reference.  The point itself has w = 1, so the divisor is at least 1, and a row that holds
 *           the point alone returns it bit for bit (a coordinate of -0 comes back as +0: 0 + 1 * -0).
 * Everything is fp32.  The order of the sums and the rounding of exp are left open (here: the row in
 * the order the search left it, expf within 1 ulp); the same input gives the same bytes on every run
 * and context.  Outputs hold n entries, in the input's order; the cloud keeps its size.
 * Non-finite coordinates are outside the contract.  What happens: such a point is in no row, its
 * own included (no d2 compares below r*r), and its outputs are NaN (0 / 0); the finite points'
 * outputs are as if it were absent.  The call terminates.
 * Limits, the reference's: search_radius > 0 with a finite square, sigma2 > 0 and finite,
 * num_max_search_points in [1, 100] (knn::NUM_MAX_NN), n < 2^31; else MI_ICP_ERR_INVALID, before any
 * buffer is touched.  n = 0 is MI_ICP_OK.  The cloud's tree is built in the private scratch context:
 * the caller's target / source / loop state survive.  No row is written out: memory on top of the
 * tree is the outputs.  Synchronises the context's stream once. */
MI_ICP_API int mi_icp_gaussian_filter(mi_icp_ctx* ctx, const float* xyz, const float* normals,
                                      const float* colors, int64_t n, float search_radius, float sigma2,
                                      int num_max_search_points, float* out_xyz, float* out_normals,
                                      float* out_colors, int mem_kind);

/* ---- integration::UniformTSDFVolume (integration/uniform_tsdfvolume.{h,cu}, integrate_functor.h,
 * tsdfvolume.h; the multiplier image of geometry/image_factory.cu:32-48,136-165) ----------------------
 * A volume of resolution^3 voxels of edge voxel_length = length / (float)resolution, each holding
 * (tsdf, weight, colour[3]), indexed x*res*res + y*res + z.  It belongs to the context that made it:
 * mi_icp_destroy frees the volumes still alive, and a volume is only accepted by its own context.
 * Stored as planes (tsdf, weight, and three colour planes only when color_type != NO_COLOR): 8 or 20
 * bytes per voxel.  Not built: ExtractTriangleMesh (there is no TriangleMesh type here), ExtractVoxelGrid,
 * IntegrateWithDepthToCameraDistanceMultiplier as an entry.  ScalableTSDFVolume is the next section.
 *
 * THE NUMERIC CONTRACT.  Everything is fp32, products and sums unfused, division and square root
 * correctly rounded, in the order written; three-term sums and dot products run left to right,
 * (a + b) + c.  h = resolution / 2 (integer division; odd resolutions are legal), half =
 * 0.5f * voxel_length, E the extrinsic, D[r] = voxel_length * E[r][2].  A numpy fp32 restatement of
 * these lines is bit-equal to the kernels (tests/tsdf_exact.py).
 *  Reset      tsdf 0, weight 0, colour (1, 1, 1); a new volume is reset.
 *  Integrate  multiplier(i, j) = sqrtf((xx*xx + yy*yy) + 1), xx = ((float)j - cx) * (1/fx),
 *             yy = ((float)i - cy) * (1/fy); built once per (width, height, intrinsic) and kept.
 *             For voxel (x, y, z), xr = x - h etc.:
 *               px = (half + voxel_length*xr) + origin[0], py likewise, pz = half + origin[2] (z = 0)
 *               P[r] = (((E[r][0]*px + E[r][1]*py) + E[r][2]*pz) + E[r][3]) + (float)zr * D[r]
 *               skip if P[2] <= 0
 *               u_f = (P[0]*fx / P[2] + cx) + 0.5f, v_f = (P[1]*fy / P[2] + cy) + 0.5f
 *               skip unless u_f >= 0.0001f && u_f < (float)width - 0.0001f && v_f >= 0.0001f &&
 *                           v_f < (float)height - 0.0001f
 *               u = floor(u_f), v = floor(v_f); d = depth(v, u); skip if d <= 0
 *               sdf = (d - P[2]) * multiplier(v, u); skip unless sdf > -sdf_trunc
 *               t = min(1, sdf * (float)(1.0 / (double)sdf_trunc))   (clamped from above only)
 *               tsdf = (tsdf*w + t) / (w + 1); each colour channel c = (c*w + s) / (w + 1) with s the
 *               RGB8 byte of that channel (kept in 0..255) or the Gray32 value (in all three);
 *               weight = w + 1.
 *             A voxel that is skipped is neither read nor written.
 *  valid      w != 0 && tsdf < 0.98f && tsdf >= -0.98f
 *  ExtractVoxelPointCloud   the valid voxels in ascending index: point ((half + voxel_length*xr) +
 *             origin[0], ...), colour (c, c, c) with c = (float)(((double)tsdf + 1.0) * 0.5).
 *  ExtractPointCloud   candidates in ascending (((x-1)*(res-2) + (y-1))*(res-2) + (z-1))*3 + axis over
 *             x, y, z in [1, res-2]: voxel 0 = (x, y, z) valid, voxel 1 = its neighbour at +1 along axis
 *             with that coordinate + 1 < res - 1, valid, and f0*f1 < 0.  Then r0 = |f0|, r1 = |f1|,
 *               q = (half + voxel_length*x, half + voxel_length*y, half + voxel_length*z)  (x not - h)
 *               q[axis] = (q[axis]*r1 + (q[axis] + voxel_length)*r0) / (r0 + r1)
 *               point = (q + origin) - (float)h * voxel_length
 *               colour = (c0*r1 + c1*r0) / (r0 + r1), for RGB8 then / 255.0f; none for NO_COLOR
 *               normal: n[k] = T(q with q[k] := (float)((double)q[k] + gap)) - T(q with q[k] :=
 *               (float)((double)q[k] - gap)), gap = 0.99 * (double)voxel_length; with zz = (n0*n0 +
 *               n1*n1) + n2*n2: n / sqrtf(zz) when zz > 0, else n as it is (Eigen's normalized()).
 *               T(p) (GetTSDFAt): g = p / voxel_length - 0.5f, i = floor(g), r = g - (float)i,
 *               s = 0; s += (1-r0)*(1-r1)*(1-r2)*t000; s += (1-r0)*(1-r1)*r2*t001; ... in the order
 *               000, 001, 010, 011, 100, 101, 110, 111 of (x, y, z) offsets, each product left to right.
 *  Raycast    pose = utility::InverseTransform(extrinsic): R = E[0..2][0..2]^T, pt[r] = ((-R[r][0])*t0 +
 *             (-R[r][1])*t1) + (-R[r][2])*t2 with t the extrinsic's last column; t = pt - origin.
 *             Pixel (x, y): pp = (((float)x - cx) / fx, ((float)y - cy) / fy, 1);
 *             dir[r] = (R[r][0]*pp0 + R[r][1]*pp1) + R[r][2]; dn = sqrtf((d0*d0 + d1*d1) + d2*d2);
 *             dir = dir / dn.  length = (float)res * voxel_length, step = sdf_trunc * 0.5f.
 *               tmin = fmax(fmax(q0, q1), q2), q_k = ((dir_k > 0 ? 0 : length) - t_k) / dir_k
 *               tmax = fmin(fmin(...)) of ((dir_k > 0 ? length : 0) - t_k) / dir_k
 *             -- IEEE quotients: a zero direction component gives +-inf or NaN, and fmax / fmin return
 *             the operand that is not NaN (np.fmax / np.fmin).  As in the reference the box tested is
 *             [0, length]^3 in t's frame although the voxels cover [-h*voxel_length, (res-h)*voxel_length).
 *               len = fmax(tmin, 0); invalid if len >= tmax; len = len + voxel_length
 *               g = floor((t + dir*len) / voxel_length) + h; invalid unless every g_k in [0, res-1)
 *               cur = tsdf(g); max = len + length * 1.41421354f
 *               for (; len < max; len = len + step):
 *                 g = floor((t + dir*(len + step)) / voxel_length) + h; unless every g_k in [1, res-1): next
 *                 prev = cur; cur = tsdf(g); if prev < 0 && cur > 0: invalid
 *                 if prev > 0 && cur < 0:
 *                   ts = len - step*prev / (cur - prev); vtx = t + dir*ts; loc = vtx / voxel_length + (float)h
 *                   invalid unless every loc_k in [1, res-1), and for each axis loc_k + 1 < res-1 and
 *                   loc_k - 1 >= 1; n[k] = I(loc + e_k) - I(loc - e_k); nn = sqrtf((n0*n0 + n1*n1) + n2*n2);
 *                   invalid if nn == 0; normal = n / nn; point = vtx + origin;
 *                   colour of voxel (int)loc: RGB8 (float)((double)c / 255.0), Gray32 c, NO_COLOR 0.
 *               I(p) (InterpolateTrilinearly): i = (int)p, i_k -= 1 where p_k < (float)i_k + 0.5f,
 *               a = p - ((float)i + 0.5f); ((((((t000*(1-a0)*(1-a1)*(1-a2) + t001*(1-a0)*(1-a1)*a2) +
 *               t010*(1-a0)*a1*(1-a2)) + t011*(1-a0)*a1*a2) + t100*a0*(1-a1)*(1-a2)) + t101*a0*(1-a1)*a2)
 *               + t110*a0*a1*(1-a2)) + t111*a0*a1*a2, each product left to right.
 *             Output in pixel order; invalid pixels are NaN in all nine values, removed
 *             (RemoveNoneFinitePoints(true, true)) when valid_only != 0.
 *  Where the reference leaves something undefined, the choice made:
 *   - float -> int of floor(x): x is held inside +-1e9 first, a NaN counting as -1e9 (out of range).
 *   - dn not > 0 (zero, or NaN): invalid (the reference tests == 0 only).
 *   - len not finite after the tmin / tmax test (tmax NaN): invalid.
 *   - a march that cannot advance, max + step == max in fp32 (camera ~1e6 steps away): invalid; the
 *     reference does not terminate.  sdf_trunc must be positive, finite and large enough for
 *     length * sqrt(2) / step <= MI_ICP_TSDF_MAX_MARCH, else MI_ICP_ERR_INVALID.
 *   - the gathers of T and I hold their indices inside [0, res-2]; for finite input they are there.
 *   - ExtractPointCloud's candidates are chosen by the crossing test; the reference tests the emitted
 *     point for NaN, which differs only for a non-finite origin.
 *   - non-finite extrinsics, intrinsics, origins or volumes are outside the contract; every call
 *     terminates and stays inside its buffers.
 *  Deviation (deliberate): the reference sizes ExtractPointCloud's outputs by the number of valid
 *  voxels and writes up to three points per voxel into them; here outputs hold the actual count.
 *
 *  raycast_levels  Raycast for every level of the camera's pyramid in one pass: mi_icp_tsdf_raycast_levels(levels, width,
 *             height, intrinsic4, ...) gives what `levels` Raycast calls with the cameras
 *             PinholeCameraIntrinsic::CreatePyramidLevel(i), i = 0 .. levels-1, give (pinhole_camera_intrinsic.h:31-36),
 *             the same extrinsic and sdf_trunc: level 0 is the intrinsic as passed; for i > 0, s = powf(0.5f, (float)i),
 *             size (width >> i) x (height >> i), fx*s, fy*s, (cx + 0.5f)*s - 0.5f, (cy + 0.5f)*s - 0.5f.  The values
 *             per pixel are those of "Raycast" above.  The levels' points are concatenated in level order, each level
 *             in pixel order: level i starts at point m[0] + ... + m[i-1] and has m[i] points (m is int64_t[levels]).
 *             `capacity` is the total in points: when it is smaller than m[0] + ... + m[levels-1] nothing is written
 *             and every m[i] is still filled.  With valid_only == 0, m[i] = (width >> i) * (height >> i) and an
 *             invalid pixel is NaN.  A level whose size is zero has 0 points.  1 <= levels <=
 *             MI_ICP_TSDF_MAX_LEVELS (an image side is at most 2^15: level 16 is always empty); otherwise the
 *             argument checks and status codes of mi_icp_tsdf_raycast.  ARRAYS ARE DEVICE POINTERS; this entry has
 *             no memory-kind argument (as the scalable volume's and the occupancy grid's).  mi_icp_tsdf_raycast is
 *             its levels == 1 form and adds the staging of MI_ICP_HOST arrays.  One launch marches every level's
 *             rays; with valid_only one scan over the concatenated pixels serves all levels, and the stream is
 *             waited for once for the counts and once after the fill, whatever the number of levels.
 *
 * OUTPUTS OF UNKNOWN SIZE follow one rule in all three calls: the caller passes a `capacity` (in
 * points) and gets the needed count in *m.  When capacity >= *m the arrays are filled with *m points;
 * otherwise nothing is written and the call is MI_ICP_OK -- call again with room (capacity 0 and null
 * arrays make a pure count query).  A raycast never needs more than width*height.
 *
 * mi_icp_tsdf_integrate: the images are described as the reference's Image fields are, and checked as
 * there (uniform_tsdfvolume.cu:677-695): depth 1 channel of 4 bytes (float32); colour 3 x 1 byte for
 * RGB8, 1 x 4 bytes (float32) for GRAY32, ignored for NO_COLOR; all sizes equal to width x height of
 * the intrinsic.  Otherwise MI_ICP_ERR_INVALID ("[UniformTSDFVolume::Integrate] Unsupported image
 * format."), the volume untouched.  intrinsic4 = fx, fy, cx, cy; extrinsic column-major 4x4 (NULL:
 * identity).  Traffic: the images once per voxel that projects into them, 8 (NO_COLOR) or 20 bytes
 * read and written per UPDATED voxel, nothing for the others.
 * mi_icp_tsdf_get_voxels: tsdf_out[n], weight_out[n], color_out[3][n] (planes; NO_COLOR volumes have
 * none: pass NULL), each may be NULL.
 * Limits: length, sdf_trunc > 0 and finite, 3 <= resolution <= MI_ICP_TSDF_MAX_RESOLUTION, image width and
 * height each at most MI_ICP_TSDF_MAX_IMAGE_SIDE (integrate and raycast; else MI_ICP_ERR_INVALID).  The extractions and a valid_only raycast wait for the stream once for the count and
 * once more after the fill; integrate waits only to release MI_ICP_HOST images. */
#define MI_ICP_TSDF_NO_COLOR 0
#define MI_ICP_TSDF_RGB8 1
#define MI_ICP_TSDF_GRAY32 2
#define MI_ICP_TSDF_MAX_RESOLUTION 1024
#define MI_ICP_TSDF_MAX_MARCH 1048576
#define MI_ICP_TSDF_MAX_IMAGE_SIDE 32768
#define MI_ICP_TSDF_MAX_LEVELS 16
typedef struct mi_icp_tsdf mi_icp_tsdf;
MI_ICP_API int mi_icp_tsdf_create(mi_icp_ctx* ctx, float length, int resolution, float sdf_trunc, int color_type,
                                  const float* origin3, mi_icp_tsdf** out);
MI_ICP_API int mi_icp_tsdf_destroy(mi_icp_ctx* ctx, mi_icp_tsdf* volume);
MI_ICP_API int mi_icp_tsdf_reset(mi_icp_ctx* ctx, mi_icp_tsdf* volume);
MI_ICP_API int mi_icp_tsdf_integrate(mi_icp_ctx* ctx, mi_icp_tsdf* volume, const void* depth, int depth_width,
                                     int depth_height, int depth_channels, int depth_bytes_per_channel,
                                     const void* color, int color_width, int color_height, int color_channels,
                                     int color_bytes_per_channel, int width, int height, const float* intrinsic4,
                                     const float* extrinsic, int mem_kind);
MI_ICP_API int mi_icp_tsdf_extract_point_cloud(mi_icp_ctx* ctx, mi_icp_tsdf* volume, float* out_xyz,
                                               float* out_normals, float* out_colors, int64_t capacity,
                                               int64_t* m, int mem_kind);
MI_ICP_API int mi_icp_tsdf_extract_voxel_point_cloud(mi_icp_ctx* ctx, mi_icp_tsdf* volume, float* out_xyz,
                                                     float* out_colors, int64_t capacity, int64_t* m,
                                                     int mem_kind);
MI_ICP_API int mi_icp_tsdf_raycast(mi_icp_ctx* ctx, mi_icp_tsdf* volume, int width, int height,
                                   const float* intrinsic4, const float* extrinsic, float sdf_trunc,
                                   int valid_only, float* out_xyz, float* out_normals, float* out_colors,
                                   int64_t capacity, int64_t* m, int mem_kind);
MI_ICP_API int mi_icp_tsdf_raycast_levels(mi_icp_ctx* ctx, mi_icp_tsdf* volume, int levels, int width, int height,
                                          const float* intrinsic4, const float* extrinsic, float sdf_trunc,
                                          int valid_only, float* out_xyz, float* out_normals, float* out_colors,
                                          int64_t capacity, int64_t* m);
MI_ICP_API int mi_icp_tsdf_get_voxels(mi_icp_ctx* ctx, mi_icp_tsdf* volume, float* tsdf_out, float* weight_out,
                                      float* color_out, int mem_kind);

/* ---- integration::ScalableTSDFVolume (integration/scalable_tsdfvolume.{h,cu}, integrate_functor.h:84-139;
 * python surface integration.cpp:153-195) ----------------------------------------------------------
 * A sparse volume: units of 16^3 voxels of edge voxel_length, opened around the surface a frame observes.
 * Unit (kx, ky, kz) -- three signed indices, each within +-(2^20 - 1) -- spans [k*L, (k+1)*L) per axis,
 * L = voxel_length * 16.0f (one fp32 product).  A voxel of a unit has index x*256 + y*16 + z and holds
 * (tsdf, weight, colour[3]).  Stored as planes over a pool of unit slots (tsdf, weight, and three colour
 * planes only when color_type != NO_COLOR: 8 or 20 bytes per voxel), slot s at [s*4096, (s+1)*4096) of
 * each plane, beside a directory: the open units' keys in ascending (kx, ky, kz) order with their slots,
 * looked up by binary search.  The volume belongs to the context that made it, as a uniform one does.
 * ARRAYS ARE DEVICE POINTERS; there is no memory-kind argument in this family (as for the occupancy grid):
 * the images and every output live on the device, a caller with host arrays copies them itself.
 * Not built: ExtractTriangleMesh (the reference's own only logs an error), a raycast (the reference has
 * none), IntegrateWithDepthToCameraDistanceMultiplier as an entry.
 *
 * THE NUMERIC CONTRACT, in the terms of the uniform volume's above (fp32, unfused, in the order written;
 * half = 0.5f * voxel_length; floor -> int as there).  tests/scalable_tsdf_exact.py restates it.
 *  Open       For each sampled pixel (row = i*stride, col = j*stride, i < height/stride, j < width/stride,
 *             integer divisions) with !(d <= 0): the world point p of mi_icp_create_from_depth(rgbd = 0,
 *             depth_scale 1000, depth_trunc 1000, stride), bit for bit: x = ((float)col - cx)*d / fx,
 *             y = ((float)row - cy)*d / fy, p[r] = ((pose[r][0]*x + pose[r][1]*y) + pose[r][2]*d) + pose[r][3],
 *             pose = the extrinsic's inverse computed in double and rounded to float.  A point with a
 *             non-finite coordinate opens nothing.  Else every unit k with
 *               floorf((p[a] - sdf_trunc) / L) <= k[a] <= floorf((p[a] + sdf_trunc) / L)   on each axis a
 *             that is not open is opened: reset to tsdf 0, weight 0, colour (1, 1, 1).  Keys outside
 *             +-(2^20 - 1) are not opened.  (The reference tests idx > n and reads one point past the end;
 *             here idx >= n.)  A frame's new keys get the slots after those in use, in ascending key
 *             order: nothing depends on thread timing.
 *  Integrate  then every voxel (x, y, z) of every open unit gets the uniform volume's Integrate lines with
 *             xr, yr, zr = x, y, z (h = 0) and origin[a] = (float)k[a] * L; the multiplier image is the same.
 *             A voxel that is skipped is neither read nor written.
 *  valid      as above.  A voxel in a unit that is not open counts as weight 0 (invalid), tsdf 0.
 *  Order of both extractions (ours; the reference's is its hash map's): units in ascending (kx, ky, kz),
 *             within a unit ascending voxel index, then the axis.
 *  ExtractVoxelPointCloud   the valid voxels: point (half + voxel_length*x) + (float)k[0]*L, ...; colour
 *             (c, c, c), c = (float)(((double)tsdf + 1.0) * 0.5).  (Declared and never defined in the
 *             reference: the uniform volume's rule.)
 *  ExtractPointCloud   for a valid voxel 0 = (x, y, z) of unit k and each axis: voxel 1 = the voxel at +1
 *             along the axis -- in the same unit, or at coordinate 0 of unit k + e_axis --, valid, f0*f1 < 0.
 *             Then r0 = |f0|, r1 = |f1|,
 *               p0[a] = (half + voxel_length*(float)x_a) + (float)k[a]*L;  p = p0
 *               p[axis] = (p0[axis]*r1 + (p0[axis] + voxel_length)*r0) / (r0 + r1)     -- the point
 *               colour = (c0*r1 + c1*r0) / (r0 + r1), for RGB8 then / 255.0f; none for NO_COLOR (the
 *               reference returns NaN colours there)
 *               normal: gap = (float)(0.99 * (double)voxel_length) (a float, unlike the uniform volume's);
 *               n[a] = T(p with p[a] := p[a] + gap) - T(p with p[a] := p[a] - gap); zz = (n0*n0 + n1*n1) +
 *               n2*n2; n / sqrtf(zz) when zz > 0, else n as it is.
 *               T(p) (GetTSDFAt): q[a] = p[a] - half; u[a] = floorf(q[a] / L); 0 when unit u is not open;
 *               g[a] = (q[a] - (float)u[a]*L) / voxel_length; i[a] = floor(g[a]) held inside [0, 15];
 *               r[a] = g[a] - (float)i[a]; f(dx, dy, dz) = the tsdf of voxel i + (dx, dy, dz) of unit u,
 *               a coordinate of 16 being coordinate 0 of the next unit along that axis, 0 where that unit
 *               is not open;
 *               T = (1-r0)*((1-r1)*((1-r2)*f(0,0,0) + r2*f(0,0,1)) + r1*((1-r2)*f(0,1,0) + r2*f(0,1,1)))
 *                 + r0*((1-r1)*((1-r2)*f(1,0,0) + r2*f(1,0,1)) + r1*((1-r2)*f(1,1,0) + r2*f(1,1,1)))
 *  Reset      closes every unit; the capacity stays.
 *  Deviations (deliberate): capacity.  map_size is the initial number of unit slots; a frame that needs
 *  more makes the pool and the directory grow by doubling before anything of the frame is integrated (the
 *  reference's map has a fixed capacity and silently drops units, which ones depending on a race).  When
 *  that allocation fails the call is MI_ICP_ERR_HIP and the volume is as it was before the frame.
 *  Outputs hold the actual count (the capacity / *m rule above).
 *
 * mi_icp_stsdf_create turns away (MI_ICP_ERR_INVALID): voxel_length or sdf_trunc not positive and finite,
 * sdf_trunc > L (so a point opens at most 4 units per axis), depth_sampling_stride < 1, map_size < 1 or
 * above MI_ICP_STSDF_MAX_UNITS, an unknown colour type.
 * mi_icp_stsdf_integrate: the images described as for mi_icp_tsdf_integrate, checked as scalable_tsdfvolume.cu:318-336
 * does; otherwise MI_ICP_ERR_INVALID ("[ScalableTSDFVolume::Integrate] Unsupported image format."), the
 * volume untouched.  A singular extrinsic is MI_ICP_ERR_INVALID.  The call waits for the stream once in
 * every frame (the number of candidate keys: zero ends stage 1) and once more in a frame that opens units
 * (their number, which growth needs); the integrate launch itself is not waited for.
 * mi_icp_stsdf_get_units: the open units in ascending key order, under the capacity rule with capacity
 * and *m in units: keys_out[m][3], tsdf_out / weight_out [m][4096], color_out[3][m][4096] (planes;
 * NO_COLOR volumes have none: pass NULL); each may be NULL.
 * mi_icp_stsdf_num_units: the number of open units and of slots (either may be NULL); does not wait. */
#define MI_ICP_STSDF_MAX_UNITS 262144
typedef struct mi_icp_stsdf mi_icp_stsdf;
MI_ICP_API int mi_icp_stsdf_create(mi_icp_ctx* ctx, float voxel_length, float sdf_trunc, int color_type,
                                   int depth_sampling_stride, int map_size, mi_icp_stsdf** out);
MI_ICP_API int mi_icp_stsdf_destroy(mi_icp_ctx* ctx, mi_icp_stsdf* volume);
MI_ICP_API int mi_icp_stsdf_reset(mi_icp_ctx* ctx, mi_icp_stsdf* volume);
MI_ICP_API int mi_icp_stsdf_integrate(mi_icp_ctx* ctx, mi_icp_stsdf* volume, const void* depth, int depth_width,
                                      int depth_height, int depth_channels, int depth_bytes_per_channel,
                                      const void* color, int color_width, int color_height, int color_channels,
                                      int color_bytes_per_channel, int width, int height, const float* intrinsic4,
                                      const float* extrinsic);
MI_ICP_API int mi_icp_stsdf_extract_point_cloud(mi_icp_ctx* ctx, mi_icp_stsdf* volume, float* out_xyz,
                                                float* out_normals, float* out_colors, int64_t capacity,
                                                int64_t* m);
MI_ICP_API int mi_icp_stsdf_extract_voxel_point_cloud(mi_icp_ctx* ctx, mi_icp_stsdf* volume, float* out_xyz,
                                                      float* out_colors, int64_t capacity, int64_t* m);
MI_ICP_API int mi_icp_stsdf_get_units(mi_icp_ctx* ctx, mi_icp_stsdf* volume, int32_t* keys_out, float* tsdf_out,
                                      float* weight_out, float* color_out, int64_t capacity, int64_t* m);
MI_ICP_API int mi_icp_stsdf_num_units(mi_icp_ctx* ctx, mi_icp_stsdf* volume, int64_t* n_units, int64_t* capacity);

/* ---- geometry::OccupancyGrid (geometry/occupancygrid.{h,cu}, densegrid.inl; the cloud of
 * geometry/pointcloud_factory.cu:418-430) ---------------------------------------------------------
 * A dense grid of resolution^3 voxels of side voxel_size around origin, each holding one fp32 log-odds,
 * NaN meaning unknown; linear index (x*res + y)*res + z; h = res / 2 (integer).  It belongs to the
 * context that made it: destroyed with mi_icp_occgrid_destroy, or with the context.  Stored as the
 * log-odds plane alone, 4 bytes per voxel (the reference keeps 24: a grid index that is the voxel's
 * position and a colour it never writes, always (0, 0, 1)), beside a one-byte mark per voxel that is
 * zero between calls.  Not built: CreateFromVoxelGrid.  The collision queries are mi_icp_collision_compute
 * (below).  The distance field of the occupied voxels is geometry::DistanceTransform (mi_icp_dt_compute_occgrid, below).
 * The occupied space leaves the library as a geometry::VoxelGrid (VoxelGrid::CreateFromOccupancyGrid, below).
 *
 * ARRAYS ARE DEVICE POINTERS; there is no memory-kind argument in this family (the preamble's one
 * exception).  `params`, viewpoint3, min3 / max3 and the counts are host memory.  voxel_size, origin and
 * the five log-odds parameters travel with every call (the reference's public members are read when a
 * call is made); only the resolution is the grid's own.
 *
 * NUMERIC CONTRACT.  fp32 in exactly the order written unless a step says double; products are never
 * fused; / and sqrt are correctly rounded.  floor(.) to int holds the value inside +-1e9 first.
 *  update(p, s)  p = isnan(p) ? 0 : p;  p = p + s;  p = p < clamping_thres_min ? clamping_thres_min : p;
 *                p = p > clamping_thres_max ? clamping_thres_max : p
 *  Insert(points, viewpoint, max_range):  n == 0 is a no-op.  A point with a coordinate that is not
 *   finite is skipped (the reference is undefined there).
 *   1 per point  d = p - viewpoint;  dist = sqrt((d.x*d.x + d.y*d.y) + d.z*d.z);
 *                hit = max_range < 0 || dist <= max_range;
 *                q = hit ? p : (dist == 0 ? viewpoint : viewpoint + (d / dist) * max_range);
 *                r = max_k |q_k - viewpoint_k|
 *   2 n_div = (int)ceil(max r / voxel_size);  n_buf = 3 * (n_div + 1).  n_div above
 *     MI_ICP_OCCGRID_MAX_NDIV: MI_ICP_ERR_INVALID, nothing changed.
 *   3 if n_div > 0, every point contributes the voxels of VoxelTraversal(start = viewpoint - origin,
 *     end = q - origin) (occupancygrid.cu:60-133):
 *       ray = end - start;  length = sqrt((ray.x*ray.x + ray.y*ray.y) + ray.z*ray.z);  length == 0: none
 *       ray = ray / length;  cur = floor(start / vs);  last = floor(end / vs);  step = sign(ray)
 *       boundary = (float)(((double)cur + 0.5 * (double)step) * (double)vs)      -- HALF a voxel
 *       tMax = (boundary - start) / ray;  tDelta = vs / |ray|;  both +inf where step == 0
 *       emit cur;  while emitted < n_buf:
 *         axis = tMaxX < tMaxY ? (tMaxX < tMaxZ ? x : z) : (tMaxY < tMaxZ ? y : z)
 *         cur[axis] += step[axis];  tMax[axis] += tDelta[axis]
 *         stop if cur == last (the end voxel is never emitted);  stop if min(tMax) > length;  emit cur
 *     emitted voxels get + h per axis; those outside [0, res)^3 are dropped
 *   4 occupied voxels: floor((q - origin) / vs) + h of the hit points, those inside the grid
 *   5 every voxel of free \ occupied: update(p, prob_miss_log), once; then every occupied voxel:
 *     update(p, prob_hit_log), once.  No sum depends on the order of the points.
 *   6 min_bound / max_bound (inclusive, both (h, h, h) at first) widen to the bounding box of the
 *     voxels step 5 updated.  (That is NOT the box of the rays' end voxels: the half-voxel boundary lets
 *     a walk leave it by a voxel.)
 *  AddVoxels(indices int32[n][3], occupied): every DISTINCT listed voxel gets update() once (the
 *   reference races on duplicates), the bounds widen.  An index outside the grid: MI_ICP_ERR_INVALID,
 *   nothing changed.
 *  SetFreeArea(min, max): imin = max(floor((min - origin) / vs) + h, 0), imax = min(floor((max - origin)
 *   / vs) + h, res - 1); the bounds are OVERWRITTEN with them; every voxel of that box gets
 *   p = isnan(p) ? 0 : p; p = p + prob_miss_log with NO clamp (both as the reference does).  A box that
 *   misses the grid leaves imin > imax on an axis: no voxel changes and the extractions are empty.
 *  query: the voxel of a point is floor((point - origin) / vs) + h per axis; out_prob_log[i] is its
 *   log-odds, NaN when it is unknown or outside the grid ON ANY AXIS (the reference tests only the
 *   linear index, so such a point aliases into another voxel); out_index (optional) int32[n][3].
 *  extract(which): the voxels of the box [min_bound, max_bound] with !isnan(p) (KNOWN), additionally
 *   p <= occ_prob_thres_log (FREE) or p > occ_prob_thres_log (OCCUPIED), ascending in linear index:
 *   out_index int32[m][3] (the voxel's position; the reference reports (0,0,0) for voxels only
 *   SetFreeArea touched), out_prob_log[m], out_xyz float[m][3] = ((float)index + (float)(0.5 - h)) * vs
 *   + origin (PointCloud::CreateFromOccupancyGrid's points), each optional.  The capacity rule of the
 *   TSDF extractions: *m is the count; with capacity < *m nothing is written.
 *  reset: every voxel unknown, the bounds (h, h, h); size and memory stay (the reference's Clear() frees
 *   the voxels and zeroes the resolution).  reconstruct: a new resolution, every voxel unknown.
 *  get_bounds: min_bound, max_bound into host int32[3] each.  get_voxels: the whole plane, res^3 floats.
 * Limits: 2 <= resolution <= MI_ICP_OCCGRID_MAX_RESOLUTION; voxel_size positive and finite; origin,
 * viewpoint and corners finite; no NaN among the five parameters, hit and miss steps finite; n_div <=
 * MI_ICP_OCCGRID_MAX_NDIV (a walk of 3 * 4097 voxels per ray at most; four times the largest grid side).
 * Else MI_ICP_ERR_INVALID and nothing changes.
 * insert and add_voxels wait for the stream once, at their end (status and bounds in one copy);
 * extract waits once for the count; get_voxels waits; the others only enqueue. */
#define MI_ICP_OCCGRID_MAX_RESOLUTION 1024
#define MI_ICP_OCCGRID_MAX_NDIV 4096
#define MI_ICP_OCCGRID_KNOWN 0
#define MI_ICP_OCCGRID_FREE 1
#define MI_ICP_OCCGRID_OCCUPIED 2
typedef struct mi_icp_occgrid mi_icp_occgrid;
typedef struct {
    float voxel_size;          /* default 0.05 */
    float origin[3];           /* default 0 */
    float clamping_thres_min;  /* default -2.0 */
    float clamping_thres_max;  /* default 3.5 */
    float prob_hit_log;        /* default 0.85 */
    float prob_miss_log;       /* default -0.4 */
    float occ_prob_thres_log;  /* default 0.0 */
} mi_icp_occgrid_params;
MI_ICP_API int mi_icp_occgrid_create(mi_icp_ctx* ctx, int resolution, mi_icp_occgrid** out);
MI_ICP_API int mi_icp_occgrid_destroy(mi_icp_ctx* ctx, mi_icp_occgrid* grid);
MI_ICP_API int mi_icp_occgrid_reset(mi_icp_ctx* ctx, mi_icp_occgrid* grid);
MI_ICP_API int mi_icp_occgrid_reconstruct(mi_icp_ctx* ctx, mi_icp_occgrid* grid, int resolution);
MI_ICP_API int mi_icp_occgrid_insert(mi_icp_ctx* ctx, mi_icp_occgrid* grid, const mi_icp_occgrid_params* params,
                                     const float* points, int64_t n, const float* viewpoint3, float max_range);
MI_ICP_API int mi_icp_occgrid_add_voxels(mi_icp_ctx* ctx, mi_icp_occgrid* grid, const mi_icp_occgrid_params* params,
                                         const int32_t* indices, int64_t n, int occupied);
MI_ICP_API int mi_icp_occgrid_set_free_area(mi_icp_ctx* ctx, mi_icp_occgrid* grid, const mi_icp_occgrid_params* params,
                                            const float* min3, const float* max3);
MI_ICP_API int mi_icp_occgrid_query(mi_icp_ctx* ctx, mi_icp_occgrid* grid, const mi_icp_occgrid_params* params,
                                    const float* points, int64_t n, float* out_prob_log, int32_t* out_index);
MI_ICP_API int mi_icp_occgrid_extract(mi_icp_ctx* ctx, mi_icp_occgrid* grid, const mi_icp_occgrid_params* params,
                                      int which, int32_t* out_index, float* out_prob_log, float* out_xyz,
                                      int64_t capacity, int64_t* m);
MI_ICP_API int mi_icp_occgrid_get_bounds(mi_icp_ctx* ctx, mi_icp_occgrid* grid, int32_t* min3, int32_t* max3);
MI_ICP_API int mi_icp_occgrid_get_voxels(mi_icp_ctx* ctx, mi_icp_occgrid* grid, float* out_prob_log);

/* ---- geometry::VoxelGrid (geometry/voxelgrid.{h,cu}, voxelgrid_factory.cu) --------------------------
 * A sparse voxel set: keys int32[m][3] (grid indices) + colors float[m][3], with voxel_size and origin[3].
 * There is no handle: a grid is those two device arrays and the two host values, and nothing is kept
 * between calls.  Every producer below emits keys DISTINCT and ASCENDING lexicographically, x most
 * significant (the reference's operator< on Vector3i, utility/helper.h:114).  Not built:
 * CreateFromTriangleMesh[WithinBounds] (no TriangleMesh here), GetOrientedBoundingBox, file I/O,
 * visualisation; OccupancyGrid::CreateFromVoxelGrid and UniformTSDFVolume::ExtractVoxelGrid.  The collision
 * queries are mi_icp_collision_compute (below).
 * The distance field of a grid's voxels is geometry::DistanceTransform (mi_icp_dt_compute_voxelgrid, below).
 *
 * ARRAYS ARE DEVICE POINTERS; there is no memory-kind argument in this family (the preamble's
 * exception).  voxel_size, bounds, origin, camera matrices, counts and the three bounds outputs are host
 * memory.  THE CAPACITY RULE of every extraction here: *m is the count; with capacity < *m nothing is
 * written.  A refusal is MI_ICP_ERR_INVALID with nothing changed.
 *
 * NUMERIC CONTRACT.  fp32 in exactly the order written unless a step says double; products are never
 * fused.  floor(.) to int holds the value inside +-1e9 first.  A key whose x is INT32_MIN is no key: the
 * sorting entries (merge, an unsorted query) leave such an entry out.
 *  from_points(xyz, colors | NULL, n, voxel_size, min_bound, max_bound)  CreateFromPointCloudWithinBounds.
 *   key = floor((p - min_bound) / voxel_size) per axis.  A point with a coordinate that is not finite is
 *   skipped (the reference is undefined there).  Keys may be negative.  Without colours every voxel is
 *   (1, 1, 1); with colours a voxel's colour is the mean of its points' colours, summed IN DOUBLE and
 *   divided by the count in double, rounded once -- the rule of mi_icp_voxel_downsample.  Runs of up to
 *   32 points are added in input order (the sort is stable); a longer run is added 64 wide: partial sum
 *   l takes elements l, l + 64, ... in order and the 64 are added in a fixed order.  Either way the same
 *   input gives the same bits on every call, and the result is within one fp32 ulp of the input-order
 *   mean.  (The reference adds in fp32 in thrust's order.)  Refused: voxel_size <= 0 or not finite;
 *   voxel_size * INT_MAX < max(max_bound - min_bound) (both as the reference logs an error); a bound that
 *   is not finite.  n == 0: an empty grid.  No span of keys is refused: key - min is packed into exactly
 *   the bits the three extents need and sorted as one 32-bit or one 64-bit key; extents that need more
 *   than 64 bits together (two clusters 3e6 voxels apart on every axis already do: 3 x 22 bits) take two
 *   stable sorts, (y, z) then x.
 *  dense(num_w, num_h, num_d)  CreateDense's keys: idx -> (idx / (h*d), (idx % (h*d)) / d, idx % d),
 *   colour (1, 1, 1); already ascending.  A count <= 0: empty.  More than 2^31 - 1 voxels: refused (the
 *   reference overflows an int).  The host makes num_* = (int)round(extent / voxel_size).
 *  merge(A, B, mode)  A's entries then B's, stable-sorted by key, one entry per key.
 *   MI_ICP_VOXELGRID_AVERAGE (operator+=): the fp32 sum of the run's colours, left to right in that
 *   order, divided by the run length in fp32.  MI_ICP_VOXELGRID_KEEP_FIRST (AddVoxel / AddVoxels): the
 *   run's first entry -- an existing voxel over an added one, the first listed among added duplicates
 *   (the reference's sort_by_key + unique_by_key does not promise which).
 *  carve(image, intrinsic4 = fx fy cx cy, extrinsic16 column-major | NULL)  CarveDepthMap and
 *   CarveSilhouette (they differ in their error text only).  Per voxel: c = ((float)key + 0.5f) * vs +
 *   origin; r = vs / 2; corners c + (-+r, -+r, -+r) in the order of GetVoxelBoundingPoints; per corner
 *   X = ((R row . p), summed left to right) + t; uvz = K X with the full 3x3 K, zeros included, each row
 *   summed left to right; z = uvz.z, u = uvz.x / z, v = uvz.y / z.  within = image is 1 channel x 4
 *   bytes && 0 <= u <= width - 1 && 0 <= v <= height - 1 (a NaN u or v is not within; the reference
 *   converts it to int, which is undefined).  d = FloatValueAt (geometry/image.h:240-264): ui =
 *   clamp((int)u, 0, width - 2), vi likewise, pu = u - ui, pv = v - vi, d = (v00*(1-pv) + v01*pv)*(1-pu)
 *   + (v10*(1-pv) + v11*pv)*pu with v01 the pixel BELOW v00.  The voxel stays iff some corner has
 *   (!within && keep_voxels_outside_image) || (within && d > 0 && z >= d).  Output: the voxels that stay,
 *   in their order; out arrays of m entries.  Refused: width or height < 2.
 *  query(keys, m, keys_sorted, queries, nq)  CheckIfIncluded: the voxel of a query is floor((q - origin) /
 *   vs); out_included[i] = 1 iff that key is in the grid -- a binary search per query; with keys_sorted
 *   == 0 the entry sorts a scratch copy once first.  A query that is not finite is not included and has
 *   index (0, 0, 0).  out_index (optional) int32[nq][3].
 *  bounds(keys, m > 0)  per-axis min and max index and, per axis, the DOUBLE sum of the voxel centres
 *   ((float)key * vs + origin) + 0.5f * vs (each in fp32), in a fixed order.  The host applies
 *   GetMinBound = min * vs + origin, GetMaxBound = (max + 1) * vs + origin, GetCenter = sum / m rounded
 *   once (the reference sums in fp32); an empty grid gives origin / origin / zero without a call.
 *  select_by_index: the rules of mi_icp_select_by_index (an index out of range is an error; invert
 *   treats a repeated index once), on keys + colours.  paint: indices == NULL paints every voxel
 *   (PaintUniformColor), else the listed ones (PaintIndexedColor; an index out of range is an error and
 *   nothing is painted).
 * Limits: counts up to 0x7fffff00; voxel_size positive and finite and origin finite wherever they are
 * used (bounds takes any finite voxel_size).
 * Waits: from_points and merge wait twice (the key extents that size the sort, the count); carve,
 * bounds, select_by_index and an indexed paint once; an unsorted query twice; dense, a sorted query and a
 * uniform paint only enqueue. */
#define MI_ICP_VOXELGRID_AVERAGE 0
#define MI_ICP_VOXELGRID_KEEP_FIRST 1
MI_ICP_API int mi_icp_voxelgrid_from_points(mi_icp_ctx* ctx, const float* xyz, const float* colors, int64_t n,
                                            float voxel_size, const float* min_bound3, const float* max_bound3,
                                            int32_t* out_keys, float* out_colors, int64_t capacity, int64_t* m);
MI_ICP_API int mi_icp_voxelgrid_dense(mi_icp_ctx* ctx, int num_w, int num_h, int num_d, int32_t* out_keys,
                                      float* out_colors, int64_t capacity, int64_t* m);
MI_ICP_API int mi_icp_voxelgrid_merge(mi_icp_ctx* ctx, const int32_t* keys_a, const float* colors_a, int64_t m_a,
                                      const int32_t* keys_b, const float* colors_b, int64_t m_b, int mode,
                                      int32_t* out_keys, float* out_colors, int64_t capacity, int64_t* m);
MI_ICP_API int mi_icp_voxelgrid_carve(mi_icp_ctx* ctx, const int32_t* keys, const float* colors, int64_t m,
                                      float voxel_size, const float* origin3, const void* image, int width, int height,
                                      int channels, int bytes_per_channel, const float* intrinsic4,
                                      const float* extrinsic16, int keep_voxels_outside_image, int32_t* out_keys,
                                      float* out_colors, int64_t* m_out);
MI_ICP_API int mi_icp_voxelgrid_query(mi_icp_ctx* ctx, const int32_t* keys, int64_t m, int keys_sorted,
                                      float voxel_size, const float* origin3, const float* queries, int64_t nq,
                                      uint8_t* out_included, int32_t* out_index);
MI_ICP_API int mi_icp_voxelgrid_bounds(mi_icp_ctx* ctx, const int32_t* keys, int64_t m, float voxel_size,
                                       const float* origin3, int32_t* out_min_index3, int32_t* out_max_index3,
                                       double* out_center_sum3);
MI_ICP_API int mi_icp_voxelgrid_select_by_index(mi_icp_ctx* ctx, const int32_t* keys, const float* colors, int64_t m,
                                                const int64_t* indices, int64_t n_indices, int invert,
                                                int32_t* out_keys, float* out_colors, int64_t* m_out);
MI_ICP_API int mi_icp_voxelgrid_paint(mi_icp_ctx* ctx, float* colors, int64_t m, const int64_t* indices,
                                      int64_t n_indices, const float* color3);

/* ---- geometry::DistanceTransform (geometry/distancetransform.{h,cu}, distancetransform_factory.cu) ----
 * The exact Euclidean distance transform of a set of SITES (obstacle cells) in a dense cube of
 * resolution^3 cells of side voxel_size around origin; linear index (x*res + y)*res + z; h = res / 2
 * (integer).  A transform belongs to the context that made it: destroyed with mi_icp_dt_destroy, or with
 * the context.  Stored as one 32-bit word per cell -- the nearest site's three 10-bit coordinates and two
 * state bits, hence the cap of 1024 -- in two planes: 8 bytes per cell, 8 GiB at 1024^3, 1 GiB at 512^3
 * (the reference keeps a 12-byte record and a buffer of the same size beside it).  Not built: the
 * planning and visualisation consumers of a transform; the collision family (below) takes grids, not transforms.
 *
 * ARRAYS ARE DEVICE POINTERS; there is no memory-kind argument in this family (the preamble's
 * exception).  voxel_size, the origins, the threshold and the counts are host memory or values.
 * voxel_size and origin travel with every call that reads them (the reference's public members are read
 * when a call is made); only the resolution is the transform's own.
 *
 * CONTRACT.
 *  compute_*: every cell gets a NEAREST SITE: a site whose integer squared distance d2 = dx^2 + dy^2 +
 *   dz^2 to the cell is the minimum over all sites -- exact, at every resolution (the one test that
 *   decides between three sites is done in 64-bit integers).  Which of several equidistant sites is
 *   reported is a pure function of the site SET: the same set in any order, with any duplicates, gives
 *   the same bytes.  With no site every cell has no nearest site.  EVERY compute REPLACES the site set.
 *   The cell's distance is sqrtf((float)d2) * voxel_size in fp32 (d2 <= 3 * 1023^2 is exact in fp32; the
 *   square root is correctly rounded; the product is not fused), +inf without a site.  Only the nearest
 *   index is stored; the distance is derived, with the voxel_size given, when it is read.
 *  compute_cells(cells int32[n][3])  ComputeEDT(device_vector<Vector3i>): grid indices.  A cell outside
 *   [0, res)^3 on any axis is dropped (the reference writes out of bounds); *dropped (optional) is their
 *   number, and asking for it costs the call its one wait.  Duplicates are fine.  n == 0: no sites.
 *  compute_voxelgrid(keys int32[m][3], grid_voxel_size, grid_origin)  ComputeEDT(VoxelGrid): the cell of a
 *   key is, in fp32 and in this order, floor((((float)key * voxel_size + grid_origin) - origin) /
 *   voxel_size) + h per axis (compute_obstacle_cells_functor; floor(.) to int holds the value inside
 *   +-1e9 first), dropped like the cells above.  |voxel_size - grid_voxel_size| > FLT_EPSILON:
 *   MI_ICP_ERR_INVALID, nothing changed.
 *  compute_occgrid(grid, occ_prob_thres_log)  CreateFromOccupancyGrid: the sites are exactly the voxels
 *   mi_icp_occgrid_extract(MI_ICP_OCCGRID_OCCUPIED) lists -- inside the grid's bounds box, p >
 *   occ_prob_thres_log -- read from the log-odds plane on the device.  The grid must be of this context
 *   and of the same resolution, else MI_ICP_ERR_INVALID, nothing changed.
 *  query(queries float[n][3]): the cell of a point is floor((q - origin) / voxel_size) + h per axis
 *   (DenseGrid::GetVoxelIndex; the reference's GetDistance uses another formula and reads out of bounds
 *   outside the grid).  out_distance[i] is the cell's distance; out_nearest (optional) int32[n][3] its
 *   nearest site, (-1, -1, -1) when there is none.  A point outside the grid on any axis (or not finite)
 *   gives NaN and (-1, -1, -1).
 *  get_voxels: the whole plane: out_nearest int32[res^3][3] and / or out_distance float[res^3].
 *  reconstruct: a new resolution, no sites.
 * Limits: 2 <= resolution <= MI_ICP_DT_MAX_RESOLUTION, any value in that range; voxel_size positive and
 * finite and origin finite wherever they are read; counts up to 0x7fffff00.  Else MI_ICP_ERR_INVALID and
 * nothing changes.  A plane that cannot be allocated is MI_ICP_ERR_HIP, not a crash (a failed
 * reconstruct leaves no handle, as mi_icp_occgrid_reconstruct).
 * Waits: compute_cells / compute_voxelgrid once when `dropped` is asked for, else none; get_voxels waits;
 * the others only enqueue. */
#define MI_ICP_DT_MAX_RESOLUTION 1024
typedef struct mi_icp_dt mi_icp_dt;
MI_ICP_API int mi_icp_dt_create(mi_icp_ctx* ctx, int resolution, mi_icp_dt** out);
MI_ICP_API int mi_icp_dt_destroy(mi_icp_ctx* ctx, mi_icp_dt* dt);
MI_ICP_API int mi_icp_dt_reconstruct(mi_icp_ctx* ctx, mi_icp_dt* dt, int resolution);
MI_ICP_API int mi_icp_dt_compute_cells(mi_icp_ctx* ctx, mi_icp_dt* dt, const int32_t* cells, int64_t n,
                                       int64_t* dropped);
MI_ICP_API int mi_icp_dt_compute_voxelgrid(mi_icp_ctx* ctx, mi_icp_dt* dt, float voxel_size, const float* origin3,
                                           const int32_t* keys, int64_t m, float grid_voxel_size,
                                           const float* grid_origin3, int64_t* dropped);
MI_ICP_API int mi_icp_dt_compute_occgrid(mi_icp_ctx* ctx, mi_icp_dt* dt, const mi_icp_occgrid* grid,
                                         float occ_prob_thres_log);
MI_ICP_API int mi_icp_dt_query(mi_icp_ctx* ctx, mi_icp_dt* dt, float voxel_size, const float* origin3,
                               const float* queries, int64_t n, float* out_distance, int32_t* out_nearest);
MI_ICP_API int mi_icp_dt_get_voxels(mi_icp_ctx* ctx, mi_icp_dt* dt, float voxel_size, int32_t* out_nearest,
                                    float* out_distance);

/* ---- collision (collision/{collision,primitives}.{h,cu}) ------------------------------------------------
 * ComputeIntersection between a grid (geometry::VoxelGrid keys, or an OccupancyGrid of this context) and
 * another grid, a LineSet or an array of primitives, and CreateVoxelGrid of one primitive.  The reference
 * walks an LBVH over the target with a per-thread buffer of 10,000 hits; here the target is addressed
 * directly -- a binary search in the ascending keys, or the dense log-odds plane -- so the structure is "the
 * cells near the query".  Not built: Primitives x Primitives (declared, never defined in the reference),
 * CreateVoxelGridWithSweeping, CreateTriangleMesh, Mesh primitives, a DistanceTransform as a target, and the
 * kinematics module that calls these (planning is built: the graph family below).
 *
 * ARRAYS ARE DEVICE POINTERS (keys, points, lines, primitive records, out_pairs, out_keys, out_colors); the
 * side structs, the one primitive of voxelize_primitive, margin, counts are host memory.
 *
 * NUMERIC CONTRACT.  fp32 in exactly the order written; products are never fused.  tests/collision_exact.py
 * restates it in numpy, csrc/collision_predicates.h is the code.
 *  CELL BOX.  A VoxelGrid voxel with key k: lo = (float)k * vs + origin, hi = (float)(k + 1) * vs + origin
 *   per axis.  An OccupancyGrid voxel with index g: the same with k = g - h, h = resolution / 2 -- the
 *   position the grid's own extract and query use, everywhere (the reference uses the shifted origin for
 *   its tree and the unshifted one for its exact tests).  Centre c = (lo + hi) * 0.5f, half extent e = hi -
 *   c.  A margin inflates a cell to lo - margin, hi + margin; against a box primitive it is added to e,
 *   against a sphere or capsule to the radius.  An occupancy grid's voxels are those
 *   mi_icp_occgrid_extract(MI_ICP_OCCGRID_OCCUPIED) lists; their index in a pair is (x*res + y)*res + z.
 *  PREDICATES, all closed (touching counts).
 *   cell-cell: per axis a.lo <= b.hi && b.lo <= a.hi, the ENUMERATED side's cell inflated.  Two grids on
 *    one lattice collide on all 26 neighbours at margin 0 (lbvh::intersects does the same).
 *   segment-cell: LineSegmentAABB (intersection_test.inl:93-118) on the inflated cell: center = (lo + hi)
 *    * 0.5f, ext = hi - center, mid = (p0 + p1) * 0.5f, dst = p1 - mid, mid -= center; reject if |mid_i| >
 *    ext_i + |dst_i|; |dst| += FLT_EPSILON; reject on the cross axes (1,2), (2,0), (0,1):
 *    |mid_a*dst_b - mid_b*dst_a| > ext_a*|dst|_b + ext_b*|dst|_a.
 *   sphere-cell: e_i = max(max(lo_i - q_i, q_i - hi_i), 0), d2 = (e0*e0 + e1*e1) + e2*e2, hit iff d2 <=
 *    (radius + margin)^2 with the sum squared as one product; q is the transform's translation.
 *   box-cell: fifteen separating axes.  R[i][j] = rot[j][i] (the box's axes are the columns of its
 *    rotation), dc = c_cell - translation, t_i = (R[i][0]*dc0 + R[i][1]*dc1) + R[i][2]*dc2 (the reference
 *    multiplies by rot, right only for symmetric rotations); A = |R| + FLT_EPSILON, ea = lengths * 0.5f,
 *    eb = e + margin; reject if |t_i| > ea_i + ((eb0*A[i][0] + eb1*A[i][1]) + eb2*A[i][2]); reject if
 *    |(t0*R[0][j] + t1*R[1][j]) + t2*R[2][j]| > ((ea0*A[0][j] + ea1*A[1][j]) + ea2*A[2][j]) + eb_j; for
 *    i, j row-major, i1 = (i+1)%3, i2 = (i+2)%3, j1, j2 likewise, reject if |t[i2]*R[i1][j] -
 *    t[i1]*R[i2][j]| > (ea[i1]*A[i2][j] + ea[i2]*A[i1][j]) + (eb[j1]*A[i][j2] + eb[j2]*A[i][j1]).
 *    A box with finite fields whose rotation is not orthonormal within 1e-4 (max |rot^T rot - I|, columns
 *    dotted (x*x + y*y) + z*z), e.g. a scaled transform, is MI_ICP_ERR_INVALID with nothing written, in
 *    compute and in voxelize_primitive: the candidate cells below are bounded for such rotations only.
 *   capsule-cell: z = the rotation's third column, p = translation - (0.5f*height)*z, d = height*z; hit
 *    iff min over 34 parameters t of the sphere rule's d2 at q = p + t*d is <= (radius + margin)^2.  Each
 *    t is clamped to [0, 1], a t that is not finite counts as 0.  In order: 0; 1; (b_a - p_a) / d_a for a
 *    = 0..2, b = lo then hi; then for the 26 non-empty choices per axis of {inactive, lo, hi},
 *    lexicographic with axis 0 most significant, t = -(sum_a d_a*(p_a - b_a)) / (sum_a d_a*d_a) over the
 *    active axes, both sums from 0 in axis order.  (CapsuleAABB of the reference returns true for every
 *    corner case; not restated.)
 *   NEVER COLLIDING: Cylinder, Mesh and Unspecified primitives (as in the reference); a primitive with a
 *    field that is not finite; a line with an end point that is not finite.  A line whose point index is
 *    outside [0, n_points) is MI_ICP_ERR_INVALID with nothing written.  margin must be finite and >= 0.
 *  RESULT.  pairs int32[m][2], column 0 indexes A, column 1 indexes B (the reference swaps the columns of
 *   its Primitives-first overloads).  One side is ENUMERATED: the lines whenever a LineSet is either
 *   argument, else B.  Every enumerated element that collides gives exactly one pair; the other column is
 *   the SMALLEST index of the other side the predicate accepts (the reference: whichever its tree walk met
 *   first).  Pairs ascend in the enumerated index.  THE CAPACITY RULE: *m is the count; with capacity <
 *   *m nothing is written.  An empty side: m = 0 without a launch.
 *   Pairs built: VoxelGrid x VoxelGrid; VoxelGrid x OccupancyGrid and the reverse; {VoxelGrid,
 *   OccupancyGrid} x LineSet and the reverse; {VoxelGrid, OccupancyGrid} x Primitives and the reverse.
 *   Every other pair of kinds is MI_ICP_ERR_INVALID.  A VoxelGrid side with keys_sorted == 0 that is NOT
 *   enumerated is sorted once into scratch with its permutation (equal keys: the smallest index stands);
 *   with keys_index the caller passes such a sorted copy and the pairs name keys_index[i].
 *  CANDIDATE CELLS.  For an enumerated voxel the other grid's cells that meet its inflated box are found
 *   EXACTLY: lo and hi above are non-decreasing in k, so the keys with b.hi >= a.lo are all keys from some
 *   key on, those with b.lo <= a.hi all keys up to some key, and a binary search finds both ends: no slack.
 *   For a line or primitive the cells are those that meet its bounds (margin included) widened by
 *   s = 1e-5 * M + 1e-30, M the largest magnitude of a bound: the predicates' axis tests are that overlap
 *   in fp32 through at most a dozen roundings, below 2e-6 * M.  A box primitive's half widths get a further
 *   1e-3 of the largest of them and of the cell size, for the rotation's tolerance.  A line is taken one
 *   x-slab at a time: the parameter interval in which it is inside the slab (widened by 8 * FLT_EPSILON *
 *   (|x0| + |x_slab| + |dx|) / |dx|, the whole line when that is not finite) bounds its y and z there.
 *   Because segment-cell adds FLT_EPSILON to |dst| before its cross-axis tests, the line may pass an
 *   accepted cell at FLT_EPSILON * (ext_0 + ext_a) / |dst_0|; that span is therefore widened by 4 *
 *   FLT_EPSILON * (vs + 2 margin) / |dx| (twice the bound) and, for the products' rounding, by 16 *
 *   FLT_EPSILON * ((vs + 2 margin) * |d_a| / |dx| + |d_a| + vs + 2 margin); a segment with |dx| <= 1e-5 *
 *   (|x0| + |x1|) takes its whole y / z range; the result is cut to the segment's whole bounds, which the
 *   three opening rejects enforce (csrc/collision_predicates.h, segment_slab_cells).
 *   Ranges are clamped to the occupancy grid's bounds box or to the VoxelGrid's key extents; a searched
 *   key whose x is INT32_MIN is no key.  k + 1 and the like are computed in 64 bits.
 *  voxelize_primitive(primitive, voxel_size)  CreateVoxelGrid (primitives.cu:238-265).  origin = the
 *   translation (*out_origin3).  [mn, mx] = GetAxisAlignedBoundingBox; per axis min_b = (mn - origin) -
 *   vs*0.5f, max_b = (mx - origin) + vs*0.5f, num = (int)roundf((max_b - min_b) / vs).  idx -> (w, h, d) =
 *   (idx/(nh*nd) - nw/2, (idx%(nh*nd))/nd - nh/2, idx%nd - nd/2); the cell is kept iff the primitive with
 *   its translation set to zero collides with the cell box of key (w, h, d) at origin 0, margin 0.  Keys
 *   ascend; colours (1, 1, 1).  Refused: voxel_size <= 0 or not finite, a type other than Box, Sphere,
 *   Capsule, a field that is not finite, a box's rotation that is not orthonormal, more than 2^31 - 1 cells.
 *  GetAxisAlignedBoundingBox (host, mi_icp_primitive_aabb): Box translation -+ |rot| * (lengths * 0.5f),
 *   row sums left to right (the reference takes |rot * half|, a bound for axis-aligned boxes only);
 *   Sphere -+ radius; Capsule pa = z * (0.5f*height), (min(pa, -pa) - radius) + translation and (max(pa,
 *   -pa) + radius) + translation; Cylinder the reference's formula with max in the max bound (it writes
 *   min); other types zeros.
 * Waits: compute waits once for the count (twice more when it sorts a VoxelGrid, once more when it lists an
 * occupancy grid, once more to check a LineSet's indices or a primitive array's boxes); voxelize_primitive
 * once; sort_keys twice. */
#define MI_ICP_PRIMITIVE_UNSPECIFIED 0
#define MI_ICP_PRIMITIVE_BOX 1
#define MI_ICP_PRIMITIVE_SPHERE 2
#define MI_ICP_PRIMITIVE_CAPSULE 3
#define MI_ICP_PRIMITIVE_CYLINDER 4
#define MI_ICP_PRIMITIVE_MESH 5
typedef struct mi_icp_primitive { /* 80 bytes */
    int32_t type;
    float transform[16]; /* column-major, as extrinsic16 is */
    float param[3];      /* Box: lengths; Sphere: radius; Capsule, Cylinder: radius, height */
} mi_icp_primitive;
#define MI_ICP_COLLISION_VOXELGRID 1
#define MI_ICP_COLLISION_OCCGRID 2
#define MI_ICP_COLLISION_LINESET 3
#define MI_ICP_COLLISION_PRIMITIVES 4
typedef struct mi_icp_collision_side {
    int32_t kind;        /* MI_ICP_COLLISION_*: which of the groups below is read */
    int32_t keys_sorted; /* VOXELGRID: keys ascend and are distinct */
    const int32_t* keys; /* VOXELGRID: int32[m][3] */
    const int32_t* keys_index; /* NULL, or with keys_sorted: the index reported for keys[i] (mi_icp_collision_sort_keys) */
    int64_t m;
    float voxel_size;    /* VOXELGRID */
    float origin[3];
    const mi_icp_occgrid* grid;        /* OCCGRID */
    mi_icp_occgrid_params grid_params; /* (voxel_size, origin and occ_prob_thres_log are read) */
    const float* points;  /* LINESET: float[n_points][3] */
    int64_t n_points;
    const int32_t* lines; /* int32[n_lines][2] */
    int64_t n_lines;
    const mi_icp_primitive* primitives; /* PRIMITIVES: [n_primitives] */
    int64_t n_primitives;
} mi_icp_collision_side;
MI_ICP_API int mi_icp_collision_compute(mi_icp_ctx* ctx, const mi_icp_collision_side* a, const mi_icp_collision_side* b,
                                        float margin, int32_t* out_pairs, int64_t capacity, int64_t* m);
MI_ICP_API int mi_icp_collision_voxelize_primitive(mi_icp_ctx* ctx, const mi_icp_primitive* primitive, float voxel_size,
                                                   int32_t* out_keys, float* out_colors, int64_t capacity, int64_t* m,
                                                   float* out_origin3);
/* The distinct keys of keys[m], ascending, and for each the smallest index it has in keys: what compute makes of a
 * searched VoxelGrid side with keys_sorted == 0, for a caller that asks many queries of one grid.  out arrays of m
 * entries; waits twice. */
MI_ICP_API int mi_icp_collision_sort_keys(mi_icp_ctx* ctx, const int32_t* keys, int64_t m, int32_t* out_keys,
                                          int32_t* out_index, int64_t* m_out);
MI_ICP_API int mi_icp_primitive_aabb(const mi_icp_primitive* primitive, float* out_min3, float* out_max3);

/* ---- graph (geometry/graph.{h,cu}, graph_factory.cu; the search planning::Pos3DPlanner runs) ---------------
 * geometry::Graph<3>: a LineSet<3> whose lines[m][2] are directed edges sorted ascending by (first, second),
 * with edge_index_offsets[n_points + 1] (the edges of node v are offsets[v] .. offsets[v + 1]) and one weight
 * per edge.  An undirected graph stores both directions of every edge.  Not built: Graph<2> (there is no
 * LineSet<2>), CreateFromTriangleMesh, visualisation, file I/O, and the kinematics module.
 *
 * ARRAYS ARE DEVICE POINTERS (points, lines, weights, colours, offsets, the listed edges, out_dist, out_prev);
 * counts, scalars, min3 / max3 / resolutions3 / point3 and info5 are host memory.  THE CAPACITY RULE of the
 * collision family holds for lattice: the counts are always written, and with too little room nothing else.
 *
 * NUMERIC CONTRACT.  fp32 in exactly the order written; products are never fused; sqrtf correctly rounded.
 * tests/graph_exact.py restates it in numpy; csrc/graph_rules.h holds what host and device share.
 *  construct(lines, weights, colors, m, n_points, out_offsets)  ConstructGraph.  Sorts the lines IN PLACE,
 *   stably: equal lines keep their input order.  weights[m] and colors[m][3] (each may be NULL) travel with
 *   their lines.  out_offsets[v] = the number of lines whose first index is below v.  A line with an index
 *   outside [0, n_points) is MI_ICP_ERR_INVALID with nothing written.  The sort is the library's radix sort
 *   (csrc/primitives.h) on the key first << b | second, b the bits of n_points - 1.
 *  weights_from_distance  SetEdgeWeightsFromDistance: with d = points[first] - points[second] per axis,
 *   w = sqrtf((dx*dx + dy*dy) + dz*dz).  An index out of range: MI_ICP_ERR_INVALID (other lines are written).
 *  node_distances(points, n, point3, out)  the same formula with d = points[i] - point3: what
 *   AddNodeAndConnect compares with max_edge_distance (strictly below) and stores as the weight.
 *  lattice(min3, max3, resolutions3, ...)  CreateFromAxisAlignedBoundingBox.  steps = (max - min) /
 *   (float)resolution per axis (the reference's formula: the last node is one step short of max); node
 *   (x*ry + y)*rz + z is min + (float)(x, y, z) * steps; every node has an edge to each of its up to 26
 *   neighbours inside the lattice, written directly at their place in ascending (i, j) order with offsets and
 *   distance weights: the count, (3rx-2)(3ry-2)(3rz-2) - rx*ry*rz, and every node's first edge are closed
 *   forms (graph_rules.h), so there is no sort and no compaction.  Refused: a resolution < 1, more than
 *   0x7fffff00 nodes or 2^31 - 1 edges.
 *  set_edge_weights(lines, weights, m, edges, k, is_directed, weight)  SetEdgeWeights: every line equal to a
 *   listed edge gets `weight`; with is_directed == 0 every line equal to the reverse of a listed edge too.
 *   The lines must be sorted (construct).  Each listed edge (and its reverse) finds the run of its lines by a
 *   binary search in the lines -- k log m steps and no sort of the list, against m log k and a sort the other
 *   way round.  A listed edge that is no line changes nothing.
 *  remove_edges(lines, weights, colors, m, n_points, edges, k, is_directed, out_offsets, m_out)  RemoveEdges:
 *   the same matching; the lines that stay are compacted IN PLACE in their order (flags, the scan, one gather:
 *   csrc/select.h's scheme), weights and colours with them, and the offsets rewritten.  *m_out = their count.
 *  sssp(offsets, lines, weights, n, m, start, end, out_dist, out_prev, info5)  DijkstraPaths.
 *   Weights are >= 0 or +inf; a negative or NaN weight is MI_ICP_ERR_INVALID, checked once on the device
 *   before any relaxation, as are the lines' indices and the offsets' ranges.
 *   DISTANCES.  dist[start] = 0, else dist[v] = min over edges (u, v) of (float)(dist[u] + w(u, v)), the
 *   least such assignment; +inf where there is no path.  With such weights the fixed point is unique --
 *   label-setting Dijkstra and Bellman-Ford in any edge order reach the same bits -- so the relaxation order
 *   is free and the result is bit-identical on every run.  An edge of weight +inf relaxes nothing.
 *   PREDECESSORS.  prev[start] = start; prev[v] = -1 where dist[v] is +inf; else
 *    tier 1: the SMALLEST u with an edge (u, v), dist[u] < dist[v] and (float)(dist[u] + w) == dist[v];
 *    tier 2, for the nodes tier 1 leaves (reached only through edges that add nothing in fp32), in rounds
 *    until none is left: every unresolved v takes the smallest u RESOLVED BEFORE THE ROUND with an edge
 *    (u, v), dist[u] == dist[v] and (float)(dist[u] + w) == dist[v].  (The plain "smallest tight u" lets two
 *    nodes joined by a zero-weight edge name each other.)
 *   EARLY END.  With end >= 0 the search stops once no open node has a tentative distance <= dist[end].  The
 *   result equals the end = -1 result at every node whose distance is <= dist[end]; every other entry is
 *   (+inf, -1).  An unreachable end gives the full result.
 *   REGIMES, chosen from n and m alone (mi_icp_graph_sssp_limits).  SMALL, n <= 8192 and m <= 262144: one
 *   workgroup keeps distance, predecessor, candidate and two open flags per node in LDS (14 bytes: 112 of
 *   the CU's 160 KiB; twice the nodes would not fit) and streams the edges (12 bytes each: 3 MiB, inside
 *   one XCD's 4 MiB L2) round after round to the end, predecessors included, in ONE launch.  LARGE: frontier
 *   rounds over the whole device, node-parallel over byte flags, launched in batches of 32; a round whose
 *   frontier is empty returns at once; the host reads one counter per batch.
 *   info5 (host, may be NULL): regime (0 small, 1 large), launches, host waits, relaxation rounds that did
 *   work, tier-2 rounds that resolved a node.
 * Waits: construct once (the index check, behind the sort); weights_from_distance once; node_distances,
 * lattice and set_edge_weights never; remove_edges once (the count); sssp once in the small regime, in the
 * large one once for the checks, once per batch of rounds and once per predecessor pass (one without tier 2). */
MI_ICP_API int mi_icp_graph_construct(mi_icp_ctx* ctx, int32_t* lines, float* weights, float* colors, int64_t m,
                                      int64_t n_points, int32_t* out_offsets);
MI_ICP_API int mi_icp_graph_weights_from_distance(mi_icp_ctx* ctx, const float* points, int64_t n_points,
                                                  const int32_t* lines, int64_t m, float* out_weights);
MI_ICP_API int mi_icp_graph_node_distances(mi_icp_ctx* ctx, const float* points, int64_t n_points, const float* point3,
                                           float* out_distances);
MI_ICP_API int mi_icp_graph_lattice(mi_icp_ctx* ctx, const float* min3, const float* max3, const int32_t* resolutions3,
                                    float* out_points, int64_t point_capacity, int32_t* out_lines, float* out_weights,
                                    int64_t edge_capacity, int32_t* out_offsets, int64_t* n_points, int64_t* m);
MI_ICP_API int mi_icp_graph_set_edge_weights(mi_icp_ctx* ctx, const int32_t* lines, float* weights, int64_t m,
                                             const int32_t* edges, int64_t k, int is_directed, float weight);
MI_ICP_API int mi_icp_graph_remove_edges(mi_icp_ctx* ctx, int32_t* lines, float* weights, float* colors, int64_t m,
                                         int64_t n_points, const int32_t* edges, int64_t k, int is_directed,
                                         int32_t* out_offsets, int64_t* m_out);
MI_ICP_API int mi_icp_graph_sssp(mi_icp_ctx* ctx, const int32_t* offsets, const int32_t* lines, const float* weights,
                                 int64_t n, int64_t m, int64_t start, int64_t end, float* out_dist, int32_t* out_prev,
                                 int32_t* info5);
/* the small regime's largest n and m, and the rounds of a batch in the large one (no context, no device) */
MI_ICP_API int mi_icp_graph_sssp_limits(int64_t* small_max_nodes, int64_t* small_max_edges, int32_t* batch_rounds);

/* ---- laserscan (geometry/laserscanbuffer.{h,cu}, laserscanbuffer_factory.cu, PointCloud::CreateFromLaserScanBuffer) ----
 * geometry::LaserScanBuffer: a ring of planar scans.  THE STORAGE BELONGS TO THE CALLER (the C++ or Python object):
 * ranges[num_max_scans][num_steps] and the optional intensities of the same shape are DEVICE memory; the library keeps
 * no scan handle.  ORIGINS ARE HOST MEMORY: origins[num_max_scans][16], one column-major 4x4 per slot, kept by the
 * surfaces on the host and passed with each call that needs them (64 bytes per scan; Transform / Rotate / Translate
 * are host arithmetic, stated below).  Counts, scalars, intrinsic4, *m and *info are host memory too.
 * The ring: live scan k (oldest first, 0 <= k < num_scans) sits in slot (first_slot + k) % num_max_scans; the surfaces
 * keep top / bottom as the reference does (first_slot = top % num_max_scans, num_scans = bottom - top, the newest
 * scan's slot is bottom % num_max_scans; a full ring overwrites its oldest scan and advances top).
 *
 * NUMERIC CONTRACT.  fp32 in exactly the order written, products never fused, division and sqrtf correctly rounded;
 * tests/laserscan_exact.py restates it in numpy.  The reference's bin update is a read, a compare and an exchange (the
 * smaller range can lose) and it reads and writes out of bounds where noted: this is a stated contract, not a
 * transcription.
 *  to_points  PointCloud::CreateFromLaserScanBuffer.  Only LIVE scans are converted, oldest first (the reference walks
 *   raw storage, popped scans included).  num_steps >= 2, else MI_ICP_ERR_INVALID.
 *   inc = (max_angle - min_angle) / (float)(num_steps - 1); a_i = min_angle + (float)i * inc; c_i, s_i = cos, sin of
 *   (double)a_i computed ON THE HOST in double and rounded to float (a table uploaded with the call: device cosf / sinf
 *   would not be bit-reproducible).  A reading r is kept when !isnan(r) && !(r < min_range) && !(max_range < r); then
 *   x = r*c_i, y = r*s_i, p_k = (O(k,0)*x + O(k,1)*y) + O(k,3) for k = 0, 1, 2 with O the scan's origin; points with a
 *   non-finite coordinate are then removed (RemoveNoneFinitePoints(true, true)), order kept.  With intensities the
 *   colour of a point is (v, v, v).  THE CAPACITY RULE: *m is always the count; with capacity < *m nothing is written.
 *   min_range >= max_range or no live scan: *m = 0, MI_ICP_OK.  Waits once (the count).
 *  from_points  LaserScanBuffer::CreateFromPointCloud into out_ranges[num_vertical_divisions][num_steps], where the
 *   CALLER computes num_steps = (int)ceilf((max_angle - min_angle) / angle_increment) (checked).  Every bin starts as
 *   the quiet NaN 0x7fc00000.  Per point: range = sqrtf(x*x + y*y) (for hypotf: the same except where the squares
 *   overflow or underflow), angle = atan2f(y, x), height_increment = (max_height - min_height) /
 *   (float)num_vertical_divisions, j = (int)((z - min_height) / height_increment), i = (int)((angle - min_angle) /
 *   angle_increment).  Dropped: a non-finite coordinate; range < min_range || range > max_range; angle < min_angle ||
 *   angle > max_angle; z < min_height; j >= num_vertical_divisions; i >= num_steps (the last three are out-of-bounds
 *   writes in the reference).  A bin ends as the EXACT MINIMUM of its points' ranges whatever the order of arrival:
 *   ranges are >= 0, so their bit patterns order as unsigned integers with the NaN pattern above +inf's, and one
 *   unsigned atomic minimum per point is the whole reduction; every run gives the same bytes.
 *   TWO PATHS, chosen from the bin count alone (mi_icp_laserscan_limits): bins <= 18432 the LDS path -- each workgroup
 *   keeps the table in LDS (72 KiB, so two workgroups share a CU's 160 KiB), reduces a contiguous share of the points
 *   with LDS atomic minima and flushes the bins it touched with global atomic minima; otherwise atomics straight to
 *   memory.  *info (may be NULL) = 0 for the LDS path, 1 for the global one.
 *   MI_ICP_ERR_INVALID: angle_increment <= 0, min_height >= max_height, min_range >= max_range, min_angle >= max_angle,
 *   num_vertical_divisions < 1, a num_steps that is not the formula's, more than 2^26 bins.  Never waits.
 *  from_depth  LaserScanBuffer::CreateFromDepthImage, one fused kernel from depth pixel to bin, no cloud in between.
 *   Pixel selection, stride, the U16 depth_scale / depth_trunc rule and depth <= 0 are exactly those of
 *   mi_icp_create_from_depth (rgbd = 0).  Camera point x = ((float)col - cx) * z / fx, y = ((float)row - cy) * z / fy;
 *   scan-frame point (x, -z, y): the inverse of the EXACT quarter turn about X with rows (1,0,0), (0,0,1), (0,-1,0)
 *   (the reference builds it from AngleAxisf(-M_PI_2, UnitX), which is not exact in float).  Then binned as above with
 *   min_y / max_y in the place of the heights.
 *  range_filter  out = (r < min_range || r > max_range) ? NaN : r over `count` readings (out may be ranges itself).
 *  shadow_filter  ScanShadowsFilter over num_rows scans of num_steps readings.  Host: min_tan = |(float)tan((double)
 *   min_angle)|, max_tan = -|(float)tan((double)max_angle)|, inc as in to_points from scan_min_angle / scan_max_angle,
 *   and a table c_y, s_y = cos, sin of (double)((float)y * inc) for y in [-window, window].  Reading (n, i) is a shadow
 *   start when for some j = i + y with 0 <= j < num_steps, j != i: py = r_j * s_y, px = r_i - r_j * c_y,
 *   t = fabsf(py) / px and (t > 0) ? (t < min_tan) : (t > max_tan).  Then out[n][index] = NaN for every index in
 *   [max(i - neighbors, 0), min(i + neighbors, num_steps - 1)] with r[n][i] < r[n][index] (the reference compares
 *   inside scan 0), and out[n][i] = NaN if remove_shadow_start_point.  Reads come from `ranges`, writes go to
 *   out_ranges, which starts as a copy (it must be another buffer): the result does not depend on order.  Waits once.
 *  scale  LaserScanBuffer::Scale: r = r * scale over `count` readings, in place.
 * The origins' arithmetic, which the surfaces do on the host: Transform O <- O*T, every element ((a0*b0 + a1*b1) +
 * a2*b2) + a3*b3; Rotate the 3x3 block times R, ((a0*b0 + a1*b1) + a2*b2); Translate adds to column 3.  The
 * factories' origins: identity with O(2,3) = min_height + ((max_height - min_height) * (float)i) /
 * (float)num_vertical_divisions for slot i; from_depth multiplies each on the left by the exact quarter turn. */
MI_ICP_API int mi_icp_laserscan_to_points(mi_icp_ctx* ctx, const float* ranges, const float* intensities,
                                          const float* origins, int32_t num_steps, int32_t num_max_scans, int32_t first_slot,
                                          int32_t num_scans, float min_angle, float max_angle, float min_range,
                                          float max_range, float* out_xyz, float* out_colors, int64_t capacity, int64_t* m);
MI_ICP_API int mi_icp_laserscan_from_points(mi_icp_ctx* ctx, const float* points, int64_t n, float angle_increment,
                                            float min_height, float max_height, int32_t num_vertical_divisions,
                                            float min_range, float max_range, float min_angle, float max_angle,
                                            int32_t num_steps, float* out_ranges, int32_t* info);
MI_ICP_API int mi_icp_laserscan_from_depth(mi_icp_ctx* ctx, const void* depth, int depth_type, int width, int height,
                                           const float* intrinsic4, float depth_scale, float depth_trunc, int stride,
                                           float angle_increment, float min_y, float max_y, int32_t num_vertical_divisions,
                                           float min_range, float max_range, float min_angle, float max_angle,
                                           int32_t num_steps, float* out_ranges, int32_t* info);
MI_ICP_API int mi_icp_laserscan_range_filter(mi_icp_ctx* ctx, const float* ranges, int64_t count, float min_range,
                                             float max_range, float* out_ranges);
MI_ICP_API int mi_icp_laserscan_shadow_filter(mi_icp_ctx* ctx, const float* ranges, int32_t num_steps, int32_t num_rows,
                                              float scan_min_angle, float scan_max_angle, float min_angle, float max_angle,
                                              int32_t window, int32_t neighbors, int remove_shadow_start_point,
                                              float* out_ranges);
MI_ICP_API int mi_icp_laserscan_scale(mi_icp_ctx* ctx, float* ranges, int64_t count, float scale);
/* the LDS path's largest bin count and the largest bin count taken at all (no context, no device) */
MI_ICP_API int mi_icp_laserscan_limits(int64_t* lds_max_bins, int64_t* max_bins);

/* ---- image (geometry/image.{h,cu}, image_factory.cu, rgbdimage.{h,cu}, rgbdimage_factory.cu) ----
 * Image processing in front of everything that takes an image: filters, pyramids, the bilateral filter and the
 * conversions between pixel formats.  An image is [height][width][channels] elements of bytes_per_channel bytes, row
 * after row, in DEVICE memory (no mem_kind: a surface stages host pixels itself); filter taps and the spatial table are
 * small HOST arrays that travel with the launch.  width and height are at most MI_ICP_TSDF_MAX_IMAGE_SIDE (else
 * MI_ICP_ERR_INVALID); a width or height of 0 launches nothing and is MI_ICP_OK.  Outputs are other buffers than inputs
 * (else MI_ICP_ERR_INVALID) except where "in place" is said.  No call waits for the stream.  All arithmetic is fp32,
 * in the order written, unfused EXCEPT where fmaf is written (tests/image_exact.py restates it in numpy); clamp(v, hi) =
 * min(max(0, v), hi).  fmaf(a, b, c) is the exact a * b + c rounded once.  It stands where the reference's own test
 * vectors pin it: src/tests/geometry/image.cpp compares BYTES, the reference is built with nvcc's multiply-add
 * contraction and --use_fast_math, and its bytes are those of the fused forms below, not of the source read literally
 * (tests/golden/reference_tests.json records the vectors; tests/test_reference_vectors_cpu.py and
 * tests/test_gpu_reference_vectors.py replay them).
 *  filter  Image::FilterHorizontal / Image::Filter(dx, dy) on 1 x float32, nx and ny odd, at most
 *   MI_ICP_IMAGE_MAX_TAPS (else MI_ICP_ERR_INVALID), hx = nx / 2, hy = ny / 2:
 *     rowsum(y, x) = t, where t = 0 and then, for i = -hx .. hx, t = fmaf(src[y][clamp(x + i, w - 1)], dx[i + hx], t);
 *     dy == NULL (ny = 0): out[y][x] = rowsum(y, x) -- FilterHorizontal;
 *     else out[y][x] = o, where o = 0 and then, for j = -hy .. hy, o = fmaf(rowsum(clamp(y + j, h - 1), x), dy[j + hy], o)
 *   -- the words of the reference's horizontal(dx), transpose, horizontal(dy), transpose, in ONE kernel with no
 *   intermediate image.  The fused tap (image.cu:201) is pinned by TEST(Image, Filter_Gaussian5) and Filter_Gaussian7,
 *   whose bytes the unfused sum misses in 3 and 4 of 25 words; taps that are powers of two (Gaussian3, the Sobels) have
 *   exact products and give the same words either way.  The named filters: Gaussian3 {.25, .5, .25}, Gaussian5 {.0625, .25, .375, .25, .0625}, Gaussian7
 *   {.03125, .109375, .21875, .28125, .21875, .109375, .03125} in both directions; Sobel3Dx dx = {-1, 0, 1}, dy =
 *   {1, 2, 1}; Sobel3Dy the other way round.
 *  downsample  Image::Downsample into (w / 2) x (h / 2): 1 x float32 (((p00 + p01) + p10) + p11) / 4.0f over the 2 x 2
 *   block (p01 to the right, p10 below); 3 x uint8 per channel the integer (p00 + p01 + p10 + p11) / 4.  Other formats
 *   MI_ICP_ERR_INVALID.
 *  pyramid_level  one level of Image::CreatePyramid with the Gaussian, 1 x float32: the words of downsample(filter(
 *   Gaussian3)), in one kernel that writes the quarter-size image only.
 *  bilateral_table  (host arithmetic, no context) table[i] = (float)exp((double)(-(x * x) / (2 * sigma2))) for i = 0 ..
 *   2 * diameter, x = (float)(i - diameter), sigma2 = sigma_space * sigma_space, the argument in fp32.
 *  bilateral  Image::BilateralFilter on 1 x float32; `diameter` is a RADIUS in [0, MI_ICP_IMAGE_MAX_DIAMETER] (else
 *   MI_ICP_ERR_INVALID), the window (2 diameter + 1)^2, table as above.  Per pixel: filtered = total = 0; for dy = -d ..
 *   d, for dx = -d .. d: cur = src[clamp(y + dy, h - 1)][clamp(x + dx, w - 1)], c = center - cur, w = (table[dy + d] *
 *   table[dx + d]) * exp(-(c * c) / ((2.0f * sigma_color) * sigma_color)), filtered = filtered + w * cur, total = total +
 *   w; out = filtered / total.  The exponential is the device's (2^x in hardware of the argument times log2(e)), so this
 *   one operation is not pinned to the bit: a result lies within (4 T + 64) 2^-24 M of the same sums carried in double,
 *   T the number of taps, M the largest |value| in the window.  (The reference clamps to h and w, one past the end.)
 *  create_float  Image::CreateFloatImage: the value of an element by bytes_per_channel (1 uint8, 2 uint16, 4 float, 3:
 *   0.0f); one channel value * denom; three channels fmaf(w2, v2, fmaf(w0, v0, w1 * v1)) * denom; any other channel
 *   count 0; weights MI_ICP_IMAGE_EQUAL (float)(1.0 / 3.0) each, MI_ICP_IMAGE_WEIGHTED {0.2990f, 0.5870f, 0.1140f}; denom
 *   = (float)(1.0 / 255.0) for one byte per channel, else 1.0f.  The order of the three-channel sum
 *   (image_factory.cu:88-105) is pinned by TEST(Image, CreateFloatImage_3_1_Weighted), _3_2_Weighted and _3_4_Weighted
 *   (the unfused sum misses 7, 7 and 2 of 25 words).  The EQUAL weights have no vector of their own -- the reference's
 *   _Equal cases call CreateFloatImage() with the default type and hold the Weighted bytes --; they take the same order
 *   because the reference compiles one expression for both weight sets.
 *  depth_to_float  Image::ConvertDepthToFloatImage: create_float (weighted), then f = f * r, r = (float)(1.0 /
 *   (double)(float)(int)depth_scale); if (f >= (float)(int)depth_trunc) f = 0 -- the reference holds both as int.
 *   |depth_scale|, |depth_trunc| < 2e9.  Under fast math the reference's `f /= (float)depth_scale_` (image.cu:345) is a
 *   product with a reciprocal; TEST(Image, ConvertDepthToFloatImage) pins it AT SCALE 1000 ONLY, where the correctly
 *   rounded reciprocal gives its bytes (the division misses 17 of 25 words, each by one ulp).  For every other scale the
 *   correctly rounded reciprocal is this library's extrapolation of fast-math division, not something a vector shows.
 *   The same rule, in one device function, serves mi_icp_create_from_depth's MI_ICP_DEPTH_U16 and LaserScanBuffer's
 *   depth entry.
 *  create_gray  Image::CreateGrayImage: the same sum with denom 1.0f (one byte per channel), (float)(255.0 / 65535.0)
 *   (two), 255.0f (else), to uint8.
 *  from_float  Image::CreateImageFromFloatImage: bytes_per_channel 1 (uint8)(f * 255.0f), 2 (uint16)f.
 *  linear_transform  Image::LinearTransform in place: 1 x float32 scale * f + offset; uint8 (any channel count up to 4)
 *   (uint8)(scale * (float)f + offset), every channel.
 *  clip  Image::ClipIntensity in place, 1 x float32: fmaxf(fminf(max, f), min) (a NaN pixel becomes max).
 *   Every float -> uint8 / uint16 conversion above truncates toward zero and SATURATES; NaN becomes 0.
 *  move  Image::Transpose (dst is `height` wide and `width` high), FlipVertical, FlipHorizontal: whole pixels of
 *   bytes_per_pixel bytes, 1 .. 16.
 *  depth_format  uint16 to uint16: MI_ICP_IMAGE_SUN d = (d >> 3) | (d << 13); MI_ICP_IMAGE_NYU swap the two bytes, xx =
 *   (float)(351.3 / (1092.5 - (double)d)), d = xx <= 0 ? 0 : (uint16)floor((double)xx * 1000 + 0.5), saturating.  src
 *   may equal dst. */
#define MI_ICP_IMAGE_MAX_TAPS 31
#define MI_ICP_IMAGE_MAX_DIAMETER 31
#define MI_ICP_IMAGE_EQUAL 0
#define MI_ICP_IMAGE_WEIGHTED 1
#define MI_ICP_IMAGE_TRANSPOSE 0
#define MI_ICP_IMAGE_FLIP_VERTICAL 1
#define MI_ICP_IMAGE_FLIP_HORIZONTAL 2
#define MI_ICP_IMAGE_SUN 0
#define MI_ICP_IMAGE_NYU 1
MI_ICP_API int mi_icp_image_filter(mi_icp_ctx* ctx, const float* src, int width, int height, const float* dx, int nx,
                                   const float* dy, int ny, float* dst);
MI_ICP_API int mi_icp_image_downsample(mi_icp_ctx* ctx, const void* src, int width, int height, int channels,
                                       int bytes_per_channel, void* dst);
MI_ICP_API int mi_icp_image_pyramid_level(mi_icp_ctx* ctx, const float* src, int width, int height, float* dst);
MI_ICP_API int mi_icp_image_bilateral_table(int diameter, float sigma_space, float* table);
MI_ICP_API int mi_icp_image_bilateral(mi_icp_ctx* ctx, const float* src, int width, int height, int diameter,
                                      float sigma_color, const float* table, float* dst);
MI_ICP_API int mi_icp_image_create_float(mi_icp_ctx* ctx, const void* src, int width, int height, int channels,
                                         int bytes_per_channel, int type, float* dst);
MI_ICP_API int mi_icp_image_depth_to_float(mi_icp_ctx* ctx, const void* src, int width, int height, int channels,
                                           int bytes_per_channel, float depth_scale, float depth_trunc, float* dst);
MI_ICP_API int mi_icp_image_create_gray(mi_icp_ctx* ctx, const void* src, int width, int height, int channels,
                                        int bytes_per_channel, int type, uint8_t* dst);
MI_ICP_API int mi_icp_image_from_float(mi_icp_ctx* ctx, const float* src, int width, int height, int bytes_per_channel,
                                       void* dst);
MI_ICP_API int mi_icp_image_linear_transform(mi_icp_ctx* ctx, void* data, int width, int height, int channels,
                                             int bytes_per_channel, float scale, float offset);
MI_ICP_API int mi_icp_image_clip(mi_icp_ctx* ctx, float* data, int width, int height, float min_value, float max_value);
MI_ICP_API int mi_icp_image_move(mi_icp_ctx* ctx, const void* src, int width, int height, int bytes_per_pixel, int op,
                                 void* dst);
MI_ICP_API int mi_icp_image_depth_format(mi_icp_ctx* ctx, const uint16_t* src, int width, int height, int format,
                                         uint16_t* dst);
/* the longest filter and the largest bilateral radius taken (no context, no device) */
MI_ICP_API int mi_icp_image_limits(int32_t* max_taps, int32_t* max_diameter);

/* ---- stereo (imageproc/sgm.{h,cpp}: imageproc::SemiGlobalMatching; pointcloud_factory.cu:432-482:
 * ---- PointCloud::CreateFromDisparity) ----
 * Semi-global matching after Hirschmueller: two rectified 8-bit images in, one 8-bit disparity image out.  The
 * reference wraps libSGM, whose sources its checkout does not hold; the contract below is this library's own, with
 * exactly the parameters of the reference's SGMOption, and tests/sgm_exact.py restates it in numpy.  Every step up to
 * the disparity image is integer arithmetic, so results are the same bytes on every run.  Images are [height][width]
 * in DEVICE memory (no mem_kind: a surface stages host pixels itself); no call here waits for the stream.
 *  mi_icp_sgm_create  a matcher for width x height frames; all of its workspace (two census planes, 4 or 8 path
 *   volumes of width * height * disp_size bytes, the two maps) is allocated here, a frame allocates nothing.  Turned
 *   away with MI_ICP_ERR_INVALID: width or height outside [1, MI_ICP_SGM_MAX_SIDE]; not 0 <= p1 <= p2 <=
 *   MI_ICP_SGM_MAX_P2 (the bound keeps every path cost within a byte); disp_size not 64, 128 or 256; path_type not
 *   MI_ICP_SGM_PATH4 / MI_ICP_SGM_PATH8; min_disp < 0 or min_disp + disp_size > 256.  MI_ICP_ERR_HIP: no memory.
 *   A matcher belongs to its context and is freed with it at the latest.
 *  mi_icp_sgm_process  left, right, dst: width * height bytes each, dst another buffer than the inputs.  With D =
 *   disp_size, H x W images, row y, column x:
 *   1 census  (mi_icp_sgm_census computes this alone) the window offsets (dy, dx), dy = -3 .. 3 outer, dx = -4 .. 4
 *     inner; bit k (bit 0 first) of the word is I(y + dy, x + dx) > I(y - dy, x - dx) for the k-th of the 31 offsets
 *     before the centre; bit 31 clear; the word is 0 where the window leaves the image (rows < 3 or >= H - 3, columns
 *     < 4 or >= W - 4).
 *   2 cost  C(y, x, d) = popcount(cenL(y, x) xor cenR(y, x - d - min_disp)), d = 0 .. D - 1, cenR = 0 left of the image.
 *   3 paths  directions r = (dy, dx): (0,1), (0,-1), (1,0), (-1,0) and, with MI_ICP_SGM_PATH8, (1,1), (1,-1), (-1,1),
 *     (-1,-1).  L_r(p, d) = C(p, d) where p - r lies outside the image (a diagonal that reaches a side border starts
 *     anew); else, with m = min_k L_r(p - r, k), L_r(p, d) = C(p, d) + min(L_r(p - r, d), L_r(p - r, d - 1) + p1,
 *     L_r(p - r, d + 1) + p1, m + p2) - m, the d - 1 and d + 1 terms dropped outside 0 .. D - 1.  S = sum_r L_r
 *     (mi_icp_sgm_get_sums: S of the last frame as uint16 [y][x][d]; MI_ICP_ERR_STATE before the first frame).
 *   4 left map (uint16, invalid 0xFFFF)  dL = argmin_d S(y, x, d), the smallest d of equals, s1 that minimum, s2 =
 *     min S(y, x, d) over |d - dL| > 1; invalid where (float)uniqueness * (float)s2 < (float)s1 (one fp32 product).
 *   5 right map  dR(y, x) = argmin_d S(y, x + d + min_disp, d) over the d with x + d + min_disp < W, the smallest d of
 *     equals, 0 where there is none; no uniqueness test.
 *   6 median  both maps, 3 x 3, on the unsigned 16-bit values (invalid sorts high); the outermost rows and columns,
 *     and a map with H < 3 or W < 3, are copied.
 *   7 check  a left value d != 0xFFFF is valid iff lr_max_diff < 0, or k = x - (d + min_disp) >= 0 and
 *     |dR(y, k) - d| <= lr_max_diff (the medianed maps).  dst = (uint8)(d + min_disp) where valid, else
 *     (uint8)(min_disp - 1): 255 at min_disp 0 -- at D = 256 that value is a disparity as well as the invalid mark.
 *  mi_icp_create_from_disparity  disp width * height bytes, color the same size with 3 channels of bytes_per_channel
 *   (1 or 2, else MI_ICP_ERR_INVALID) bytes; q the HOST array {q00, q03, q11, q13, q23, q32, q33} (with tx = -baseline:
 *   fy * tx, -fy * cx * tx, fx * tx, -fx * cy * tx, fx * fy * tx, -fy, fy * (cx - cx_right), formed by the caller in
 *   fp32, left to right).  points and colors: width * height * 3 floats, pixel after pixel, none left out.  Pixel
 *   (u, v) of disparity d: w = q32 * d + q33, r = (float)(1.0 / (double)w), point = ((q00 * u + q03) * r,
 *   (q11 * v + q13) * r, q23 * r), every operation one fp32 rounding, nothing fused; w = 0 gives non-finite
 *   coordinates, which are kept.  Colour channel value / 255.0f or value / 65535.0f.  (The reference reads the colour
 *   through a byte's VALUE as an address; this reads the channel stored at that place.) */
#define MI_ICP_SGM_MAX_SIDE 8192
#define MI_ICP_SGM_MAX_P2 224
#define MI_ICP_SGM_PATH4 0
#define MI_ICP_SGM_PATH8 1
typedef struct mi_icp_sgm mi_icp_sgm;
MI_ICP_API int mi_icp_sgm_create(mi_icp_ctx* ctx, int width, int height, int p1, int p2, float uniqueness,
                                 int disp_size, int path_type, int min_disp, int lr_max_diff, mi_icp_sgm** out);
MI_ICP_API int mi_icp_sgm_destroy(mi_icp_ctx* ctx, mi_icp_sgm* matcher);
MI_ICP_API int mi_icp_sgm_process(mi_icp_ctx* ctx, mi_icp_sgm* matcher, const uint8_t* left, const uint8_t* right,
                                  uint8_t* dst);
MI_ICP_API int mi_icp_sgm_census(mi_icp_ctx* ctx, const uint8_t* src, int width, int height, uint32_t* dst);
MI_ICP_API int mi_icp_sgm_get_sums(mi_icp_ctx* ctx, mi_icp_sgm* matcher, uint16_t* dst);
/* the largest image side and the largest p2 taken (no context, no device) */
MI_ICP_API int mi_icp_sgm_limits(int32_t* max_side, int32_t* max_p2);
MI_ICP_API int mi_icp_create_from_disparity(mi_icp_ctx* ctx, const uint8_t* disp, const void* color, int width,
                                            int height, int bytes_per_channel, const float* q, float* points,
                                            float* colors);

/* ---- feature matching and FastGlobalRegistration (registration/feature.h, knn/bruteforce_nn.{h,inl},
 * ---- registration/fast_global_registration.{h,cu}) ----
 * Everything downstream of the descriptors: they come in as data, float[n][dim] row-major.  Every array below is in
 * DEVICE memory (no mem_kind: a surface stages host arrays itself); counts and the option are host values.  The calls
 * run in the private scratch context: the caller's target / source / loop state survive, except that
 * mi_icp_fast_global_registration ends with EvaluateRegistration on the caller's context and loads both clouds there.
 * tests/fgr_exact.py restates all of it in numpy; csrc/fgr_rules.h holds the sampler, the tuple test and the par
 * schedule for host and device alike.
 *  mi_icp_feature_match  (knn::BruteForceNN in both directions at once) features q[nq][dim], r[nr][dim]:
 *   distance  D(i, j): acc = 0; for k = 0 .. dim - 1 in order: e = q[i][k] - r[j][k] (one fp32 rounding),
 *             acc = fma(e, e, acc).  fp32 subtraction is sign-symmetric, so D is the same bits from either side; the
 *             kernel computes every D once and both directions read that value.  (The difference form, not
 *             |q|^2 + |r|^2 - 2 q.r, whose cancellation error is of the size of the distances between like descriptors.)
 *   neighbour q_idx[i] = the j of smallest D(i, j), the smallest j among equals; q_d[i] = that D.  r_idx[j] / r_d[j]
 *             likewise over i.  A NaN distance never wins; a row whose distances are all NaN gets -1 and a NaN.
 *             Any of the four outputs may be NULL.
 *   method    one pass over the pair space: 128 x 128 tiles staged through LDS, 8 x 8 pairs per lane, running minima
 *             joined by 64-bit unsigned atomic minima on (bits of D) << 32 | index (D >= 0, so the bits order as the
 *             values, the smallest index wins ties and the order of arrival cannot matter).  The nq x nr matrix is
 *             never written: memory beyond the arguments is 8 (nq + nr) bytes.
 *   limits    dim in [1, MI_ICP_FEATURE_MAX_DIM], nq, nr in [1, 2^31); else, or with q or r NULL, MI_ICP_ERR_INVALID
 *             before any launch.  Does not wait for the stream.
 *  mi_icp_fgr_correspondences  (AdvancedMatching behind its two searches) s_idx[ns]: every source point's neighbour
 *   among the target's features, t_idx[nt] the reverse (mi_icp_feature_match's q_idx / r_idx); src_xyz, tgt_xyz the
 *   points.
 *   pairs     (i, j) with s_idx[i] = j in [0, nt) and t_idx[j] = i, ascending in i -> pairs (room for min(ns, nt) rows
 *             of two int32), *n_pairs = ncorr.
 *   trials    100 * ncorr of them.  Trial t takes the pairs numbered floor(u(3t + m) * ncorr / 2^64), m = 0, 1, 2, u(j)
 *             = output j of the splitmix64 stream seeded with `seed` that mi_icp_segment_plane draws from.  With p0, p1,
 *             p2 its source points and q0, q1, q2 the target points paired with them -- the caller's coordinates: the
 *             test is invariant to the normalisation -- the squared sides are L(a, b) = (dx*dx + dy*dy) + dz*dz, d = a
 *             - b, every operation one fp32 rounding, none fused; Li = L(p0,p1), L(p1,p2), L(p2,p0), Lj likewise; s2 =
 *             tuple_scale * tuple_scale.  The trial PASSES iff for all three sides Li * s2 < Lj and Lj * s2 < Li.  No
 *             square root, no division; a repeated pair fails by itself.
 *   list      the passing trials' three correspondences (source index, target index), in trial order, cut to
 *             maximum_tuple_count entries (1000: 333 triples and one more) -> corr (room for min(maximum_tuple_count,
 *             300 * min(ns, nt)) rows), *n_corr.  Only the first ceil(max / 3) passing trials are written.
 *   limits    ns, nt in [1, 0x7fffff00], 100 * ncorr <= 0x7fffff00, maximum_tuple_count >= 0; else MI_ICP_ERR_INVALID.
 *             Integers throughout: the same bytes on every run and context.  Waits for the stream twice.
 *  mi_icp_fgr_optimize  (OptimizePairwiseRegistration) points as given (normalised or not), corr[n_corr][2]:
 *   fewer than 10 correspondences, or iteration_number = 0: T16 = identity, the sums zero, *par_out = par_start.  Else
 *   q_c = tgt[j_c] for every correspondence c = (i_c, j_c), par = par_start, trans = I, and iteration_number times:
 *   weight  r = p - q (p = src[i_c]), w = t * t, t = par / (((rx*rx + ry*ry) + rz*rz) + par): fp32, every operation
 *           rounded, IEEE division;
 *   sums    JTJ (21 upper-triangle entries, row-major) and JTr (6) of the rows (0, -qz, qy, -1, 0, 0 | rx), (qz, 0,
 *           -qx, 0, -1, 0 | ry), (-qy, qx, 0, 0, 0, -1 | rz), each weighted by w: every term formed and added in fp64
 *           from the fp32 p, q, r, w, in a fixed order (per thread, wave, then the four waves);
 *   step    x solves (-JTJ) x = JTr in fp32 (the LDL^T of mi_icp_solve_system, no determinant check), delta =
 *           mi_icp_vector6_to_matrix4(x), trans = delta * trans, q_c = ((d00 x + d01 y) + d02 z) + t0, ... in fp32,
 *           nothing fused;
 *   par     if decrease_mu and itr % 4 == 0 and par > maximum_correspondence_distance: par = par / division_factor.
 *   T16 (column-major) = trans; sums27 (may be NULL) = the last iteration's 27 sums; par_out (may be NULL) = par
 *   after the last iteration.  One workgroup runs all iterations: no host round trip, no wait.  A correspondence with
 *   an index outside its cloud takes no part.  Same input, same bytes.
 *  mi_icp_correspondences_from_features  (declared in feature.h, defined nowhere in the reference; this definition is
 *   the library's) row i = (i, nn(i)) for every source row that has a neighbour, ascending; with mutual_filter only
 *   the rows whose neighbour points back -- unless fewer than mutual_consistency_ratio * ns (one fp32 product) remain:
 *   then the unfiltered list.  corr: room for ns rows.  Waits once, twice when it falls back.
 *  mi_icp_fast_global_registration  the whole call:
 *   1 match   mi_icp_feature_match(source features, target features), the reciprocal pairs, the cut tuple list;
 *   2 normalise  per cloud mean = (float)(sum / n), the sums in fp64 in a fixed order; points centred in fp32; scale
 *             = sqrt of the largest (x*x + y*y) + z*z over both centred clouds; scale_global = use_absolute_scale ? 1
 *             : scale; points / scale_global (IEEE division);
 *   3 optimise  mi_icp_fgr_optimize on the normalised clouds with par_start = scale_global (the reference hands
 *             scale_global to the parameter its optimiser calls scale_start; kept, callers see its effect);
 *   4 map back  (GetInvTransformationOriginalScale) R, t of trans; v = (-(R m_tgt) + t * scale_global) + m_src; T =
 *             [R^T, -(R^T v)] in fp32, products summed left to right;
 *   5 result  mi_icp_set_target(target), mi_icp_set_source(source) and mi_icp_evaluate_registration(
 *             maximum_correspondence_distance, T) on the caller's context: *out is its result, and
 *             mi_icp_get_correspondences gives its correspondence_set.
 *   The number of waits and launches does not depend on iteration_number.  Same input and seed, same bytes.
 * Deviations (deliberate): the pairs ascend in the source index (the reference orders them by the larger cloud's index
 * after a swap; the order only feeds the random draw).  The random stream is not thrust::default_random_engine's: same
 * distribution of triples, other triples.  The tuple test compares squared lengths by multiplication (the reference:
 * norms and a division).  The sums are fp64 (the reference: fp32 in thrust's order). */
#define MI_ICP_FEATURE_MAX_DIM 512
typedef struct mi_icp_fgr_option {        /* registration::FastGlobalRegistrationOption and its defaults */
    float division_factor;                /* 1.4 */
    int32_t use_absolute_scale;           /* 0 */
    int32_t decrease_mu;                  /* 1 */
    float maximum_correspondence_distance;/* 0.025 */
    int32_t iteration_number;             /* 64 */
    float tuple_scale;                    /* 0.95 */
    int32_t maximum_tuple_count;          /* 1000 */
} mi_icp_fgr_option;
MI_ICP_API int mi_icp_feature_match(mi_icp_ctx* ctx, const float* q, int64_t nq, const float* r, int64_t nr, int dim,
                                    int32_t* q_idx, float* q_d, int32_t* r_idx, float* r_d);
MI_ICP_API int mi_icp_fgr_correspondences(mi_icp_ctx* ctx, const int32_t* s_idx, int64_t ns, const int32_t* t_idx,
                                          int64_t nt, const float* src_xyz, const float* tgt_xyz, float tuple_scale,
                                          int64_t maximum_tuple_count, uint64_t seed, int32_t* pairs, int64_t* n_pairs,
                                          int32_t* corr, int64_t* n_corr);
MI_ICP_API int mi_icp_fgr_optimize(mi_icp_ctx* ctx, const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt,
                                   const int32_t* corr, int64_t n_corr, float par_start,
                                   const mi_icp_fgr_option* option, float* T16, double* sums27, float* par_out);
MI_ICP_API int mi_icp_correspondences_from_features(mi_icp_ctx* ctx, const float* src_feat, int64_t ns,
                                                    const float* tgt_feat, int64_t nt, int dim, int mutual_filter,
                                                    float mutual_consistency_ratio, int32_t* corr, int64_t* n_corr);
MI_ICP_API int mi_icp_fast_global_registration(mi_icp_ctx* ctx, const float* src_xyz, const float* src_feat, int64_t ns,
                                               const float* tgt_xyz, const float* tgt_feat, int64_t nt, int dim,
                                               const mi_icp_fgr_option* option, uint64_t seed, mi_icp_result* out);

/* ---- knn::KDTreeFlann as a search object (knn/kdtree_flann.h:43-124) ---------
 * SearchKNN / SearchRadius (knn/kdtree_flann.inl:46-122) of arbitrary queries
 * float[nq][3] against the cloud given to mi_icp_set_target: per query the knn
 * (<= 100 = knn::NUM_MAX_NN) nearest target points -- with d2 < radius^2 when radius > 0, i.e.
 * SearchRadius(radius, max_nn = knn) -- ascending in distance (ties ascending in
 * index).  idx_out / d2_out are [nq][knn] row-major in the caller's query order,
 * original target indices, padded with -1 / +inf.  *found (optional) = number of
 * neighbours over all queries (the reference's return value for one query).
 * The queries are staged in the context's SOURCE slot: a cloud set with
 * mi_icp_set_source is replaced. */
MI_ICP_API int mi_icp_search_knn(mi_icp_ctx* ctx, const float* queries, int64_t nq, int knn,
                                 float radius, int32_t* idx_out, float* d2_out, int64_t* found,
                                 int mem_kind);

/* ---- Colored ICP (registration/colored_icp.cu) -----------------------------
 * Colours are float[n][3] RGB in the order of the cloud last given to
 * mi_icp_set_target / mi_icp_set_source (call these afterwards; a new
 * set_target / set_source drops them).  Only the intensity (r+g+b)/3 is kept,
 * as the reference's functors only use that (colored_icp.cu:91,195-200).  The
 * target needs normals (colored_icp.cu:222-224). */
MI_ICP_API int mi_icp_set_target_colors(mi_icp_ctx* ctx, const float* rgb, int mem_kind);
MI_ICP_API int mi_icp_set_source_colors(mi_icp_ctx* ctx, const float* rgb, int mem_kind);
/* TransformationEstimationForColoredICP::lambda_geometric_ (default 0.968;
 * values outside [0,1] fall back to it, colored_icp.cu:47-51).  Used by every
 * MI_ICP_EST_COLORED evaluation. */
MI_ICP_API int mi_icp_set_lambda_geometric(mi_icp_ctx* ctx, float lambda_geometric);
/* InitializePointCloudForColoredICP (colored_icp.cu:108-148): per target point
 * the intensity gradient in the tangent plane over the max_nn (<= 100) nearest
 * points within `radius` (the nearest -- the point itself -- excluded; fewer
 * than 4 others -> 0).  Kept on the device for MI_ICP_EST_COLORED;
 * gradients_out (float[nt][3], target's original order) may be NULL. */
MI_ICP_API int mi_icp_compute_color_gradients(mi_icp_ctx* ctx, float radius, int max_nn,
                                              float* gradients_out, int mem_kind);
/* registration::RegistrationColoredICP (colored_icp.cu:329-341) =
 * compute_color_gradients(2 * max_distance, 30) + registration_icp(COLORED).
 * params->det_thresh is the estimator's det_thresh (default 1e-6).
 * NOTE the reference's ComputeRMSE for this estimator returns the plain sum of
 * squared residuals (colored_icp.cu:302-306); mi_icp_compute_rmse(COLORED)
 * does the same. */
MI_ICP_API int mi_icp_registration_colored_icp(mi_icp_ctx* ctx, float max_distance,
                                               const float* init, const mi_icp_params* params,
                                               float lambda_geometric, mi_icp_result* out);

/* ---- multi-GPU (new: the reference is single-GPU) -------------------------
 * One context per rank/GPU, each holding the full target and its own shard of
 * the source.  After mi_icp_comm_init every accumulated system (32 doubles) is
 * summed across ranks before the solve, in a fixed order, so all ranks take
 * bit-identical steps.  How:
 *  - ranks of ONE node (<= 16) exchange through a MAILBOX in POSIX shared memory
 *    that every rank's GPU maps (csrc/mailbox.h): the reduction's finishing block
 *    posts its sums, waits for the peers' and goes on to the step -- an iteration
 *    stays two launches, no collective is launched;
 *  - otherwise (MI_ICP_NO_MAILBOX=1, more ranks, mailbox set-up failed) one
 *    ncclAllReduce(double, 32) on the context's stream, then the step kernel.
 * mi_icp_comm_init: RCCL communicator from a shared ncclUniqueId + the mailbox (named after
 * the id); ncclCommInitRank blocks until every rank has joined -- the call waits MI_ICP_COMM_INIT_MS (default 120000;
 * <= 0: for ever) for it and fails with MI_ICP_ERR_COMM past that.  mi_icp_comm_init_local: the mailbox alone, no RCCL -- all ranks pass the same
 * job_name (letters, digits, '_', '-'), one node only.  mi_icp_comm_kind: 0 none, 1 RCCL
 * all-reduce, 2 mailbox, 3 mailbox with device inboxes (every rank keeps an inbox in fine-grained device memory
 * that its peers open through HIP IPC and write their posts into -- GPU to GPU, polls stay local; any rank failing
 * to set that up keeps all of them on the host-memory box; USED when MI_ICP_MAILBOX=device is set ON RANK 0
 * (published through the box: the peers' own environment is not consulted) or
 * mi_icp_comm_autotune below measured them faster; MI_ICP_MAILBOX=host on rank 0: not even set up).  Set-up: rank 0 makes the box and waits (MI_ICP_MAIL_ATTACH_MS, default 30 s)
 * until every other rank has mapped and registered it; mi_icp_comm_init then lets the ranks agree over the
 * RCCL communicator whether ALL of them have it (else none uses it).  A peer that does not post within ~10 s
 * fails the call with MI_ICP_ERR_COMM; the communicator is void from then on (the ranks' exchange counters
 * are apart): every further call that would exchange fails the same way until mi_icp_comm_destroy /
 * mi_icp_comm_init[_local] have made a new one. */
MI_ICP_API int mi_icp_comm_unique_id(char* id128);
MI_ICP_API int mi_icp_comm_init(mi_icp_ctx* ctx, const char* id128, int nranks, int rank);
MI_ICP_API int mi_icp_comm_init_local(mi_icp_ctx* ctx, const char* job_name, int nranks, int rank);
MI_ICP_API int mi_icp_comm_kind(const mi_icp_ctx* ctx);
MI_ICP_API int mi_icp_comm_destroy(mi_icp_ctx* ctx);
/* Which way the ranks exchange is MEASURED, not assumed (collective: every rank calls it, right after
 * mi_icp_comm_init[_local] and before any registration).  Each available path -- [0] the box's host-memory words,
 * [1] device inboxes over HIP IPC (set up next to the box unless MI_ICP_MAILBOX=host), [2] the in-library
 * ncclAllReduce followed by a one-block kernel, as the loop's step kernel follows it -- performs `exchanges`
 * (<= 0: 200) all-reduces of a KNOWN vector that changes with every exchange; every total is checked exactly on the
 * device, the run is timed with events on the context's stream, and the ranks' CPUs gather the figures through the
 * shared-memory box (through the communicator when there is no box).  lat_us3[p]: microseconds per exchange, the
 * maximum over the ranks; -1: path not available, -2: it failed its self-test (timed out or summed wrongly) on some
 * rank -- such a path is skipped, never fatal, and the ranks' exchange counters are re-aligned behind it.  The
 * fastest path that passed everywhere becomes the one the loops use (identical on every rank: all decide on the same
 * gathered figures).  info4 = {chosen path (1 host words, 2 device inboxes, 3 RCCL; 0: single rank), ncclCommCount
 * of the communicator (0: none), exchanges timed per path, 1 if every path that was tried passed}.
 * MI_ICP_ERR_COMM when no path passed or the ranks did not meet (the communicator is void then). */
MI_ICP_API int mi_icp_comm_autotune(mi_icp_ctx* ctx, int exchanges, double* lat_us3, int* info4);
/* total source size over all ranks (fitness denominator, registration.cu:76) */
MI_ICP_API int mi_icp_set_global_source_count(mi_icp_ctx* ctx, int64_t n_total);
/* The order in which a source cloud is cut into per-rank shards: order_out[s] = original index
 * of the s-th point along the engine's space-filling (Morton) order, so that rank r of R takes
 * order_out[r*n/R .. (r+1)*n/R) -- one compact region of the target tree per GPU.  Computed on
 * the device (bounds, keys, radix sort); xyz and order_out on the side named by mem_kind. */
MI_ICP_API int mi_icp_spatial_order(mi_icp_ctx* ctx, const float* xyz, int64_t n, uint32_t* order_out,
                                    int mem_kind);

/* ---- per-iteration report (registration.cu:155-156: utility::LogDebug("ICP Iteration #{:d}: Fitness {:.4f},
 * RMSE {:.4f}", i, ...) at the top of every iteration) ----------------------------------------------
 * The loop runs on the device, several iterations per host look; with a callback set every update records
 * the evaluation it starts from, and the callback is called -- on the calling thread, in iteration order,
 * from inside mi_icp_registration_icp / mi_icp_icp_begin / mi_icp_icp_iterate / mi_icp_registration_colored_icp
 * -- once per iteration with the iteration's number (from 0), fitness and inlier RMSE: the values the reference
 * logs.  NULL removes it.  Costs one small device-to-host copy per look; nothing when unset. */
typedef void (*mi_icp_iteration_fn)(void* user, int iteration, float fitness, float inlier_rmse);
MI_ICP_API int mi_icp_set_iteration_callback(mi_icp_ctx* ctx, mi_icp_iteration_fn fn, void* user);

/* ---- instrumentation ----------------------------------------------------
 * enable != 0: every nearest-neighbour and reduction launch is bracketed by
 * hipEvents on the context's stream.  out[8] = {nn_ms_total, nn_launches,
 * reduce_ms_total, reduce_launches, build_ms_target, build_ms_source, halo builds
 * started by registration loops on this context (always counted), 0}. */
MI_ICP_API int mi_icp_set_profiling(mi_icp_ctx* ctx, int enable);
MI_ICP_API int mi_icp_get_profile(mi_icp_ctx* ctx, double* out8);

#ifdef __cplusplus
}
#endif
#endif /* MI_ICP_H_ */
