// mi_geometry.hip -- the geometry entry points beside the registration: Transform, bounds / centre, Translate / Scale /
// Rotate, GICP covariances, SelectByIndex / SelectByMask / UniformDownSample and the compaction behind them and the
// outlier filters; FarthestPointDownSample, PassThroughFilter / Crop / RemoveNoneFinitePoints; SegmentPlane; colours
// (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "farthest_point.h"
#include "geometry_kernels.h"
#include "lbvh.h"
#include "reduce.h"
#include "segment_plane.h"
#include "select.h"

using namespace mi;
using namespace mi::eng;
using host::Mat4;

namespace mi {
namespace eng {
int compact_by_flags(mi_icp_ctx* c, const uint32_t* flags, int64_t n, const float* const in[3], float* const out[3],
                     int64_t* out_idx, int mem_kind, const uint32_t* status, int64_t* m, uint32_t* status_out) {
    *m = 0;
    if (status_out) *status_out = 0u;
    if (n <= 0) return MI_ICP_OK;
    uint32_t* pos;
    const uint32_t* total;
    TRY(scan_flags(c, flags, n, &pos, &total));
    float* dst[3];
    int64_t* didx;
    TRY(cloud_out(c, in, out, n, mem_kind, c->vpay, dst));
    TRY(out_slot(c, out_idx, (size_t)n, mem_kind, c->pairs_out, &didx));
    select_gather<<<blocks_for(n), 256, 0, c->stream>>>(flags, pos, n, in[0], in[1], in[2], dst[0], dst[1], dst[2], didx);
    KCHK(c);
    // the count (and the caller's status word) come back with the one wait of the call
    TRY(read_total(c, total));
    if (status) HIPCHK(c, hipMemcpyAsync(c->u_host + 1, status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t cnt = (int64_t)c->u_host[0];
    if (status_out && status) *status_out = c->u_host[1];
    if (dst[0] != out[0] || didx != out_idx) {  // staged: a second wait, for the copies to the caller
        TRY(cloud_out_back(c, dst, out, cnt, mem_kind));
        TRY(from_device(c, (const int64_t*)didx, out_idx, (size_t)cnt, mem_kind));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    *m = cnt;
    return MI_ICP_OK;
}

}  // namespace eng
}  // namespace mi

extern "C" {

// ---------------------------------------------------------------------------
int mi_icp_transform(mi_icp_ctx* c, const float* T, float* xyz, float* normals, float* covs,
                     int64_t n, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "transform"));
    if (n < 0) return fail(c, MI_ICP_ERR_INVALID, "transform: negative size");
    if (n == 0 || (!xyz && !normals && !covs)) return MI_ICP_OK;
    const Xform X = make_xform(load_T(T));
    const float *dp, *dn, *dc;
    TRY(to_device(c, (const float*)xyz, (size_t)n * 3, mem_kind, c->stage[0], &dp));
    TRY(to_device(c, (const float*)normals, (size_t)n * 3, mem_kind, c->stage[1], &dn));
    TRY(to_device(c, (const float*)covs, (size_t)n * 9, mem_kind, c->stage[2], &dc));
    transform_cloud<<<blocks_for(n), 256, 0, c->stream>>>(X, (float*)dp, (float*)dn, (float*)dc, n);
    KCHK(c);
    TRY(from_device(c, dp, xyz, (size_t)n * 3, mem_kind));
    TRY(from_device(c, dn, normals, (size_t)n * 3, mem_kind));
    TRY(from_device(c, dc, covs, (size_t)n * 9, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // pointcloud.cu:297 cudaDeviceSynchronize
    return MI_ICP_OK;
}

// GeometryBase3D::GetMinBound / GetMaxBound / GetCenter (geometry/pointcloud.cu:205-215)
int mi_icp_compute_bounds(mi_icp_ctx* c, const float* xyz, int64_t n, int mem_kind, float* min3, float* max3,
                          float* center3) {
    TRY(check_ctx(c, mem_kind, "compute_bounds"));
    if (n < 0 || (n > 0 && !xyz)) return fail(c, MI_ICP_ERR_INVALID, "compute_bounds: bad size/pointer");
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    if (n == 0) {  // the reference returns zero vectors for an empty cloud
        if (min3) std::memcpy(min3, zero, sizeof(zero));
        if (max3) std::memcpy(max3, zero, sizeof(zero));
        if (center3) std::memcpy(center3, zero, sizeof(zero));
        return MI_ICP_OK;
    }
    const float* d_pts;
    TRY(to_device(c, xyz, (size_t)n * 3, mem_kind, c->stage[0], &d_pts));
    float* bnd;
    TRY(compute_bounds(c, d_pts, n, &bnd));  // min[3], max[3], extent
    float* rec;
    TRY(ensure(c, c->flags, 16, &rec));
    HIPCHK(c, hipMemcpyAsync(rec, bnd, 7 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    if (center3) {
        double* part;
        TRY(ensure(c, c->partial, (size_t)kReduceBlocks * kSysSize, &part));
        const int blocks = (int)std::min<int64_t>(kCenterBlocks, blocks_for(n));
        center_partial<<<blocks, 256, 0, c->stream>>>(d_pts, n, part);
        KCHK(c);
        center_final<<<1, 64, 0, c->stream>>>(part, blocks, n, rec);
        KCHK(c);
    }
    HIPCHK(c, hipMemcpyAsync(c->f_host, rec, 10 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (min3) std::memcpy(min3, c->f_host, 3 * sizeof(float));
    if (max3) std::memcpy(max3, c->f_host + 3, 3 * sizeof(float));
    if (center3) std::memcpy(center3, c->f_host + 7, 3 * sizeof(float));
    return MI_ICP_OK;
}

// GeometryBase3D::Translate / Scale / Rotate (geometry/pointcloud.cu:225-242)
int mi_icp_affine(mi_icp_ctx* c, const float* R9, float scale, int use_scale, const float* center3,
                  const float* translate3, float* xyz, float* normals, float* covs, int64_t n, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "affine"));
    if (n < 0) return fail(c, MI_ICP_ERR_INVALID, "affine: negative size");
    if (n == 0 || (!xyz && !normals && !covs)) return MI_ICP_OK;
    Affine A;
    std::memset(&A, 0, sizeof(A));
    A.use_r = R9 != nullptr;
    A.use_s = use_scale != 0;
    A.use_c = center3 != nullptr;
    A.use_t = translate3 != nullptr;
    A.s = scale;
    if (R9)   // column-major (Eigen::Matrix3f::data()) -> row-major
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) A.r[r * 3 + q] = R9[q * 3 + r];
    if (center3) std::memcpy(A.c, center3, sizeof(A.c));
    if (translate3) std::memcpy(A.t, translate3, sizeof(A.t));
    const float *dp, *dn, *dc;
    TRY(to_device(c, (const float*)xyz, (size_t)n * 3, mem_kind, c->stage[0], &dp));
    TRY(to_device(c, (const float*)normals, (size_t)n * 3, mem_kind, c->stage[1], &dn));
    TRY(to_device(c, (const float*)covs, (size_t)n * 9, mem_kind, c->stage[2], &dc));
    affine_cloud<<<blocks_for(n), 256, 0, c->stream>>>(A, const_cast<float*>(dp), const_cast<float*>(dn),
                                                        const_cast<float*>(dc), n);
    KCHK(c);
    TRY(from_device(c, dp, xyz, (size_t)n * 3, mem_kind));
    TRY(from_device(c, dn, normals, (size_t)n * 3, mem_kind));
    TRY(from_device(c, dc, covs, (size_t)n * 9, mem_kind));
    if (dp != xyz || dn != normals || dc != covs) HIPCHK(c, hipStreamSynchronize(c->stream));  // (staged: the copies)
    return MI_ICP_OK;
}

int mi_icp_covariances_from_normals(mi_icp_ctx* c, const float* normals, int64_t n, float epsilon,
                                    float* covs, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "covariances_from_normals"));
    if (n < 0 || (n > 0 && (!normals || !covs))) return fail(c, MI_ICP_ERR_INVALID, "covariances_from_normals: bad arguments");
    if (n == 0) return MI_ICP_OK;
    const float* dn;
    TRY(to_device(c, normals, (size_t)n * 3, mem_kind, c->stage[1], &dn));
    float* dc;
    TRY(out_slot(c, covs, (size_t)n * 9, mem_kind, c->stage[2], &dc));
    cov_from_normals<<<blocks_for(n), 256, 0, c->stream>>>(dn, n, epsilon, dc);
    KCHK(c);
    TRY(from_device(c, (const float*)dc, covs, (size_t)n * 9, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

// ---------------------------------------------------------------------------
// PointCloud::SelectByIndex (geometry/down_sample.cu:40-62,110-129)
int mi_icp_select_by_index(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                           const int64_t* indices, int64_t n_indices, int invert, float* out_xyz, float* out_normals,
                           float* out_colors, int64_t* m, int mem_kind) {
    TRY(check_sizes(c, "select_by_index", n, m, mem_kind));
    TRY(count_ok(c, "select_by_index", n_indices));
    // (its own null-buffer rule: an empty cloud or an empty list needs no array)
    if ((n > 0 && !xyz) || (n_indices > 0 && !indices)) return fail(c, MI_ICP_ERR_INVALID, "select_by_index: null buffer");
    const int64_t count = invert ? n : n_indices;  // the most points the output can hold
    if (count > 0 && (!out_xyz || (normals && !out_normals) || (colors && !out_colors)))
        return fail(c, MI_ICP_ERR_INVALID, "select_by_index: null buffer");
    if (n == 0 && n_indices > 0) return fail(c, MI_ICP_ERR_INVALID, "select_by_index: index out of range [0, 0)");
    if (count == 0) return MI_ICP_OK;

    Cloud cl{{xyz, normals, colors}, {out_xyz, out_normals, out_colors}};
    TRY(cloud_upload(c, &cl, n, mem_kind, c->stage));
    const float* const* in = cl.in;
    float* const* out = cl.out;
    const int64_t* idx = nullptr;
    TRY(to_device(c, indices, (size_t)n_indices, mem_kind, c->keys0, &idx));
    uint32_t* flags;
    TRY(ensure(c, c->flags, (size_t)n + 1, &flags));  // [n]: the status word (an index outside [0, n))
    uint32_t* status = flags + n;
    uint32_t bad = 0u;
    int64_t got = 0;
    if (!invert) {
        HIPCHK(c, hipMemsetAsync(status, 0, sizeof(uint32_t), c->stream));
        float* dst[3];
        TRY(cloud_out(c, in, out, n_indices, mem_kind, c->vpay, dst));
        select_list<<<blocks_for(n_indices), 256, 0, c->stream>>>(idx, n_indices, n, in[0], in[1], in[2], dst[0], dst[1],
                                                                  dst[2], status);
        KCHK(c);
        TRY(cloud_out_back(c, dst, out, n_indices, mem_kind));
        HIPCHK(c, hipMemcpyAsync(c->u_host + 1, status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        bad = c->u_host[1];
        got = n_indices;
    } else {
        // the points not named, ascending; a repeated index counts once (the reference sizes the output n - n_indices)
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)flags, 1, (size_t)n, c->stream));
        HIPCHK(c, hipMemsetAsync(status, 0, sizeof(uint32_t), c->stream));
        if (n_indices > 0) {
            select_mark<<<blocks_for(n_indices), 256, 0, c->stream>>>(idx, n_indices, n, flags, status);
            KCHK(c);
        }
        TRY(compact_by_flags(c, flags, n, in, out, nullptr, mem_kind, status, &got, &bad));
    }
    if (bad) return fail(c, MI_ICP_ERR_INVALID, "select_by_index: index out of range [0, %lld)", (long long)n);
    *m = got;
    return MI_ICP_OK;
}

// PointCloud::SelectByMask (geometry/down_sample.cu:131-168): the entries whose mask byte is set (invert: clear),
// ascending.  A byte per point becomes the flags; the scan and the gather are SelectByIndex's.
int mi_icp_select_by_mask(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                          const uint8_t* mask, int64_t n_mask, int invert, float* out_xyz, float* out_normals,
                          float* out_colors, int64_t* m, int mem_kind) {
    const char* what = "select_by_mask";
    TRY(check_sizes(c, what, n, m, mem_kind));
    if (n_mask != n)
        return fail(c, MI_ICP_ERR_INVALID, "%s: the mask has %lld entries, the cloud %lld points", what, (long long)n_mask, (long long)n);
    if (n == 0) return MI_ICP_OK;
    if (!mask) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    Cloud cl{{xyz, normals, colors}, {out_xyz, out_normals, out_colors}};
    TRY(cloud_in(c, what, &cl, n, mem_kind, c->stage));
    const uint8_t* dmask;
    TRY(to_device(c, mask, (size_t)n, mem_kind, c->keys0, &dmask));
    uint32_t* flags;
    TRY(ensure(c, c->flags, (size_t)n, &flags));
    select_mask_flags<<<blocks_for(n), 256, 0, c->stream>>>(dmask, n, invert, flags);
    KCHK(c);
    return compact_by_flags(c, flags, n, cl.in, cl.out, nullptr, mem_kind, nullptr, m, nullptr);
}

// PointCloud::UniformDownSample (geometry/down_sample.cu:275-316): points 0, k, 2k, ... -- n / k of them (the size the
// reference allocates).  A strided copy per attribute, no kernel.
int mi_icp_uniform_downsample(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                              int64_t every_k_points, float* out_xyz, float* out_normals, float* out_colors, int64_t* m,
                              int mem_kind) {
    // (its own size rule: a strided copy with 64-bit offsets and no staging, so no upper bound)
    TRY(check_ctx(c, mem_kind, "uniform_downsample"));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "uniform_downsample: m is null");
    *m = 0;
    if (n < 0) return fail(c, MI_ICP_ERR_INVALID, "uniform_downsample: bad size");
    if (every_k_points <= 0) return fail(c, MI_ICP_ERR_INVALID, "uniform_downsample: every_k_points must be positive");
    const int64_t cnt = n / every_k_points;
    if (cnt == 0) return MI_ICP_OK;
    const Cloud cl{{xyz, normals, colors}, {out_xyz, out_normals, out_colors}};
    TRY(cloud_check(c, "uniform_downsample", cl));
    const float* const* in = cl.in;
    float* const* out = cl.out;
    const size_t row = 3 * sizeof(float), pitch = row * (size_t)every_k_points;
    for (int k = 0; k < 3; ++k) {
        if (!in[k]) continue;
        if (mem_kind == MI_ICP_DEVICE) {
            HIPCHK(c, hipMemcpy2DAsync(out[k], row, in[k], pitch, row, (size_t)cnt, hipMemcpyDeviceToDevice, c->stream));
        } else {  // host arrays: the same strided copy on the host
            for (int64_t j = 0; j < cnt; ++j) std::memcpy(out[k] + j * 3, in[k] + j * 3 * every_k_points, row);
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *m = cnt;
    return MI_ICP_OK;
}

// ---------------------------------------------------------------------------
// PointCloud::FarthestPointDownSample (geometry/pointcloud.cu:122-139, 301-338; farthest_point.h): one launch per sample,
// all of them enqueued before the one wait; the gather is SelectByIndex's select_list over the device-resident sel.
int mi_icp_farthest_point_downsample(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                                     int64_t num_samples, float* out_xyz, float* out_normals, float* out_colors,
                                     int64_t* out_idx, int64_t* m, int mem_kind) {
    const char* what = "farthest_point_downsample";
    TRY(check_sizes(c, what, n, m, mem_kind));
    if (num_samples < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: num_samples must not be negative", what);
    if (num_samples > n)
        return fail(c, MI_ICP_ERR_INVALID, "%s: %lld samples asked of %lld points", what, (long long)num_samples, (long long)n);
    if (num_samples == 0) return MI_ICP_OK;
    Cloud cl{{xyz, normals, colors}, {out_xyz, out_normals, out_colors}};
    TRY(cloud_in(c, what, &cl, n, mem_kind, c->stage));
    const float* const* in = cl.in;
    float* const* out = cl.out;
    int64_t* sel;
    TRY(out_slot(c, out_idx, (size_t)num_samples, mem_kind, c->keys0, &sel));
    if (!sel) TRY(ensure(c, c->keys0, (size_t)num_samples, &sel));  // (the caller does not want it; the gather does)
    hipStream_t s = c->stream;
    if (num_samples == n) {  // the reference's early return: the cloud itself
        fps_iota<<<blocks_for(n), 256, 0, s>>>(sel, n);
    } else {
        float* dist;
        FpsState* st;
        TRY(ensure(c, c->stage[3], (size_t)n, &dist));
        TRY(ensure(c, c->keys1, 1, &st));
        const int blocks = std::min(kFpsMaxBlocks, blocks_for(n, kFpsThreads));
        fps_init<<<1, 64, 0, s>>>(in[0], st, sel);
        for (int64_t t = 0; t + 1 < num_samples; ++t) {
            if (t == 0) fps_step<true><<<blocks, kFpsThreads, 0, s>>>(in[0], dist, n, t, st, sel);
            else fps_step<false><<<blocks, kFpsThreads, 0, s>>>(in[0], dist, n, t, st, sel);
        }
    }
    KCHK(c);
    uint32_t* status;
    TRY(ensure(c, c->flags, 1, &status));
    HIPCHK(c, hipMemsetAsync(status, 0, sizeof(uint32_t), s));
    float* dst[3];  // (not cloud_emit: the indices and the status word ride on the same wait)
    TRY(cloud_out(c, in, out, num_samples, mem_kind, c->vpay, dst));
    select_list<<<blocks_for(num_samples), 256, 0, s>>>(sel, num_samples, n, in[0], in[1], in[2], dst[0], dst[1], dst[2], status);
    KCHK(c);
    TRY(cloud_out_back(c, dst, out, num_samples, mem_kind));
    TRY(from_device(c, (const int64_t*)sel, out_idx, (size_t)num_samples, mem_kind));
    HIPCHK(c, hipMemcpyAsync(c->u_host + 1, status, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(c, hipStreamSynchronize(s));
    if (c->u_host[1]) return fail(c, MI_ICP_ERR_STATE, "%s: a selected index left [0, %lld)", what, (long long)n);
    *m = num_samples;
    return MI_ICP_OK;
}

// ---------------------------------------------------------------------------
// PointCloud::PassThroughFilter / Crop(AxisAlignedBoundingBox) / RemoveNoneFinitePoints (geometry/pointcloud.cu:40-54,
// 108-120, 340-348, 360-385, 436-466): a flags kernel per predicate (select.h), then the scan and gather of the selections.
}  // extern "C"

template <class Flags>
static int predicate_filter(mi_icp_ctx* c, const char* what, const float* xyz, const float* normals, const float* colors,
                            int64_t n, float* out_xyz, float* out_normals, float* out_colors, int64_t* out_idx, int64_t* m,
                            int mem_kind, Flags launch_flags) {
    if (n == 0) return MI_ICP_OK;
    Cloud cl{{xyz, normals, colors}, {out_xyz, out_normals, out_colors}};
    TRY(cloud_in(c, what, &cl, n, mem_kind, c->stage));
    uint32_t* flags;
    TRY(ensure(c, c->flags, (size_t)n, &flags));
    launch_flags(cl.in[0], flags);
    KCHK(c);
    return compact_by_flags(c, flags, n, cl.in, cl.out, out_idx, mem_kind, nullptr, m, nullptr);
}

extern "C" {

int mi_icp_pass_through_filter(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                               int axis_no, float min_bound, float max_bound, float* out_xyz, float* out_normals,
                               float* out_colors, int64_t* out_idx, int64_t* m, int mem_kind) {
    const char* what = "pass_through_filter";
    TRY(check_sizes(c, what, n, m, mem_kind));
    if (axis_no < 0 || axis_no > 2) return fail(c, MI_ICP_ERR_INVALID, "%s: axis_no must be 0, 1 or 2", what);
    return predicate_filter(c, what, xyz, normals, colors, n, out_xyz, out_normals, out_colors, out_idx, m, mem_kind,
                            [&](const float* p, uint32_t* flags) {
                                pass_through_flags<<<blocks_for(n), 256, 0, c->stream>>>(p, n, axis_no, min_bound, max_bound, flags);
                            });
}

int mi_icp_crop_aabb(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                     const float* min_bound3, const float* max_bound3, float* out_xyz, float* out_normals,
                     float* out_colors, int64_t* out_idx, int64_t* m, int mem_kind) {
    const char* what = "crop_aabb";
    TRY(check_sizes(c, what, n, m, mem_kind));
    if (!min_bound3 || !max_bound3) return fail(c, MI_ICP_ERR_INVALID, "%s: null bounds", what);
    CropBox b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = min_bound3[k];
        b.hi[k] = max_bound3[k];
    }
    // AxisAlignedBoundingBox::Volume() (the product of the extents, in fp32) must be positive
    const float volume = ((b.hi[0] - b.lo[0]) * (b.hi[1] - b.lo[1])) * (b.hi[2] - b.lo[2]);
    if (!(volume > 0.0f)) return fail(c, MI_ICP_ERR_INVALID, "%s: the bounding box is empty", what);
    return predicate_filter(c, what, xyz, normals, colors, n, out_xyz, out_normals, out_colors, out_idx, m, mem_kind,
                            [&](const float* p, uint32_t* flags) {
                                crop_flags<<<blocks_for(n), 256, 0, c->stream>>>(p, n, b, flags);
                            });
}

int mi_icp_remove_none_finite(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                              int remove_nan, int remove_infinite, float* out_xyz, float* out_normals, float* out_colors,
                              int64_t* out_idx, int64_t* m, int mem_kind) {
    const char* what = "remove_none_finite";
    TRY(check_sizes(c, what, n, m, mem_kind));
    return predicate_filter(c, what, xyz, normals, colors, n, out_xyz, out_normals, out_colors, out_idx, m, mem_kind,
                            [&](const float* p, uint32_t* flags) {
                                finite_flags<<<blocks_for(n), 256, 0, c->stream>>>(p, n, remove_nan, remove_infinite, flags);
                            });
}

// ---------------------------------------------------------------------------
// PointCloud::SegmentPlane (geometry/segmentation.cu:187-268; segment_plane.h): every hypothesis drawn up front and
// scored in one pass over the points, the winner chosen on the device, its inlier list and the refit behind it.  Runs
// in the private scratch context; the state, the count and the list come back with the one wait at the end.
int mi_icp_segment_plane(mi_icp_ctx* c, const float* xyz, int64_t n, float distance_threshold, int64_t ransac_n,
                         int64_t num_iterations, uint64_t seed, float* plane4, float* ransac_plane4, int64_t* inliers,
                         int64_t* m, int64_t* best_iteration, int64_t* best_count, int mem_kind) {
    const char* what = "segment_plane";
    // (its own preamble: plane4 is as mandatory as m and is zeroed with it)
    TRY(check_ctx(c, mem_kind, what));
    if (!plane4 || !m) return fail(c, MI_ICP_ERR_INVALID, "%s: plane4 or m is null", what);
    for (int k = 0; k < 4; ++k) {
        plane4[k] = 0.0f;
        if (ransac_plane4) ransac_plane4[k] = 0.0f;
    }
    *m = 0;
    if (best_iteration) *best_iteration = -1;
    if (best_count) *best_count = 0;
    TRY(count_ok(c, what, n));
    if (num_iterations > kSegMaxIterations)
        return fail(c, MI_ICP_ERR_INVALID, "%s: more than %lld iterations are not supported", what, (long long)kSegMaxIterations);
    if (ransac_n < 3 || n < ransac_n) return MI_ICP_OK;  // segmentation.cu:204-212: the zero plane, no inliers
    if (!xyz || !inliers) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const int H = (int)std::max<int64_t>(num_iterations, 0);
    const float thr = distance_threshold;
    return in_scratch(c, what, [&](mi_icp_ctx* a) -> int {
        const float* pts;
        TRY(to_device(a, xyz, (size_t)n * 3, mem_kind, a->stage[0], &pts));
        float4* plane;
        uint32_t *words, *flags, *pos;
        const uint32_t* total;
        double *tie, *sums;
        int64_t* didx;
        const size_t hw = (size_t)std::max(H, 1);
        TRY(ensure(a, a->seg[0], hw, &plane));
        TRY(ensure(a, a->seg[1], 3 * hw + sizeof(SegState) / sizeof(uint32_t), &words));
        TRY(ensure(a, a->seg[2], hw * kSegTieBlocks, &tie));
        TRY(ensure(a, a->seg[3], (size_t)kSegRefitBlocks * 8 + 4, &sums));
        TRY(ensure(a, a->flags, (size_t)n, &flags));
        TRY(out_slot(a, inliers, (size_t)n, mem_kind, a->pairs_out, &didx));
        uint32_t *valid = words, *count = words + hw;
        int32_t* tied_list = (int32_t*)(words + 2 * hw);
        SegState* st = (SegState*)(words + 3 * hw);
        double* centroid = sums + (size_t)kSegRefitBlocks * 8;
        hipStream_t s = a->stream;
        HIPCHK(a, hipMemsetAsync(count, 0, hw * sizeof(uint32_t), s));
        if (H > 0) {
            seg_hypotheses<<<blocks_for(H), 256, 0, s>>>(pts, n, seed, H, plane, valid);
            const int grid = (int)std::min<int64_t>((n + kSegChunk - 1) / kSegChunk, kSegMaxBlocks);
            seg_score<<<grid, 256, 0, s>>>(pts, n, plane, H, thr, count);
        }
        seg_select<<<1, 64, 0, s>>>(count, valid, H, st, tied_list);
        if (H > 1) seg_tie_partial<<<dim3(kSegTieBlocks, std::min(H, 32)), 256, 0, s>>>(pts, n, plane, thr, st, tied_list, tie);
        seg_pick<<<1, 64, 0, s>>>(plane, tied_list, tie, st);
        const int nb = blocks_for(n), rb = std::min(kSegRefitBlocks, nb);
        seg_flags<<<nb, 256, 0, s>>>(pts, n, st, thr, flags);
        TRY(scan_flags(a, flags, n, &pos, &total));
        seg_list<<<nb, 256, 0, s>>>(flags, pos, n, didx);
        seg_centroid_partial<<<rb, 256, 0, s>>>(pts, flags, n, sums);
        seg_centroid_final<<<1, 64, 0, s>>>(sums, rb, centroid);
        seg_moments_partial<<<rb, 256, 0, s>>>(pts, flags, n, centroid, sums);
        seg_refit_final<<<1, 64, 0, s>>>(sums, rb, centroid, st);
        KCHK(a);
        constexpr int kStateWords = (int)(sizeof(SegState) / sizeof(uint32_t));
        static_assert(kStateWords + 1 <= 16, "the state and the count share the 16 pinned words");
        HIPCHK(a, hipMemcpyAsync(a->u_host, st, sizeof(SegState), hipMemcpyDeviceToHost, s));
        TRY(read_total(a, total, kStateWords));
        HIPCHK(a, hipStreamSynchronize(s));
        SegState h;
        std::memcpy(&h, a->u_host, sizeof(h));
        const int64_t cnt = (int64_t)a->u_host[kStateWords];
        if (didx != inliers) {  // staged: a second wait, for the copy to the caller
            TRY(from_device(a, (const int64_t*)didx, inliers, (size_t)cnt, mem_kind));
            HIPCHK(a, hipStreamSynchronize(s));
        }
        std::memcpy(plane4, h.refit, sizeof(h.refit));
        if (ransac_plane4) std::memcpy(ransac_plane4, h.ransac, sizeof(h.ransac));
        *m = cnt;
        if (best_iteration) *best_iteration = h.best;
        if (best_count) *best_count = (int64_t)h.best_count;
        return MI_ICP_OK;
    });
}


// ---------------------------------------------------------------------------
// Colored ICP (registration/colored_icp.cu)
int mi_icp_set_target_colors(mi_icp_ctx* c, const float* rgb, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "set_target_colors"));
    c->t_has_int = c->t_has_grad = false;
    if (!rgb || c->nt <= 0) return MI_ICP_OK;
    if (!c->t_has_nrm)  // the intensities ride in the normals' 4th lane; colored ICP needs normals anyway
        return fail(c, MI_ICP_ERR_STATE, "set_target_colors: the target has no normals");
    const float* d_rgb;
    TRY(to_device(c, rgb, (size_t)c->nt * 3, mem_kind, c->stage[1], &d_rgb));
    target_intensity<<<blocks_for(c->nts), 256, 0, c->stream>>>((const int32_t*)c->tidx.p, d_rgb, (int)c->nts,
                                                              (float4*)c->tnrm.p);
    KCHK(c);
    c->t_has_int = true;
    return MI_ICP_OK;
}

int mi_icp_set_source_colors(mi_icp_ctx* c, const float* rgb, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "set_source_colors"));
    c->s_has_int = false;
    if (!rgb || c->ns <= 0) return MI_ICP_OK;
    const float* d_rgb;
    float* sint;
    TRY(to_device(c, rgb, (size_t)c->ns * 3, mem_kind, c->stage[4], &d_rgb));
    TRY(ensure(c, c->sint, (size_t)c->ns, &sint));
    source_intensity<<<blocks_for(c->ns), 256, 0, c->stream>>>((const int32_t*)c->sperm.p, d_rgb, (int)c->ns, sint);
    KCHK(c);
    c->s_has_int = true;
    return MI_ICP_OK;
}

int mi_icp_set_lambda_geometric(mi_icp_ctx* c, float lambda_geometric) {
    if (!c) return MI_ICP_ERR_INVALID;
    // colored_icp.cu:49-50: out-of-range values fall back to the default
    c->lambda_geometric = (lambda_geometric < 0.0f || lambda_geometric > 1.0f) ? 0.968f : lambda_geometric;
    return MI_ICP_OK;
}

}  // extern "C"
