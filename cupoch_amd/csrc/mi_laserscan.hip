// mi_laserscan.hip -- geometry::LaserScanBuffer: scans to points, points and depth frames to scans, the range and shadow
// filters (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "laserscan_kernels.h"

using namespace mi;
using namespace mi::eng;

// ---------------------------------------------------------------------------
// The contract is in include/mi_icp.h ("laserscan"), the kernels in laserscan_kernels.h.  Scratch: flags the per-reading
// keep flags of to_points, dense_idx their positions, stage[0] the cos / sin table, stage[1] the live scans' origins.
// A call that uploads a host table waits before it returns, so the table may go.

static int upload(mi_icp_ctx* c, DevBuf& b, const std::vector<float>& v, const float** out) {
    float* d;
    TRY(ensure(c, b, v.size(), &d));
    HIPCHK(c, hipMemcpyAsync(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice, c->stream));
    *out = d;
    return MI_ICP_OK;
}

static float scan_increment(float min_angle, float max_angle, int num_steps) { return (max_angle - min_angle) / (float)(num_steps - 1); }

// the factories' common checks; `a` filled
static int bins_open(mi_icp_ctx* c, const char* what, float angle_inc, float min_h, float max_h, int32_t divisions, float min_r,
                     float max_r, float min_a, float max_a, int32_t num_steps, LsBins* a) {
    if (!(angle_inc > 0.0f)) return fail(c, MI_ICP_ERR_INVALID, "%s: angle_increment must be positive", what);
    if (!(min_h < max_h)) return fail(c, MI_ICP_ERR_INVALID, "%s: the lower height limit must be smaller than the upper", what);
    if (!(min_r < max_r)) return fail(c, MI_ICP_ERR_INVALID, "%s: min_range must be smaller than max_range", what);
    if (!(min_a < max_a)) return fail(c, MI_ICP_ERR_INVALID, "%s: min_angle must be smaller than max_angle", what);
    if (divisions < 1) return fail(c, MI_ICP_ERR_INVALID, "%s: num_vertical_divisions below 1", what);
    const float q = ceilf((max_a - min_a) / angle_inc);
    if (!(q >= 1.0f && q <= (float)kLsMaxBins) || num_steps != (int32_t)q)
        return fail(c, MI_ICP_ERR_INVALID, "%s: num_steps is not (int)ceilf((max_angle - min_angle) / angle_increment) in [1, %d]", what, kLsMaxBins);
    if ((int64_t)num_steps * divisions > (int64_t)kLsMaxBins) return fail(c, MI_ICP_ERR_INVALID, "%s: more than %d bins", what, kLsMaxBins);
    a->min_h = min_h;
    a->h_inc = (max_h - min_h) / (float)divisions;
    if (!(a->h_inc > 0.0f && a->h_inc < INFINITY)) return fail(c, MI_ICP_ERR_INVALID, "%s: the height increment is not a positive number", what);
    a->min_r = min_r;
    a->max_r = max_r;
    a->min_a = min_a;
    a->max_a = max_a;
    a->a_inc = angle_inc;
    a->divisions = divisions;
    a->steps = num_steps;
    return MI_ICP_OK;
}

// NaN bins, then the minimum of n items of `src` per bin; *info = the path (0 LDS, 1 global)
template <class Source>
static int bins_run(mi_icp_ctx* c, const Source& src, int64_t n, const LsBins& a, float* out_ranges, int32_t* info) {
    const int64_t bins = (int64_t)a.divisions * a.steps;
    uint32_t* out = reinterpret_cast<uint32_t*>(out_ranges);
    ls_fill_u32<<<blocks_for(bins), 256, 0, c->stream>>>(out, bins, kLsNaN);
    KCHK(c);
    const bool lds = bins <= (int64_t)kLsLdsBins;
    if (info) *info = lds ? 0 : 1;
    if (n == 0) return MI_ICP_OK;
    if (lds) {
        int dev_cus = 256;
        (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, c->device);
        const int64_t want = (n + (int64_t)kLsThreads * kLsPerThread - 1) / ((int64_t)kLsThreads * kLsPerThread);
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(want, 2 * (int64_t)std::max(dev_cus, 1)));
        const int64_t per_block = (n + blocks - 1) / blocks;
        ls_bin_lds<Source><<<(int)blocks, kLsThreads, 0, c->stream>>>(src, n, per_block, a, out);
    } else {
        ls_bin_global<Source><<<blocks_for(n), 256, 0, c->stream>>>(src, n, a, out);
    }
    KCHK(c);
    return MI_ICP_OK;
}

extern "C" {

int mi_icp_laserscan_limits(int64_t* lds_max_bins, int64_t* max_bins) {
    if (lds_max_bins) *lds_max_bins = kLsLdsBins;
    if (max_bins) *max_bins = kLsMaxBins;
    return MI_ICP_OK;
}

int mi_icp_laserscan_to_points(mi_icp_ctx* c, const float* ranges, const float* intensities, const float* origins,
                               int32_t num_steps, int32_t num_max_scans, int32_t first_slot, int32_t num_scans, float min_angle,
                               float max_angle, float min_range, float max_range, float* out_xyz, float* out_colors,
                               int64_t capacity, int64_t* m) {
    const char* what = "laserscan_to_points";
    TRY(check_ctx(c));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    if (num_steps < 2) return fail(c, MI_ICP_ERR_INVALID, "%s: num_steps below 2", what);
    if (num_max_scans < 1 || num_scans < 0 || num_scans > num_max_scans || first_slot < 0 || first_slot >= num_max_scans || capacity < 0)
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad ring arguments", what);
    const int64_t count = (int64_t)num_scans * num_steps;
    if ((int64_t)num_max_scans * num_steps > kMaxCount) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    if (!(min_range < max_range) || count == 0) return MI_ICP_OK;
    if (!ranges || !origins) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);

    const float inc = scan_increment(min_angle, max_angle, num_steps);
    std::vector<float> cs((size_t)num_steps * 2), org((size_t)num_scans * 12, 0.0f);
    for (int i = 0; i < num_steps; ++i) {
        const float ang = min_angle + (float)i * inc;
        cs[(size_t)i * 2] = (float)std::cos((double)ang);
        cs[(size_t)i * 2 + 1] = (float)std::sin((double)ang);
    }
    for (int k = 0; k < num_scans; ++k) {
        const float* O = origins + (size_t)((first_slot + k) % num_max_scans) * 16;  // column-major: O(r, col) = O[col * 4 + r]
        for (int r = 0; r < 3; ++r) {
            org[(size_t)k * 12 + r * 3] = O[r];
            org[(size_t)k * 12 + r * 3 + 1] = O[4 + r];
            org[(size_t)k * 12 + r * 3 + 2] = O[12 + r];
        }
    }
    LsScans a;
    a.ranges = ranges;
    a.intensities = intensities;
    TRY(upload(c, c->stage[0], cs, &a.cs));
    TRY(upload(c, c->stage[1], org, &a.origins));
    a.steps = num_steps;
    a.max_scans = num_max_scans;
    a.first = first_slot;
    a.scans = num_scans;
    a.min_r = min_range;
    a.max_r = max_range;
    uint32_t *flags, *pos;
    const uint32_t* total;
    TRY(ensure(c, c->flags, (size_t)count, &flags));
    ls_point_flags<<<blocks_for(count), 256, 0, c->stream>>>(a, count, flags);
    KCHK(c);
    TRY(scan_flags(c, flags, count, &pos, &total));
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t cnt = (int64_t)c->u_host[0];
    *m = cnt;
    if (cnt == 0 || capacity < cnt) return MI_ICP_OK;
    if (!out_xyz || (intensities && !out_colors)) return fail(c, MI_ICP_ERR_INVALID, "%s: null output", what);
    ls_point_emit<<<blocks_for(count), 256, 0, c->stream>>>(a, count, pos, out_xyz, intensities ? out_colors : nullptr);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_laserscan_from_points(mi_icp_ctx* c, const float* points, int64_t n, float angle_increment, float min_height,
                                 float max_height, int32_t num_vertical_divisions, float min_range, float max_range,
                                 float min_angle, float max_angle, int32_t num_steps, float* out_ranges, int32_t* info) {
    const char* what = "laserscan_from_points";
    TRY(check_ctx(c));
    if (info) *info = -1;
    TRY(count_ok(c, what, n));
    LsBins a;
    TRY(bins_open(c, what, angle_increment, min_height, max_height, num_vertical_divisions, min_range, max_range, min_angle,
                  max_angle, num_steps, &a));
    if (!out_ranges || (n > 0 && !points)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    LsPointSource src{points};
    return bins_run(c, src, n, a, out_ranges, info);
}

int mi_icp_laserscan_from_depth(mi_icp_ctx* c, const void* depth, int depth_type, int width, int height, const float* intrinsic4,
                                float depth_scale, float depth_trunc, int stride, float angle_increment, float min_y, float max_y,
                                int32_t num_vertical_divisions, float min_range, float max_range, float min_angle,
                                float max_angle, int32_t num_steps, float* out_ranges, int32_t* info) {
    const char* what = "laserscan_from_depth";
    TRY(check_ctx(c));
    if (info) *info = -1;
    if (width < 0 || height < 0 || stride < 1 || !intrinsic4 || (depth_type != MI_ICP_DEPTH_F32 && depth_type != MI_ICP_DEPTH_U16))
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad arguments", what);
    if ((int64_t)width * height > kMaxCount) return fail(c, MI_ICP_ERR_INVALID, "%s: image too large", what);
    LsBins a;
    TRY(bins_open(c, what, angle_increment, min_y, max_y, num_vertical_divisions, min_range, max_range, min_angle, max_angle,
                  num_steps, &a));
    const int64_t count = (int64_t)(width / stride) * (height / stride);
    if (!out_ranges || (count > 0 && !depth)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    LsDepthSource src;
    std::memset(&src, 0, sizeof(src));
    src.d.depth = depth;
    src.d.width = width;
    src.d.height = height;
    src.d.stride = stride;
    src.d.depth_u16 = depth_type == MI_ICP_DEPTH_U16;
    src.d.depth_recip = depth_reciprocal((int)depth_scale);
    src.d.depth_trunc = (int)depth_trunc;
    src.d.fx = intrinsic4[0];
    src.d.fy = intrinsic4[1];
    src.d.cx = intrinsic4[2];
    src.d.cy = intrinsic4[3];
    return bins_run(c, src, count, a, out_ranges, info);
}

int mi_icp_laserscan_range_filter(mi_icp_ctx* c, const float* ranges, int64_t count, float min_range, float max_range,
                                  float* out_ranges) {
    const char* what = "laserscan_range_filter";
    TRY(check_ctx(c));
    TRY(count_ok(c, what, count));
    if (count == 0) return MI_ICP_OK;
    if (!ranges || !out_ranges) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    ls_range_filter<<<blocks_for(count), 256, 0, c->stream>>>(ranges, count, min_range, max_range, out_ranges);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_laserscan_shadow_filter(mi_icp_ctx* c, const float* ranges, int32_t num_steps, int32_t num_rows, float scan_min_angle,
                                   float scan_max_angle, float min_angle, float max_angle, int32_t window, int32_t neighbors,
                                   int remove_shadow_start_point, float* out_ranges) {
    const char* what = "laserscan_shadow_filter";
    TRY(check_ctx(c));
    if (num_steps < 2) return fail(c, MI_ICP_ERR_INVALID, "%s: num_steps below 2", what);
    if (num_rows < 0 || window < 0 || neighbors < 0 || window > (1 << 20) || (int64_t)num_rows * num_steps > kMaxCount)
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    const int64_t count = (int64_t)num_rows * num_steps;
    if (count == 0) return MI_ICP_OK;
    if (!ranges || !out_ranges || ranges == out_ranges) return fail(c, MI_ICP_ERR_INVALID, "%s: null or aliased buffer", what);
    const float min_tan = std::fabs((float)std::tan((double)min_angle));
    const float max_tan = -std::fabs((float)std::tan((double)max_angle));
    const float inc = scan_increment(scan_min_angle, scan_max_angle, num_steps);
    std::vector<float> cs((size_t)(2 * window + 1) * 2);
    for (int y = -window; y <= window; ++y) {
        const float ang = (float)y * inc;
        cs[(size_t)(y + window) * 2] = (float)std::cos((double)ang);
        cs[(size_t)(y + window) * 2 + 1] = (float)std::sin((double)ang);
    }
    const float* dcs;
    TRY(upload(c, c->stage[0], cs, &dcs));
    HIPCHK(c, hipMemcpyAsync(out_ranges, ranges, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    ls_shadow_filter<<<blocks_for(count), 256, 0, c->stream>>>(ranges, count, num_steps, window, neighbors,
                                                                remove_shadow_start_point ? 1 : 0, min_tan, max_tan, dcs, out_ranges);
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

int mi_icp_laserscan_scale(mi_icp_ctx* c, float* ranges, int64_t count, float scale) {
    const char* what = "laserscan_scale";
    TRY(check_ctx(c));
    TRY(count_ok(c, what, count));
    if (count == 0) return MI_ICP_OK;
    if (!ranges) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    ls_scale<<<blocks_for(count), 256, 0, c->stream>>>(ranges, count, scale);
    KCHK(c);
    return MI_ICP_OK;
}

}  // extern "C"
