// mi_voxelgrid.hip -- geometry::VoxelGrid: voxelise a cloud, dense grids, merge, carve, queries, bounds, selections, paint
// (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "select.h"
#include "voxelgrid_kernels.h"

#include <climits>

using namespace mi;
using namespace mi::eng;

// ---------------------------------------------------------------------------
// geometry::VoxelGrid (geometry/voxelgrid.cu, voxelgrid_factory.cu; voxelgrid_kernels.h).  A grid at this boundary is
// keys int32[m][3] + colors float[m][3] on the device and voxel_size / origin on the host: no handle, nothing kept
// between calls but the context's scratch buffers.

static int bit_length(uint64_t v) {
    int b = 0;
    while (v) {
        ++b;
        v >>= 1;
    }
    return b;
}

// Brings equal keys together: keys3[n][3] on the device (x == kVgNoKey: the entry does not count) -> the stable order,
// the runs of equal keys and their number.  Two waits: the extents of the keys size the packed key (the sort's passes),
// the number of runs sizes the caller's output.  Extents that need more than 64 bits together take two sorts.
int mi::eng::vg_sort_runs(mi_icp_ctx* c, const int32_t* keys3, int64_t n, VgRuns* r) {
    *r = VgRuns();
    if (n == 0) return MI_ICP_OK;
    int32_t *part, *bnd;
    TRY(ensure(c, c->bounds_part, (size_t)kVgBlocks * 8, &part));
    TRY(ensure(c, c->bounds, 8, &bnd));
    const int nb = blocks_for(n), rb = std::min(kVgBlocks, nb);
    vg_key_bounds_partial<<<rb, 256, 0, c->stream>>>(keys3, n, part);
    KCHK(c);
    vg_key_bounds_final<<<1, 64, 0, c->stream>>>(part, rb, bnd);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->u_host, bnd, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    int32_t h[8];
    std::memcpy(h, c->u_host, sizeof(h));
    if ((uint32_t)h[6] == 0u) return MI_ICP_OK;  // no entry counts
    VgPack p;
    uint64_t ext[3];
    for (int k = 0; k < 3; ++k) {
        p.lo[k] = h[k];
        ext[k] = (uint64_t)((int64_t)h[3 + k] - (int64_t)h[k]) + 1u;
    }
    const int bx = bit_length(ext[0]), by = bit_length(ext[1] - 1u), bz = bit_length(ext[2] - 1u);  // (x: one slot more)
    const int bits = bx + by + bz;
    p.shift_x = by + bz;
    p.shift_y = bz;
    p.nokey_x = (uint32_t)ext[0];
    SortBuffers sb;
    TRY(sort_buffers(c, n, &sb));
    uint32_t *head, *pos, *run_start;
    const uint32_t* total;
    TRY(ensure(c, c->flags, (size_t)n, &head));
    TRY(ensure(c, c->seg_start, (size_t)n + 1, &run_start));
    uint32_t* const k32 = reinterpret_cast<uint32_t*>(sb.keys[0]);
    if (bits <= 32) {
        vg_pack<uint32_t><<<nb, 256, 0, c->stream>>>(keys3, n, p, kVgWhole, nullptr, k32, sb.vals[0]);
        const int cur = radix_sort_pairs<uint32_t>(c->stream, sb, n, bits);
        KCHK(c);
        const uint32_t* sk = reinterpret_cast<const uint32_t*>(sb.keys[cur]);
        r->order = sb.vals[cur];
        vg_heads_packed<uint32_t><<<nb, 256, 0, c->stream>>>(sk, n, p, head);
        KCHK(c);
        TRY(scan_flags(c, head, n, &pos, &total));
        vg_run_starts_packed<uint32_t><<<nb, 256, 0, c->stream>>>(sk, head, pos, n, p, run_start);
    } else if (bits <= 64) {
        vg_pack<uint64_t><<<nb, 256, 0, c->stream>>>(keys3, n, p, kVgWhole, nullptr, sb.keys[0], sb.vals[0]);
        const int cur = radix_sort_pairs<uint64_t>(c->stream, sb, n, bits);
        KCHK(c);
        const uint64_t* sk = sb.keys[cur];
        r->order = sb.vals[cur];
        vg_heads_packed<uint64_t><<<nb, 256, 0, c->stream>>>(sk, n, p, head);
        KCHK(c);
        TRY(scan_flags(c, head, n, &pos, &total));
        vg_run_starts_packed<uint64_t><<<nb, 256, 0, c->stream>>>(sk, head, pos, n, p, run_start);
    } else {  // (keys inside +-1e9: by + bz <= 62, bx <= 32) two stable sorts, the less significant part first
        vg_pack<uint64_t><<<nb, 256, 0, c->stream>>>(keys3, n, p, kVgLow, nullptr, sb.keys[0], sb.vals[0]);
        int cur = radix_sort_pairs<uint64_t>(c->stream, sb, n, by + bz);
        vg_pack<uint32_t><<<nb, 256, 0, c->stream>>>(keys3, n, p, kVgHigh, sb.vals[cur], k32, sb.vals[0]);
        cur = radix_sort_pairs<uint32_t>(c->stream, sb, n, bx);
        KCHK(c);
        r->order = sb.vals[cur];
        vg_heads<<<nb, 256, 0, c->stream>>>(keys3, r->order, n, head);  // (no one key holds the voxel: the keys themselves)
        KCHK(c);
        TRY(scan_flags(c, head, n, &pos, &total));
        vg_run_starts<<<nb, 256, 0, c->stream>>>(keys3, r->order, head, pos, n, run_start);
    }
    KCHK(c);
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    r->run_start = run_start;
    r->nvox = (int64_t)c->u_host[0];
    return MI_ICP_OK;
}

extern "C" {

int mi_icp_voxelgrid_from_points(mi_icp_ctx* c, const float* xyz, const float* colors, int64_t n, float voxel_size,
                                 const float* min_bound3, const float* max_bound3, int32_t* out_keys, float* out_colors,
                                 int64_t capacity, int64_t* m) {
    const char* what = "voxelgrid_from_points";
    TRY(check_ctx(c));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    TRY(count_ok(c, what, n));
    if (capacity < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: negative capacity", what);
    GridFrame f;
    if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size))
        return fail(c, MI_ICP_ERR_INVALID, "[VoxelGridFromPointCloud] voxel_size <= 0.");
    if (!finite3(min_bound3) || !finite3(max_bound3)) return fail(c, MI_ICP_ERR_INVALID, "%s: a bound is not a number", what);
    TRY(frame_check(c, what, voxel_size, min_bound3, &f));
    const float span = std::max(std::max(max_bound3[0] - min_bound3[0], max_bound3[1] - min_bound3[1]), max_bound3[2] - min_bound3[2]);
    if (voxel_size * (float)INT_MAX < span) return fail(c, MI_ICP_ERR_INVALID, "[VoxelGridFromPointCloud] voxel_size is too small.");
    if (n == 0) return MI_ICP_OK;
    if (!xyz) return fail(c, MI_ICP_ERR_INVALID, "%s: null points", what);
    int32_t* keys3;
    TRY(ensure(c, c->stage[3], (size_t)n * 3, &keys3));
    vg_point_keys<<<blocks_for(n), 256, 0, c->stream>>>(xyz, n, f, keys3);
    KCHK(c);
    VgRuns r;
    TRY(vg_sort_runs(c, keys3, n, &r));
    *m = r.nvox;
    if (r.nvox == 0 || capacity < r.nvox) return MI_ICP_OK;  // nothing is written: the caller learns the room to make
    if (!out_keys || !out_colors) return fail(c, MI_ICP_ERR_INVALID, "%s: null output", what);
    vg_emit_keys<<<blocks_for(r.nvox), 256, 0, c->stream>>>(keys3, r.order, r.run_start, r.nvox, out_keys);
    KCHK(c);
    vg_run_color_means<<<blocks_for(r.nvox), 256, 0, c->stream>>>(colors, r.order, r.run_start, r.nvox, out_colors);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_voxelgrid_dense(mi_icp_ctx* c, int num_w, int num_h, int num_d, int32_t* out_keys, float* out_colors, int64_t capacity,
                           int64_t* m) {
    const char* what = "voxelgrid_dense";
    TRY(check_ctx(c));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    if (capacity < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: negative capacity", what);
    if (num_w <= 0 || num_h <= 0 || num_d <= 0) return MI_ICP_OK;
    // (each factor is below 2^31, so the first product is exact in 64 bits and the second is compared before it is made)
    const int64_t wh = (int64_t)num_w * num_h;
    if (wh > (int64_t)INT_MAX || wh * num_d > (int64_t)INT_MAX)
        return fail(c, MI_ICP_ERR_INVALID, "%s: %d x %d x %d voxels are more than 2^31 - 1", what, num_w, num_h, num_d);
    const int64_t total = wh * num_d;
    *m = total;
    if (capacity < total) return MI_ICP_OK;
    if (!out_keys || !out_colors) return fail(c, MI_ICP_ERR_INVALID, "%s: null output", what);
    vg_dense<<<blocks_for(total), 256, 0, c->stream>>>(total, num_h, num_d, out_keys, out_colors);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_voxelgrid_merge(mi_icp_ctx* c, const int32_t* keys_a, const float* colors_a, int64_t m_a, const int32_t* keys_b,
                           const float* colors_b, int64_t m_b, int mode, int32_t* out_keys, float* out_colors, int64_t capacity,
                           int64_t* m) {
    const char* what = "voxelgrid_merge";
    TRY(check_ctx(c));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    TRY(count_ok(c, what, m_a));
    TRY(count_ok(c, what, m_b));
    TRY(count_ok(c, what, m_a + m_b));
    if (capacity < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: negative capacity", what);
    if (mode != MI_ICP_VOXELGRID_AVERAGE && mode != MI_ICP_VOXELGRID_KEEP_FIRST)
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad mode", what);
    if ((m_a > 0 && (!keys_a || !colors_a)) || (m_b > 0 && (!keys_b || !colors_b)))
        return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const int64_t n = m_a + m_b;
    if (n == 0) return MI_ICP_OK;
    // A then B, side by side in scratch: the stable sort keeps that order inside a run
    int32_t* keys3;
    float* cols;
    TRY(ensure(c, c->stage[3], (size_t)n * 3, &keys3));
    TRY(ensure(c, c->stage[4], (size_t)n * 3, &cols));
    const size_t row = 3 * sizeof(int32_t);
    if (m_a > 0) {
        HIPCHK(c, hipMemcpyAsync(keys3, keys_a, (size_t)m_a * row, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(cols, colors_a, (size_t)m_a * row, hipMemcpyDeviceToDevice, c->stream));
    }
    if (m_b > 0) {
        HIPCHK(c, hipMemcpyAsync(keys3 + m_a * 3, keys_b, (size_t)m_b * row, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(cols + m_a * 3, colors_b, (size_t)m_b * row, hipMemcpyDeviceToDevice, c->stream));
    }
    VgRuns r;
    TRY(vg_sort_runs(c, keys3, n, &r));
    *m = r.nvox;
    if (r.nvox == 0 || capacity < r.nvox) return MI_ICP_OK;
    if (!out_keys || !out_colors) return fail(c, MI_ICP_ERR_INVALID, "%s: null output", what);
    vg_emit_keys<<<blocks_for(r.nvox), 256, 0, c->stream>>>(keys3, r.order, r.run_start, r.nvox, out_keys);
    KCHK(c);
    vg_merge_colors<<<blocks_for(r.nvox), 256, 0, c->stream>>>(cols, r.order, r.run_start, r.nvox, mode, out_colors);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_voxelgrid_carve(mi_icp_ctx* c, const int32_t* keys, const float* colors, int64_t m, float voxel_size,
                           const float* origin3, const void* image, int width, int height, int channels, int bytes_per_channel,
                           const float* intrinsic4, const float* extrinsic16, int keep_voxels_outside_image, int32_t* out_keys,
                           float* out_colors, int64_t* m_out) {
    const char* what = "voxelgrid_carve";
    TRY(check_ctx(c));
    if (!m_out) return fail(c, MI_ICP_ERR_INVALID, "%s: m_out is null", what);
    *m_out = 0;
    TRY(count_ok(c, what, m));
    GridFrame f;
    TRY(frame_check(c, what, voxel_size, origin3, &f));
    if (width < 2 || height < 2) return fail(c, MI_ICP_ERR_INVALID, "%s: the image must be at least 2 x 2", what);
    if (channels < 1 || bytes_per_channel < 1 || !intrinsic4) return fail(c, MI_ICP_ERR_INVALID, "%s: bad image or camera", what);
    VgCamera cam;
    std::memset(&cam, 0, sizeof(cam));
    cam.K[0] = intrinsic4[0];
    cam.K[4] = intrinsic4[1];
    cam.K[2] = intrinsic4[2];
    cam.K[5] = intrinsic4[3];
    cam.K[8] = 1.0f;
    for (int r = 0; r < 3; ++r) {  // extrinsic16: column-major (Eigen::Matrix4f::data()); null: the identity
        for (int q = 0; q < 3; ++q) cam.R[r * 3 + q] = extrinsic16 ? extrinsic16[q * 4 + r] : (r == q ? 1.0f : 0.0f);
        cam.t[r] = extrinsic16 ? extrinsic16[12 + r] : 0.0f;
    }
    cam.width = width;
    cam.height = height;
    cam.float_image = (channels == 1 && bytes_per_channel == 4) ? 1 : 0;
    cam.keep_outside = keep_voxels_outside_image ? 1 : 0;
    if (m == 0) return MI_ICP_OK;
    if (!keys || !colors || !out_keys || !out_colors || (cam.float_image && !image))
        return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    uint32_t *flags, *pos;
    const uint32_t* total;
    TRY(ensure(c, c->flags, (size_t)m, &flags));
    vg_carve_flags<<<blocks_for(m), 256, 0, c->stream>>>(keys, m, f, cam, (const float*)image, flags);
    KCHK(c);
    TRY(scan_flags(c, flags, m, &pos, &total));
    select_gather<int32_t><<<blocks_for(m), 256, 0, c->stream>>>(flags, pos, m, keys, nullptr, colors, out_keys, nullptr, out_colors, nullptr);
    KCHK(c);
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *m_out = (int64_t)c->u_host[0];
    return MI_ICP_OK;
}

int mi_icp_voxelgrid_query(mi_icp_ctx* c, const int32_t* keys, int64_t m, int keys_sorted, float voxel_size, const float* origin3,
                           const float* queries, int64_t nq, uint8_t* out_included, int32_t* out_index) {
    const char* what = "voxelgrid_query";
    TRY(check_ctx(c));
    TRY(count_ok(c, what, m));
    TRY(count_ok(c, what, nq));
    GridFrame f;
    TRY(frame_check(c, what, voxel_size, origin3, &f));
    if (nq == 0) return MI_ICP_OK;
    if (!queries || !out_included || (m > 0 && !keys)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const int32_t* sorted = keys;
    int64_t ms = m;
    if (m > 1 && !keys_sorted) {  // a scratch copy, sorted once (and distinct)
        VgRuns r;
        TRY(vg_sort_runs(c, keys, m, &r));
        int32_t* tmp;
        TRY(ensure(c, c->stage[3], (size_t)m * 3, &tmp));
        vg_emit_keys<<<blocks_for(r.nvox), 256, 0, c->stream>>>(keys, r.order, r.run_start, r.nvox, tmp);
        KCHK(c);
        sorted = tmp;
        ms = r.nvox;
    }
    vg_query<<<blocks_for(nq), 256, 0, c->stream>>>(sorted, ms, f, queries, nq, out_included, out_index);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_voxelgrid_bounds(mi_icp_ctx* c, const int32_t* keys, int64_t m, float voxel_size, const float* origin3,
                            int32_t* out_min_index3, int32_t* out_max_index3, double* out_center_sum3) {
    const char* what = "voxelgrid_bounds";
    TRY(check_ctx(c));
    TRY(count_ok(c, what, m));
    if (!out_min_index3 || !out_max_index3 || !out_center_sum3) return fail(c, MI_ICP_ERR_INVALID, "%s: null output", what);
    if (m == 0) return fail(c, MI_ICP_ERR_INVALID, "%s: an empty grid has no index bounds", what);
    if (!keys) return fail(c, MI_ICP_ERR_INVALID, "%s: null keys", what);
    // (voxel_size may be anything finite here: Clear() leaves 0, Scale may make it negative)
    if (!std::isfinite(voxel_size) || !finite3(origin3)) return fail(c, MI_ICP_ERR_INVALID, "%s: voxel_size or origin is not finite", what);
    GridFrame f;
    f.vs = voxel_size;
    for (int k = 0; k < 3; ++k) f.origin[k] = origin3[k];
    int32_t *ipart, *iout;
    double *dpart, *dout;
    TRY(ensure(c, c->bounds_part, (size_t)kVgBlocks * 8 + 8, &ipart));
    TRY(ensure(c, c->partial, (size_t)kVgBlocks * 4 + 4, &dpart));
    iout = ipart + (size_t)kVgBlocks * 8;
    dout = dpart + (size_t)kVgBlocks * 4;
    const int rb = std::min(kVgBlocks, blocks_for(m));
    vg_bounds_partial<<<rb, 256, 0, c->stream>>>(keys, m, f, ipart, dpart);
    KCHK(c);
    vg_bounds_final<<<1, 64, 0, c->stream>>>(ipart, dpart, rb, iout, dout);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->u_host, iout, 6 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->sys_host, dout, 3 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::memcpy(out_min_index3, c->u_host, 3 * sizeof(int32_t));
    std::memcpy(out_max_index3, c->u_host + 3, 3 * sizeof(int32_t));
    std::memcpy(out_center_sum3, c->sys_host, 3 * sizeof(double));
    return MI_ICP_OK;
}

// VoxelGrid::SelectByIndex (voxelgrid.cu:432-475): the rules of mi_icp_select_by_index, on keys + colours
int mi_icp_voxelgrid_select_by_index(mi_icp_ctx* c, const int32_t* keys, const float* colors, int64_t m, const int64_t* indices,
                                     int64_t n_indices, int invert, int32_t* out_keys, float* out_colors, int64_t* m_out) {
    const char* what = "voxelgrid_select_by_index";
    TRY(check_ctx(c));
    if (!m_out) return fail(c, MI_ICP_ERR_INVALID, "%s: m_out is null", what);
    *m_out = 0;
    TRY(count_ok(c, what, m));
    TRY(count_ok(c, what, n_indices));
    if ((m > 0 && (!keys || !colors)) || (n_indices > 0 && !indices)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const int64_t count = invert ? m : n_indices;
    if (count > 0 && (!out_keys || !out_colors)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    if (m == 0 && n_indices > 0) return fail(c, MI_ICP_ERR_INVALID, "%s: index out of range [0, 0)", what);
    if (count == 0) return MI_ICP_OK;
    uint32_t* flags;
    TRY(ensure(c, c->flags, (size_t)m + 1, &flags));  // [m]: the status word
    uint32_t* status = flags + m;
    HIPCHK(c, hipMemsetAsync(status, 0, sizeof(uint32_t), c->stream));
    int64_t got = n_indices;
    if (!invert) {
        select_list<int32_t><<<blocks_for(n_indices), 256, 0, c->stream>>>(indices, n_indices, m, keys, nullptr, colors, out_keys, nullptr,
                                                                          out_colors, status);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(c->u_host + 1, status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)flags, 1, (size_t)m, c->stream));
        if (n_indices > 0) {
            select_mark<<<blocks_for(n_indices), 256, 0, c->stream>>>(indices, n_indices, m, flags, status);
            KCHK(c);
        }
        uint32_t* pos;
        const uint32_t* total;
        TRY(scan_flags(c, flags, m, &pos, &total));
        select_gather<int32_t><<<blocks_for(m), 256, 0, c->stream>>>(flags, pos, m, keys, nullptr, colors, out_keys, nullptr, out_colors, nullptr);
        KCHK(c);
        TRY(read_total(c, total));
        HIPCHK(c, hipMemcpyAsync(c->u_host + 1, status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        got = (int64_t)c->u_host[0];
    }
    if (c->u_host[1]) return fail(c, MI_ICP_ERR_INVALID, "%s: index out of range [0, %lld)", what, (long long)m);
    *m_out = got;
    return MI_ICP_OK;
}

// PaintUniformColor (indices == NULL) / PaintIndexedColor (voxelgrid.cu:321-336); an index outside [0, m) is an error and
// nothing is painted
int mi_icp_voxelgrid_paint(mi_icp_ctx* c, float* colors, int64_t m, const int64_t* indices, int64_t n_indices, const float* color3) {
    const char* what = "voxelgrid_paint";
    TRY(check_ctx(c));
    TRY(count_ok(c, what, m));
    TRY(count_ok(c, what, n_indices));
    if (!color3) return fail(c, MI_ICP_ERR_INVALID, "%s: null colour", what);
    if (!indices && n_indices > 0) return fail(c, MI_ICP_ERR_INVALID, "%s: null indices", what);
    const int64_t count = indices ? n_indices : m;
    if (count == 0) return MI_ICP_OK;
    if (m == 0) return fail(c, MI_ICP_ERR_INVALID, "%s: index out of range [0, 0)", what);
    if (!colors) return fail(c, MI_ICP_ERR_INVALID, "%s: null colours", what);
    if (indices) {
        uint32_t* status;
        TRY(ensure(c, c->flags, 1, &status));
        HIPCHK(c, hipMemsetAsync(status, 0, sizeof(uint32_t), c->stream));
        vg_check_indices<<<blocks_for(n_indices), 256, 0, c->stream>>>(indices, n_indices, m, status);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(c->u_host, status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->u_host[0]) return fail(c, MI_ICP_ERR_INVALID, "%s: index out of range [0, %lld)", what, (long long)m);
    }
    vg_paint<<<blocks_for(count), 256, 0, c->stream>>>(colors, indices, count, color3[0], color3[1], color3[2]);
    KCHK(c);
    return MI_ICP_OK;
}

}  // extern "C"
