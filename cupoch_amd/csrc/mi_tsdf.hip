// mi_tsdf.hip -- integration::UniformTSDFVolume: integrate, raycast, extract clouds
// (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "select.h"
#include "tsdf_host.h"

using namespace mi;
using namespace mi::eng;
using host::Mat4;

// ---------------------------------------------------------------------------
// integration::UniformTSDFVolume (integration/uniform_tsdfvolume.cu; tsdf_kernels.h).  A volume belongs to the context
// that made it and is freed with it at the latest.
struct mi_icp_tsdf {
    mi_icp_ctx* owner = nullptr;
    TsdfVol v = {};
    float length = 0.0f, sdf_trunc = 0.0f;
    DevBuf planes;  // tsdf, weight and, with a colour type, three colour planes
    TsdfMult mult;
    void free_buffers() {
        release(planes);
        release(mult.buf);
    }
};

void mi::eng::tsdf_release_all(mi_icp_ctx* c) { handle_release_all(c->tsdf_volumes); }

static int tsdf_check(mi_icp_ctx* c, const mi_icp_tsdf* t, const char* what) {
    return handle_check(c, t, c->tsdf_volumes, what, "volume");
}

static_assert(kTsdfMaxLevels == MI_ICP_TSDF_MAX_LEVELS, "the kernel's level table holds every level of the C ABI");

// Raycast for `levels` levels of the camera's pyramid in one pass (include/mi_icp.h "Raycast", "raycast_levels"): one
// tsdf_raycast launch over the tiles of every level, and with valid_only one finite_flags, one scan and one
// select_gather over the concatenated pixels; m[i] = the points of level i.  mi_icp_tsdf_raycast is levels == 1.
static int tsdf_raycast_levels(mi_icp_ctx* c, mi_icp_tsdf* t, const char* what, int levels, int width, int height,
                               const float* intrinsic4, const float* extrinsic, float sdf_trunc, int valid_only,
                               float* const out[3], int64_t capacity, int64_t* m, int mem_kind) {
    TRY(tsdf_extract_args(c, t, c->tsdf_volumes, what, capacity, m, mem_kind));
    if (levels < 1 || levels > MI_ICP_TSDF_MAX_LEVELS)
        return fail(c, MI_ICP_ERR_INVALID, "%s: levels must be in [1, %d]", what, MI_ICP_TSDF_MAX_LEVELS);
    for (int i = 0; i < levels; ++i) m[i] = 0;
    if (!intrinsic4 || width < 0 || height < 0 || width > MI_ICP_TSDF_MAX_IMAGE_SIDE || height > MI_ICP_TSDF_MAX_IMAGE_SIDE)
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad arguments (an image side is at most %d)", what, MI_ICP_TSDF_MAX_IMAGE_SIDE);
    // the march takes length * sqrt(2) / (sdf_trunc / 2) steps at most
    if (!(sdf_trunc > 0.0f) || !std::isfinite(sdf_trunc) ||
        !((double)t->v.res * t->v.voxel_length * 1.4142136 / (0.5 * (double)sdf_trunc) <= (double)MI_ICP_TSDF_MAX_MARCH))
        return fail(c, MI_ICP_ERR_INVALID, "%s: sdf_trunc must be positive and at least length * sqrt(2) * 2 / %d", what,
                    MI_ICP_TSDF_MAX_MARCH);

    TsdfRaycast a = {};
    const Mat4 E = load_T(extrinsic);
    // utility::InverseTransform: R^T and -(R^T t), the sums left to right
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) a.R[r][k] = E.data()[r * 4 + k];  // R^T[r][k] = E(k, r)
        const float t0 = E.data()[12], t1 = E.data()[13], t2 = E.data()[14];
        const float p = ((-a.R[r][0]) * t0 + (-a.R[r][1]) * t1) + (-a.R[r][2]) * t2;
        a.t[r] = p - t->v.origin[r];
    }
    a.sdf_trunc = sdf_trunc;
    a.levels = levels;
    // the levels' cameras (PinholeCameraIntrinsic::CreatePyramidLevel), tiles and pixels, one level after the other
    int64_t npix = 0, ntiles = 0;
    for (int i = 0; i < levels; ++i) {
        TsdfRayLevel& L = a.level[i];
        const float s = i == 0 ? 1.0f : powf(0.5f, (float)i);
        L.fx = i == 0 ? intrinsic4[0] : intrinsic4[0] * s;
        L.fy = i == 0 ? intrinsic4[1] : intrinsic4[1] * s;
        L.cx = i == 0 ? intrinsic4[2] : (intrinsic4[2] + 0.5f) * s - 0.5f;
        L.cy = i == 0 ? intrinsic4[3] : (intrinsic4[3] + 0.5f) * s - 0.5f;
        L.width = width >> i;
        L.height = height >> i;
        L.tiles_x = (L.width + 15) / 16;
        L.first_tile = (int)ntiles;
        L.first_pixel = npix;
        m[i] = (int64_t)L.width * L.height;  // (valid_only: until the counts are known)
        npix += m[i];
        ntiles += m[i] ? (int64_t)L.tiles_x * ((L.height + 15) / 16) : 0;
    }
    if (npix == 0) return MI_ICP_OK;  // (the sides are at most 2^15: npix < 2^31 and ntiles < 2^23)

    if (!valid_only) {  // every pixel stays, an invalid one as NaN
        if (capacity < npix) return MI_ICP_OK;
        if (!out[0] || !out[1] || !out[2]) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
        return cloud_emit(c, out, out, npix, npix, mem_kind, c->vpay, [&](float* const dst[3]) {
            tsdf_raycast<<<(unsigned)ntiles, 256, 0, c->stream>>>(t->v, a, dst[0], dst[1], dst[2]);
        });
    }
    for (int i = 0; i < levels; ++i) m[i] = 0;
    float* raw[3];
    for (int k = 0; k < 3; ++k) TRY(ensure(c, c->stage[3 + k], (size_t)npix * 3, &raw[k]));
    uint32_t *flags, *pos;
    TRY(ensure(c, c->flags, (size_t)npix + MI_ICP_TSDF_MAX_LEVELS, &flags));  // and, behind them, the levels' ends
    uint32_t* const ends = flags + npix;
    tsdf_raycast<<<(unsigned)ntiles, 256, 0, c->stream>>>(t->v, a, raw[0], raw[1], raw[2]);
    KCHK(c);
    finite_flags<<<blocks_for(npix), 256, 0, c->stream>>>(raw[0], npix, 1, 1, flags);  // RemoveNoneFinitePoints(true, true)
    KCHK(c);
    // the counts before anything is written (the capacity rule), all levels' in one read-back
    const uint32_t* total;
    TRY(scan_flags(c, flags, npix, &pos, &total));
    tsdf_level_ends<<<1, 64, 0, c->stream>>>(a, npix, pos, total, ends);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->u_host, ends, (size_t)levels * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int i = 0; i < levels; ++i) m[i] = (int64_t)c->u_host[i] - (i ? (int64_t)c->u_host[i - 1] : 0);
    const int64_t cnt = (int64_t)c->u_host[levels - 1];
    if (cnt == 0 || capacity < cnt) return MI_ICP_OK;
    if (!out[0] || !out[1] || !out[2]) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    return cloud_emit(c, out, out, cnt, cnt, mem_kind, c->vpay, [&](float* const dst[3]) {
        select_gather<<<blocks_for(npix), 256, 0, c->stream>>>(flags, pos, npix, raw[0], raw[1], raw[2], dst[0], dst[1], dst[2],
                                                              (int64_t*)nullptr);
    });
}

extern "C" {

int mi_icp_tsdf_create(mi_icp_ctx* c, float length, int resolution, float sdf_trunc, int color_type, const float* origin3,
                       mi_icp_tsdf** out) {
    TRY(check_ctx(c));
    if (!out) return fail(c, MI_ICP_ERR_INVALID, "tsdf_create: out is null");
    *out = nullptr;
    if (!(length > 0.0f) || !std::isfinite(length) || resolution < 3 || resolution > MI_ICP_TSDF_MAX_RESOLUTION ||
        !(sdf_trunc > 0.0f) || !std::isfinite(sdf_trunc) ||
        (color_type != MI_ICP_TSDF_NO_COLOR && color_type != MI_ICP_TSDF_RGB8 && color_type != MI_ICP_TSDF_GRAY32))
        return fail(c, MI_ICP_ERR_INVALID, "tsdf_create: bad arguments");
    mi_icp_tsdf* t = new mi_icp_tsdf;
    t->owner = c;
    t->length = length;
    t->sdf_trunc = sdf_trunc;
    TsdfVol& v = t->v;
    v.res = resolution;
    v.h_res = resolution / 2;
    const int64_t n = (int64_t)resolution * resolution * resolution;
    v.voxel_length = length / (float)resolution;
    v.half = 0.5f * v.voxel_length;
    for (int k = 0; k < 3; ++k) v.origin[k] = origin3 ? origin3[k] : 0.0f;
    float* base;
    const int rc = ensure(c, t->planes, (size_t)n * (color_type == MI_ICP_TSDF_NO_COLOR ? 2 : 5), &base);
    if (rc != MI_ICP_OK) {
        delete t;
        return rc;
    }
    v.p = {base, base + n, color_type == MI_ICP_TSDF_NO_COLOR ? nullptr : base + 2 * n, n, color_type};
    tsdf_reset<<<blocks_for(n), 256, 0, c->stream>>>(v.p, 0, n);
    if (hipGetLastError() != hipSuccess) {
        t->free_buffers();
        delete t;
        return fail(c, MI_ICP_ERR_HIP, "tsdf_create: launch failed");
    }
    c->tsdf_volumes.push_back(t);
    *out = t;
    return MI_ICP_OK;
}

int mi_icp_tsdf_destroy(mi_icp_ctx* c, mi_icp_tsdf* t) {
    return handle_destroy(c, t, c->tsdf_volumes, "tsdf_destroy", "volume");
}

int mi_icp_tsdf_reset(mi_icp_ctx* c, mi_icp_tsdf* t) {
    TRY(check_ctx(c));
    TRY(tsdf_check(c, t, "tsdf_reset"));
    tsdf_reset<<<blocks_for(t->v.p.stride), 256, 0, c->stream>>>(t->v.p, 0, t->v.p.stride);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_tsdf_integrate(mi_icp_ctx* c, mi_icp_tsdf* t, const void* depth, int depth_width, int depth_height,
                          int depth_channels, int depth_bytes_per_channel, const void* color, int color_width,
                          int color_height, int color_channels, int color_bytes_per_channel, int width, int height,
                          const float* intrinsic4, const float* extrinsic, int mem_kind) {
    const char* what = "tsdf_integrate";
    TRY(check_ctx(c, mem_kind, what));
    TRY(tsdf_check(c, t, what));
    const int ct = t->v.p.color_type;
    TRY(tsdf_frame_check(c, "UniformTSDFVolume", what, ct, {depth, depth_width, depth_height, depth_channels, depth_bytes_per_channel},
                         {color, color_width, color_height, color_channels, color_bytes_per_channel}, width, height, intrinsic4));
    const int64_t npix = (int64_t)width * height;
    TRY(tsdf_mult_ensure(c, t->mult, width, height, intrinsic4));

    const uint8_t *dd, *dc;
    TRY(to_device(c, (const uint8_t*)depth, (size_t)npix * 4, mem_kind, c->stage[0], &dd));
    TRY(to_device(c, (const uint8_t*)(ct == MI_ICP_TSDF_NO_COLOR ? nullptr : color),
                  (size_t)npix * (ct == MI_ICP_TSDF_RGB8 ? 3 : 4), mem_kind, c->stage[1], &dc));
    TsdfIntegrate a = tsdf_frame_args(load_T(extrinsic), intrinsic4, width, height, t->v.voxel_length, t->sdf_trunc);
    a.depth = (const float*)dd;
    a.color = dc;
    a.mult = (const float*)t->mult.buf.p;
    const int zchunks = (t->v.res + 255) / 256;
    tsdf_integrate<<<(unsigned)((int64_t)t->v.res * t->v.res * zchunks), 256, 0, c->stream>>>(t->v, a, zchunks);
    KCHK(c);
    if (mem_kind == MI_ICP_HOST) HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's images may go now
    return MI_ICP_OK;
}

int mi_icp_tsdf_extract_voxel_point_cloud(mi_icp_ctx* c, mi_icp_tsdf* t, float* out_xyz, float* out_colors, int64_t capacity,
                                          int64_t* m, int mem_kind) {
    const char* what = "tsdf_extract_voxel_point_cloud";
    TRY(tsdf_extract_args(c, t, c->tsdf_volumes, what, capacity, m, mem_kind));
    const int64_t n = t->v.p.stride;
    uint32_t* flags;
    TRY(ensure(c, c->flags, (size_t)n, &flags));
    tsdf_voxel_flags<<<blocks_for(n), 256, 0, c->stream>>>(t->v, flags);
    KCHK(c);
    float* const out[3] = {out_xyz, nullptr, out_colors};
    return cloud_emit_counted(c, what, flags, n, out, {true, false, true}, capacity, m, mem_kind,
                              [&](const uint32_t* pos, float* const dst[3]) {
                                  tsdf_voxel_gather<<<blocks_for(n), 256, 0, c->stream>>>(t->v, flags, pos, dst[0], dst[2]);
                              });
}

int mi_icp_tsdf_extract_point_cloud(mi_icp_ctx* c, mi_icp_tsdf* t, float* out_xyz, float* out_normals, float* out_colors,
                                    int64_t capacity, int64_t* m, int mem_kind) {
    const char* what = "tsdf_extract_point_cloud";
    TRY(tsdf_extract_args(c, t, c->tsdf_volumes, what, capacity, m, mem_kind));
    const int64_t r2 = t->v.res - 2, n = r2 * r2 * r2;  // the interior voxels; each has three candidate edges
    uint32_t* count;
    TRY(ensure(c, c->flags, (size_t)n, &count));
    tsdf_cloud_count<<<blocks_for(n), 256, 0, c->stream>>>(t->v, n, count);
    KCHK(c);
    float* const out[3] = {out_xyz, out_normals, out_colors};
    return cloud_emit_counted(c, what, count, n, out, {true, true, t->v.p.color_type != MI_ICP_TSDF_NO_COLOR}, capacity, m, mem_kind,
                              [&](const uint32_t* pos, float* const dst[3]) {
                                  tsdf_cloud_gather<<<blocks_for(n), 256, 0, c->stream>>>(t->v, n, count, pos, dst[0], dst[1], dst[2]);
                              });
}

int mi_icp_tsdf_raycast(mi_icp_ctx* c, mi_icp_tsdf* t, int width, int height, const float* intrinsic4, const float* extrinsic,
                        float sdf_trunc, int valid_only, float* out_xyz, float* out_normals, float* out_colors,
                        int64_t capacity, int64_t* m, int mem_kind) {
    float* const out[3] = {out_xyz, out_normals, out_colors};
    return tsdf_raycast_levels(c, t, "tsdf_raycast", 1, width, height, intrinsic4, extrinsic, sdf_trunc, valid_only, out, capacity,
                               m, mem_kind);
}

int mi_icp_tsdf_raycast_levels(mi_icp_ctx* c, mi_icp_tsdf* t, int levels, int width, int height, const float* intrinsic4,
                               const float* extrinsic, float sdf_trunc, int valid_only, float* out_xyz, float* out_normals,
                               float* out_colors, int64_t capacity, int64_t* m) {
    float* const out[3] = {out_xyz, out_normals, out_colors};
    return tsdf_raycast_levels(c, t, "tsdf_raycast_levels", levels, width, height, intrinsic4, extrinsic, sdf_trunc, valid_only, out,
                               capacity, m, MI_ICP_DEVICE);
}

int mi_icp_tsdf_get_voxels(mi_icp_ctx* c, mi_icp_tsdf* t, float* tsdf_out, float* weight_out, float* color_out, int mem_kind) {
    const char* what = "tsdf_get_voxels";
    TRY(check_ctx(c, mem_kind, what));
    TRY(tsdf_check(c, t, what));
    if (color_out && !t->v.p.color) return fail(c, MI_ICP_ERR_INVALID, "%s: the volume has no colour planes", what);
    TRY(from_device(c, (const float*)t->v.p.tsdf, tsdf_out, (size_t)t->v.p.stride, mem_kind));
    TRY(from_device(c, (const float*)t->v.p.weight, weight_out, (size_t)t->v.p.stride, mem_kind));
    TRY(from_device(c, (const float*)t->v.p.color, color_out, (size_t)t->v.p.stride * 3, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

}  // extern "C"
