// mi_stsdf.hip -- integration::ScalableTSDFVolume: open units, integrate, extract clouds, read units back
// (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "scalable_tsdf_kernels.h"
#include "tsdf_host.h"

using namespace mi;
using namespace mi::eng;
using host::Mat4;

// ---------------------------------------------------------------------------
// A volume belongs to the context that made it and is freed with it at the latest.
struct mi_icp_stsdf {
    mi_icp_ctx* owner = nullptr;
    StsdfVol v = {};
    int stride = 4;
    int capacity = 0;  // unit slots the pool and the directory have room for
    int n_units = 0;   // open units (the host knows: every frame waits for its new-unit count)
    void* planes = nullptr;            // tsdf, weight and, with a colour type, three colour planes of capacity * 4096 floats
    void* dir[2] = {nullptr, nullptr};  // the directory, twice: capacity keys (uint64) and then capacity slots (uint32)
    int cur = 0;                        // which of the two holds it
    DevBuf fresh;   // a frame's new keys
    DevBuf edges;   // ExtractPointCloud's list of crossing edges
    TsdfMult mult;
    void free_buffers() {
        if (planes) (void)hipFree(planes);
        for (int k = 0; k < 2; ++k)
            if (dir[k]) (void)hipFree(dir[k]);
        release(fresh);
        release(edges);
        release(mult.buf);
    }
};

static int stsdf_planes_of(int color_type) { return color_type == MI_ICP_TSDF_NO_COLOR ? 2 : 5; }

static void stsdf_point_planes(mi_icp_stsdf* t, void* planes, int capacity) {
    float* base = (float*)planes;
    TsdfPlanes& p = t->v.p;
    p.stride = (int64_t)capacity * kStsdfUnit;
    p.tsdf = base;
    p.weight = base + p.stride;
    p.color = p.color_type == MI_ICP_TSDF_NO_COLOR ? nullptr : base + 2 * p.stride;
}

static uint64_t* dir_keys(void* d) { return (uint64_t*)d; }
static uint32_t* dir_slots(void* d, int capacity) { return (uint32_t*)((uint64_t*)d + capacity); }

static StsdfDir stsdf_dir(const mi_icp_stsdf* t) {
    StsdfDir d;
    d.keys = dir_keys(t->dir[t->cur]);
    d.slots = dir_slots(t->dir[t->cur], t->capacity);
    d.n = t->n_units;
    return d;
}

// Room for `capacity` units: new planes and directories, the open units' contents copied over.  Either everything is
// allocated and the volume moves, or nothing changes and the call reports MI_ICP_ERR_HIP.
static int stsdf_reserve(mi_icp_ctx* c, mi_icp_stsdf* t, int capacity) {
    void *planes = nullptr, *d0 = nullptr, *d1 = nullptr;
    const int np = stsdf_planes_of(t->v.p.color_type);
    const size_t pbytes = (size_t)capacity * kStsdfUnit * np * sizeof(float), dbytes = (size_t)capacity * 12;
    if (hipMalloc(&planes, pbytes) != hipSuccess || hipMalloc(&d0, dbytes) != hipSuccess || hipMalloc(&d1, dbytes) != hipSuccess) {
        (void)hipGetLastError();
        if (planes) (void)hipFree(planes);
        if (d0) (void)hipFree(d0);
        if (d1) (void)hipFree(d1);
        return fail(c, MI_ICP_ERR_HIP, "scalable tsdf: out of memory for %d units (%zu bytes)", capacity, pbytes + 2 * dbytes);
    }
    if (t->n_units > 0) {
        const size_t live = (size_t)t->n_units * kStsdfUnit * sizeof(float);
        for (int p = 0; p < np; ++p)
            HIPCHK(c, hipMemcpyAsync((float*)planes + (size_t)p * capacity * kStsdfUnit, (const float*)t->planes + (size_t)p * t->v.p.stride,
                                     live, hipMemcpyDeviceToDevice, c->stream));
        const StsdfDir d = stsdf_dir(t);
        HIPCHK(c, hipMemcpyAsync(dir_keys(d0), d.keys, (size_t)t->n_units * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(dir_slots(d0, capacity), d.slots, (size_t)t->n_units * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (t->planes) (void)hipFree(t->planes);
    for (int k = 0; k < 2; ++k)
        if (t->dir[k]) (void)hipFree(t->dir[k]);
    t->planes = planes;
    t->dir[0] = d0;
    t->dir[1] = d1;
    t->cur = 0;
    t->capacity = capacity;
    stsdf_point_planes(t, planes, capacity);
    return MI_ICP_OK;
}

void mi::eng::stsdf_release_all(mi_icp_ctx* c) { handle_release_all(c->stsdf_volumes); }

static int stsdf_check(mi_icp_ctx* c, const mi_icp_stsdf* t, const char* what) {
    return handle_check(c, t, c->stsdf_volumes, what, "volume");
}

// Stage 1 of Integrate: the units this frame's sampled points want and the directory lacks are opened.
static int stsdf_open_units(mi_icp_ctx* c, mi_icp_stsdf* t, const DepthArgs& a) {
    const int64_t count = (int64_t)(a.width / a.stride) * (a.height / a.stride);
    if (count == 0) return MI_ICP_OK;
    uint32_t* cnt;
    TRY(ensure(c, c->flags, (size_t)count, &cnt));
    const StsdfDir dir = stsdf_dir(t);
    stsdf_open<false><<<blocks_for(count), 256, 0, c->stream>>>(a, count, t->v.sdf_trunc, t->v.unit_length, dir, cnt, nullptr, nullptr, nullptr);
    KCHK(c);
    uint32_t* pos;
    const uint32_t* total;
    TRY(scan_flags(c, cnt, count, &pos, &total));
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the wait of every frame: how many candidate keys
    const int64_t ncand = (int64_t)c->u_host[0];
    if (ncand == 0) return MI_ICP_OK;
    if (ncand > kMaxCount) return fail(c, MI_ICP_ERR_INVALID, "stsdf_integrate: too many candidate units in one frame");

    SortBuffers sb;
    TRY(sort_buffers(c, ncand, &sb));
    stsdf_open<true><<<blocks_for(count), 256, 0, c->stream>>>(a, count, t->v.sdf_trunc, t->v.unit_length, dir, nullptr, pos, sb.keys[0], sb.vals[0]);
    KCHK(c);
    const int cur = radix_sort_pairs<uint64_t>(c->stream, sb, ncand, 63);
    KCHK(c);
    uint32_t* heads;
    TRY(ensure(c, c->flags, (size_t)ncand, &heads));
    stsdf_heads<<<blocks_for(ncand), 256, 0, c->stream>>>(sb.keys[cur], ncand, heads);
    KCHK(c);
    TRY(scan_flags(c, heads, ncand, &pos, &total));
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));  // a frame that opens units waits once more: how many distinct ones
    const int64_t n_new = (int64_t)c->u_host[0];
    const int64_t need = (int64_t)t->n_units + n_new;
    if (need > MI_ICP_STSDF_MAX_UNITS)
        return fail(c, MI_ICP_ERR_INVALID, "stsdf_integrate: more than %d units", MI_ICP_STSDF_MAX_UNITS);
    uint64_t* fresh;
    TRY(ensure(c, t->fresh, (size_t)n_new, &fresh));
    if (need > t->capacity) {  // grow by doubling, before anything of the volume has changed
        int64_t cap = t->capacity;
        while (cap < need) cap *= 2;
        TRY(stsdf_reserve(c, t, (int)std::min<int64_t>(cap, MI_ICP_STSDF_MAX_UNITS)));
    }
    stsdf_new_keys<<<blocks_for(ncand), 256, 0, c->stream>>>(sb.keys[cur], ncand, pos, fresh);
    KCHK(c);
    const StsdfDir old = stsdf_dir(t);
    void* dst = t->dir[t->cur ^ 1];
    stsdf_merge<<<blocks_for(need), 256, 0, c->stream>>>(old, fresh, (int)n_new, dir_keys(dst), dir_slots(dst, t->capacity));
    KCHK(c);
    tsdf_reset<<<blocks_for(n_new * kStsdfUnit), 256, 0, c->stream>>>(t->v.p, (int64_t)t->n_units * kStsdfUnit, n_new * kStsdfUnit);
    KCHK(c);
    t->cur ^= 1;
    t->n_units = (int)need;
    return MI_ICP_OK;
}

extern "C" {

int mi_icp_stsdf_create(mi_icp_ctx* c, float voxel_length, float sdf_trunc, int color_type, int depth_sampling_stride,
                        int map_size, mi_icp_stsdf** out) {
    TRY(check_ctx(c));
    if (!out) return fail(c, MI_ICP_ERR_INVALID, "stsdf_create: out is null");
    *out = nullptr;
    const float L = voxel_length * 16.0f;
    if (!(voxel_length > 0.0f) || !std::isfinite(voxel_length) || !std::isfinite(L) || !(sdf_trunc > 0.0f) ||
        !std::isfinite(sdf_trunc) || sdf_trunc > L || depth_sampling_stride < 1 || map_size < 1 ||
        map_size > MI_ICP_STSDF_MAX_UNITS ||
        (color_type != MI_ICP_TSDF_NO_COLOR && color_type != MI_ICP_TSDF_RGB8 && color_type != MI_ICP_TSDF_GRAY32))
        return fail(c, MI_ICP_ERR_INVALID, "stsdf_create: bad arguments");
    mi_icp_stsdf* t = new mi_icp_stsdf;
    t->owner = c;
    t->stride = depth_sampling_stride;
    t->v.voxel_length = voxel_length;
    t->v.half = 0.5f * voxel_length;
    t->v.unit_length = L;
    t->v.sdf_trunc = sdf_trunc;
    t->v.p.color_type = color_type;
    const int rc = stsdf_reserve(c, t, map_size);
    if (rc != MI_ICP_OK) {
        t->free_buffers();
        delete t;
        return rc;
    }
    c->stsdf_volumes.push_back(t);
    *out = t;
    return MI_ICP_OK;
}

int mi_icp_stsdf_destroy(mi_icp_ctx* c, mi_icp_stsdf* t) {
    return handle_destroy(c, t, c->stsdf_volumes, "stsdf_destroy", "volume");
}

int mi_icp_stsdf_reset(mi_icp_ctx* c, mi_icp_stsdf* t) {
    TRY(check_ctx(c));
    TRY(stsdf_check(c, t, "stsdf_reset"));
    t->n_units = 0;  // (a unit's voxels are reset when it is opened)
    return MI_ICP_OK;
}

int mi_icp_stsdf_num_units(mi_icp_ctx* c, mi_icp_stsdf* t, int64_t* n_units, int64_t* capacity) {
    TRY(check_ctx(c));
    TRY(stsdf_check(c, t, "stsdf_num_units"));
    if (n_units) *n_units = t->n_units;
    if (capacity) *capacity = t->capacity;
    return MI_ICP_OK;
}

int mi_icp_stsdf_integrate(mi_icp_ctx* c, mi_icp_stsdf* t, const void* depth, int depth_width, int depth_height,
                           int depth_channels, int depth_bytes_per_channel, const void* color, int color_width,
                           int color_height, int color_channels, int color_bytes_per_channel, int width, int height,
                           const float* intrinsic4, const float* extrinsic) {
    const char* what = "stsdf_integrate";
    TRY(check_ctx(c));
    TRY(stsdf_check(c, t, what));
    const int ct = t->v.p.color_type;
    TRY(tsdf_frame_check(c, "ScalableTSDFVolume", what, ct, {depth, depth_width, depth_height, depth_channels, depth_bytes_per_channel},
                         {color, color_width, color_height, color_channels, color_bytes_per_channel}, width, height, intrinsic4));
    const Mat4 E = load_T(extrinsic);

    DepthArgs da = {};
    da.width = width;
    da.height = height;
    da.stride = t->stride;
    da.depth_recip = depth_reciprocal(1000);
    da.depth_trunc = 1000;
    da.depth_cutoff = -1.0f;
    da.fx = intrinsic4[0];
    da.fy = intrinsic4[1];
    da.cx = intrinsic4[2];
    da.cy = intrinsic4[3];
    if (!invert4(E.data(), da.pose)) return fail(c, MI_ICP_ERR_INVALID, "%s: singular extrinsic", what);
    da.depth = (const uint8_t*)depth;

    TRY(tsdf_mult_ensure(c, t->mult, width, height, intrinsic4));
    TRY(stsdf_open_units(c, t, da));
    if (t->n_units == 0) return MI_ICP_OK;  // nothing to integrate into

    TsdfIntegrate a = tsdf_frame_args(E, intrinsic4, width, height, t->v.voxel_length, t->v.sdf_trunc);
    a.depth = (const float*)depth;
    a.color = ct == MI_ICP_TSDF_NO_COLOR ? nullptr : color;
    a.mult = (const float*)t->mult.buf.p;
    stsdf_integrate<<<(unsigned)t->n_units, 256, 0, c->stream>>>(t->v, stsdf_dir(t), a);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_stsdf_extract_voxel_point_cloud(mi_icp_ctx* c, mi_icp_stsdf* t, float* out_xyz, float* out_colors, int64_t capacity,
                                           int64_t* m) {
    const char* what = "stsdf_extract_voxel_point_cloud";
    TRY(tsdf_extract_args(c, t, c->stsdf_volumes, what, capacity, m, MI_ICP_DEVICE));
    const int64_t n = (int64_t)t->n_units * kStsdfUnit;
    if (n == 0) return MI_ICP_OK;
    uint32_t* flags;
    TRY(ensure(c, c->flags, (size_t)n, &flags));
    const StsdfDir dir = stsdf_dir(t);
    stsdf_voxel_flags<<<blocks_for(n), 256, 0, c->stream>>>(t->v, dir, n, flags);
    KCHK(c);
    float* const out[3] = {out_xyz, nullptr, out_colors};
    return cloud_emit_counted(c, what, flags, n, out, {true, false, true}, capacity, m, MI_ICP_DEVICE,
                              [&](const uint32_t* pos, float* const dst[3]) {
                                  stsdf_voxel_gather<<<blocks_for(n), 256, 0, c->stream>>>(t->v, dir, n, flags, pos, dst[0], dst[2]);
                              });
}

int mi_icp_stsdf_extract_point_cloud(mi_icp_ctx* c, mi_icp_stsdf* t, float* out_xyz, float* out_normals, float* out_colors,
                                     int64_t capacity, int64_t* m) {
    const char* what = "stsdf_extract_point_cloud";
    TRY(tsdf_extract_args(c, t, c->stsdf_volumes, what, capacity, m, MI_ICP_DEVICE));
    const int64_t n = (int64_t)t->n_units * kStsdfUnit;  // every voxel has three candidate edges
    if (n == 0) return MI_ICP_OK;
    uint32_t* count;
    TRY(ensure(c, c->flags, (size_t)n, &count));
    const StsdfDir dir = stsdf_dir(t);
    stsdf_cloud_count<<<blocks_for(n), 256, 0, c->stream>>>(t->v, dir, n, count);
    KCHK(c);
    float* const out[3] = {out_xyz, out_normals, out_colors};
    int listed = MI_ICP_OK;
    TRY(cloud_emit_counted(c, what, count, n, out, {true, true, t->v.p.color_type != MI_ICP_TSDF_NO_COLOR}, capacity, m, MI_ICP_DEVICE,
                           [&](const uint32_t* pos, float* const dst[3]) {
                               uint32_t* list;  // (*m is the count by now)
                               if ((listed = ensure(c, t->edges, (size_t)*m, &list)) != MI_ICP_OK) return;
                               stsdf_cloud_list<<<blocks_for(n), 256, 0, c->stream>>>(t->v, dir, n, count, pos, list);
                               stsdf_cloud_points<<<blocks_for(*m), 256, 0, c->stream>>>(t->v, dir, *m, list, dst[0], dst[1], dst[2]);
                           }));
    return listed;
}

int mi_icp_stsdf_get_units(mi_icp_ctx* c, mi_icp_stsdf* t, int32_t* keys_out, float* tsdf_out, float* weight_out,
                           float* color_out, int64_t capacity, int64_t* m) {
    const char* what = "stsdf_get_units";
    TRY(tsdf_extract_args(c, t, c->stsdf_volumes, what, capacity, m, MI_ICP_DEVICE));
    if (color_out && !t->v.p.color) return fail(c, MI_ICP_ERR_INVALID, "%s: the volume has no colour planes", what);
    *m = t->n_units;
    if (t->n_units == 0 || capacity < t->n_units) return MI_ICP_OK;
    const int64_t n = (int64_t)t->n_units * kStsdfUnit;
    stsdf_gather_units<<<blocks_for(n), 256, 0, c->stream>>>(t->v, stsdf_dir(t), n, keys_out, tsdf_out, weight_out, color_out);
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

}  // extern "C"
