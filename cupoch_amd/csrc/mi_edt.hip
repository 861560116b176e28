// mi_edt.hip -- geometry::DistanceTransform: seeding from cells, VoxelGrid keys or an OccupancyGrid, the three passes,
// queries and the whole-plane read-back (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include <cfloat>

#include "ctx.h"
#include "edt_kernels.h"

using namespace mi;
using namespace mi::eng;

// ---------------------------------------------------------------------------
// geometry::DistanceTransform (geometry/distancetransform.cu; edt_kernels.h).  A transform belongs to the context that
// made it and is freed with it at the latest.  Nothing here waits for the stream except a compute that is asked for its
// count of dropped cells, and get_voxels.
struct mi_icp_dt {
    mi_icp_ctx* owner = nullptr;
    EdtGrid g = {};
    DevBuf a, b;
    DevBuf dropped;  // one 64-bit counter
    void free_buffers() {
        release(a);
        release(b);
        release(dropped);
    }
};

void mi::eng::dt_release_all(mi_icp_ctx* c) { handle_release_all(c->dts); }

static int dt_check(mi_icp_ctx* c, const mi_icp_dt* d, const char* what) {
    return handle_check(c, d, c->dts, what, "distance transform");
}

// both planes of a transform of `resolution`, no site anywhere; on failure *d is left without buffers.  A plane that
// cannot be had is an error code: the runtime's sticky error is taken off so that the next launch check does not see it.
static int dt_allocate(mi_icp_ctx* c, mi_icp_dt* d, int resolution) {
    EdtGrid& g = d->g;
    g.res = resolution;
    g.h_res = resolution / 2;
    g.n = (int64_t)resolution * resolution * resolution;
    unsigned long long* cnt;
    int rc = ensure(c, d->a, (size_t)g.n, &g.a);
    if (rc == MI_ICP_OK) rc = ensure(c, d->b, (size_t)g.n, &g.b);
    if (rc == MI_ICP_OK) rc = ensure(c, d->dropped, (size_t)1, &cnt);
    if (rc != MI_ICP_OK) {
        (void)hipGetLastError();
        d->free_buffers();
        return rc;
    }
    if (hipMemsetAsync(g.b, 0xff, (size_t)g.n * sizeof(uint32_t), c->stream) != hipSuccess) {
        (void)hipGetLastError();
        d->free_buffers();
        return fail(c, MI_ICP_ERR_HIP, "distance transform: the plane could not be cleared");
    }
    return MI_ICP_OK;
}

// a new site set begins: plane A without a site, the counter of dropped cells at zero
static int dt_begin(mi_icp_ctx* c, mi_icp_dt* d) {
    HIPCHK(c, hipMemsetAsync(d->g.a, 0xff, (size_t)d->g.n * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(d->dropped.p, 0, sizeof(unsigned long long), c->stream));
    return MI_ICP_OK;
}

// the three passes over the seeded plane; then the count of dropped cells if it is asked for (the call's one wait)
static int dt_passes(mi_icp_ctx* c, mi_icp_dt* d, int64_t* dropped) {
    const EdtGrid& g = d->g;
    const int64_t lines = (int64_t)g.res * g.res;
    edt_pass_z<<<blocks_for(lines, 4), 256, 0, c->stream>>>(g);
    KCHK(c);
    edt_pass<1><<<blocks_for(lines), 256, 0, c->stream>>>(g);
    KCHK(c);
    edt_pass<0><<<blocks_for(lines), 256, 0, c->stream>>>(g);
    KCHK(c);
    if (dropped) {
        unsigned long long* host = (unsigned long long*)c->u_host;
        HIPCHK(c, hipMemcpyAsync(host, d->dropped.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        *dropped = (int64_t)host[0];
    }
    return MI_ICP_OK;
}

extern "C" {

int mi_icp_dt_create(mi_icp_ctx* c, int resolution, mi_icp_dt** out) {
    TRY(check_ctx(c));
    if (!out) return fail(c, MI_ICP_ERR_INVALID, "dt_create: out is null");
    *out = nullptr;
    TRY(resolution_ok(c, "dt_create", resolution, MI_ICP_DT_MAX_RESOLUTION));
    mi_icp_dt* d = new mi_icp_dt;
    d->owner = c;
    const int rc = dt_allocate(c, d, resolution);
    if (rc != MI_ICP_OK) {
        d->free_buffers();
        delete d;
        return rc;
    }
    c->dts.push_back(d);
    *out = d;
    return MI_ICP_OK;
}

int mi_icp_dt_destroy(mi_icp_ctx* c, mi_icp_dt* d) {
    return handle_destroy(c, d, c->dts, "dt_destroy", "distance transform");
}

int mi_icp_dt_reconstruct(mi_icp_ctx* c, mi_icp_dt* d, int resolution) {
    TRY(check_ctx(c));
    TRY(dt_check(c, d, "dt_reconstruct"));
    TRY(resolution_ok(c, "dt_reconstruct", resolution, MI_ICP_DT_MAX_RESOLUTION));
    const int rc = dt_allocate(c, d, resolution);
    if (rc != MI_ICP_OK) handle_drop(d, c->dts);  // no planes left: the handle is gone
    return rc;
}

int mi_icp_dt_compute_cells(mi_icp_ctx* c, mi_icp_dt* d, const int32_t* cells, int64_t n, int64_t* dropped) {
    const char* what = "dt_compute_cells";
    TRY(check_ctx(c));
    TRY(dt_check(c, d, what));
    TRY(count_ok(c, what, n));
    if (n > 0 && !cells) return fail(c, MI_ICP_ERR_INVALID, "%s: null cells", what);
    TRY(dt_begin(c, d));
    if (n > 0) {
        edt_seed_cells<<<blocks_for(n), 256, 0, c->stream>>>(d->g, cells, n, (unsigned long long*)d->dropped.p);
        KCHK(c);
    }
    return dt_passes(c, d, dropped);
}

int mi_icp_dt_compute_voxelgrid(mi_icp_ctx* c, mi_icp_dt* d, float voxel_size, const float* origin3, const int32_t* keys,
                                int64_t m, float grid_voxel_size, const float* grid_origin3, int64_t* dropped) {
    const char* what = "dt_compute_voxelgrid";
    TRY(check_ctx(c));
    TRY(dt_check(c, d, what));
    GridFrame dt, grid;
    TRY(frame_check(c, what, voxel_size, origin3, &dt));
    TRY(frame_check(c, what, grid_voxel_size, grid_origin3, &grid));
    TRY(count_ok(c, what, m));
    if (m > 0 && !keys) return fail(c, MI_ICP_ERR_INVALID, "%s: null keys", what);
    if (std::fabs(voxel_size - grid_voxel_size) > FLT_EPSILON)
        return fail(c, MI_ICP_ERR_INVALID, "Unsupport computing Voronoi diagrams from different voxel size.");
    TRY(dt_begin(c, d));
    if (m > 0) {
        edt_seed_keys<<<blocks_for(m), 256, 0, c->stream>>>(d->g, keys, m, grid, dt, (unsigned long long*)d->dropped.p);
        KCHK(c);
    }
    return dt_passes(c, d, dropped);
}

int mi_icp_dt_compute_occgrid(mi_icp_ctx* c, mi_icp_dt* d, const mi_icp_occgrid* grid, float occ_prob_thres_log) {
    const char* what = "dt_compute_occgrid";
    TRY(check_ctx(c));
    TRY(dt_check(c, d, what));
    const float* prob;
    int res, bd[6];
    TRY(occgrid_view(c, grid, what, &prob, &res, bd));
    if (std::isnan(occ_prob_thres_log)) return fail(c, MI_ICP_ERR_INVALID, "%s: the threshold is not a number", what);
    if (res != d->g.res) return fail(c, MI_ICP_ERR_INVALID, "%s: the resolutions differ (%d, %d)", what, res, d->g.res);
    TRY(dt_begin(c, d));
    const GridBox box = box_of_bounds(bd);
    if (box.count > 0) {
        edt_seed_occupied<<<blocks_for(box.count), 256, 0, c->stream>>>(d->g, prob, box, occ_prob_thres_log);
        KCHK(c);
    }
    return dt_passes(c, d, nullptr);
}

int mi_icp_dt_query(mi_icp_ctx* c, mi_icp_dt* d, float voxel_size, const float* origin3, const float* queries, int64_t n,
                    float* out_distance, int32_t* out_nearest) {
    const char* what = "dt_query";
    TRY(check_ctx(c));
    TRY(dt_check(c, d, what));
    GridFrame f;
    TRY(frame_check(c, what, voxel_size, origin3, &f));
    TRY(count_ok(c, what, n));
    if (n == 0) return MI_ICP_OK;
    if (!queries || !out_distance) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    edt_query<<<blocks_for(n), 256, 0, c->stream>>>(d->g, f, queries, n, out_distance, out_nearest);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_dt_get_voxels(mi_icp_ctx* c, mi_icp_dt* d, float voxel_size, int32_t* out_nearest, float* out_distance) {
    const char* what = "dt_get_voxels";
    TRY(check_ctx(c));
    TRY(dt_check(c, d, what));
    if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size))
        return fail(c, MI_ICP_ERR_INVALID, "%s: voxel_size must be positive and finite", what);
    if (!out_nearest && !out_distance) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffers", what);
    edt_unpack<<<blocks_for(d->g.n), 256, 0, c->stream>>>(d->g, voxel_size, out_nearest, out_distance);
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

}  // extern "C"
