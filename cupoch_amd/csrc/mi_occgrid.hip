// mi_occgrid.hip -- geometry::OccupancyGrid: insert, add voxels, free area, queries, extractions
// (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "occupancy_kernels.h"

using namespace mi;
using namespace mi::eng;

// ---------------------------------------------------------------------------
// geometry::OccupancyGrid (geometry/occupancygrid.cu; occupancy_kernels.h).  A grid belongs to the context that made it
// and is freed with it at the latest.  Every call that changes the bounds waits for the stream once, at its end, for its
// status; the bounds come back in the same copy, so the host's copy of them is always current.
struct mi_icp_occgrid {
    mi_icp_ctx* owner = nullptr;
    OccGrid g = {};
    DevBuf prob, marks, touch, state;
    DevBuf part;        // occ_prepare's per-block maxima
    int bounds[6] = {0, 0, 0, 0, 0, 0};  // min[3], max[3], inclusive (a SetFreeArea beside the grid leaves min > max on an axis)
    void free_buffers() {
        release(prob);
        release(marks);
        release(touch);
        release(state);
        release(part);
    }
};

namespace mi {
namespace eng {
void occgrid_release_all(mi_icp_ctx* c) { handle_release_all(c->occ_grids); }

static int occ_check(mi_icp_ctx* c, const mi_icp_occgrid* o, const char* what) {
    return handle_check(c, o, c->occ_grids, what, "grid");
}

int occgrid_view(mi_icp_ctx* c, const mi_icp_occgrid* o, const char* what, const float** prob, int* resolution, int* bounds6) {
    TRY(occ_check(c, o, what));
    *prob = o->g.prob;
    *resolution = o->g.res;
    for (int k = 0; k < 6; ++k) bounds6[k] = o->bounds[k];
    return MI_ICP_OK;
}

int occgrid_select(mi_icp_ctx* c, const mi_icp_occgrid* o, int which, float thres, int64_t* count) {
    *count = 0;
    const GridBox b = box_of_bounds(o->bounds);
    if (b.count == 0) return MI_ICP_OK;
    uint32_t *flags, *pos;
    const uint32_t* total;
    TRY(ensure(c, c->flags, (size_t)b.count, &flags));
    occ_box_flags<<<blocks_for(b.count), 256, 0, c->stream>>>(o->g, b, which, thres, flags);
    KCHK(c);
    TRY(scan_flags(c, flags, b.count, &pos, &total));
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *count = (int64_t)c->u_host[0];
    return MI_ICP_OK;
}

int occgrid_gather(mi_icp_ctx* c, const mi_icp_occgrid* o, const GridFrame& f, int32_t* out_index, float* out_prob_log, float* out_xyz) {
    const GridBox b = box_of_bounds(o->bounds);
    occ_box_gather<<<blocks_for(b.count), 256, 0, c->stream>>>(o->g, b, f, (const uint32_t*)c->flags.p, (const uint32_t*)c->dense_idx.p,
                                                             out_index, out_prob_log, out_xyz);
    KCHK(c);
    return MI_ICP_OK;
}
}  // namespace eng
}  // namespace mi

// the context, the grid, and the parameters every call reads: voxel_size positive and finite, a finite origin, no NaN
// among the log-odds parameters and finite hit / miss steps
static int occ_args(mi_icp_ctx* c, const mi_icp_occgrid* o, const mi_icp_occgrid_params* p, const char* what, GridFrame* f) {
    TRY(check_ctx(c));
    TRY(occ_check(c, o, what));
    if (!p) return fail(c, MI_ICP_ERR_INVALID, "%s: null parameters", what);
    TRY(frame_check(c, what, p->voxel_size, p->origin, f));
    if (std::isnan(p->clamping_thres_min) || std::isnan(p->clamping_thres_max) || !std::isfinite(p->prob_hit_log) ||
        !std::isfinite(p->prob_miss_log) || std::isnan(p->occ_prob_thres_log))
        return fail(c, MI_ICP_ERR_INVALID, "%s: a log-odds parameter is not a number", what);
    return MI_ICP_OK;
}

// planes of a grid of `resolution`, every voxel unknown; on failure *o is left without buffers
static int occ_allocate(mi_icp_ctx* c, mi_icp_occgrid* o, int resolution) {
    OccGrid& g = o->g;
    g.res = resolution;
    g.h_res = resolution / 2;
    g.n = (int64_t)resolution * resolution * resolution;
    const size_t mark_bytes = (size_t)((g.n + kOccSweepBytes - 1) / kOccSweepBytes) * kOccSweepBytes;
    int rc = ensure(c, o->prob, (size_t)g.n, &g.prob);
    if (rc == MI_ICP_OK) rc = ensure(c, o->marks, mark_bytes, &g.marks);
    if (rc == MI_ICP_OK) rc = ensure(c, o->touch, (size_t)3 * resolution, &g.touch);
    if (rc == MI_ICP_OK) rc = ensure(c, o->state, (size_t)kOccStateWords, &g.state);
    if (rc != MI_ICP_OK) {
        o->free_buffers();
        return rc;
    }
    // (whole buffers: a grid rebuilt smaller keeps its larger ones, and everything past the marks in use stays zero)
    HIPCHK(c, hipMemsetAsync(g.marks, 0, o->marks.bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(g.touch, 0, o->touch.bytes, c->stream));
    HIPCHK(c, hipMemsetAsync(g.state, 0, o->state.bytes, c->stream));
    occ_reset<<<blocks_for(g.n), 256, 0, c->stream>>>(g);
    KCHK(c);
    for (int k = 0; k < 6; ++k) o->bounds[k] = g.h_res;
    return MI_ICP_OK;
}

// sweep the marks, widen the bounds, wait, and read the state back: the call's status and the new bounds
static int occ_sweep_and_wait(mi_icp_ctx* c, mi_icp_occgrid* o, const mi_icp_occgrid_params* p, const char* what) {
    const OccGrid& g = o->g;
    const int64_t blocks = (g.n + kOccSweepBytes - 1) / kOccSweepBytes;
    occ_sweep<<<(unsigned)blocks, 256, 0, c->stream>>>(g, p->prob_miss_log, p->prob_hit_log, p->clamping_thres_min,
                                                     p->clamping_thres_max);
    KCHK(c);
    occ_bounds<<<1, 256, 0, c->stream>>>(g);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->u_host, g.state, sizeof(int) * 9, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int* st = (const int*)c->u_host;
    if (st[kOccBad] == kOccBadNDiv)
        return fail(c, MI_ICP_ERR_INVALID, "%s: the longest ray spans more than %d voxels along an axis (or is not a number)",
                    what, MI_ICP_OCCGRID_MAX_NDIV);
    if (st[kOccBad] == kOccBadIndex) return fail(c, MI_ICP_ERR_INVALID, "[OccupancyGrid] a provided voxel is not in the occupancy grid range.");
    for (int k = 0; k < 6; ++k) o->bounds[k] = st[k];
    return MI_ICP_OK;
}

extern "C" {

int mi_icp_occgrid_create(mi_icp_ctx* c, int resolution, mi_icp_occgrid** out) {
    TRY(check_ctx(c));
    if (!out) return fail(c, MI_ICP_ERR_INVALID, "occgrid_create: out is null");
    *out = nullptr;
    TRY(resolution_ok(c, "occgrid_create", resolution, MI_ICP_OCCGRID_MAX_RESOLUTION));
    mi_icp_occgrid* o = new mi_icp_occgrid;
    o->owner = c;
    const int rc = occ_allocate(c, o, resolution);
    if (rc != MI_ICP_OK) {
        o->free_buffers();
        delete o;
        return rc;
    }
    c->occ_grids.push_back(o);
    *out = o;
    return MI_ICP_OK;
}

int mi_icp_occgrid_destroy(mi_icp_ctx* c, mi_icp_occgrid* o) {
    return handle_destroy(c, o, c->occ_grids, "occgrid_destroy", "grid");
}

int mi_icp_occgrid_reset(mi_icp_ctx* c, mi_icp_occgrid* o) {
    TRY(check_ctx(c));
    TRY(occ_check(c, o, "occgrid_reset"));
    occ_reset<<<blocks_for(o->g.n), 256, 0, c->stream>>>(o->g);
    KCHK(c);
    for (int k = 0; k < 6; ++k) o->bounds[k] = o->g.h_res;
    return MI_ICP_OK;
}

int mi_icp_occgrid_reconstruct(mi_icp_ctx* c, mi_icp_occgrid* o, int resolution) {
    TRY(check_ctx(c));
    TRY(occ_check(c, o, "occgrid_reconstruct"));
    TRY(resolution_ok(c, "occgrid_reconstruct", resolution, MI_ICP_OCCGRID_MAX_RESOLUTION));
    const int rc = occ_allocate(c, o, resolution);
    if (rc != MI_ICP_OK) handle_drop(o, c->occ_grids);  // no planes left: the handle is gone
    return rc;
}

int mi_icp_occgrid_insert(mi_icp_ctx* c, mi_icp_occgrid* o, const mi_icp_occgrid_params* p, const float* points, int64_t n,
                          const float* viewpoint3, float max_range) {
    const char* what = "occgrid_insert";
    GridFrame f;
    TRY(occ_args(c, o, p, what, &f));
    TRY(count_ok(c, what, n));
    if (n == 0) return MI_ICP_OK;
    if (!points || !finite3(viewpoint3) || std::isnan(max_range))
        return fail(c, MI_ICP_ERR_INVALID, "%s: null points, or a viewpoint or range that is not a number", what);
    OccRays a;
    for (int k = 0; k < 3; ++k) a.vp[k] = viewpoint3[k];
    a.max_range = max_range;
    const int nb = blocks_for(n);
    uint32_t* part;
    TRY(ensure(c, o->part, (size_t)nb, &part));
    const OccGrid& g = o->g;
    occ_prepare<<<nb, 256, 0, c->stream>>>(points, n, a, part);
    KCHK(c);
    occ_plan<<<1, 256, 0, c->stream>>>(g, part, (int64_t)nb, f.vs, MI_ICP_OCCGRID_MAX_NDIV);
    KCHK(c);
    occ_mark_rays<<<nb, 256, 0, c->stream>>>(g, f, points, n, a);
    KCHK(c);
    occ_mark_hits<<<nb, 256, 0, c->stream>>>(g, f, points, n, a);
    KCHK(c);
    return occ_sweep_and_wait(c, o, p, what);
}

int mi_icp_occgrid_add_voxels(mi_icp_ctx* c, mi_icp_occgrid* o, const mi_icp_occgrid_params* p, const int32_t* indices,
                              int64_t n, int occupied) {
    const char* what = "occgrid_add_voxels";
    GridFrame f;
    TRY(occ_args(c, o, p, what, &f));
    TRY(count_ok(c, what, n));
    if (n == 0) return MI_ICP_OK;
    if (!indices) return fail(c, MI_ICP_ERR_INVALID, "%s: null indices", what);
    const OccGrid& g = o->g;
    HIPCHK(c, hipMemsetAsync(g.state + kOccBad, 0, sizeof(int), c->stream));
    occ_check_indices<<<blocks_for(n), 256, 0, c->stream>>>(g, indices, n);
    KCHK(c);
    occ_mark_indices<<<blocks_for(n), 256, 0, c->stream>>>(g, indices, n, occupied ? kOccHit : kOccFree);
    KCHK(c);
    return occ_sweep_and_wait(c, o, p, what);
}

int mi_icp_occgrid_set_free_area(mi_icp_ctx* c, mi_icp_occgrid* o, const mi_icp_occgrid_params* p, const float* min3,
                                 const float* max3) {
    const char* what = "occgrid_set_free_area";
    GridFrame f;
    TRY(occ_args(c, o, p, what, &f));
    if (!finite3(min3) || !finite3(max3)) return fail(c, MI_ICP_ERR_INVALID, "%s: a corner is not a number", what);
    const OccGrid& g = o->g;
    int lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = std::max(cell_of(f, min3[k], k) + g.h_res, 0);
        hi[k] = std::min(cell_of(f, max3[k], k) + g.h_res, g.res - 1);
    }
    for (int k = 0; k < 3; ++k) {
        o->bounds[k] = lo[k];
        o->bounds[3 + k] = hi[k];
    }
    const GridBox b = box_of_bounds(o->bounds);
    occ_free_box<<<blocks_for(b.count), 256, 0, c->stream>>>(g, b, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], p->prob_miss_log);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_occgrid_query(mi_icp_ctx* c, mi_icp_occgrid* o, const mi_icp_occgrid_params* p, const float* points, int64_t n,
                         float* out_prob_log, int32_t* out_index) {
    const char* what = "occgrid_query";
    GridFrame f;
    TRY(occ_args(c, o, p, what, &f));
    TRY(count_ok(c, what, n));
    if (n == 0) return MI_ICP_OK;
    if (!points || !out_prob_log) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    occ_query<<<blocks_for(n), 256, 0, c->stream>>>(o->g, f, points, n, out_prob_log, out_index);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_occgrid_extract(mi_icp_ctx* c, mi_icp_occgrid* o, const mi_icp_occgrid_params* p, int which, int32_t* out_index,
                           float* out_prob_log, float* out_xyz, int64_t capacity, int64_t* m) {
    const char* what = "occgrid_extract";
    GridFrame f;
    TRY(occ_args(c, o, p, what, &f));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    if (which < MI_ICP_OCCGRID_KNOWN || which > MI_ICP_OCCGRID_OCCUPIED || capacity < 0)
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad selection or negative capacity", what);
    TRY(occgrid_select(c, o, which, p->occ_prob_thres_log, m));
    if (*m == 0 || capacity < *m) return MI_ICP_OK;  // nothing is written: the caller learns the room to make
    return occgrid_gather(c, o, f, out_index, out_prob_log, out_xyz);
}

int mi_icp_occgrid_get_bounds(mi_icp_ctx* c, mi_icp_occgrid* o, int32_t* min3, int32_t* max3) {
    TRY(check_ctx(c));
    TRY(occ_check(c, o, "occgrid_get_bounds"));
    if (!min3 || !max3) return fail(c, MI_ICP_ERR_INVALID, "occgrid_get_bounds: null buffer");
    for (int k = 0; k < 3; ++k) {
        min3[k] = o->bounds[k];
        max3[k] = o->bounds[3 + k];
    }
    return MI_ICP_OK;
}

int mi_icp_occgrid_get_voxels(mi_icp_ctx* c, mi_icp_occgrid* o, float* out_prob_log) {
    TRY(check_ctx(c));
    TRY(occ_check(c, o, "occgrid_get_voxels"));
    if (!out_prob_log) return fail(c, MI_ICP_ERR_INVALID, "occgrid_get_voxels: null buffer");
    TRY(from_device(c, (const float*)o->g.prob, out_prob_log, (size_t)o->g.n, MI_ICP_DEVICE));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

}  // extern "C"
