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
    int bounds[6] = {0, 0, 0, 0, 0, 0};  // min[3], max[3], inclusive
};

namespace mi {
namespace eng {
static void occgrid_release(mi_icp_occgrid* o) {
    release(o->prob);
    release(o->marks);
    release(o->touch);
    release(o->state);
    release(o->part);
}

void occgrid_release_all(mi_icp_ctx* c) {
    for (mi_icp_occgrid* o : c->occ_grids) {
        occgrid_release(o);
        delete o;
    }
    c->occ_grids.clear();
}

static int occ_check(mi_icp_ctx* c, const mi_icp_occgrid* o, const char* what) {
    if (!owned(c, o, c->occ_grids)) return fail(c, MI_ICP_ERR_INVALID, "%s: not a grid of this context", what);
    return MI_ICP_OK;
}

int occgrid_view(mi_icp_ctx* c, const mi_icp_occgrid* o, const char* what, const float** prob, int* resolution, int* bounds6) {
    TRY(occ_check(c, o, what));
    *prob = o->g.prob;
    *resolution = o->g.res;
    for (int k = 0; k < 6; ++k) bounds6[k] = o->bounds[k];
    return MI_ICP_OK;
}
}  // namespace eng
}  // namespace mi

static bool finite3(const float* v) { return v && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// the context, the grid, and the parameters every call reads: voxel_size positive and finite, a finite origin, no NaN
// among the log-odds parameters and finite hit / miss steps
static int occ_args(mi_icp_ctx* c, const mi_icp_occgrid* o, const mi_icp_occgrid_params* p, const char* what, OccFrame* f) {
    TRY(check_ctx(c));
    TRY(occ_check(c, o, what));
    if (!p) return fail(c, MI_ICP_ERR_INVALID, "%s: null parameters", what);
    if (!(p->voxel_size > 0.0f) || !std::isfinite(p->voxel_size) || !finite3(p->origin))
        return fail(c, MI_ICP_ERR_INVALID, "%s: voxel_size must be positive and finite, the origin finite", what);
    if (std::isnan(p->clamping_thres_min) || std::isnan(p->clamping_thres_max) || !std::isfinite(p->prob_hit_log) ||
        !std::isfinite(p->prob_miss_log) || std::isnan(p->occ_prob_thres_log))
        return fail(c, MI_ICP_ERR_INVALID, "%s: a log-odds parameter is not a number", what);
    f->vs = p->voxel_size;
    for (int k = 0; k < 3; ++k) f->origin[k] = p->origin[k];
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
        occgrid_release(o);
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

static int occ_resolution_ok(mi_icp_ctx* c, int resolution, const char* what) {
    if (resolution < 2 || resolution > MI_ICP_OCCGRID_MAX_RESOLUTION)
        return fail(c, MI_ICP_ERR_INVALID, "%s: the resolution must be in [2, %d]", what, MI_ICP_OCCGRID_MAX_RESOLUTION);
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

// the bounds box, or an empty one (a SetFreeArea beside the grid leaves min > max on an axis)
static OccBox occ_bounds_box(const mi_icp_occgrid* o) {
    OccBox b = {};
    const int* lo = o->bounds;
    const int* hi = o->bounds + 3;
    if (lo[0] > hi[0] || lo[1] > hi[1] || lo[2] > hi[2]) return b;
    b.x0 = lo[0];
    b.y0 = lo[1];
    b.z0 = lo[2];
    b.ex = hi[0] - lo[0] + 1;
    b.ey = hi[1] - lo[1] + 1;
    b.ez = hi[2] - lo[2] + 1;
    b.count = (int64_t)b.ex * b.ey * b.ez;
    return b;
}

static int host_floor_int(float x) { return (int)std::fmin(std::fmax(std::floor(x), -1.0e9f), 1.0e9f); }

extern "C" {

int mi_icp_occgrid_create(mi_icp_ctx* c, int resolution, mi_icp_occgrid** out) {
    TRY(check_ctx(c));
    if (!out) return fail(c, MI_ICP_ERR_INVALID, "occgrid_create: out is null");
    *out = nullptr;
    TRY(occ_resolution_ok(c, resolution, "occgrid_create"));
    mi_icp_occgrid* o = new mi_icp_occgrid;
    o->owner = c;
    const int rc = occ_allocate(c, o, resolution);
    if (rc != MI_ICP_OK) {
        occgrid_release(o);
        delete o;
        return rc;
    }
    c->occ_grids.push_back(o);
    *out = o;
    return MI_ICP_OK;
}

int mi_icp_occgrid_destroy(mi_icp_ctx* c, mi_icp_occgrid* o) {
    TRY(check_ctx(c));
    if (!o) return MI_ICP_OK;
    TRY(occ_check(c, o, "occgrid_destroy"));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->occ_grids.erase(std::find(c->occ_grids.begin(), c->occ_grids.end(), o));
    occgrid_release(o);
    delete o;
    return MI_ICP_OK;
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
    TRY(occ_resolution_ok(c, resolution, "occgrid_reconstruct"));
    const int rc = occ_allocate(c, o, resolution);
    if (rc != MI_ICP_OK) {  // no planes left: the handle is gone
        c->occ_grids.erase(std::find(c->occ_grids.begin(), c->occ_grids.end(), o));
        delete o;
    }
    return rc;
}

int mi_icp_occgrid_insert(mi_icp_ctx* c, mi_icp_occgrid* o, const mi_icp_occgrid_params* p, const float* points, int64_t n,
                          const float* viewpoint3, float max_range) {
    const char* what = "occgrid_insert";
    OccFrame f;
    TRY(occ_args(c, o, p, what, &f));
    if (n < 0 || n > 0x7fffff00ll) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
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
    OccFrame f;
    TRY(occ_args(c, o, p, what, &f));
    if (n < 0 || n > 0x7fffff00ll) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
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
    OccFrame f;
    TRY(occ_args(c, o, p, what, &f));
    if (!finite3(min3) || !finite3(max3)) return fail(c, MI_ICP_ERR_INVALID, "%s: a corner is not a number", what);
    const OccGrid& g = o->g;
    int lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = std::max(host_floor_int((min3[k] - f.origin[k]) / f.vs) + g.h_res, 0);
        hi[k] = std::min(host_floor_int((max3[k] - f.origin[k]) / f.vs) + g.h_res, g.res - 1);
    }
    for (int k = 0; k < 3; ++k) {
        o->bounds[k] = lo[k];
        o->bounds[3 + k] = hi[k];
    }
    const OccBox b = occ_bounds_box(o);
    occ_free_box<<<blocks_for(b.count), 256, 0, c->stream>>>(g, b, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], p->prob_miss_log);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_occgrid_query(mi_icp_ctx* c, mi_icp_occgrid* o, const mi_icp_occgrid_params* p, const float* points, int64_t n,
                         float* out_prob_log, int32_t* out_index) {
    const char* what = "occgrid_query";
    OccFrame f;
    TRY(occ_args(c, o, p, what, &f));
    if (n < 0 || n > 0x7fffff00ll) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    if (n == 0) return MI_ICP_OK;
    if (!points || !out_prob_log) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    occ_query<<<blocks_for(n), 256, 0, c->stream>>>(o->g, f, points, n, out_prob_log, out_index);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_occgrid_extract(mi_icp_ctx* c, mi_icp_occgrid* o, const mi_icp_occgrid_params* p, int which, int32_t* out_index,
                           float* out_prob_log, float* out_xyz, int64_t capacity, int64_t* m) {
    const char* what = "occgrid_extract";
    OccFrame f;
    TRY(occ_args(c, o, p, what, &f));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    if (which < MI_ICP_OCCGRID_KNOWN || which > MI_ICP_OCCGRID_OCCUPIED || capacity < 0)
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad selection or negative capacity", what);
    const OccBox b = occ_bounds_box(o);
    if (b.count == 0) return MI_ICP_OK;
    uint32_t *flags, *pos;
    const uint32_t* total;
    TRY(ensure(c, c->flags, (size_t)b.count, &flags));
    occ_box_flags<<<blocks_for(b.count), 256, 0, c->stream>>>(o->g, b, which, p->occ_prob_thres_log, flags);
    KCHK(c);
    TRY(scan_flags(c, flags, b.count, &pos, &total));
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t cnt = (int64_t)c->u_host[0];
    *m = cnt;
    if (cnt == 0 || capacity < cnt) return MI_ICP_OK;  // nothing is written: the caller learns the room to make
    occ_box_gather<<<blocks_for(b.count), 256, 0, c->stream>>>(o->g, b, f, flags, pos, out_index, out_prob_log, out_xyz);
    KCHK(c);
    return MI_ICP_OK;
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
