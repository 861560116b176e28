// mi_collision.hip -- collision::ComputeIntersection (grids against grids, line sets and primitives) and CreateVoxelGrid
// of a primitive (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "collision_kernels.h"

#include <climits>

using namespace mi;
using namespace mi::eng;

// ---------------------------------------------------------------------------
// The contract is in include/mi_icp.h ("collision"), the kernels in collision_kernels.h.  A call prepares the side that is
// searched (ColGrid), then the enumerated side, launches one kernel that leaves hit[i] per enumerated element, and
// compacts: flags, the scan, one wait for the count, the pairs.  Scratch: stage[0] hit, stage[1] the primitives' reach,
// stage[3] / stage[4] a VoxelGrid's sorted copy and its permutation, stage[5] an occupancy grid's listed voxels,
// bounds the key extents.

static bool is_grid(const mi_icp_collision_side* s) { return s->kind == MI_ICP_COLLISION_VOXELGRID || s->kind == MI_ICP_COLLISION_OCCGRID; }

static int64_t side_count(const mi_icp_collision_side* s) {
    switch (s->kind) {
        case MI_ICP_COLLISION_VOXELGRID: return s->m;
        case MI_ICP_COLLISION_LINESET: return s->n_lines;
        case MI_ICP_COLLISION_PRIMITIVES: return s->n_primitives;
        default: return 1;  // (an occupancy grid's count is known only after it is listed)
    }
}

static int side_check(mi_icp_ctx* c, const char* what, const mi_icp_collision_side* s) {
    switch (s->kind) {
        case MI_ICP_COLLISION_VOXELGRID: {
            TRY(count_ok(c, what, s->m));
            if (s->m > 0 && !s->keys) return fail(c, MI_ICP_ERR_INVALID, "%s: null keys", what);
            GridFrame f;  // (an empty grid's frame is not looked at)
            return s->m > 0 ? frame_check(c, what, s->voxel_size, s->origin, &f) : MI_ICP_OK;
        }
        case MI_ICP_COLLISION_OCCGRID: {
            const mi_icp_occgrid_params& p = s->grid_params;
            if (!(p.voxel_size > 0.0f) || !std::isfinite(p.voxel_size) || !finite3(p.origin) || std::isnan(p.occ_prob_thres_log))
                return fail(c, MI_ICP_ERR_INVALID, "%s: voxel_size must be positive and finite, the origin finite, the threshold a number", what);
            return MI_ICP_OK;
        }
        case MI_ICP_COLLISION_LINESET:
            TRY(count_ok(c, what, s->n_lines));
            TRY(count_ok(c, what, s->n_points));
            if (s->n_lines > 0 && (!s->lines || (s->n_points > 0 && !s->points))) return fail(c, MI_ICP_ERR_INVALID, "%s: null lines or points", what);
            return MI_ICP_OK;
        case MI_ICP_COLLISION_PRIMITIVES:
            TRY(count_ok(c, what, s->n_primitives));
            if (s->n_primitives > 0 && !s->primitives) return fail(c, MI_ICP_ERR_INVALID, "%s: null primitives", what);
            return MI_ICP_OK;
        default: return fail(c, MI_ICP_ERR_INVALID, "%s: bad side kind %d", what, (int)s->kind);
    }
}

// a grid side's frame: a VoxelGrid's own, an occupancy grid's from its parameters
static GridFrame side_frame(const mi_icp_collision_side* s) {
    const bool occ = s->kind == MI_ICP_COLLISION_OCCGRID;
    const float* o = occ ? s->grid_params.origin : s->origin;
    return {occ ? s->grid_params.voxel_size : s->voxel_size, {o[0], o[1], o[2]}};
}

// the side that is searched; *none: it has no voxel a query could meet
static int make_grid(mi_icp_ctx* c, const char* what, const mi_icp_collision_side* s, ColGrid* G, bool* none) {
    std::memset(G, 0, sizeof(*G));
    *none = false;
    G->f = side_frame(s);
    if (s->kind == MI_ICP_COLLISION_OCCGRID) {
        TRY(occgrid_view(c, s->grid, what, &G->prob, &G->res, G->b));
        G->occ = 1;
        G->h = G->res / 2;
        G->thres = s->grid_params.occ_prob_thres_log;
        *none = box_of_bounds(G->b).count == 0;
        return MI_ICP_OK;
    }
    G->keys = s->keys;
    G->m = s->m;
    if (s->keys_sorted && s->keys_index) G->perm = reinterpret_cast<const uint32_t*>(s->keys_index);
    if (s->m > 1 && !s->keys_sorted) {  // a scratch copy, sorted once, distinct, with the caller's index of every key
        VgRuns r;
        TRY(vg_sort_runs(c, s->keys, s->m, &r));
        if (r.nvox == 0) {
            *none = true;
            return MI_ICP_OK;
        }
        int32_t* sorted;
        uint32_t* perm;
        TRY(ensure(c, c->stage[3], (size_t)s->m * 3, &sorted));
        TRY(ensure(c, c->stage[4], (size_t)s->m, &perm));
        vg_emit_keys<<<blocks_for(r.nvox), 256, 0, c->stream>>>(s->keys, r.order, r.run_start, r.nvox, sorted);
        KCHK(c);
        col_run_heads<<<blocks_for(r.nvox), 256, 0, c->stream>>>(r.order, r.run_start, r.nvox, perm);
        KCHK(c);
        G->keys = sorted;
        G->perm = perm;
        G->m = r.nvox;
    }
    int32_t *part, *ext;
    TRY(ensure(c, c->bounds_part, (size_t)kVgBlocks * 8, &part));
    TRY(ensure(c, c->bounds, 8, &ext));
    const int rb = std::min(kVgBlocks, blocks_for(G->m));
    vg_key_bounds_partial<<<rb, 256, 0, c->stream>>>(G->keys, G->m, part);
    KCHK(c);
    vg_key_bounds_final<<<1, 64, 0, c->stream>>>(part, rb, ext);
    KCHK(c);
    G->ext = ext;
    return MI_ICP_OK;
}

// the enumerated voxels of a grid side; an occupancy grid is listed first (one wait)
static int make_cells(mi_icp_ctx* c, const char* what, const mi_icp_collision_side* s, ColCells* E) {
    std::memset(E, 0, sizeof(*E));
    E->f = side_frame(s);
    if (s->kind == MI_ICP_COLLISION_VOXELGRID) {
        E->keys = s->keys;
        E->n = s->m;
        return MI_ICP_OK;
    }
    const float* prob;
    int bd[6];
    TRY(occgrid_view(c, s->grid, what, &prob, &E->res, bd));
    E->h = E->res / 2;
    int64_t n;
    TRY(occgrid_select(c, s->grid, MI_ICP_OCCGRID_OCCUPIED, s->grid_params.occ_prob_thres_log, &n));
    if (n == 0) return MI_ICP_OK;
    int32_t* list;
    TRY(ensure(c, c->stage[5], (size_t)n * 3, &list));
    TRY(occgrid_gather(c, s->grid, E->f, list, nullptr, nullptr));
    E->keys = list;
    E->n = n;
    return MI_ICP_OK;
}

extern "C" {

int mi_icp_collision_compute(mi_icp_ctx* c, const mi_icp_collision_side* a, const mi_icp_collision_side* b, float margin,
                             int32_t* out_pairs, int64_t capacity, int64_t* m) {
    const char* what = "collision_compute";
    TRY(check_ctx(c));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    if (!a || !b) return fail(c, MI_ICP_ERR_INVALID, "%s: null side", what);
    if (capacity < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: negative capacity", what);
    if (!std::isfinite(margin) || margin < 0.0f) return fail(c, MI_ICP_ERR_INVALID, "%s: the margin must be finite and >= 0", what);
    TRY(side_check(c, what, a));
    TRY(side_check(c, what, b));
    // which side is enumerated: the lines whenever there are lines, else B; the other one is searched
    const bool pair_ok = (is_grid(a) && is_grid(b) && !(a->kind == MI_ICP_COLLISION_OCCGRID && b->kind == MI_ICP_COLLISION_OCCGRID)) ||
                         (is_grid(a) && (b->kind == MI_ICP_COLLISION_LINESET || b->kind == MI_ICP_COLLISION_PRIMITIVES)) ||
                         (is_grid(b) && (a->kind == MI_ICP_COLLISION_LINESET || a->kind == MI_ICP_COLLISION_PRIMITIVES));
    if (!pair_ok) return fail(c, MI_ICP_ERR_INVALID, "%s: this pair of kinds (%d, %d) is not built", what, (int)a->kind, (int)b->kind);
    const bool a_enumerated = a->kind == MI_ICP_COLLISION_LINESET;
    const mi_icp_collision_side* en = a_enumerated ? a : b;
    const mi_icp_collision_side* ot = a_enumerated ? b : a;
    if (side_count(a) == 0 || side_count(b) == 0) return MI_ICP_OK;  // an empty side: no launch

    if (en->kind == MI_ICP_COLLISION_LINESET) {  // every point index inside [0, n_points), else nothing is written
        uint32_t* status;
        TRY(ensure(c, c->flags, 1, &status));
        HIPCHK(c, hipMemsetAsync(status, 0, sizeof(uint32_t), c->stream));
        col_check_lines<<<blocks_for(en->n_lines), 256, 0, c->stream>>>(en->lines, en->n_lines, en->n_points, status);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(c->u_host, status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->u_host[0]) return fail(c, MI_ICP_ERR_INVALID, "%s: a line's point index is out of range [0, %lld)", what, (long long)en->n_points);
    }

    if (a->kind == MI_ICP_COLLISION_PRIMITIVES || b->kind == MI_ICP_COLLISION_PRIMITIVES) {  // no box with a skewed or scaled rotation
        const mi_icp_collision_side* pr = a->kind == MI_ICP_COLLISION_PRIMITIVES ? a : b;
        uint32_t* status;
        TRY(ensure(c, c->flags, 1, &status));
        HIPCHK(c, hipMemsetAsync(status, 0, sizeof(uint32_t), c->stream));
        col_check_prims<<<blocks_for(pr->n_primitives), 256, 0, c->stream>>>(pr->primitives, pr->n_primitives, status);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(c->u_host, status, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->u_host[0]) return fail(c, MI_ICP_ERR_INVALID, "%s: a box's rotation is not orthonormal within 1e-4 (scaled or skewed)", what);
    }

    int32_t* hit = nullptr;
    int64_t n = 0;
    const int32_t* occ_index = nullptr;
    int occ_res = 0;
    if (ot->kind == MI_ICP_COLLISION_PRIMITIVES) {  // voxels against primitives
        ColCells E;
        TRY(make_cells(c, what, en, &E));
        if (E.n == 0) return MI_ICP_OK;
        float* reach;
        TRY(ensure(c, c->stage[1], (size_t)ot->n_primitives * 6, &reach));
        TRY(ensure(c, c->stage[0], (size_t)E.n, &hit));
        col_prim_reach<<<blocks_for(ot->n_primitives), 256, 0, c->stream>>>(ot->primitives, ot->n_primitives, margin, E.f.vs, reach);
        KCHK(c);
        col_cells_prims<<<blocks_for(E.n), 256, 0, c->stream>>>(E, ot->primitives, reach, ot->n_primitives, margin, hit);
        KCHK(c);
        n = E.n;
        if (E.res > 0) {
            occ_index = E.keys;
            occ_res = E.res;
        }
    } else {
        ColGrid G;
        bool none;
        TRY(make_grid(c, what, ot, &G, &none));
        if (none) return MI_ICP_OK;
        if (is_grid(en)) {
            ColCells E;
            TRY(make_cells(c, what, en, &E));
            if (E.n == 0) return MI_ICP_OK;
            TRY(ensure(c, c->stage[0], (size_t)E.n, &hit));
            col_cells_grid<<<blocks_for(E.n), 256, 0, c->stream>>>(E, G, margin, hit);
            n = E.n;
            if (E.res > 0) {
                occ_index = E.keys;
                occ_res = E.res;
            }
        } else if (en->kind == MI_ICP_COLLISION_LINESET) {
            n = en->n_lines;
            TRY(ensure(c, c->stage[0], (size_t)n, &hit));
            col_lines_grid<<<blocks_for(n, 4), 256, 0, c->stream>>>(en->points, en->lines, n, G, margin, hit);
        } else {
            n = en->n_primitives;
            TRY(ensure(c, c->stage[0], (size_t)n, &hit));
            col_prims_grid<<<(unsigned)n, 256, 0, c->stream>>>(en->primitives, n, G, margin, hit);
        }
        KCHK(c);
    }

    uint32_t *flags, *pos;
    const uint32_t* total;
    TRY(ensure(c, c->flags, (size_t)n, &flags));
    col_hit_flags<<<blocks_for(n), 256, 0, c->stream>>>(hit, n, flags);
    KCHK(c);
    TRY(scan_flags(c, flags, n, &pos, &total));
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t cnt = (int64_t)c->u_host[0];
    *m = cnt;
    if (cnt == 0 || capacity < cnt) return MI_ICP_OK;  // nothing is written: the caller learns the room to make
    if (!out_pairs) return fail(c, MI_ICP_ERR_INVALID, "%s: null output", what);
    col_emit_pairs<<<blocks_for(n), 256, 0, c->stream>>>(hit, pos, n, a_enumerated ? 1 : 0, occ_index, occ_res, out_pairs);
    KCHK(c);
    return MI_ICP_OK;
}

int mi_icp_collision_sort_keys(mi_icp_ctx* c, const int32_t* keys, int64_t m, int32_t* out_keys, int32_t* out_index, int64_t* m_out) {
    const char* what = "collision_sort_keys";
    TRY(check_ctx(c));
    if (!m_out) return fail(c, MI_ICP_ERR_INVALID, "%s: m_out is null", what);
    *m_out = 0;
    TRY(count_ok(c, what, m));
    if (m == 0) return MI_ICP_OK;
    if (!keys || !out_keys || !out_index) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    VgRuns r;
    TRY(vg_sort_runs(c, keys, m, &r));
    *m_out = r.nvox;
    if (r.nvox == 0) return MI_ICP_OK;
    vg_emit_keys<<<blocks_for(r.nvox), 256, 0, c->stream>>>(keys, r.order, r.run_start, r.nvox, out_keys);
    KCHK(c);
    col_run_heads<<<blocks_for(r.nvox), 256, 0, c->stream>>>(r.order, r.run_start, r.nvox, reinterpret_cast<uint32_t*>(out_index));
    KCHK(c);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

int mi_icp_primitive_aabb(const mi_icp_primitive* primitive, float* out_min3, float* out_max3) {
    if (!primitive || !out_min3 || !out_max3) return MI_ICP_ERR_INVALID;
    col::primitive_aabb(*primitive, out_min3, out_max3);
    return MI_ICP_OK;
}

int mi_icp_collision_voxelize_primitive(mi_icp_ctx* c, const mi_icp_primitive* primitive, float voxel_size, int32_t* out_keys,
                                        float* out_colors, int64_t capacity, int64_t* m, float* out_origin3) {
    const char* what = "collision_voxelize_primitive";
    TRY(check_ctx(c));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    if (!primitive) return fail(c, MI_ICP_ERR_INVALID, "%s: null primitive", what);
    if (capacity < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: negative capacity", what);
    if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size)) return fail(c, MI_ICP_ERR_INVALID, "[CreateVoxelGrid] voxel_size <= 0.");
    if (primitive->type != MI_ICP_PRIMITIVE_BOX && primitive->type != MI_ICP_PRIMITIVE_SPHERE && primitive->type != MI_ICP_PRIMITIVE_CAPSULE)
        return fail(c, MI_ICP_ERR_INVALID, "[CreateVoxelGrid] Unsupported primitive type.");
    if (!col::primitive_finite(*primitive)) return fail(c, MI_ICP_ERR_INVALID, "%s: a field of the primitive is not finite", what);
    if (primitive->type == MI_ICP_PRIMITIVE_BOX && !col::box_rotation_ok(primitive->transform))
        return fail(c, MI_ICP_ERR_INVALID, "[CreateVoxelGrid] the box's rotation is not orthonormal within 1e-4 (scaled or skewed).");
    mi_icp_primitive P = *primitive;
    float mn[3], mx[3];
    col::primitive_aabb(P, mn, mx);
    int num[3];
    for (int k = 0; k < 3; ++k) {
        const float origin = P.transform[12 + k];
        if (out_origin3) out_origin3[k] = origin;
        const float min_b = (mn[k] - origin) - voxel_size * 0.5f, max_b = (mx[k] - origin) + voxel_size * 0.5f;
        const float cells = roundf((max_b - min_b) / voxel_size);
        if (!(cells <= (float)INT_MAX)) return fail(c, MI_ICP_ERR_INVALID, "%s: more than 2^31 - 1 cells", what);
        num[k] = cells < 1.0f ? 0 : (int)cells;
        P.transform[12 + k] = 0.0f;
    }
    if (num[0] == 0 || num[1] == 0 || num[2] == 0) return MI_ICP_OK;
    const int64_t wh = (int64_t)num[0] * num[1];
    if (wh > (int64_t)INT_MAX || wh * num[2] > (int64_t)INT_MAX) return fail(c, MI_ICP_ERR_INVALID, "%s: more than 2^31 - 1 cells", what);
    ColDense D;
    D.nw = num[0];
    D.nh = num[1];
    D.nd = num[2];
    D.total = wh * num[2];
    D.vs = voxel_size;
    uint32_t *flags, *pos;
    const uint32_t* total;
    TRY(ensure(c, c->flags, (size_t)D.total, &flags));
    col_voxelize_flags<<<blocks_for(D.total), 256, 0, c->stream>>>(P, D, flags);
    KCHK(c);
    TRY(scan_flags(c, flags, D.total, &pos, &total));
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t cnt = (int64_t)c->u_host[0];
    *m = cnt;
    if (cnt == 0 || capacity < cnt) return MI_ICP_OK;
    if (!out_keys || !out_colors) return fail(c, MI_ICP_ERR_INVALID, "%s: null output", what);
    col_voxelize_emit<<<blocks_for(D.total), 256, 0, c->stream>>>(D, flags, pos, out_keys, out_colors);
    KCHK(c);
    return MI_ICP_OK;
}

}  // extern "C"
