// mi_voxel.hip -- PointCloud::VoxelDownSample: the dense-grid path (voxel_dense.h) and the general one (radix passes,
// geometry_kernels.h), and the occupancy of their kernels
// (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "geometry_kernels.h"
#include "lbvh.h"
#include "voxel_dense.h"

using namespace mi;
using namespace mi::eng;
using host::Mat4;

namespace mi {
namespace eng {
int occupancy_geometry(int which) {
    int blocks = -1;
    hipError_t e = hipErrorInvalidValue;
    if (which == 5) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, rs_scatter_pay<8>, kSortThreads, 0);
    else if (which == 6) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, voxel_means_wave, 64, 0);
    else if (which == 7) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, vx_scatter<1>, kVxThreads, 0);
    else if (which == 8) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, vx_finish<false, false>, kVxFinThreads, 0);
    else return -1;
    return e == hipSuccess ? blocks : -2;
}

}  // namespace eng
}  // namespace mi

extern "C" {

static int vx_cu_count() {
    static const int ncu = [] { hipDeviceProp_t p; int dev = 0; (void)hipGetDevice(&dev); return (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256; }();
    return ncu;
}

// the order of LDS adds inside one instruction (voxel_dense.h "Ranks"), checked once per context
static int vx_order_ok(mi_icp_ctx* c, bool* ok) {
    if (c->vx_order == 0) {
        uint32_t* w;
        TRY(ensure(c, c->vx_tab, (size_t)64, &w));
        HIPCHK(c, hipMemsetAsync(w, 0, sizeof(uint32_t), c->stream));
        vx_probe_order<<<64, 256, 0, c->stream>>>(w);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(c->u_host, w, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->vx_order = (c->u_host[0] == 0u) ? 1 : -1;
    }
    *ok = c->vx_order > 0;
    return MI_ICP_OK;
}

// The partition kernels' tables in c->vx_tab, behind `head` words the caller keeps for itself: [ntiles][2048],
// [nsegs][2048], bucket_start[2049], the control words (the rows are sized for 2048 buckets whatever the plan's B is)
struct VxTables {
    uint32_t *head, *tab, *seg_tot, *bucket_start, *ctl;
    int ntiles, nsegs;
};

static int vx_tables(mi_icp_ctx* c, int64_t n, size_t head, VxTables* t) {
    t->ntiles = (int)((n + kVxTile - 1) / kVxTile);
    t->nsegs = (t->ntiles + kVxSeg - 1) / kVxSeg;
    const size_t words = head + ((size_t)t->ntiles + t->nsegs) * kVxMaxBins + kVxMaxBins + 1 + kVxCtlWords;
    TRY(ensure(c, c->vx_tab, words, &t->head));
    t->tab = t->head + head;
    t->seg_tot = t->tab + (size_t)t->ntiles * kVxMaxBins;
    t->bucket_start = t->seg_tot + (size_t)t->nsegs * kVxMaxBins;
    t->ctl = t->bucket_start + kVxMaxBins + 1;
    return MI_ICP_OK;
}

// the arrays that are there (the points always), packed to the front for vx_scatter<na>; returns na
static int vx_pack(const Pay3* const in[3], Pay3* const out[3], VxArrays* a) {
    int na = 0;
    for (int k = 0; k < 3; ++k) {
        a->in[k] = nullptr;
        a->out[k] = nullptr;
    }
    for (int k = 0; k < 3; ++k)
        if (in[k]) {
            a->in[na] = in[k];
            a->out[na] = out[k];
            ++na;
        }
    return na;
}

// one stable partition of the cloud by the plan at d (voxel_dense.h 1-3): the dense path's bucket pass, or one 11-bit
// radix pass of voxel_wide_sort.  Every kernel reads the plan on the device.
static void vx_partition(mi_icp_ctx* c, const VxDev* d, const VxArrays& a, int na, int n, const VxTables& t) {
    vx_hist<<<t.ntiles, kVxThreads, 0, c->stream>>>(a.in[0], n, d, t.tab);
    vx_colsum<<<dim3((unsigned)t.nsegs, (unsigned)(kVxMaxBins / 256)), 256, 0, c->stream>>>(t.tab, t.ntiles, d, t.seg_tot);
    vx_colscan<<<1, 1024, 0, c->stream>>>(t.seg_tot, t.nsegs, n, d, t.bucket_start, t.ctl);
    const int grid = std::min(t.ntiles, vx_cu_count());
    if (na == 1) vx_scatter<1><<<grid, kVxThreads, 0, c->stream>>>(a, n, t.ntiles, d, t.tab, t.seg_tot, t.bucket_start, t.ctl);
    else if (na == 2) vx_scatter<2><<<grid, kVxThreads, 0, c->stream>>>(a, n, t.ntiles, d, t.tab, t.seg_tot, t.bucket_start, t.ctl);
    else vx_scatter<3><<<grid, kVxThreads, 0, c->stream>>>(a, n, t.ntiles, d, t.tab, t.seg_tot, t.bucket_start, t.ctl);
}

// VoxelDownSample of a DENSE grid (voxel_dense.h): every point moves once.  Launched BEHIND the bounds kernels without
// waiting for them: the plan is made on the device (vx_bounds_plan: a packed key of 14 ... 22 bits and enough points per
// bucket), every kernel reads it there and does nothing when the grid is not one for this path.  The caller then waits
// ONCE, for the bounds and this path's control words together.  *launched = false: nothing was started.
static int voxel_dense_launch(mi_icp_ctx* c, const float* const in[3], int64_t n, float voxel, float* const out[3], int mem_kind,
                              bool* launched, float* dst[3]) {
    *launched = false;
    if (std::getenv("MI_ICP_NO_DENSE_VOXEL")) return MI_ICP_OK;  // A/B switch, read at every call (tests compare both paths)
    if (n < (1 << 17) || n > ((int64_t)1 << 26)) return MI_ICP_OK;
    bool ordered = false;
    TRY(vx_order_ok(c, &ordered));
    if (!ordered) return MI_ICP_OK;
    // ahead of the tables: the buckets' occupied-voxel counts, the plan
    const size_t plan_words = (sizeof(VxDev) + 7) / 8 * 2;
    VxTables t;
    TRY(vx_tables(c, n, (size_t)kVxMaxBins + plan_words, &t));
    uint32_t* occ = t.head;
    VxDev* plan = reinterpret_cast<VxDev*>(t.head + (size_t)kVxMaxBins);
    const Pay3* pin[3];
    Pay3* pout[3] = {nullptr, nullptr, nullptr};
    Pay3* tmp[3] = {nullptr, nullptr, nullptr};  // the buckets' means before they are moved together: a slot per cell of the grid
    for (int k = 0; k < 3; ++k) {
        pin[k] = reinterpret_cast<const Pay3*>(in[k]);
        if (in[k]) {
            TRY(ensure(c, c->vpay[k], (size_t)n, &pout[k]));
            TRY(ensure(c, c->vpay[3 + k], (size_t)1 << 22, &tmp[k]));
        }
    }
    TRY(cloud_out(c, in, out, std::min<int64_t>(n, (int64_t)1 << 22), mem_kind, c->stage + 3, dst));
    {   // the bounds (compute_bounds' two launches, the second one making the plan as well)
        float* part;
        TRY(ensure(c, c->bounds_part, (size_t)kBoundsBlocks * 6, &part));
        const int nb = (int)std::min<int64_t>(kBoundsBlocks, blocks_for(n));
        bounds_partial<<<nb, 256, 0, c->stream>>>(in[0], (int)n, part);
        vx_bounds_plan<<<1, 64, 0, c->stream>>>(part, nb, voxel, (long long)n, plan, t.ctl);
    }
    VxArrays a;
    const int na = vx_pack(pin, pout, &a);
    vx_partition(c, plan, a, na, (int)n, t);
#define MI_VX_FINISH(N, C)                                                                                                     \
    vx_finish<N, C><<<std::min(kVxMaxBins, vx_cu_count()), kVxFinThreads, 0, c->stream>>>(pout[0], pout[1], pout[2], plan,   \
                                                                                         t.bucket_start, t.ctl, occ, tmp[0], \
                                                                                         tmp[1], tmp[2])
    if (in[1] && in[2]) MI_VX_FINISH(true, true);
    else if (in[1]) MI_VX_FINISH(true, false);
    else if (in[2]) MI_VX_FINISH(false, true);
    else MI_VX_FINISH(false, false);
#undef MI_VX_FINISH
    vx_compact<<<kVxMaxBins, 256, 0, c->stream>>>(plan, t.ctl, occ, tmp[0], tmp[1], tmp[2], reinterpret_cast<Pay3*>(dst[0]),
                                                   reinterpret_cast<Pay3*>(dst[1]), reinterpret_cast<Pay3*>(dst[2]));
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->u_host, t.ctl, kVxCtlWords * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));  // (with the bounds)
    *launched = true;
    return MI_ICP_OK;
}

// The general path's sort for LARGE clouds on fine grids (the key sorted whole, L = 0): the dense path's partition
// kernels as a radix sort of 11-bit digits -- two or three stable passes for a key of up to 32 bits where 8-bit digits
// take three or four, keys recomputed from the points in every pass instead of carried and stored, four launches a pass
// instead of five.  The plans of the passes (digit = (key >> L) & (B - 1)) are written by the host, which knows the grid
// here.  Its ranks, like the dense path's, need vx_order_ok.  pay[]: the arrays that hold the sorted cloud.
static int voxel_wide_sort(mi_icp_ctx* c, const Pay3* const first[3], int64_t n, const VoxelGrid& grid, int bits, const Pay3* pay[3]) {
    const int npass = (bits + 10) / 11, width = (bits + npass - 1) / npass;
    static_assert(sizeof(VxDev) == 64, "three plans in 192 bytes of the pinned block");
    VxTables t;
    TRY(vx_tables(c, n, 3 * sizeof(VxDev) / 4, &t));
    VxDev* plans = reinterpret_cast<VxDev*>(t.head);
    VxDev* hp = reinterpret_cast<VxDev*>(c->f_host + 16);  // (pinned; [0..7] hold the bounds)
    for (int p = 0; p < npass; ++p) {
        VxDev v;
        v.g = vx_grid(grid, bits);
        v.bits = bits;
        v.L = p * width;
        v.hb = std::min(width, bits - p * width);
        v.B = 1 << v.hb;
        v.ok = 1;
        v.max_bucket = 0xffffffffu;
        v.empty = 0;
        v.pad = 0;
        hp[p] = v;
    }
    HIPCHK(c, hipMemcpyAsync(plans, hp, (size_t)npass * sizeof(VxDev), hipMemcpyHostToDevice, c->stream));
    Pay3* buf[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
    for (int set = 0; set < std::min(npass, 2); ++set)
        for (int a = 0; a < 3; ++a)
            if (first[a]) TRY(ensure(c, c->vpay[set * 3 + a], (size_t)n, &buf[set][a]));
    for (int a = 0; a < 3; ++a) pay[a] = first[a];
    for (int p = 0; p < npass; ++p) {
        VxArrays pk;
        const int na = vx_pack(pay, buf[p & 1], &pk);
        vx_partition(c, plans + p, pk, na, (int)n, t);
        for (int a = 0; a < 3; ++a)
            if (first[a]) pay[a] = buf[p & 1][a];
    }
    KCHK(c);
    return MI_ICP_OK;
}

// VoxelDownSample for grids whose packed (x, y, z) key fits 32 bits (geometry_kernels.h, "the path for grids ..."):
// keys -> radix passes on the bits above the lowest L that carry the payload -> runs of equal key >> L -> which voxels
// occur in each run -> their output positions -> means.  Two host synchronisations in the whole call (the bounds that
// place the grid, the voxel count that sizes the output).
static int voxel_downsample_keys32(mi_icp_ctx* c, const float* const in[3], int64_t n, const VoxelGrid& g, int bits,
                                   float* const out[3], int64_t* m, int mem_kind) {
    SortBuffers sb;
    TRY(sort_buffers(c, n, &sb));
    uint32_t* const keys[2] = {reinterpret_cast<uint32_t*>(sb.keys[0]), reinterpret_cast<uint32_t*>(sb.keys[1])};
    // the lowest L <= 5 key bits stay unsorted where that saves a pass (21 bits: 2 passes, L = 5; 24 bits: 3, L = 0)
    int passes = std::max(0, (bits - 5 + 7) / 8);
    int L = std::min(5, std::max(0, bits - 8 * passes));
    // ... but only where runs are long enough to give a wave work: with more possible runs than an eighth of the points
    // (a fine grid over a sparse cloud: most runs a point or two) the key is sorted whole and 8 lanes take a voxel
    if (L > 0 && (bits - L >= 31 || ((int64_t)1 << (bits - L)) > n / 8)) {
        L = 0;
        passes = (bits + 7) / 8;
    }
    int32_t* const plan = c->last_voxel_plan;
    plan[2] = L;
    plan[3] = passes;
    plan[4] = passes > 0 ? 1 : 0;
    const Pay3* first[3] = {reinterpret_cast<const Pay3*>(in[0]), reinterpret_cast<const Pay3*>(in[1]), reinterpret_cast<const Pay3*>(in[2])};
    const Pay3* pay[3];
    const uint32_t* skeys;
    bool wide = false;
    if (L == 0 && n >= (1 << 17) && n <= ((int64_t)1 << 26) && bits >= 12) TRY(vx_order_ok(c, &wide));
    if (wide) {
        // a large cloud, the key sorted whole: 11-bit digits, the keys made once, from the sorted points
        TRY(voxel_wide_sort(c, first, n, g, bits, pay));
        plan[3] = (bits + 10) / 11;  // (voxel_wide_sort's npass)
        plan[4] = 2;
        voxel_keys32<<<blocks_for(n), 256, 0, c->stream>>>(reinterpret_cast<const float*>(pay[0]), n, g, keys[0]);
        KCHK(c);
        skeys = keys[0];
    } else {
        voxel_keys32<<<blocks_for(n), 256, 0, c->stream>>>(in[0], n, g, keys[0]);
        KCHK(c);
        Pay3* scratch[2][3] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};
        for (int set = 0; set < std::min(passes, 2); ++set)
            for (int a = 0; a < 3; ++a)
                if (first[a]) TRY(ensure(c, c->vpay[set * 3 + a], (size_t)n, &scratch[set][a]));
        const int cur = radix_sort_payload32(c->stream, sb, first, scratch, n, L, bits, pay);
        KCHK(c);
        skeys = keys[cur];
    }
    // runs of equal key >> L
    const int ntiles = scan_num_tiles(n);
    uint32_t *run_start, *mask = nullptr, *voff = nullptr, *tmp = sb.scan_tmp;
    TRY(ensure(c, c->seg_start, (size_t)n + 4, &run_start));
    vox_head_sums<<<ntiles, kScanThreads, 0, c->stream>>>(skeys, (int)n, L, tmp);
    scan_tile_offsets<<<1, kScanThreads, 0, c->stream>>>(tmp, ntiles);
    vox_head_apply<<<ntiles, kScanThreads, 0, c->stream>>>(skeys, (int)n, L, tmp, ntiles, run_start);
    KCHK(c);
    uint32_t* nruns = run_start + n + 2;  // (R, written by vox_head_apply; kept apart: the scan below reuses tmp)
    const uint32_t* total = nruns;
    if (L > 0) {
        const int64_t rmax = (bits - L >= 31) ? n : std::min<int64_t>(n, (int64_t)1 << (bits - L));
        TRY(ensure(c, c->flags, (size_t)n, &mask));
        TRY(ensure(c, c->dense_idx, (size_t)n, &voff));
        vox_run_masks<<<blocks_for(rmax * 16), 256, 0, c->stream>>>(skeys, run_start, nruns, rmax, L, mask, voff);
        KCHK(c);
        TRY(scan_into(c, voff, voff, rmax, &total));  // (in sb.scan_tmp, as the runs' scan above)
    }
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t nvox = (int64_t)c->u_host[0];
    plan[5] = L > 0 ? 1 : (n <= 16 * nvox ? 3 : 2);  // (the branches below)
    plan[6] = (int32_t)nvox;
    TRY(cloud_emit(c, in, out, nvox, nvox, mem_kind, c->stage + 3, [&](float* const dst[3]) {
        if (L > 0) {  // a wave per run
            const int64_t rmax = (bits - L >= 31) ? n : std::min<int64_t>(n, (int64_t)1 << (bits - L));
            voxel_means_wave<<<(unsigned)rmax, 64, 0, c->stream>>>(skeys, pay[0], pay[1], pay[2], run_start, voff, mask, nruns, rmax, L,
                                                                          dst[0], dst[1], dst[2]);
        } else if (n <= 16 * nvox) {  // a run is a voxel, and a short one: a thread each
            voxel_means_thread<<<blocks_for(nvox), 256, 0, c->stream>>>(pay[0], pay[1], pay[2], run_start, nvox, dst[0], dst[1], dst[2]);
        } else {      // a run is a voxel: 8 lanes each
            voxel_means_runs<<<blocks_for(nvox * 8), 256, 0, c->stream>>>(skeys, pay[0], pay[1], pay[2], run_start, voff, mask, nruns, L,
                                                                         nvox, dst[0], dst[1], dst[2]);
        }
    }));
    *m = nvox;
    return MI_ICP_OK;
}

int mi_icp_voxel_downsample(mi_icp_ctx* c, const float* xyz, const float* normals,
                            const float* colors, int64_t n, float voxel, float* out_xyz,
                            float* out_normals, float* out_colors, int64_t* m, int mem_kind) {
    TRY(check_sizes(c, "voxel_downsample", n, m, mem_kind));
    c->last_voxel_path = -1;
    std::memset(c->last_voxel_plan, 0, sizeof(c->last_voxel_plan));  // (mi_icp_debug_last_voxel_plan: what this call decides, below)
    if (n == 0 || !(voxel > 0.0f)) return MI_ICP_OK;  // down_sample.cu:173-176
    Cloud cl{{xyz, normals, colors}, {out_xyz, out_normals, out_colors}};
    TRY(cloud_in(c, "voxel_downsample", &cl, n, mem_kind, c->stage));
    const float* const* in = cl.in;
    float* const* out = cl.out;

    // a dense grid: one move of every point (voxel_dense.h), started behind the bounds without waiting for them; the
    // bounds come back with its control words
    bool dense = false;
    float* dst[3];
    // (a context whose last call with this voxel size and a cloud of about this size was turned away by the plan -- a grid
    // of too many or too few cells -- does not try again: the attempt is seven launches that do nothing, ~25 us in front
    // of the general path.  Speed only; a stream of scans of one scene is the case in mind.)
    const bool turned_away = c->vx_refused_voxel == voxel && n >= c->vx_refused_n / 2 && n <= c->vx_refused_n * 2;
    if (!turned_away) TRY(voxel_dense_launch(c, in, n, voxel, out, mem_kind, &dense, dst));
    if (!dense) {
        float* bnd;
        TRY(compute_bounds(c, in[0], n, &bnd));
        HIPCHK(c, hipMemcpyAsync(c->f_host, bnd, 8 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (dense) {
        std::memcpy(c->f_host, c->u_host + kVxCtlBounds, 6 * sizeof(float));
        if (c->u_host[0] == 2u) {
            c->vx_refused_voxel = voxel;
            c->vx_refused_n = n;
        } else {
            c->vx_refused_n = 0;
        }
    }
    if (dense && c->u_host[0] == 0u) {  // (1: the cloud crowds into a few buckets, 2: not a grid for that path -- nothing was written)
        const int64_t nvox = (int64_t)c->u_host[2];
        TRY(cloud_out_back(c, dst, out, nvox, mem_kind));
        if (dst[0] != out[0]) HIPCHK(c, hipStreamSynchronize(c->stream));  // (staged: the copies; device arrays: already waited for)
        *m = nvox;
        c->last_voxel_path = 1;
        {   // the plan word: the key's bits as the device plan counted them (the same bounds, the same function); no sort, vx_finish
            const VoxelGridFit df = voxel_grid_fit(c->f_host, voxel);
            c->last_voxel_plan[1] = df.bits[0] + df.bits[1] + df.bits[2];
            c->last_voxel_plan[6] = (int32_t)nvox;
        }
        return MI_ICP_OK;
    }
    const VoxelGridFit f = voxel_grid_fit(c->f_host, voxel);
    if (f.overflow) return MI_ICP_OK;
    c->last_voxel_path = 0;
    const VoxelGrid& g = f.g;
    const int bits = f.bits[0] + f.bits[1] + f.bits[2];
    int32_t* const plan = c->last_voxel_plan;
    plan[1] = bits;

    // (grids whose packed key needs more than 32 bits keep the first form below: 64-bit keys + indices, one gather)
    if (bits <= 32) return voxel_downsample_keys32(c, in, n, g, bits, out, m, mem_kind);

    const float* dp = in[0];
    SortBuffers sb;
    TRY(sort_buffers(c, n, &sb));
    const uint32_t* order;
    const uint64_t* packed_sorted = nullptr;  // sorted voxel keys when one key identifies the voxel
    const int nb = blocks_for(n);
    if (bits <= 64) {
        voxel_keys<<<nb, 256, 0, c->stream>>>(dp, n, g, -1, nullptr, sb.keys[0], sb.vals[0]);
        KCHK(c);
        const int cur = radix_sort_pairs<uint64_t>(c->stream, sb, n, bits);
        plan[3] = (bits + 7) / 8;  // (radix_sort_pairs' passes)
        plan[4] = 3;
        order = sb.vals[cur];
        packed_sorted = sb.keys[cur];
    } else {
        // three stable sorts, least significant axis first
        const uint32_t* prev = nullptr;
        for (int axis = 2; axis >= 0; --axis) {
            uint32_t* tmp_order = nullptr;
            if (prev) {  // keys are rebuilt from the current order; keep it out of the sort's way
                TRY(ensure(c, c->seg_start, (size_t)n + 1, &tmp_order));
                HIPCHK(c, hipMemcpyAsync(tmp_order, prev, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
            }
            voxel_keys<<<nb, 256, 0, c->stream>>>(dp, n, g, axis, tmp_order, sb.keys[0], sb.vals[0]);
            KCHK(c);
            prev = sb.vals[radix_sort_pairs<uint64_t>(c->stream, sb, n, f.bits[axis])];
            plan[3] += (f.bits[axis] + 7) / 8;
        }
        plan[4] = 4;
        order = prev;
    }
    KCHK(c);

    uint32_t *head, *pos, *seg_start;
    const uint32_t* total;
    TRY(ensure(c, c->flags, (size_t)n, &head));
    if (packed_sorted) voxel_heads_keys<<<nb, 256, 0, c->stream>>>(packed_sorted, n, head);
    else voxel_heads<<<nb, 256, 0, c->stream>>>(dp, n, g, order, head);
    KCHK(c);
    TRY(scan_flags(c, head, n, &pos, &total));
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t nvox = (int64_t)c->u_host[0];
    plan[5] = 4;
    plan[6] = (int32_t)nvox;
    // `order` may live in seg_start's buffer only in the fallback's intermediate rounds, never at the end
    TRY(ensure(c, c->seg_start, (size_t)n + 1, &seg_start));
    voxel_seg_starts<<<nb, 256, 0, c->stream>>>(head, pos, n, seg_start);
    KCHK(c);
    TRY(cloud_emit(c, in, out, nvox, nvox, mem_kind, c->stage + 3, [&](float* const d3[3]) {
        voxel_means<<<blocks_for(nvox * 8), 256, 0, c->stream>>>(dp, in[1], in[2], order, seg_start, nvox, n, d3[0], d3[1], d3[2]);
    }));
    *m = nvox;
    return MI_ICP_OK;
}

}  // extern "C"
