// mi_geometry.hip -- the geometry entry points beside the registration: Transform, bounds / centre, Translate / Scale /
// Rotate, GICP covariances, VoxelDownSample, depth / RGB-D frame -> cloud, RGB-D odometry, colours
// SelectByIndex / SelectByMask / UniformDownSample, and the compaction behind them and the outlier filters; SegmentPlane;
// FarthestPointDownSample, PassThroughFilter / Crop / RemoveNoneFinitePoints; UniformTSDFVolume
// (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "depth_kernels.h"
#include "farthest_point.h"
#include "geometry_kernels.h"
#include "lbvh.h"
#include "odometry.h"
#include "reduce.h"
#include "segment_plane.h"
#include "select.h"
#include "tsdf_kernels.h"
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

// Where up to `count` points of an output cloud (points, normals, colours) go: the caller's arrays out[], or (MI_ICP_HOST)
// stage[0..2]; nullptr for an attribute that in[] does not have.  cloud_out_back copies `m` of them to the caller.
static int cloud_out(mi_icp_ctx* c, const float* const in[3], float* const out[3], int64_t count, int mem_kind,
                     DevBuf* stage, float* dst[3]) {
    for (int k = 0; k < 3; ++k) TRY(out_slot(c, in[k] ? out[k] : nullptr, (size_t)count * 3, mem_kind, stage[k], &dst[k]));
    return MI_ICP_OK;
}

static int cloud_out_back(mi_icp_ctx* c, float* const dst[3], float* const out[3], int64_t m, int mem_kind) {
    for (int k = 0; k < 3; ++k)
        if (dst[k]) TRY(from_device(c, (const float*)dst[k], out[k], (size_t)m * 3, mem_kind));
    return MI_ICP_OK;
}

int compact_by_flags(mi_icp_ctx* c, const uint32_t* flags, int64_t n, const float* const in[3], float* const out[3],
                     int64_t* out_idx, int mem_kind, const uint32_t* status, int64_t* m, uint32_t* status_out) {
    *m = 0;
    if (status_out) *status_out = 0u;
    if (n <= 0) return MI_ICP_OK;
    uint32_t *pos, *tmp;
    TRY(ensure(c, c->dense_idx, (size_t)n, &pos));
    TRY(ensure(c, c->scan_tmp, (size_t)scan_num_tiles(n) + 2, &tmp));
    exclusive_scan_u32(c->stream, flags, pos, n, tmp);
    KCHK(c);
    float* dst[3];
    int64_t* didx;
    TRY(cloud_out(c, in, out, n, mem_kind, c->vpay, dst));
    TRY(out_slot(c, out_idx, (size_t)n, mem_kind, c->pairs_out, &didx));
    select_gather<<<blocks_for(n), 256, 0, c->stream>>>(flags, pos, n, in[0], in[1], in[2], dst[0], dst[1], dst[2], didx);
    KCHK(c);
    // the count (and the caller's status word) come back with the one wait of the call
    HIPCHK(c, hipMemcpyAsync(c->u_host, tmp + scan_num_tiles(n), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
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
    const Pay3* first[3] = {reinterpret_cast<const Pay3*>(in[0]), reinterpret_cast<const Pay3*>(in[1]), reinterpret_cast<const Pay3*>(in[2])};
    const Pay3* pay[3];
    const uint32_t* skeys;
    bool wide = false;
    if (L == 0 && n >= (1 << 17) && n <= ((int64_t)1 << 26) && bits >= 12) TRY(vx_order_ok(c, &wide));
    if (wide) {
        // a large cloud, the key sorted whole: 11-bit digits, the keys made once, from the sorted points
        TRY(voxel_wide_sort(c, first, n, g, bits, pay));
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
        exclusive_scan_u32(c->stream, voff, voff, rmax, tmp);
        KCHK(c);
        total = tmp + scan_num_tiles(rmax);
    }
    HIPCHK(c, hipMemcpyAsync(c->u_host, total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t nvox = (int64_t)c->u_host[0];
    float* dst[3];
    TRY(cloud_out(c, in, out, nvox, mem_kind, c->stage + 3, dst));
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
    KCHK(c);
    TRY(cloud_out_back(c, dst, out, nvox, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *m = nvox;
    return MI_ICP_OK;
}

int mi_icp_voxel_downsample(mi_icp_ctx* c, const float* xyz, const float* normals,
                            const float* colors, int64_t n, float voxel, float* out_xyz,
                            float* out_normals, float* out_colors, int64_t* m, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "voxel_downsample"));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "voxel_downsample: m is null");
    *m = 0;
    c->last_voxel_path = -1;
    if (n < 0 || n > 0x7fffff00ll) return fail(c, MI_ICP_ERR_INVALID, "voxel_downsample: bad size");
    if (n == 0 || !(voxel > 0.0f)) return MI_ICP_OK;  // down_sample.cu:173-176
    if (!xyz || !out_xyz || (normals && !out_normals) || (colors && !out_colors))
        return fail(c, MI_ICP_ERR_INVALID, "voxel_downsample: null buffer");

    const float* in[3];
    TRY(to_device(c, xyz, (size_t)n * 3, mem_kind, c->stage[0], &in[0]));
    TRY(to_device(c, normals, (size_t)n * 3, mem_kind, c->stage[1], &in[1]));
    TRY(to_device(c, colors, (size_t)n * 3, mem_kind, c->stage[2], &in[2]));
    float* const out[3] = {out_xyz, out_normals, out_colors};

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
        return MI_ICP_OK;
    }
    const VoxelGridFit f = voxel_grid_fit(c->f_host, voxel);
    if (f.overflow) return MI_ICP_OK;
    c->last_voxel_path = 0;
    const VoxelGrid& g = f.g;
    const int bits = f.bits[0] + f.bits[1] + f.bits[2];

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
        }
        order = prev;
    }
    KCHK(c);

    uint32_t *head, *pos, *seg_start, *tmp;
    TRY(ensure(c, c->flags, (size_t)n, &head));
    TRY(ensure(c, c->dense_idx, (size_t)n, (uint32_t**)&pos));
    // `order` may live in seg_start's buffer only in the fallback's intermediate rounds, never at the end
    TRY(ensure(c, c->scan_tmp, (size_t)scan_num_tiles(n) + 2, &tmp));
    if (packed_sorted) voxel_heads_keys<<<nb, 256, 0, c->stream>>>(packed_sorted, n, head);
    else voxel_heads<<<nb, 256, 0, c->stream>>>(dp, n, g, order, head);
    KCHK(c);
    exclusive_scan_u32(c->stream, head, pos, n, tmp);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->u_host, tmp + scan_num_tiles(n), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t nvox = (int64_t)c->u_host[0];
    TRY(ensure(c, c->seg_start, (size_t)n + 1, &seg_start));
    voxel_seg_starts<<<nb, 256, 0, c->stream>>>(head, pos, n, seg_start);
    KCHK(c);

    TRY(cloud_out(c, in, out, nvox, mem_kind, c->stage + 3, dst));
    voxel_means<<<blocks_for(nvox * 8), 256, 0, c->stream>>>(dp, in[1], in[2], order, seg_start, nvox, n, dst[0], dst[1], dst[2]);
    KCHK(c);
    TRY(cloud_out_back(c, dst, out, nvox, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *m = nvox;
    return MI_ICP_OK;
}

// ---------------------------------------------------------------------------
// PointCloud::SelectByIndex (geometry/down_sample.cu:40-62,110-129)
int mi_icp_select_by_index(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                           const int64_t* indices, int64_t n_indices, int invert, float* out_xyz, float* out_normals,
                           float* out_colors, int64_t* m, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "select_by_index"));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "select_by_index: m is null");
    *m = 0;
    if (n < 0 || n > 0x7fffff00ll || n_indices < 0 || n_indices > 0x7fffff00ll)
        return fail(c, MI_ICP_ERR_INVALID, "select_by_index: bad size");
    if ((n > 0 && !xyz) || (n_indices > 0 && !indices)) return fail(c, MI_ICP_ERR_INVALID, "select_by_index: null buffer");
    const int64_t count = invert ? n : n_indices;  // the most points the output can hold
    if (count > 0 && (!out_xyz || (normals && !out_normals) || (colors && !out_colors)))
        return fail(c, MI_ICP_ERR_INVALID, "select_by_index: null buffer");
    if (n == 0 && n_indices > 0) return fail(c, MI_ICP_ERR_INVALID, "select_by_index: index out of range [0, 0)");
    if (count == 0) return MI_ICP_OK;

    const float* in[3];
    TRY(to_device(c, xyz, (size_t)n * 3, mem_kind, c->stage[0], &in[0]));
    TRY(to_device(c, normals, (size_t)n * 3, mem_kind, c->stage[1], &in[1]));
    TRY(to_device(c, colors, (size_t)n * 3, mem_kind, c->stage[2], &in[2]));
    const int64_t* idx = nullptr;
    TRY(to_device(c, indices, (size_t)n_indices, mem_kind, c->keys0, &idx));
    float* const out[3] = {out_xyz, out_normals, out_colors};
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
    TRY(check_ctx(c, mem_kind, what));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    if (n < 0 || n > 0x7fffff00ll) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    if (n_mask != n)
        return fail(c, MI_ICP_ERR_INVALID, "%s: the mask has %lld entries, the cloud %lld points", what, (long long)n_mask, (long long)n);
    if (n == 0) return MI_ICP_OK;
    if (!xyz || !mask || !out_xyz || (normals && !out_normals) || (colors && !out_colors))
        return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const float* in[3];
    TRY(to_device(c, xyz, (size_t)n * 3, mem_kind, c->stage[0], &in[0]));
    TRY(to_device(c, normals, (size_t)n * 3, mem_kind, c->stage[1], &in[1]));
    TRY(to_device(c, colors, (size_t)n * 3, mem_kind, c->stage[2], &in[2]));
    const uint8_t* dmask;
    TRY(to_device(c, mask, (size_t)n, mem_kind, c->keys0, &dmask));
    uint32_t* flags;
    TRY(ensure(c, c->flags, (size_t)n, &flags));
    select_mask_flags<<<blocks_for(n), 256, 0, c->stream>>>(dmask, n, invert, flags);
    KCHK(c);
    float* const out[3] = {out_xyz, out_normals, out_colors};
    return compact_by_flags(c, flags, n, in, out, nullptr, mem_kind, nullptr, m, nullptr);
}

// PointCloud::UniformDownSample (geometry/down_sample.cu:275-316): points 0, k, 2k, ... -- n / k of them (the size the
// reference allocates).  A strided copy per attribute, no kernel.
int mi_icp_uniform_downsample(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                              int64_t every_k_points, float* out_xyz, float* out_normals, float* out_colors, int64_t* m,
                              int mem_kind) {
    TRY(check_ctx(c, mem_kind, "uniform_downsample"));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "uniform_downsample: m is null");
    *m = 0;
    if (n < 0) return fail(c, MI_ICP_ERR_INVALID, "uniform_downsample: bad size");
    if (every_k_points <= 0) return fail(c, MI_ICP_ERR_INVALID, "uniform_downsample: every_k_points must be positive");
    const int64_t cnt = n / every_k_points;
    if (cnt == 0) return MI_ICP_OK;
    if (!xyz || !out_xyz || (normals && !out_normals) || (colors && !out_colors))
        return fail(c, MI_ICP_ERR_INVALID, "uniform_downsample: null buffer");
    const float* const in[3] = {xyz, normals, colors};
    float* const out[3] = {out_xyz, out_normals, out_colors};
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
    TRY(check_ctx(c, mem_kind, what));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    if (n < 0 || n > 0x7fffff00ll) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    if (num_samples < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: num_samples must not be negative", what);
    if (num_samples > n)
        return fail(c, MI_ICP_ERR_INVALID, "%s: %lld samples asked of %lld points", what, (long long)num_samples, (long long)n);
    if (num_samples == 0) return MI_ICP_OK;
    if (!xyz || !out_xyz || (normals && !out_normals) || (colors && !out_colors))
        return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const float* in[3];
    TRY(to_device(c, xyz, (size_t)n * 3, mem_kind, c->stage[0], &in[0]));
    TRY(to_device(c, normals, (size_t)n * 3, mem_kind, c->stage[1], &in[1]));
    TRY(to_device(c, colors, (size_t)n * 3, mem_kind, c->stage[2], &in[2]));
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
    float* const out[3] = {out_xyz, out_normals, out_colors};
    float* dst[3];
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
    if (!xyz || !out_xyz || (normals && !out_normals) || (colors && !out_colors))
        return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    const float* in[3];
    TRY(to_device(c, xyz, (size_t)n * 3, mem_kind, c->stage[0], &in[0]));
    TRY(to_device(c, normals, (size_t)n * 3, mem_kind, c->stage[1], &in[1]));
    TRY(to_device(c, colors, (size_t)n * 3, mem_kind, c->stage[2], &in[2]));
    uint32_t* flags;
    TRY(ensure(c, c->flags, (size_t)n, &flags));
    launch_flags(in[0], flags);
    KCHK(c);
    float* const out[3] = {out_xyz, out_normals, out_colors};
    return compact_by_flags(c, flags, n, in, out, out_idx, mem_kind, nullptr, m, nullptr);
}

extern "C" {

static int predicate_args(mi_icp_ctx* c, const char* what, int64_t n, int64_t* m, int mem_kind) {
    TRY(check_ctx(c, mem_kind, what));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    if (n < 0 || n > 0x7fffff00ll) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    return MI_ICP_OK;
}

int mi_icp_pass_through_filter(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                               int axis_no, float min_bound, float max_bound, float* out_xyz, float* out_normals,
                               float* out_colors, int64_t* out_idx, int64_t* m, int mem_kind) {
    const char* what = "pass_through_filter";
    TRY(predicate_args(c, what, n, m, mem_kind));
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
    TRY(predicate_args(c, what, n, m, mem_kind));
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
    TRY(predicate_args(c, what, n, m, mem_kind));
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
    TRY(check_ctx(c, mem_kind, what));
    if (!plane4 || !m) return fail(c, MI_ICP_ERR_INVALID, "%s: plane4 or m is null", what);
    for (int k = 0; k < 4; ++k) {
        plane4[k] = 0.0f;
        if (ransac_plane4) ransac_plane4[k] = 0.0f;
    }
    *m = 0;
    if (best_iteration) *best_iteration = -1;
    if (best_count) *best_count = 0;
    if (n < 0 || n > 0x7fffff00ll) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
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
        uint32_t *words, *flags, *pos, *tmp;
        double *tie, *sums;
        int64_t* didx;
        const size_t hw = (size_t)std::max(H, 1);
        TRY(ensure(a, a->seg[0], hw, &plane));
        TRY(ensure(a, a->seg[1], 3 * hw + sizeof(SegState) / sizeof(uint32_t), &words));
        TRY(ensure(a, a->seg[2], hw * kSegTieBlocks, &tie));
        TRY(ensure(a, a->seg[3], (size_t)kSegRefitBlocks * 8 + 4, &sums));
        TRY(ensure(a, a->flags, (size_t)n, &flags));
        TRY(ensure(a, a->dense_idx, (size_t)n, &pos));
        TRY(ensure(a, a->scan_tmp, (size_t)scan_num_tiles(n) + 2, &tmp));
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
        exclusive_scan_u32(s, flags, pos, n, tmp);
        seg_list<<<nb, 256, 0, s>>>(flags, pos, n, didx);
        seg_centroid_partial<<<rb, 256, 0, s>>>(pts, flags, n, sums);
        seg_centroid_final<<<1, 64, 0, s>>>(sums, rb, centroid);
        seg_moments_partial<<<rb, 256, 0, s>>>(pts, flags, n, centroid, sums);
        seg_refit_final<<<1, 64, 0, s>>>(sums, rb, centroid, st);
        KCHK(a);
        constexpr int kStateWords = (int)(sizeof(SegState) / sizeof(uint32_t));
        static_assert(kStateWords + 1 <= 16, "the state and the count share the 16 pinned words");
        HIPCHK(a, hipMemcpyAsync(a->u_host, st, sizeof(SegState), hipMemcpyDeviceToHost, s));
        HIPCHK(a, hipMemcpyAsync(a->u_host + kStateWords, tmp + scan_num_tiles(n), sizeof(uint32_t), hipMemcpyDeviceToHost, s));
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
// PointCloud::CreateFromDepthImage / CreateFromRGBDImage (geometry/pointcloud_factory.cu)
static bool invert4(const float* M, float* out) {  // column-major general inverse, in double
    double a[4][8];
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) {
            a[r][k] = (double)M[k * 4 + r];
            a[r][4 + k] = (r == k) ? 1.0 : 0.0;
        }
    for (int col = 0; col < 4; ++col) {
        int piv = col;
        for (int r = col + 1; r < 4; ++r)
            if (std::fabs(a[r][col]) > std::fabs(a[piv][col])) piv = r;
        if (!(std::fabs(a[piv][col]) > 0.0)) return false;
        if (piv != col)
            for (int k = 0; k < 8; ++k) std::swap(a[piv][k], a[col][k]);
        const double d = a[col][col];
        for (int k = 0; k < 8; ++k) a[col][k] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == col) continue;
            const double f = a[r][col];
            if (f != 0.0)
                for (int k = 0; k < 8; ++k) a[r][k] -= f * a[col][k];
        }
    }
    for (int r = 0; r < 4; ++r)
        for (int k = 0; k < 4; ++k) out[k * 4 + r] = (float)a[r][4 + k];
    return true;
}

int mi_icp_create_from_depth(mi_icp_ctx* c, const void* depth, int depth_type, const void* color, int color_type,
                             int width, int height, const float* intrinsic4, const float* extrinsic,
                             float depth_scale, float depth_trunc, float depth_cutoff, int stride, int rgbd,
                             int compute_normals, int valid_only, float* out_xyz, float* out_normals,
                             float* out_colors, int64_t* m, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "create_from_depth"));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: m is null");
    *m = 0;
    if (width < 0 || height < 0 || stride < 1 || !intrinsic4 || (depth_type != MI_ICP_DEPTH_F32 && depth_type != MI_ICP_DEPTH_U16) ||
        (color_type != MI_ICP_COLOR_NONE && color_type != MI_ICP_COLOR_U8X3 && color_type != MI_ICP_COLOR_F32X1))
        return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: bad arguments");
    if (rgbd && (stride != 1 || depth_type != MI_ICP_DEPTH_F32))
        return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: an RGB-D image has a float depth and stride 1");
    if (!rgbd && (color || compute_normals || !valid_only))
        return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: colours, normals and valid_only = 0 belong to the RGB-D form");
    if ((color != nullptr) != (color_type != MI_ICP_COLOR_NONE))
        return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: color and color_type disagree");
    const int64_t npix = (int64_t)width * height;
    const int64_t count = (int64_t)(width / stride) * (height / stride);
    if (npix > 0x7fffff00ll) return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: image too large");
    if (count == 0) return MI_ICP_OK;
    if (!depth || !out_xyz || (color && !out_colors) || (compute_normals && !out_normals))
        return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: null buffer");

    DepthArgs a;
    const size_t dbytes = (size_t)npix * (depth_type == MI_ICP_DEPTH_U16 ? 2 : 4);
    const size_t cbytes = color ? (size_t)npix * (color_type == MI_ICP_COLOR_U8X3 ? 3 : 4) : 0;
    const uint8_t *dd, *dc;
    TRY(to_device(c, (const uint8_t*)depth, dbytes, mem_kind, c->stage[0], &dd));
    TRY(to_device(c, (const uint8_t*)color, cbytes, mem_kind, c->stage[1], &dc));
    a.depth = dd;
    a.color = dc;
    a.width = width;
    a.height = height;
    a.stride = stride;
    a.depth_u16 = depth_type == MI_ICP_DEPTH_U16;
    a.color_kind = color_type;
    a.rgbd = rgbd ? 1 : 0;
    a.depth_scale = (int)depth_scale;  // image.cu:340-343 holds both as int
    a.depth_trunc = (int)depth_trunc;
    a.depth_cutoff = depth_cutoff;
    a.fx = intrinsic4[0];
    a.fy = intrinsic4[1];
    a.cx = intrinsic4[2];
    a.cy = intrinsic4[3];
    const Mat4 E = load_T(extrinsic);
    if (!invert4(E.data(), a.pose)) return fail(c, MI_ICP_ERR_INVALID, "create_from_depth: singular extrinsic");

    const int nb = blocks_for(count);
    uint32_t* pos = nullptr;
    int64_t kept = count;
    if (valid_only) {
        uint32_t* tmp;
        TRY(ensure(c, c->flags, (size_t)count, &pos));
        TRY(ensure(c, c->scan_tmp, (size_t)scan_num_tiles(count) + 2, &tmp));
        depth_valid_flags<<<nb, 256, 0, c->stream>>>(a, count, pos);
        KCHK(c);
        exclusive_scan_u32(c->stream, pos, pos, count, tmp);
        KCHK(c);
        HIPCHK(c, hipMemcpyAsync(c->u_host, tmp + scan_num_tiles(count), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        kept = (int64_t)c->u_host[0];
    }
    float* const out[3] = {out_xyz, compute_normals ? out_normals : nullptr, color ? out_colors : nullptr};
    float* dst[3];
    TRY(cloud_out(c, out, out, count, mem_kind, c->stage + 3, dst));
    depth_emit<<<nb, 256, 0, c->stream>>>(a, count, pos, dst[0], dst[1], dst[2]);
    KCHK(c);
    TRY(cloud_out_back(c, dst, out, kept, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *m = kept;
    return MI_ICP_OK;
}

// ---------------------------------------------------------------------------
// odometry::ComputeRGBDOdometry (odometry/odometry.cu); helpers above the extern "C" block
static int rgbd_odometry_impl(mi_icp_ctx* c, const float* source_color, const float* source_depth,
                              const float* target_color, const float* target_depth, int width, int height,
                              const float* intrinsic4, const float* odo_init, int jacobian,
                              const mi_icp_odometry_option* option, int* success, float* transformation16,
                              double* information36, int mem_kind, bool weighted, const float* prev_twist6,
                              float* twist6) {
    TRY(check_ctx(c, mem_kind, "compute_rgbd_odometry"));
    c->od_levels = 0;  // (mi_icp_debug_odometry_image: nothing to show until this call has run)
    if (twist6)
        for (int i = 0; i < 6; ++i) twist6[i] = 0.0f;
    if (!success || !transformation16 || !information36 || !intrinsic4 || !option)
        return fail(c, MI_ICP_ERR_INVALID, "compute_rgbd_odometry: null argument");
    *success = 0;
    const Mat4 I4 = host::identity4();
    std::memcpy(transformation16, I4.data(), 16 * sizeof(float));
    for (int i = 0; i < 36; ++i) information36[i] = (i % 7 == 0) ? 1.0 : 0.0;
    if (width <= 0 || height <= 0 || (int64_t)width * height > 0x3fffffffll || !source_color || !source_depth ||
        !target_color || !target_depth)
        return fail(c, MI_ICP_ERR_INVALID, "compute_rgbd_odometry: bad image arguments");
    if (jacobian != MI_ICP_ODOMETRY_COLOR_TERM && jacobian != MI_ICP_ODOMETRY_HYBRID_TERM)
        return fail(c, MI_ICP_ERR_INVALID, "compute_rgbd_odometry: unknown jacobian type %d", jacobian);
    const int L = option->num_levels;
    if (L < 1 || L > MI_ICP_ODOMETRY_MAX_LEVELS || (width >> (L - 1)) < 1 || (height >> (L - 1)) < 1)
        return fail(c, MI_ICP_ERR_INVALID, "compute_rgbd_odometry: bad number of pyramid levels");

    const int64_t n0 = (int64_t)width * height;
    const float *in_sc, *in_sd, *in_tc, *in_td;
    TRY(to_device(c, source_color, (size_t)n0, mem_kind, c->stage[0], &in_sc));
    TRY(to_device(c, source_depth, (size_t)n0, mem_kind, c->stage[1], &in_sd));
    TRY(to_device(c, target_color, (size_t)n0, mem_kind, c->stage[2], &in_tc));
    TRY(to_device(c, target_depth, (size_t)n0, mem_kind, c->stage[3], &in_td));

    // one arena: per level colour + depth of both frames, a scratch image, and (target) 4 gradient images
    int lw[MI_ICP_ODOMETRY_MAX_LEVELS], lh[MI_ICP_ODOMETRY_MAX_LEVELS];
    size_t total = 0;
    for (int l = 0; l < L; ++l) {
        lw[l] = l ? lw[l - 1] / 2 : width;
        lh[l] = l ? lh[l - 1] / 2 : height;
        total += (size_t)lw[l] * lh[l] * 8;
    }
    total += (size_t)n0 + 64;
    float* arena;
    TRY(ensure(c, c->stage[4], total, &arena));
    double *sums, *rows;  // the 32 totals; the rows of od_accumulate's larger grids (the ICP reduction's row buffer: transient there too)
    TRY(ensure(c, c->sys_dev, kSysSize, &sums));
    TRY(ensure(c, c->partial, (size_t)kSysSize * kOdMaxBlocks, &rows));
    float *col[2][MI_ICP_ODOMETRY_MAX_LEVELS], *dep[2][MI_ICP_ODOMETRY_MAX_LEVELS], *grad[4][MI_ICP_ODOMETRY_MAX_LEVELS];
    {
        float* p = arena;
        for (int l = 0; l < L; ++l) {
            const size_t n = (size_t)lw[l] * lh[l];
            for (int s = 0; s < 2; ++s) {
                col[s][l] = p;
                p += n;
                dep[s][l] = p;
                p += n;
            }
            for (int g = 0; g < 4; ++g) {
                grad[g][l] = p;
                p += n;
            }
        }
    }
    float* scratch = arena + (total - (size_t)n0 - 64);
    auto blocks = [](int64_t n) { return (int)((n + kOdThreads - 1) / kOdThreads); };

    // ---- InitializeRGBDOdometry (odometry.cu:498-528)
    for (int s = 0; s < 2; ++s) {
        od_filter3<0, false><<<blocks(n0), kOdThreads, 0, c->stream>>>(s ? in_tc : in_sc, width, height, col[s][0], 0.0f, 0.0f);
        od_filter3<0, true><<<blocks(n0), kOdThreads, 0, c->stream>>>(s ? in_td : in_sd, width, height, dep[s][0],
                                                                       option->min_depth, option->max_depth);
    }
    KCHK(c);
    OdCamera cam[MI_ICP_ODOMETRY_MAX_LEVELS];
    {
        const float k0[9] = {intrinsic4[0], 0.0f, intrinsic4[2], 0.0f, intrinsic4[1], intrinsic4[3], 0.0f, 0.0f, 1.0f};
        std::memcpy(cam[0].k, k0, sizeof(k0));
        for (int l = 1; l < L; ++l) {  // CreateCameraMatrixPyramid (:332-347)
            for (int i = 0; i < 9; ++i) cam[l].k[i] = (float)(0.5 * (double)cam[l - 1].k[i]);
            cam[l].k[8] = 1.0f;
        }
    }
    // the running transformation and everything derived from it live on the device (OdState);
    // the host enqueues the whole run and synchronises once, at the end
    float* state_mem;
    TRY(ensure(c, c->stage[5], sizeof(OdState) / sizeof(float) + 16, &state_mem));
    OdState* state = reinterpret_cast<OdState*>(state_mem);
    const Mat4 init = load_T(odo_init);
    if (!c->od_host) HIPCHK(c, hipHostMalloc(&c->od_host, sizeof(OdState) + 64, hipHostMallocDefault));
    OdState* hst = reinterpret_cast<OdState*>(c->od_host);
    if (weighted) {  // the weighted variant's constants and its velocity, once
        std::memset(hst, 0, sizeof(OdState));
        hst->vel = I4;
        hst->sigma2 = option->sigma2_init;
        hst->nu = option->nu;
        for (int i = 0; i < 6; ++i) {
            hst->prev_twist[i] = prev_twist6 ? prev_twist6[i] : 0.0f;
            hst->inv_sigma[i] = option->inv_sigma_mat_diag[i];
        }
        HIPCHK(c, hipMemcpyAsync(state, hst, sizeof(OdState), hipMemcpyHostToDevice, c->stream));
    }
    // (two pinned slots: an asynchronous copy reads its host source when it executes, so the second
    // value must not overwrite the first one's source)
    Mat4* t_slots[2] = {&hst->T, reinterpret_cast<Mat4*>(reinterpret_cast<char*>(c->od_host) + sizeof(OdState))};
    int t_slot = 0;
    auto set_T = [&](const Mat4& T) -> int {
        Mat4* src = t_slots[t_slot++ & 1];
        *src = T;
        HIPCHK(c, hipMemcpyAsync(&state->T, src, sizeof(Mat4), hipMemcpyHostToDevice, c->stream));
        return MI_ICP_OK;
    };
    HIPCHK(c, hipMemsetAsync(sums, 0, 32 * sizeof(double), c->stream));
    OdArgs a{};
    a.out = sums;
    a.rows = rows;
    a.state = state;
    a.max_depth_diff = option->max_depth_diff;
    auto level_args = [&](int l) {
        a.depth_s = dep[0][l];
        a.depth_t = dep[1][l];
        a.color_s = col[0][l];
        a.color_t = col[1][l];
        a.dx_color = grad[0][l];
        a.dy_color = grad[1][l];
        a.dx_depth = grad[2][l];
        a.dy_depth = grad[3][l];
        a.w = lw[l];
        a.h = lh[l];
    };
    auto grid_for = [&](int l) {
        const int64_t n = (int64_t)lw[l] * lh[l];
        return (int)std::min<int64_t>(kOdMaxBlocks, std::max<int64_t>(1, (n + kOdThreads - 1) / kOdThreads));
    };
    // rows left by an evaluation of level l for whoever consumes its sums (0: it added to the totals itself)
    auto rows_of = [&](int l) { const int g = grid_for(l); return g > kOdAtomicBlocks ? g : 0; };
    {   // NormalizeIntensity (:416-436) over the correspondences under odo_init
        TRY(set_T(init));
        od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[0], 0, rows, 0);
        level_args(0);
        od_accumulate<kOdMeans><<<grid_for(0), kOdThreads, 0, c->stream>>>(a);
        if (rows_of(0)) od_total<<<1, kOdStepThreads, 0, c->stream>>>(rows, rows_of(0), sums);
        od_scale_by_mean<<<blocks(n0), kOdThreads, 0, c->stream>>>(col[0][0], n0, sums, 0);
        od_scale_by_mean<<<blocks(n0), kOdThreads, 0, c->stream>>>(col[1][0], n0, sums, 1);
        KCHK(c);
    }
    // ---- pyramids (rgbdimage.cu:96-112, image_factory.cu:251-278): colour Gaussian3 + Downsample,
    // depth Downsample only; Sobel3Dx / Sobel3Dy of the target per level (RGBDImage::FilterPyramid)
    for (int l = 1; l < L; ++l) {
        const int64_t np = (int64_t)lw[l - 1] * lh[l - 1], nn = (int64_t)lw[l] * lh[l];
        for (int s = 0; s < 2; ++s) {
            od_filter3<0, false><<<blocks(np), kOdThreads, 0, c->stream>>>(col[s][l - 1], lw[l - 1], lh[l - 1], scratch, 0.0f, 0.0f);
            od_downsample<<<blocks(nn), kOdThreads, 0, c->stream>>>(scratch, lw[l - 1], lh[l - 1], col[s][l]);
            od_downsample<<<blocks(nn), kOdThreads, 0, c->stream>>>(dep[s][l - 1], lw[l - 1], lh[l - 1], dep[s][l]);
        }
    }
    for (int l = 0; l < L; ++l) {
        const int64_t n = (int64_t)lw[l] * lh[l];
        od_filter3<1, false><<<blocks(n), kOdThreads, 0, c->stream>>>(col[1][l], lw[l], lh[l], grad[0][l], 0.0f, 0.0f);
        od_filter3<2, false><<<blocks(n), kOdThreads, 0, c->stream>>>(col[1][l], lw[l], lh[l], grad[1][l], 0.0f, 0.0f);
        od_filter3<1, false><<<blocks(n), kOdThreads, 0, c->stream>>>(dep[1][l], lw[l], lh[l], grad[2][l], 0.0f, 0.0f);
        od_filter3<2, false><<<blocks(n), kOdThreads, 0, c->stream>>>(dep[1][l], lw[l], lh[l], grad[3][l], 0.0f, 0.0f);
    }
    KCHK(c);

    // ---- ComputeMultiscale (:708-764): one accumulate + one step launch per iteration
    {
        bool zero = true;
        for (int i = 0; i < 16; ++i) zero = zero && (init.data()[i] == 0.0f);
        TRY(set_T(zero ? I4 : init));
        od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[L - 1], 0, rows, 0);  // terms for the coarsest level; zeroes the sums
    }
    for (int level = L - 1; level >= 0; --level) {
        level_args(level);
        const int iters = option->iterations[L - level - 1];
        for (int iter = 0; iter < iters; ++iter) {
            // the next evaluation: this level again, the next finer one, or level 0 (information matrix)
            const int next = (iter + 1 < iters) ? level : std::max(level - 1, 0);
            if (weighted) {  // two passes: the weights' normalisation, then the weighted system
                od_accumulate<kOdWeightSum><<<grid_for(level), kOdThreads, 0, c->stream>>>(a);
                od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[level], 3, rows, rows_of(level));
                od_accumulate<kOdWeighted><<<grid_for(level), kOdThreads, 0, c->stream>>>(a);
                od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[next], 2, rows, rows_of(level));
                continue;
            }
            if (jacobian == MI_ICP_ODOMETRY_COLOR_TERM) od_accumulate<kOdColor><<<grid_for(level), kOdThreads, 0, c->stream>>>(a);
            else od_accumulate<kOdHybrid><<<grid_for(level), kOdThreads, 0, c->stream>>>(a);
            od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[next], 1, rows, rows_of(level));
        }
        if (iters <= 0 && level > 0) od_step<<<1, kOdStepThreads, 0, c->stream>>>(state, sums, cam[level - 1], 0, rows, 0);
    }
    KCHK(c);
    // CreateInformationMatrix (:349-394): I + sum G^T G over the final correspondences
    level_args(0);
    od_accumulate<kOdInformation><<<grid_for(0), kOdThreads, 0, c->stream>>>(a);
    if (rows_of(0)) od_total<<<1, kOdStepThreads, 0, c->stream>>>(rows, rows_of(0), sums);
    KCHK(c);
    HIPCHK(c, hipMemcpyAsync(c->sys_host, sums, 32 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(&hst->T, &state->T, sizeof(Mat4), hipMemcpyDeviceToHost, c->stream));
    if (weighted) HIPCHK(c, hipMemcpyAsync(&hst->vel, &state->vel, sizeof(Mat4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (weighted && twist6) od_matrix4_to_vector6(hst->vel, twist6);
    {
        int k = 0;
        for (int r = 0; r < 6; ++r)
            for (int q = r; q < 6; ++q, ++k) {
                information36[r * 6 + q] += c->sys_host[k];
                if (q != r) information36[q * 6 + r] += c->sys_host[k];
            }
        std::memcpy(transformation16, hst->T.data(), 16 * sizeof(float));
        *success = 1;  // without its determinant check the solver never reports failure (utility/eigen.cu:76-122)
    }
    for (int l = 0; l < L; ++l) {  // what mi_icp_debug_odometry_image hands out
        c->od_lw[l] = lw[l];
        c->od_lh[l] = lh[l];
        const float* img[8] = {col[0][l], dep[0][l], col[1][l], dep[1][l], grad[0][l], grad[1][l], grad[2][l], grad[3][l]};
        for (int k = 0; k < 8; ++k) c->od_img[l][k] = img[k];
    }
    c->od_levels = L;
    return MI_ICP_OK;
}

int mi_icp_compute_rgbd_odometry(mi_icp_ctx* c, const float* source_color, const float* source_depth,
                                 const float* target_color, const float* target_depth, int width, int height,
                                 const float* intrinsic4, const float* odo_init, int jacobian,
                                 const mi_icp_odometry_option* option, int* success, float* transformation16,
                                 double* information36, int mem_kind) {
    return rgbd_odometry_impl(c, source_color, source_depth, target_color, target_depth, width, height, intrinsic4,
                              odo_init, jacobian, option, success, transformation16, information36, mem_kind, false,
                              nullptr, nullptr);
}

int mi_icp_compute_weighted_rgbd_odometry(mi_icp_ctx* c, const float* source_color, const float* source_depth,
                                          const float* target_color, const float* target_depth, int width, int height,
                                          const float* intrinsic4, const float* odo_init, const float* prev_twist6,
                                          const mi_icp_odometry_option* option, int* success, float* transformation16,
                                          float* twist6, double* information36, int mem_kind) {
    if (!twist6) return c ? fail(c, MI_ICP_ERR_INVALID, "compute_weighted_rgbd_odometry: twist6 is null") : MI_ICP_ERR_INVALID;
    return rgbd_odometry_impl(c, source_color, source_depth, target_color, target_depth, width, height, intrinsic4,
                              odo_init, MI_ICP_ODOMETRY_HYBRID_TERM, option, success, transformation16, information36,
                              mem_kind, true, prev_twist6, twist6);
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

// ---------------------------------------------------------------------------
// integration::UniformTSDFVolume (integration/uniform_tsdfvolume.cu; tsdf_kernels.h).  A volume belongs to the context
// that made it and is freed with it at the latest.
struct mi_icp_tsdf {
    mi_icp_ctx* owner = nullptr;
    TsdfVol v = {};
    float length = 0.0f, sdf_trunc = 0.0f;
    DevBuf planes;  // tsdf, weight and, with a colour type, three colour planes
    DevBuf mult;    // the depth -> camera-distance multiplier image of the intrinsic below
    int mult_w = 0, mult_h = 0;
    float mult_k[4] = {0, 0, 0, 0};
};

namespace mi {
namespace eng {
void tsdf_release_all(mi_icp_ctx* c) {
    for (mi_icp_tsdf* t : c->tsdf_volumes) {
        release(t->planes);
        release(t->mult);
        delete t;
    }
    c->tsdf_volumes.clear();
}
}  // namespace eng
}  // namespace mi

static int tsdf_check(mi_icp_ctx* c, const mi_icp_tsdf* t, const char* what) {
    if (!t || t->owner != c || std::find(c->tsdf_volumes.begin(), c->tsdf_volumes.end(), t) == c->tsdf_volumes.end())
        return fail(c, MI_ICP_ERR_INVALID, "%s: not a volume of this context", what);
    return MI_ICP_OK;
}

// the count the scan left behind `tiles` tile sums, with one wait
static int tsdf_scan_total(mi_icp_ctx* c, const uint32_t* tmp, int64_t n, int64_t* total) {
    HIPCHK(c, hipMemcpyAsync(c->u_host, tmp + scan_num_tiles(n), sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    *total = (int64_t)c->u_host[0];
    return MI_ICP_OK;
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
    v.n = (int64_t)resolution * resolution * resolution;
    v.voxel_length = length / (float)resolution;
    v.half = 0.5f * v.voxel_length;
    for (int k = 0; k < 3; ++k) v.origin[k] = origin3 ? origin3[k] : 0.0f;
    v.color_type = color_type;
    float* base;
    const int rc = ensure(c, t->planes, (size_t)v.n * (color_type == MI_ICP_TSDF_NO_COLOR ? 2 : 5), &base);
    if (rc != MI_ICP_OK) {
        delete t;
        return rc;
    }
    v.tsdf = base;
    v.weight = base + v.n;
    v.color = color_type == MI_ICP_TSDF_NO_COLOR ? nullptr : base + 2 * v.n;
    tsdf_reset<<<blocks_for(v.n), 256, 0, c->stream>>>(v);
    if (hipGetLastError() != hipSuccess) {
        release(t->planes);
        delete t;
        return fail(c, MI_ICP_ERR_HIP, "tsdf_create: launch failed");
    }
    c->tsdf_volumes.push_back(t);
    *out = t;
    return MI_ICP_OK;
}

int mi_icp_tsdf_destroy(mi_icp_ctx* c, mi_icp_tsdf* t) {
    TRY(check_ctx(c));
    if (!t) return MI_ICP_OK;
    TRY(tsdf_check(c, t, "tsdf_destroy"));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->tsdf_volumes.erase(std::find(c->tsdf_volumes.begin(), c->tsdf_volumes.end(), t));
    release(t->planes);
    release(t->mult);
    delete t;
    return MI_ICP_OK;
}

int mi_icp_tsdf_reset(mi_icp_ctx* c, mi_icp_tsdf* t) {
    TRY(check_ctx(c));
    TRY(tsdf_check(c, t, "tsdf_reset"));
    tsdf_reset<<<blocks_for(t->v.n), 256, 0, c->stream>>>(t->v);
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
    if (!intrinsic4) return fail(c, MI_ICP_ERR_INVALID, "%s: null intrinsic", what);
    const int ct = t->v.color_type;
    // the reference's format checks (uniform_tsdfvolume.cu:677-695)
    if (depth_channels != 1 || depth_bytes_per_channel != 4 || depth_width != width || depth_height != height ||
        (ct == MI_ICP_TSDF_RGB8 && (color_channels != 3 || color_bytes_per_channel != 1)) ||
        (ct == MI_ICP_TSDF_GRAY32 && (color_channels != 1 || color_bytes_per_channel != 4)) ||
        (ct != MI_ICP_TSDF_NO_COLOR && (color_width != width || color_height != height)))
        return fail(c, MI_ICP_ERR_INVALID, "[UniformTSDFVolume::Integrate] Unsupported image format.");
    if (width < 1 || height < 1 || width > MI_ICP_TSDF_MAX_IMAGE_SIDE || height > MI_ICP_TSDF_MAX_IMAGE_SIDE)
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad image size (a side is at most %d)", what, MI_ICP_TSDF_MAX_IMAGE_SIDE);
    if (!depth || (ct != MI_ICP_TSDF_NO_COLOR && !color)) return fail(c, MI_ICP_ERR_INVALID, "%s: null image", what);
    const int64_t npix = (int64_t)width * height;
    const float fx = intrinsic4[0], fy = intrinsic4[1], cx = intrinsic4[2], cy = intrinsic4[3];

    if (!t->mult.p || t->mult_w != width || t->mult_h != height || std::memcmp(t->mult_k, intrinsic4, sizeof(float) * 4) != 0) {
        float* m;
        TRY(ensure(c, t->mult, (size_t)npix, &m));
        tsdf_multiplier<<<blocks_for(npix), 256, 0, c->stream>>>(m, width, height, cx, cy, 1.0f / fx, 1.0f / fy);
        KCHK(c);
        t->mult_w = width;
        t->mult_h = height;
        std::memcpy(t->mult_k, intrinsic4, sizeof(float) * 4);
    }

    TsdfIntegrate a;
    const uint8_t *dd, *dc;
    TRY(to_device(c, (const uint8_t*)depth, (size_t)npix * 4, mem_kind, c->stage[0], &dd));
    TRY(to_device(c, (const uint8_t*)(ct == MI_ICP_TSDF_NO_COLOR ? nullptr : color),
                  (size_t)npix * (ct == MI_ICP_TSDF_RGB8 ? 3 : 4), mem_kind, c->stage[1], &dc));
    a.depth = (const float*)dd;
    a.color = dc;
    a.mult = (const float*)t->mult.p;
    const Mat4 E = load_T(extrinsic);
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 4; ++k) a.E[r][k] = E.data()[k * 4 + r];
        a.D[r] = t->v.voxel_length * a.E[r][2];
    }
    a.fx = fx;
    a.fy = fy;
    a.cx = cx;
    a.cy = cy;
    a.width = width;
    a.height = height;
    a.safe_w = (float)width - 0.0001f;
    a.safe_h = (float)height - 0.0001f;
    a.sdf_trunc = t->sdf_trunc;
    a.sdf_trunc_inv = (float)(1.0 / (double)t->sdf_trunc);
    a.cull = (std::fabs(cx) <= 65536.0f && std::fabs(cy) <= 65536.0f) ? 1 : 0;  // (the sides are at most 2^15)
    a.k_left = cx + 1.5f;
    a.k_right = ((float)width + 0.5f) - cx;
    a.k_top = cy + 1.5f;
    a.k_bottom = ((float)height + 0.5f) - cy;
    const int zchunks = (t->v.res + 255) / 256;
    tsdf_integrate<<<(unsigned)((int64_t)t->v.res * t->v.res * zchunks), 256, 0, c->stream>>>(t->v, a, zchunks);
    KCHK(c);
    if (mem_kind == MI_ICP_HOST) HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's images may go now
    return MI_ICP_OK;
}

static int tsdf_extract_args(mi_icp_ctx* c, mi_icp_tsdf* t, const char* what, int64_t capacity, int64_t* m, int mem_kind) {
    TRY(check_ctx(c, mem_kind, what));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    TRY(tsdf_check(c, t, what));
    if (capacity < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: negative capacity", what);
    return MI_ICP_OK;
}

int mi_icp_tsdf_extract_voxel_point_cloud(mi_icp_ctx* c, mi_icp_tsdf* t, float* out_xyz, float* out_colors, int64_t capacity,
                                          int64_t* m, int mem_kind) {
    const char* what = "tsdf_extract_voxel_point_cloud";
    TRY(tsdf_extract_args(c, t, what, capacity, m, mem_kind));
    const int64_t n = t->v.n;
    uint32_t *flags, *pos, *tmp;
    TRY(ensure(c, c->flags, (size_t)n, &flags));
    TRY(ensure(c, c->dense_idx, (size_t)n, &pos));
    TRY(ensure(c, c->scan_tmp, (size_t)scan_num_tiles(n) + 2, &tmp));
    tsdf_voxel_flags<<<blocks_for(n), 256, 0, c->stream>>>(t->v, flags);
    KCHK(c);
    exclusive_scan_u32(c->stream, flags, pos, n, tmp);
    KCHK(c);
    int64_t cnt;
    TRY(tsdf_scan_total(c, tmp, n, &cnt));
    *m = cnt;
    if (cnt == 0 || capacity < cnt) return MI_ICP_OK;
    if (!out_xyz || !out_colors) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    float* const out[3] = {out_xyz, nullptr, out_colors};
    float* dst[3];
    TRY(cloud_out(c, out, out, cnt, mem_kind, c->vpay, dst));
    tsdf_voxel_gather<<<blocks_for(n), 256, 0, c->stream>>>(t->v, flags, pos, dst[0], dst[2]);
    KCHK(c);
    TRY(cloud_out_back(c, dst, out, cnt, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

int mi_icp_tsdf_extract_point_cloud(mi_icp_ctx* c, mi_icp_tsdf* t, float* out_xyz, float* out_normals, float* out_colors,
                                    int64_t capacity, int64_t* m, int mem_kind) {
    const char* what = "tsdf_extract_point_cloud";
    TRY(tsdf_extract_args(c, t, what, capacity, m, mem_kind));
    const int64_t r2 = t->v.res - 2, n = r2 * r2 * r2;  // the interior voxels; each has three candidate edges
    uint32_t *count, *pos, *tmp;
    TRY(ensure(c, c->flags, (size_t)n, &count));
    TRY(ensure(c, c->dense_idx, (size_t)n, &pos));
    TRY(ensure(c, c->scan_tmp, (size_t)scan_num_tiles(n) + 2, &tmp));
    tsdf_cloud_count<<<blocks_for(n), 256, 0, c->stream>>>(t->v, n, count);
    KCHK(c);
    exclusive_scan_u32(c->stream, count, pos, n, tmp);
    KCHK(c);
    int64_t cnt;
    TRY(tsdf_scan_total(c, tmp, n, &cnt));
    *m = cnt;
    if (cnt == 0 || capacity < cnt) return MI_ICP_OK;
    const bool colored = t->v.color_type != MI_ICP_TSDF_NO_COLOR;
    if (!out_xyz || !out_normals || (colored && !out_colors)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    float* const out[3] = {out_xyz, out_normals, colored ? out_colors : nullptr};
    float* dst[3];
    TRY(cloud_out(c, out, out, cnt, mem_kind, c->vpay, dst));
    tsdf_cloud_gather<<<blocks_for(n), 256, 0, c->stream>>>(t->v, n, count, pos, dst[0], dst[1], dst[2]);
    KCHK(c);
    TRY(cloud_out_back(c, dst, out, cnt, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

int mi_icp_tsdf_raycast(mi_icp_ctx* c, mi_icp_tsdf* t, int width, int height, const float* intrinsic4, const float* extrinsic,
                        float sdf_trunc, int valid_only, float* out_xyz, float* out_normals, float* out_colors,
                        int64_t capacity, int64_t* m, int mem_kind) {
    const char* what = "tsdf_raycast";
    TRY(tsdf_extract_args(c, t, what, capacity, m, mem_kind));
    if (!intrinsic4 || width < 0 || height < 0 || width > MI_ICP_TSDF_MAX_IMAGE_SIDE || height > MI_ICP_TSDF_MAX_IMAGE_SIDE)
        return fail(c, MI_ICP_ERR_INVALID, "%s: bad arguments (an image side is at most %d)", what, MI_ICP_TSDF_MAX_IMAGE_SIDE);
    // the march takes length * sqrt(2) / (sdf_trunc / 2) steps at most
    if (!(sdf_trunc > 0.0f) || !std::isfinite(sdf_trunc) ||
        !((double)t->v.res * t->v.voxel_length * 1.4142136 / (0.5 * (double)sdf_trunc) <= (double)MI_ICP_TSDF_MAX_MARCH))
        return fail(c, MI_ICP_ERR_INVALID, "%s: sdf_trunc must be positive and at least length * sqrt(2) * 2 / %d", what,
                    MI_ICP_TSDF_MAX_MARCH);
    const int64_t npix = (int64_t)width * height;
    if (npix == 0) return MI_ICP_OK;

    TsdfRaycast a;
    const Mat4 E = load_T(extrinsic);
    // utility::InverseTransform: R^T and -(R^T t), the sums left to right
    for (int r = 0; r < 3; ++r) {
        for (int k = 0; k < 3; ++k) a.R[r][k] = E.data()[r * 4 + k];  // R^T[r][k] = E(k, r)
        const float t0 = E.data()[12], t1 = E.data()[13], t2 = E.data()[14];
        const float p = ((-a.R[r][0]) * t0 + (-a.R[r][1]) * t1) + (-a.R[r][2]) * t2;
        a.t[r] = p - t->v.origin[r];
    }
    a.fx = intrinsic4[0];
    a.fy = intrinsic4[1];
    a.cx = intrinsic4[2];
    a.cy = intrinsic4[3];
    a.sdf_trunc = sdf_trunc;
    a.width = width;
    a.height = height;
    const dim3 grid((unsigned)((width + 15) / 16), (unsigned)((height + 15) / 16));
    float* const out[3] = {out_xyz, out_normals, out_colors};

    if (!valid_only) {  // every pixel stays, an invalid one as NaN
        *m = npix;
        if (capacity < npix) return MI_ICP_OK;
        if (!out_xyz || !out_normals || !out_colors) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
        float* dst[3];
        TRY(cloud_out(c, out, out, npix, mem_kind, c->vpay, dst));
        tsdf_raycast<<<grid, 256, 0, c->stream>>>(t->v, a, dst[0], dst[1], dst[2]);
        KCHK(c);
        TRY(cloud_out_back(c, dst, out, npix, mem_kind));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        return MI_ICP_OK;
    }
    float* raw[3];
    for (int k = 0; k < 3; ++k) TRY(ensure(c, c->stage[3 + k], (size_t)npix * 3, &raw[k]));
    uint32_t *flags, *pos, *tmp;
    TRY(ensure(c, c->flags, (size_t)npix, &flags));
    TRY(ensure(c, c->dense_idx, (size_t)npix, &pos));
    TRY(ensure(c, c->scan_tmp, (size_t)scan_num_tiles(npix) + 2, &tmp));
    tsdf_raycast<<<grid, 256, 0, c->stream>>>(t->v, a, raw[0], raw[1], raw[2]);
    KCHK(c);
    finite_flags<<<blocks_for(npix), 256, 0, c->stream>>>(raw[0], npix, 1, 1, flags);  // RemoveNoneFinitePoints(true, true)
    KCHK(c);
    exclusive_scan_u32(c->stream, flags, pos, npix, tmp);
    KCHK(c);
    int64_t cnt;
    TRY(tsdf_scan_total(c, tmp, npix, &cnt));
    *m = cnt;
    if (cnt == 0 || capacity < cnt) return MI_ICP_OK;
    if (!out_xyz || !out_normals || !out_colors) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    float* dst[3];
    TRY(cloud_out(c, out, out, cnt, mem_kind, c->vpay, dst));
    select_gather<<<blocks_for(npix), 256, 0, c->stream>>>(flags, pos, npix, raw[0], raw[1], raw[2], dst[0], dst[1], dst[2],
                                                          (int64_t*)nullptr);
    KCHK(c);
    TRY(cloud_out_back(c, dst, out, cnt, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

int mi_icp_tsdf_get_voxels(mi_icp_ctx* c, mi_icp_tsdf* t, float* tsdf_out, float* weight_out, float* color_out, int mem_kind) {
    const char* what = "tsdf_get_voxels";
    TRY(check_ctx(c, mem_kind, what));
    TRY(tsdf_check(c, t, what));
    if (color_out && !t->v.color) return fail(c, MI_ICP_ERR_INVALID, "%s: the volume has no colour planes", what);
    TRY(from_device(c, (const float*)t->v.tsdf, tsdf_out, (size_t)t->v.n, mem_kind));
    TRY(from_device(c, (const float*)t->v.weight, weight_out, (size_t)t->v.n, mem_kind));
    TRY(from_device(c, (const float*)t->v.color, color_out, (size_t)t->v.n * 3, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

}  // extern "C"
