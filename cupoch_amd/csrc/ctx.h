// ctx.h -- what the translation units of libmi_icp.so share: the context (mi_icp_ctx), its buffers, the error /
// allocation / staging helpers, and the declarations of the host-side functions one unit offers the others.
//   mi_icp.hip       context life cycle, the correspondence search, the reduction, the device-resident loop
//   mi_build.hip     target tree (kd cells, groups, levels, halos), source staging, the match-order re-sort
//   mi_geometry.hip  Transform / bounds / affine / covariances / SelectByIndex / SelectByMask / UniformDownSample /
//                    FarthestPointDownSample / the predicate filters / compact_by_flags / SegmentPlane / colours
//   mi_voxel.hip     VoxelDownSample (the dense-grid path and the general one)
//   mi_rgbd.hip      depth / RGB-D frame -> cloud, RGB-D odometry
//   mi_tsdf.hip      UniformTSDFVolume
//   mi_stsdf.hip     ScalableTSDFVolume (tsdf_host.h: the host side the two volumes' units share)
//   mi_occgrid.hip   OccupancyGrid
//   mi_edt.hip       DistanceTransform
//   mi_voxelgrid.hip VoxelGrid (from points, dense, merge, carve, query, bounds, selections, paint)
//   mi_collision.hip collision::ComputeIntersection (grids against grids, line sets, primitives), CreateVoxelGrid
//   mi_graph.hip     geometry::Graph<3> (construct, lattice, edge weights and removal) and its shortest-path search
//   mi_laserscan.hip geometry::LaserScanBuffer (scans to points, points / depth frames to scans, the two filters)
//   mi_image.hip     geometry::Image / RGBDImage processing (filters, the pyramid level, bilateral, conversions, moves)
//   mi_sgm.hip       imageproc::SemiGlobalMatching, PointCloud::CreateFromDisparity
//   mi_feature.hip   registration::Feature matching, CorrespondencesFromFeatures, FastGlobalRegistration
//   mi_knn.hip       EstimateNormals, KDTreeFlann::SearchKNN / SearchRadius, colour gradients, Colored ICP's entry,
//                    RemoveStatisticalOutliers / RemoveRadiusOutliers, ClusterDBSCAN, ComputeISSKeypoints
//   mi_comm.hip      the ranks' exchange: mailbox, device inboxes, in-library RCCL, self-test and choice
//   mi_debug.hip     include/mi_icp_debug.h (test-only entry points)
// Kernels without template parameters are `static` in their headers, so a header may be included by several units.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mi_icp.h"
#include "../../include/mi_icp_debug.h"
#include "device_utils.h"
#include "grid_rules.h"
#include "host_solver.h"
#include "loop.h"
#include "loop_policy.h"
#include "mailbox.h"
#include "primitives.h"

namespace mi {
namespace eng {

using host::Mat4;

struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
};

}  // namespace eng
}  // namespace mi

struct mi_icp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;

    // ---- target (Morton order) ----
    int64_t nt = 0;
    int nleaf = 0;
    int64_t nts = 0;  // sorted positions of the target incl. padding slots (kd_cells.h)
    uint32_t leaf_first = 1, nrecords = 0;  // 8-ary tree: first last-level node id, record count
    bool t_has_nrm = false, t_has_cov = false, t_has_int = false, t_has_grad = false, t_has_rec = false;
    mi::eng::DevBuf tblk, tnrm, trec, tcov, tgrad, nodes, inv_t, tidx, thalo, tlinks_tmp;  // (leaf regions: the leaf lines' fourth rows, lreg_of)
    mi::eng::DevBuf cell_planes, cell_samples, cell_cstart, cell_gstart, cell_boxes, cell_hist;  // (kd_planes.h: the sample's boxes and histograms)
    mi::eng::DevBuf gplanes;   // every group's own 511 split planes (kd_build.h): with cell_planes / cell_gstart the binary descent of locate_by_planes
    int cell_levels = -1;      // levels of cell planes of the present target; < 0: no target built yet
    uint32_t* cell_total_host = nullptr;  // pinned
    bool inv_t_valid = false;
    bool links_ready = false, links_allowed = false;  // leaf_halo.h
    // the halos are built on a private stream (start_links_async)
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_links = nullptr;
    bool links_inflight = false;
    int last_search_kind = -1;  // mi_icp_debug.h
    int last_voxel_path = -1;   // mi_icp_debug.h
    int32_t last_voxel_plan[8] = {-1, 0, 0, 0, 0, 0, 0, 0};  // mi_icp_debug_last_voxel_plan ([0] is filled from last_voxel_path)
    mi::eng::HaloPolicy halo;    // when they are built (loop_policy.h)
    bool halo_use = false;       // the loop's launches take the halos (looked up once per chunk: an event query costs microseconds)
    mi::eng::DevBuf halo_want;            // the counter (nn_search.h kWantSlots words, summed by the host)

    // ---- source (Morton order) ----
    int64_t ns = 0, ns_global = 0;
    bool s_has_nrm = false, s_has_cov = false, s_has_int = false;
    float lambda_geometric = 0.968f;  // colored ICP (colored_icp.cu:47-51)
    mi::eng::DevBuf sx, sy, sz, sperm, snrm, scov, sint, nn_idx, nn_d2, inv_s;
    mi::eng::DevBuf alt[9];  // second set of the source arrays (match-order re-sort ping-pong)
    bool inv_s_valid = false;
    bool nn_valid = false;  // nn_idx holds a search result (usable as seed / correspondences)
    // THE SEARCH SKIP (nn_search.h): one limit on the loop's odometer per packet of 64 source points, left by the loop's
    // seeded searches.  Whatever rewrites nn_idx, re-forms the packets or starts another odometer calls drop_expiry.
    mi::eng::DevBuf expiry;
    bool expiry_live = false;  // the array may hold limits (else: NaN -- all ones -- or -inf throughout: no odometer reading is below either)
    float skip_r2 = NAN;       // the squared radius those limits were measured against; NaN: none on record
    // THE PAIR STREAM (reduce.h PairArgs): per packet a state byte and a mask of matched lanes, per staged source point the
    // 24-byte record of its match, kept once the packet's matches have stood still through a whole search.  State and mask are
    // sized with expiry; tpair only by a loop whose iterations take reduce_pt2pl_kernel (loop_begin), else -- or when that
    // allocation failed -- pairs_on is false and the loop gathers as ever.  drop_expiry voids the states as well.
    mi::eng::DevBuf pair_state, pair_mask, tpair;
    bool pairs_on = false;    // this loop's reductions keep and read pair records
    bool pairs_live = false;  // a state may be non-zero
    mi::eng::DevBuf src_bounds;    // min[3], max[3] of the staged source (the loop's step sizes the displacement of its corners: loop.h)
    mi::eng::Relocation relocate;  // whether the loop's chunks carry the gated re-location launches (loop_policy.h)

    // ---- explicit correspondence set ----
    mi::eng::DevBuf user_pairs;
    int64_t n_user_pairs = -1;  // < 0: use the nearest-neighbour result

    // ---- scratch ----
    mi::eng::DevBuf keys0, keys1, vals0, vals1, hist, scan_tmp, bounds_part, bounds;
    mi::eng::DevBuf partial, sys_dev, dense_idx, flags, pairs_out, seg_start;
    mi::eng::DevBuf stage[6];
    mi::eng::DevBuf tscale;   // scratch of kd_build.h tree_scale
    mi::eng::DevBuf knn_idx, knn_flags;  // the k-NN lists' index rows, [XCD][row][slot][lane], and the rows' claim flags (knn_normals.h KnnSlab)
    mi::eng::DevBuf dbs[4];   // ClusterDBSCAN (dbscan.h): the rows, the per-point words, the one-way masks, the state
    mi::eng::DevBuf seg[4];   // SegmentPlane (segment_plane.h): the planes, the per-hypothesis words and the state, the tie sums, the refit's sums
    mi::eng::DevBuf fgr[8];   // Feature matching and FastGlobalRegistration (mi_feature.hip says what each holds)
    float vx_refused_voxel = 0.0f;  // the last voxel size / cloud size the dense path's plan turned away (mi_icp_voxel_downsample)
    int64_t vx_refused_n = 0;
    int vx_order = 0;         // LDS adds of one instruction served in lane order (voxel_dense.h)?  0: not checked yet, 1: yes, -1: no
    mi::eng::DevBuf vx_tab;   // VoxelDownSample of a dense grid (voxel_dense.h): the [tile][bucket] table, bucket starts, status and control words
    mi::eng::DevBuf vpay[6];  // VoxelDownSample: two sets of payload arrays (points, normals, colours) the radix passes alternate between
    double* sys_host = nullptr;  // pinned, 32 doubles + spare
    float* f_host = nullptr;     // pinned, 16 floats
    uint32_t* u_host = nullptr;  // pinned, 16 + kWantSlots words ([0]: counts read back by the one-shot entry points, [16..]: the halo_want counter's words)
    void* od_host = nullptr;     // pinned OdState mirror (odometry), allocated on first use
    // the last odometry call's images in stage[4] (mi_icp_debug_odometry_image): levels (0: no call yet), sizes and,
    // per level, source colour / depth, target colour / depth, dx / dy colour, dx / dy depth
    int od_levels = 0, od_lw[MI_ICP_ODOMETRY_MAX_LEVELS] = {}, od_lh[MI_ICP_ODOMETRY_MAX_LEVELS] = {};
    const float* od_img[MI_ICP_ODOMETRY_MAX_LEVELS][8] = {};

    // ---- registration loop (device-resident, loop.h) ----
    mi::eng::DevBuf loop_dev, ticket;
    mi::DevLoop* loop_host = nullptr;  // pinned mirror of the device state
    bool loop_active = false;
    mi_icp_iteration_fn iter_fn = nullptr;  // per-iteration report (mi_icp_set_iteration_callback)
    void* iter_user = nullptr;
    mi::eng::DevBuf loop_hist;
    float* hist_host = nullptr;  // pinned, kLoopHistory * 2 floats
    int iter_reported = 0;       // iterations of this loop the callback has seen
    float loop_r2 = 0.0f;
    int loop_est = 0;

    // ---- multi-GPU ----
    ncclComm_t comm = nullptr;
    int nranks = 1, rank = 0;
    // the node's mailbox (mailbox.h): POSIX shared memory registered with HIP, or null
    mi::MailBox* mail_host = nullptr;
    mi::MailBox* mail_dev = nullptr;
    size_t mail_bytes = 0;
    std::string mail_name;
    bool mail_linked = false;   // the name still exists and is this context's to remove
    // device inboxes (mailbox.h): this rank's, the peers' as opened through HIP IPC, and the device-side table of all
    unsigned long long* inbox = nullptr;
    unsigned long long* inbox_peer[mi::kMailRanks] = {};
    mi::eng::DevBuf inbox_table;
    bool comm_broken = false;   // an exchange has failed: the ranks' counters are apart
    // how the ranks exchange their sums: 0 nothing to exchange, 1 the box's host-memory words, 2 device inboxes,
    // 3 in-library RCCL all-reduce.  Set when the communicator is made, changed by mi_icp_comm_autotune.
    int xchg = 0;
    uint32_t tune_epoch = 0;    // this rank's count of host-side gathers through the box (box_gather)
    mi::eng::DevBuf mail_state;  // [0]: this rank's exchange counter, [1]: error flag of the one-shot exchange

    // ---- private scratch context: PointCloud::EstimateNormals builds its own tree there, so
    // that the target / source / loop state of THIS context survive the call ----
    mi_icp_ctx* aux = nullptr;

    // ---- integration::UniformTSDFVolume: the volumes this context made (mi_tsdf.hip), freed with it ----
    std::vector<mi_icp_tsdf*> tsdf_volumes;
    // ---- integration::ScalableTSDFVolume: likewise (mi_stsdf.hip) ----
    std::vector<mi_icp_stsdf*> stsdf_volumes;
    // ---- geometry::OccupancyGrid: the grids this context made (mi_occgrid.hip), freed with it ----
    std::vector<mi_icp_occgrid*> occ_grids;
    // ---- geometry::DistanceTransform: the transforms this context made (mi_edt.hip), freed with it ----
    std::vector<mi_icp_dt*> dts;
    // ---- imageproc::SemiGlobalMatching: the matchers this context made (mi_sgm.hip), freed with it ----
    std::vector<mi_icp_sgm*> sgm_matchers;

    // ---- instrumentation ----
    mi::eng::DevBuf stamps;    // loop.h "where an iteration's time goes" (mi_icp_debug_set_step_stamps)
    bool stamps_on = false;
    bool profiling = false;
    static constexpr int kEvPairs = 16;   // per kind: one pair per launch of a chunk
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t evp[2][kEvPairs][2] = {};
    int evp_n[2] = {0, 0};
    bool ev_pending_nn = false, ev_pending_red = false;
    double prof[8] = {0, 0, 0, 0, 0, 0, 0, 0};
};

namespace mi {
namespace eng {

// the leaves' region records: the fourth row of every leaf line (device_utils.h: kLeafRegOffset, kLeafRegStride)
inline float* lreg_of(const mi_icp_ctx* c) { return c->tblk.p ? (float*)c->tblk.p + mi::kLeafRegOffset : nullptr; }

inline int fail(mi_icp_ctx* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    return code;
}

#define HIPCHK(c, expr)                                                                       \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return fail((c), MI_ICP_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                  \
                        hipGetErrorString(e_), __FILE__, __LINE__);                           \
    } while (0)

#define KCHK(c) HIPCHK(c, hipGetLastError())

#define TRY(expr)                \
    do {                         \
        int rc_ = (expr);        \
        if (rc_ != MI_ICP_OK) return rc_; \
    } while (0)

template <class T>
int ensure(mi_icp_ctx* c, DevBuf& b, size_t count, T** out) {
    const size_t bytes = std::max<size_t>(count * sizeof(T), 256);
    if (b.bytes < bytes) {
        if (b.p) {
            // buffers may still be in use by enqueued work
            HIPCHK(c, hipStreamSynchronize(c->stream));
            HIPCHK(c, hipFree(b.p));
            b.p = nullptr;
            b.bytes = 0;
        }
        HIPCHK(c, hipMalloc(&b.p, bytes));
        b.bytes = bytes;
    }
    *out = (T*)b.p;
    return MI_ICP_OK;
}

inline void release(DevBuf& b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.bytes = 0;
}

// How an entry point handles a caller's buffer: MI_ICP_HOST stages it through a context-owned DevBuf, MI_ICP_DEVICE
// reads and writes it in place (check_ctx below turns away every other kind).  None of the three helpers waits.
//   to_device   an input: the device view of `src`
//   out_slot    an output: where a kernel writes `count` elements for `dst` (dst itself, or `stage`); nullptr for no dst
//   from_device back to the caller: `count` elements of `dev` into `dst`, unless dst is null or is `dev` itself
template <class T>
int to_device(mi_icp_ctx* c, const T* src, size_t count, int mem_kind, DevBuf& stage,
              const T** out) {
    if (!src || count == 0) {
        *out = nullptr;
        return MI_ICP_OK;
    }
    if (mem_kind == MI_ICP_DEVICE) {
        *out = src;
        return MI_ICP_OK;
    }
    T* d;
    TRY(ensure(c, stage, count, &d));
    HIPCHK(c, hipMemcpyAsync(d, src, count * sizeof(T), hipMemcpyHostToDevice, c->stream));
    *out = d;
    return MI_ICP_OK;
}

template <class T>
int out_slot(mi_icp_ctx* c, T* dst, size_t count, int mem_kind, DevBuf& stage, T** out) {
    if (!dst || mem_kind == MI_ICP_DEVICE) {
        *out = dst;
        return MI_ICP_OK;
    }
    return ensure(c, stage, count, out);
}

template <class T>
int from_device(mi_icp_ctx* c, const T* dev, T* dst, size_t count, int mem_kind) {
    if (!dst || dst == dev || count == 0) return MI_ICP_OK;
    HIPCHK(c, hipMemcpyAsync(dst, dev, count * sizeof(T),
                             mem_kind == MI_ICP_DEVICE ? hipMemcpyDeviceToDevice
                                                       : hipMemcpyDeviceToHost,
                             c->stream));
    return MI_ICP_OK;
}

// Every packet's pair state back to 0: no record is read until the reduction has seen the packet twice more.
inline int drop_pairs(mi_icp_ctx* c) {
    if (c->pairs_live && c->pair_state.p) HIPCHK(c, hipMemsetAsync(c->pair_state.p, 0, c->pair_state.bytes, c->stream));
    c->pairs_live = false;
    return MI_ICP_OK;
}

// The per-packet limits of the search skip are void from here on: nothing is skipped until a seeded search of a loop
// has left new ones.  So are the pair records (above), unless the caller is a seeded search of the loop, which lowers
// the state of every packet it changes itself (keep_pairs).
inline int drop_expiry(mi_icp_ctx* c, bool keep_pairs = false) {
    c->skip_r2 = NAN;
    if (c->expiry_live && c->expiry.p) HIPCHK(c, hipMemsetAsync(c->expiry.p, 0xff, c->expiry.bytes, c->stream));
    c->expiry_live = false;
    return keep_pairs ? MI_ICP_OK : drop_pairs(c);
}

static_assert(sizeof(DevLoop::live) == kSkipSamples, "loop_policy.h skip_pays reads DevLoop::live[]");

inline int blocks_for(int64_t n, int per = 256) { return (int)std::max<int64_t>(1, (n + per - 1) / per); }

inline Xform make_xform(const Mat4& T) { return xform_from(T); }

inline Mat4 load_T(const float* T) {
    if (!T) return host::identity4();
    Mat4 m;
    std::memcpy(m.data(), T, sizeof(float) * 16);
    return m;
}

struct EvTimer {
    mi_icp_ctx* c;
    int slot;  // 0: nn, 1: reduce
    hipEvent_t stop = nullptr;
    bool pooled;
    EvTimer(mi_icp_ctx* ctx, int s, bool in_loop) : c(ctx), slot(s), pooled(in_loop) {
        if (!c->profiling) return;
        if (pooled) {
            if (c->evp_n[slot] >= mi_icp_ctx::kEvPairs) return;
            const int i = c->evp_n[slot]++;
            (void)hipEventRecord(c->evp[slot][i][0], c->stream);
            stop = c->evp[slot][i][1];
        } else {
            (void)hipEventRecord(c->ev[slot * 2], c->stream);
            stop = c->ev[slot * 2 + 1];
        }
    }
    ~EvTimer() {
        if (!stop) return;
        (void)hipEventRecord(stop, c->stream);
        if (!pooled) (slot == 0 ? c->ev_pending_nn : c->ev_pending_red) = true;
    }
};

inline void collect_events(mi_icp_ctx* c) {  // call after the stream has been synchronised
    float ms = 0.0f;
    if (c->ev_pending_nn && hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) {
        c->prof[0] += ms;
        c->prof[1] += 1;
    }
    if (c->ev_pending_red && hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) {
        c->prof[2] += ms;
        c->prof[3] += 1;
    }
    c->ev_pending_nn = c->ev_pending_red = false;
}

// pooled events of a loop chunk: only the first `executed` launches did real work
inline void collect_pooled(mi_icp_ctx* c, int executed) {
    for (int slot = 0; slot < 2; ++slot) {
        for (int i = 0; i < c->evp_n[slot] && i < executed; ++i) {
            float ms = 0.0f;
            if (hipEventElapsedTime(&ms, c->evp[slot][i][0], c->evp[slot][i][1]) == hipSuccess) {
                c->prof[slot * 2] += ms;
                c->prof[slot * 2 + 1] += 1;
            }
        }
        c->evp_n[slot] = 0;
    }
}

// the ranks exchange through the mailbox (host-memory words or device inboxes), not through RCCL
inline bool mail_on(const mi_icp_ctx* c) { return c->mail_dev != nullptr && (c->xchg == 1 || c->xchg == 2); }

inline int check_ctx(mi_icp_ctx* c) {
    if (!c) return MI_ICP_ERR_INVALID;
    hipError_t e = hipSetDevice(c->device);
    if (e != hipSuccess) return fail(c, MI_ICP_ERR_HIP, "hipSetDevice(%d): %s", c->device, hipGetErrorString(e));
    return MI_ICP_OK;
}

// ... and of an entry point that takes a mem_kind, before any buffer is touched
inline int check_ctx(mi_icp_ctx* c, int mem_kind, const char* what) {
    TRY(check_ctx(c));
    if (mem_kind != MI_ICP_HOST && mem_kind != MI_ICP_DEVICE) return fail(c, MI_ICP_ERR_INVALID, "%s: bad mem_kind", what);
    return MI_ICP_OK;
}

// ---- The life of a handle (a volume, a grid, a distance transform, a matcher): a struct with an `owner` and a member
// ---- free_buffers(), kept in the list of the context that made it and freed with that context at the latest.
// Is `h` one that context c made and still holds in `list`?  `noun` names the kind in the message.  (The list is looked
// at first: a handle that is not in it may have been destroyed, and is not read.)
template <class T>
int handle_check(mi_icp_ctx* c, const T* h, const std::vector<T*>& list, const char* what, const char* noun) {
    if (!h || std::find(list.begin(), list.end(), h) == list.end() || h->owner != c)
        return fail(c, MI_ICP_ERR_INVALID, "%s: not a %s of this context", what, noun);
    return MI_ICP_OK;
}

// out of the list and deleted; its buffers are the caller's business
template <class T>
void handle_drop(T* h, std::vector<T*>& list) {
    list.erase(std::find(list.begin(), list.end(), h));
    delete h;
}

// the destroy entry point: a null handle is fine; work in flight may still use the buffers, so the stream is waited for
template <class T>
int handle_destroy(mi_icp_ctx* c, T* h, std::vector<T*>& list, const char* what, const char* noun) {
    TRY(check_ctx(c));
    if (!h) return MI_ICP_OK;
    TRY(handle_check(c, h, list, what, noun));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    h->free_buffers();
    handle_drop(h, list);
    return MI_ICP_OK;
}

template <class T>
void handle_release_all(std::vector<T*>& list) {
    for (T* h : list) {
        h->free_buffers();
        delete h;
    }
    list.clear();
}

// ---- The argument checks the entry points share.  An entry point makes each check where its contract places it: the
// ---- order is part of the interface.
constexpr int64_t kMaxCount = 0x7fffff00ll;  // positions and counts are 32-bit

inline int count_ok(mi_icp_ctx* c, const char* what, int64_t n) {
    if (n < 0 || n > kMaxCount) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    return MI_ICP_OK;
}

inline bool finite3(const float* v) { return v && mi::finite3(v[0], v[1], v[2]); }

// a grid's frame at the time of a call -> *f
inline int frame_check(mi_icp_ctx* c, const char* what, float voxel_size, const float* origin3, GridFrame* f) {
    if (!(voxel_size > 0.0f) || !std::isfinite(voxel_size) || !finite3(origin3))
        return fail(c, MI_ICP_ERR_INVALID, "%s: voxel_size must be positive and finite, the origin finite", what);
    f->vs = voxel_size;
    for (int k = 0; k < 3; ++k) f->origin[k] = origin3[k];
    return MI_ICP_OK;
}

inline int resolution_ok(mi_icp_ctx* c, const char* what, int resolution, int max) {
    if (resolution < 2 || resolution > max) return fail(c, MI_ICP_ERR_INVALID, "%s: the resolution must be in [2, %d]", what, max);
    return MI_ICP_OK;
}

// ---- What the cloud-in, cloud-out entry points share.  A cloud is three arrays: points, normals, colours (the last two
// ---- optional).
// Sizes: the context and the memory kind, m (zeroed from here on), 0 <= n <= kMaxCount.
inline int check_sizes(mi_icp_ctx* c, const char* what, int64_t n, int64_t* m, int mem_kind) {
    TRY(check_ctx(c, mem_kind, what));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    return count_ok(c, what, n);
}

struct Cloud {
    const float* in[3];  // the caller's arrays; after cloud_in / cloud_upload their device view
    float* out[3];       // the caller's outputs
};

// the null-buffer rule: points in and out, and an output for every attribute that comes in
inline int cloud_check(mi_icp_ctx* c, const char* what, const Cloud& a) {
    if (!a.in[0] || !a.out[0] || (a.in[1] && !a.out[1]) || (a.in[2] && !a.out[2]))
        return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    return MI_ICP_OK;
}

inline int cloud_upload(mi_icp_ctx* c, Cloud* a, int64_t n, int mem_kind, DevBuf* stage) {
    for (int k = 0; k < 3; ++k) TRY(to_device(c, a->in[k], (size_t)n * 3, mem_kind, stage[k], &a->in[k]));
    return MI_ICP_OK;
}

inline int cloud_in(mi_icp_ctx* c, const char* what, Cloud* a, int64_t n, int mem_kind, DevBuf* stage) {
    TRY(cloud_check(c, what, *a));
    return cloud_upload(c, a, n, mem_kind, stage);
}

// Where up to `count` points of an output cloud go: the caller's arrays out[], or (MI_ICP_HOST) stage[0..2]; nullptr for
// an attribute that in[] does not have.  cloud_out_back copies `m` of them to the caller.
inline int cloud_out(mi_icp_ctx* c, const float* const in[3], float* const out[3], int64_t count, int mem_kind,
                     DevBuf* stage, float* dst[3]) {
    for (int k = 0; k < 3; ++k) TRY(out_slot(c, in[k] ? out[k] : nullptr, (size_t)count * 3, mem_kind, stage[k], &dst[k]));
    return MI_ICP_OK;
}

inline int cloud_out_back(mi_icp_ctx* c, float* const dst[3], float* const out[3], int64_t m, int mem_kind) {
    for (int k = 0; k < 3; ++k)
        if (dst[k]) TRY(from_device(c, (const float*)dst[k], out[k], (size_t)m * 3, mem_kind));
    return MI_ICP_OK;
}

// Emit: room for `count` points, launch(dst) writes them, `m` of them go back to the caller, one wait.
template <class Launch>
int cloud_emit(mi_icp_ctx* c, const float* const in[3], float* const out[3], int64_t count, int64_t m, int mem_kind,
               DevBuf* stage, Launch launch) {
    float* dst[3];
    TRY(cloud_out(c, in, out, count, mem_kind, stage, dst));
    launch(dst);
    KCHK(c);
    TRY(cloud_out_back(c, dst, out, m, mem_kind));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return MI_ICP_OK;
}

// Scan: pos[i] = flags[0] + ... + flags[i - 1] (pos may be flags itself); *total is the device word that holds the sum
// of all n.  The one place that knows where exclusive_scan_u32 leaves it.
inline int scan_into(mi_icp_ctx* c, const uint32_t* flags, uint32_t* pos, int64_t n, const uint32_t** total) {
    uint32_t* tmp;
    TRY(ensure(c, c->scan_tmp, (size_t)scan_num_tiles(n) + 2, &tmp));
    exclusive_scan_u32(c->stream, flags, pos, n, tmp);
    KCHK(c);
    *total = tmp + scan_num_tiles(n);
    return MI_ICP_OK;
}

// ... with the positions in c->dense_idx
inline int scan_flags(mi_icp_ctx* c, const uint32_t* flags, int64_t n, uint32_t** pos, const uint32_t** total) {
    TRY(ensure(c, c->dense_idx, (size_t)n, pos));
    return scan_into(c, flags, *pos, n, total);
}

// the total on its way to c->u_host[slot]: there after the next wait
inline int read_total(mi_icp_ctx* c, const uint32_t* total, int slot = 0) {
    HIPCHK(c, hipMemcpyAsync(c->u_host + slot, total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    return MI_ICP_OK;
}

// Counted compaction, for a caller that gives a capacity: scan, wait for the count, *m = it; nothing is written when it
// is zero or above `capacity` (the caller learns the room to make).  Else out[k] must be there wherever want[k], and
// launch(pos, dst) writes the cloud.
template <class Launch>
int cloud_emit_counted(mi_icp_ctx* c, const char* what, const uint32_t* flags, int64_t n, float* const out_all[3],
                       const bool (&want)[3], int64_t capacity, int64_t* m, int mem_kind, Launch launch) {
    uint32_t* pos;
    const uint32_t* total;
    TRY(scan_flags(c, flags, n, &pos, &total));
    TRY(read_total(c, total));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int64_t cnt = (int64_t)c->u_host[0];
    *m = cnt;
    if (cnt == 0 || capacity < cnt) return MI_ICP_OK;
    float* out[3];
    for (int k = 0; k < 3; ++k) {
        if (want[k] && !out_all[k]) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
        out[k] = want[k] ? out_all[k] : nullptr;
    }
    return cloud_emit(c, out, out, cnt, cnt, mem_kind, c->vpay, [&](float* const dst[3]) { launch(pos, dst); });
}

// Runs body(a) in the private scratch context a = c->aux (made on first use, on c's stream): a registration in flight
// on c (user estimators may call EstimateNormals between iterations) keeps its target, source, correspondences and
// loop state.  A failure is reported on c as "what: <a's error>".
template <class Body>
int in_scratch(mi_icp_ctx* c, const char* what, Body body) {
    if (!c->aux) {
        const int rc = mi_icp_create(c->device, &c->aux);
        if (rc != MI_ICP_OK) return fail(c, rc, "%s: cannot create the scratch context", what);
    }
    mi_icp_ctx* a = c->aux;
    a->stream = c->stream;
    const int rc = body(a);
    if (rc != MI_ICP_OK) return fail(c, rc, "%s: %s", what, a->err.c_str());
    return MI_ICP_OK;
}

// ---- mi_build.hip
int compute_bounds(mi_icp_ctx* c, const float* pts, int64_t n, float** bounds_out);  // min[3], max[3], extent into c->bounds
int sort_buffers(mi_icp_ctx* c, int64_t n, SortBuffers* sb);
int morton_order(mi_icp_ctx* c, const float* pts, int64_t n, const uint32_t** order, const float* grid_bounds = nullptr,
                 int grid_bits = 0, float** own_bounds = nullptr);
int ensure_links(mi_icp_ctx* c);          // the halos complete before the next kernel on the context's stream
int start_links_async(mi_icp_ctx* c);     // ... started on the private stream
bool halo_poll(mi_icp_ctx* c);            // are they there?  never waits
int drain_links(mi_icp_ctx* c);
void release_links_scratch(mi_icp_ctx* c);
int resort_source_by_match(mi_icp_ctx* c);
int occupancy_build(int which);           // mi_icp_debug_occupancy: the kernels each unit owns
// ---- mi_icp.hip
int launch_nn(mi_icp_ctx* c, const Mat4& T, float r2, bool seed, unsigned long long* stats = nullptr,
              const DevLoop* loop = nullptr);
int occupancy_loop(int which);
bool planes_available(const mi_icp_ctx* c);
int launch_locate_by_planes(mi_icp_ctx* c, const Xform& X, const DevLoop* loop, int gated);
// ---- mi_voxel.hip
int occupancy_geometry(int which);
// ---- mi_rgbd.hip
bool invert4(const float* M, float* out);  // column-major 4x4 inverse (false: singular); the pose of CreateFromDepthImage
// ---- mi_tsdf.hip
void tsdf_release_all(mi_icp_ctx* c);     // mi_icp_destroy: the volumes of mi_icp_tsdf_create
// ---- mi_stsdf.hip
void stsdf_release_all(mi_icp_ctx* c);    // mi_icp_destroy: the volumes of mi_icp_stsdf_create
// ---- mi_occgrid.hip
void occgrid_release_all(mi_icp_ctx* c);  // mi_icp_destroy: the grids of mi_icp_occgrid_create
// a grid's log-odds plane, resolution and inclusive bounds (min[3], max[3]) for a reader on the device
int occgrid_view(mi_icp_ctx* c, const mi_icp_occgrid* o, const char* what, const float** prob, int* resolution, int* bounds6);
// The listing of a grid's voxels, ascending linear index.  occgrid_select: those of the bounds box that `which`
// (MI_ICP_OCCGRID_*) selects at threshold `thres`; their flags and positions stay in c->flags and c->dense_idx, *count is
// their number (one wait).  occgrid_gather, while those stand: their indices and, where asked for, log-odds and points.
int occgrid_select(mi_icp_ctx* c, const mi_icp_occgrid* o, int which, float thres, int64_t* count);
int occgrid_gather(mi_icp_ctx* c, const mi_icp_occgrid* o, const GridFrame& f, int32_t* out_index, float* out_prob_log, float* out_xyz);
// ---- mi_voxelgrid.hip
struct VgRuns {
    const uint32_t* order = nullptr;      // sorted position -> entry of keys3
    const uint32_t* run_start = nullptr;  // [nvox + 1]
    int64_t nvox = 0;
};
// the stable order of keys3[n][3] and its runs of equal keys (in the context's sort and scan buffers); waits twice
int vg_sort_runs(mi_icp_ctx* c, const int32_t* keys3, int64_t n, VgRuns* r);
// ---- mi_edt.hip
void dt_release_all(mi_icp_ctx* c);       // mi_icp_destroy: the transforms of mi_icp_dt_create
// ---- mi_sgm.hip
void sgm_release_all(mi_icp_ctx* c);      // mi_icp_destroy: the matchers of mi_icp_sgm_create
// ---- mi_geometry.hip
// The points whose flags[0..n) are set, ascending (select.h: exclusive_scan_u32 + select_gather), into out[] (the
// caller's, staged when mem_kind is MI_ICP_HOST) and their original indices into out_idx (may be null); *m = their
// count.  One wait on the stream, which also brings back the device word *status (may be null) into *status_out.
int compact_by_flags(mi_icp_ctx* c, const uint32_t* flags, int64_t n, const float* const in[3], float* const out[3],
                     int64_t* out_idx, int mem_kind, const uint32_t* status, int64_t* m, uint32_t* status_out);
// ---- mi_comm.hip
MailArgs mail_args(const mi_icp_ctx* c);
void mailbox_close(mi_icp_ctx* c);
int comm_failed(mi_icp_ctx* c, const char* what);
int comm_usable(mi_icp_ctx* c);
int allreduce_system(mi_icp_ctx* c);
void comm_release(mi_icp_ctx* c);         // mi_icp_destroy: the mailbox and the communicator

}  // namespace eng
}  // namespace mi
