// mi_knn.hip -- k-nearest-neighbour work on the target tree: PointCloud::EstimateNormals, KDTreeFlann::SearchKNN /
// SearchRadius, Colored ICP's colour gradients and its registration entry, RemoveStatisticalOutliers /
// RemoveRadiusOutliers, ClusterDBSCAN, ComputeISSKeypoints, GaussianFilter (knn_normals.h, select.h, dbscan.h, iss.h,
// gaussian_filter.h)
// (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include <cstring>

#include "ctx.h"
#include "dbscan.h"
#include "gaussian_filter.h"
#include "iss.h"
#include "knn_normals.h"
#include "select.h"

using namespace mi;
using namespace mi::eng;
using host::Mat4;

namespace {

// The index rows of one k-NN launch (knn_normals.h KnnSlab): a quarter more rows per XCD than the XCD can hold waves of
// this kernel, flags cleared on the stream ahead of the launch.  `kernel`: the instantiation about to be launched.
template <class K>
int knn_slab(mi_icp_ctx* c, K kernel, int cap, KnnSlab* out) {
    static const int ncu = [] { hipDeviceProp_t p; int dev = 0; (void)hipGetDevice(&dev); return (hipGetDeviceProperties(&p, dev) == hipSuccess && p.multiProcessorCount > 0) ? p.multiProcessorCount : 256; }();
    int occ = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, 64, 0) != hipSuccess || occ <= 0) {
        (void)hipGetLastError();
        occ = std::min(32, (160 * 1024) / (cap * 64 * 4));  // one wave per workgroup; the lists' distances fill the LDS
    }
    const uint32_t per_xcc = (uint32_t)(((int64_t)occ * ((ncu + 7) / 8) * 5 + 3) / 4 + 8);
    TRY(ensure(c, c->knn_idx, (size_t)8 * per_xcc * cap * 64, &out->rows));
    TRY(ensure(c, c->knn_flags, (size_t)8 * per_xcc, &out->flags));
    HIPCHK(c, hipMemsetAsync(out->flags, 0, (size_t)8 * per_xcc * sizeof(uint32_t), c->stream));
    out->per_xcc = per_xcc;
    return MI_ICP_OK;
}

template <int KCAP>
using Cap = std::integral_constant<int, KCAP>;

// Launches one k-NN kernel over `nblocks` packets (one 64-lane workgroup each, the grid rounded up to whole rounds of
// the 8 XCDs for xcd_remap) in the instantiation for k's capacity, `pick(Cap<KCAP>())`, with a slab sized for that
// same instantiation; args...: the kernel's arguments ahead of nblocks and the slab.
template <class Pick, class... Args>
int knn_launch(mi_icp_ctx* c, int k, uint32_t nblocks, Pick pick, Args... args) {
    const int cap = knn_capacity(k);
    auto go = [&](auto kernel) -> int {
        KnnSlab slab;
        TRY(knn_slab(c, kernel, cap, &slab));
        kernel<<<((nblocks + 7u) / 8u) * 8u, 64, 0, c->stream>>>(args..., nblocks, slab);
        KCHK(c);
        return MI_ICP_OK;
    };
    if (cap == kMaxKnn) return go(pick(Cap<kMaxKnn>()));
    if (cap == kMaxKnnMid) return go(pick(Cap<kMaxKnnMid>()));
    return go(pick(Cap<kMaxKnnBig>()));
}

// knn_normals_kernel<OUT> over the target's leaves: EstimateNormals (OUT = 0), the colour gradients (OUT = 1), the
// outlier filters' mean squared distance (OUT = 2) or neighbour count (OUT = 3)
template <int OUT>
int launch_knn_normals(mi_icp_ctx* c, int k, float r2, float* out, const float4* tnrm, float4* tgrad) {
    return knn_launch(c, k, (uint32_t)((c->nleaf + 7) / 8), [](auto kc) { return knn_normals_kernel<OUT, decltype(kc)::value>; },
                      (const float*)c->nodes.p, (const float*)c->tblk.p, (const int32_t*)c->tidx.p, c->leaf_first, c->nts,
                      c->nleaf, k, r2, out, tnrm, tgrad);
}

}  // namespace

extern "C" {

static int estimate_normals_impl(mi_icp_ctx* c, const float* xyz, int64_t n, int knn, float r2,
                                 float* normals, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "estimate_normals"));
    if (n < 0 || (n > 0 && (!xyz || !normals))) return fail(c, MI_ICP_ERR_INVALID, "estimate_normals: bad arguments");
    if (knn > kKnnLimit) return fail(c, MI_ICP_ERR_INVALID, "estimate_normals: more than %d neighbours (knn::NUM_MAX_NN) are not supported", kKnnLimit);
    if (n == 0) return MI_ICP_OK;
    // the cloud gets a tree of its own in the private scratch context
    return in_scratch(c, "estimate_normals", [&](mi_icp_ctx* a) -> int {
        TRY(mi_icp_set_target(a, xyz, nullptr, nullptr, n, mem_kind));
        float* dn;
        TRY(out_slot(a, normals, (size_t)n * 3, mem_kind, a->stage[1], &dn));
        TRY(launch_knn_normals<0>(a, knn, r2, dn, nullptr, nullptr));
        TRY(from_device(a, (const float*)dn, normals, (size_t)n * 3, mem_kind));
        HIPCHK(a, hipStreamSynchronize(a->stream));
        return MI_ICP_OK;
    });
}

int mi_icp_estimate_normals_knn(mi_icp_ctx* c, const float* xyz, int64_t n, int knn, float* normals,
                                int mem_kind) {
    return estimate_normals_impl(c, xyz, n, knn, INFINITY, normals, mem_kind);
}

int mi_icp_estimate_normals_radius(mi_icp_ctx* c, const float* xyz, int64_t n, float radius, int max_nn,
                                   float* normals, int mem_kind) {
    return estimate_normals_impl(c, xyz, n, max_nn, radius * radius, normals, mem_kind);
}

// ---------------------------------------------------------------------------
// PointCloud::RemoveStatisticalOutliers / RemoveRadiusOutliers (geometry/down_sample.cu:317-438).  The cloud gets a tree
// in the private scratch context, as in EstimateNormals (the caller's target, source, correspondences and loop state
// survive); knn_normals_kernel<2 | 3> leaves one number per point, and the tail (select.h) keeps, compacts and gathers
// on the stream -- the count comes back with the one wait at the end.
//   radius = false: k = nb_neighbors nearest (r2 = +inf), kept iff 0 < avg < mean + std_ratio * std
//   radius = true:  k = nb_points + 1 nearest with d2 < r2, kept iff all k were found
static int outlier_impl(mi_icp_ctx* c, const char* what, bool radius, const float* xyz, const float* normals,
                        const float* colors, int64_t n, int k, float r2, double std_ratio, float* out_xyz,
                        float* out_normals, float* out_colors, int64_t* out_indices, void* stat_out, int64_t* m,
                        int mem_kind) {
    if (n == 0) return MI_ICP_OK;
    return in_scratch(c, what, [&](mi_icp_ctx* a) -> int {
        Cloud cl{{xyz, normals, colors}, {out_xyz, out_normals, out_colors}};
        TRY(cloud_upload(a, &cl, n, mem_kind, a->stage));
        TRY(mi_icp_set_target(a, cl.in[0], nullptr, nullptr, n, MI_ICP_DEVICE));
        float* stat;  // float avg or int32 count, [n] in the cloud's order
        TRY(out_slot(a, (float*)stat_out, (size_t)n, mem_kind, a->stage[3], &stat));
        if (!stat) TRY(ensure(a, a->stage[3], (size_t)n, &stat));  // (the caller does not want them)
        uint32_t* flags;
        TRY(ensure(a, a->flags, (size_t)n, &flags));
        if (!radius) {
            TRY(launch_knn_normals<2>(a, k, INFINITY, stat, nullptr, nullptr));
            double *part, *thr;
            const int blocks = std::min(kOutlierBlocks, blocks_for(n));
            TRY(ensure(a, a->partial, (size_t)kOutlierBlocks * 4, &part));
            TRY(ensure(a, a->sys_dev, (size_t)kSysSize, &thr));
            outlier_stats_partial<<<blocks, 256, 0, a->stream>>>(stat, n, part);
            outlier_stats_final<<<1, 64, 0, a->stream>>>(part, blocks, n, std_ratio, thr);
            outlier_flags_stat<<<blocks_for(n), 256, 0, a->stream>>>(stat, n, thr, flags);
        } else {
            TRY(launch_knn_normals<3>(a, k, r2, stat, nullptr, nullptr));
            outlier_flags_radius<<<blocks_for(n), 256, 0, a->stream>>>((const int32_t*)stat, n, k, flags);
        }
        KCHK(a);
        TRY(from_device(a, (const float*)stat, (float*)stat_out, (size_t)n, mem_kind));
        return compact_by_flags(a, flags, n, cl.in, cl.out, out_indices, mem_kind, nullptr, m, nullptr);
    });
}

// (the buffers before the filter's own parameters)
static int outlier_args(mi_icp_ctx* c, const char* what, const float* xyz, const float* normals, const float* colors,
                        int64_t n, float* out_xyz, float* out_normals, float* out_colors, int64_t* m, int mem_kind) {
    TRY(check_sizes(c, what, n, m, mem_kind));
    if (n > 0) TRY(cloud_check(c, what, Cloud{{xyz, normals, colors}, {out_xyz, out_normals, out_colors}}));
    return MI_ICP_OK;
}

int mi_icp_remove_statistical_outliers(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors,
                                       int64_t n, int nb_neighbors, float std_ratio, float* out_xyz, float* out_normals,
                                       float* out_colors, int64_t* out_indices, float* avg_d2, int64_t* m, int mem_kind) {
    const char* what = "remove_statistical_outliers";
    TRY(outlier_args(c, what, xyz, normals, colors, n, out_xyz, out_normals, out_colors, m, mem_kind));
    if (nb_neighbors < 1) return fail(c, MI_ICP_ERR_INVALID, "%s: nb_neighbors must be positive", what);
    if (!(std_ratio > 0.0f)) return fail(c, MI_ICP_ERR_INVALID, "%s: std_ratio must be positive", what);
    if (nb_neighbors > kKnnLimit)
        return fail(c, MI_ICP_ERR_INVALID, "%s: more than %d neighbours (knn::NUM_MAX_NN) are not supported", what, kKnnLimit);
    return outlier_impl(c, what, false, xyz, normals, colors, n, nb_neighbors, INFINITY, (double)std_ratio, out_xyz,
                        out_normals, out_colors, out_indices, avg_d2, m, mem_kind);
}

int mi_icp_remove_radius_outliers(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                                  int nb_points, float radius, float* out_xyz, float* out_normals, float* out_colors,
                                  int64_t* out_indices, int32_t* counts, int64_t* m, int mem_kind) {
    const char* what = "remove_radius_outliers";
    TRY(outlier_args(c, what, xyz, normals, colors, n, out_xyz, out_normals, out_colors, m, mem_kind));
    if (nb_points < 1) return fail(c, MI_ICP_ERR_INVALID, "%s: nb_points must be positive", what);
    if (!(radius > 0.0f)) return fail(c, MI_ICP_ERR_INVALID, "%s: search_radius must be positive", what);
    if (nb_points + 1 > kKnnLimit)
        return fail(c, MI_ICP_ERR_INVALID, "%s: nb_points + 1 above %d (knn::NUM_MAX_NN) is not supported", what, kKnnLimit);
    return outlier_impl(c, what, true, xyz, normals, colors, n, nb_points + 1, radius * radius, 0.0, out_xyz, out_normals,
                        out_colors, out_indices, counts, m, mem_kind);
}

// ---------------------------------------------------------------------------
// PointCloud::ClusterDBSCAN (geometry/pointcloud_cluster.cu:109-179).  The cloud gets a tree in the private scratch
// context, as in EstimateNormals; knn_normals_kernel<4> writes every point's row, SearchRadius(eps, max_edges + 1) in
// (d2, index) order without the point itself, and dbscan.h turns the rows into labels.  The rounds over the one-way
// edges run in gated batches (a settled phase returns at once); the state, the cluster count and the labels come back
// with one wait when the first batch settles, as it does whenever no row is truncated.
static int dbscan_impl(mi_icp_ctx* c, const float* xyz, int64_t n, float r2, int min_points, int max_edges,
                       int32_t* labels, int32_t* degrees, int64_t* n_clusters, int mem_kind) {
    const int k = max_edges + 1;
    return in_scratch(c, "cluster_dbscan", [&](mi_icp_ctx* a) -> int {
        TRY(mi_icp_set_target(a, xyz, nullptr, nullptr, n, mem_kind));
        int32_t *rows, *node;
        uint4* mask;
        DbscanState* st;
        const uint32_t* total;
        TRY(ensure(a, a->dbs[0], (size_t)n * k, &rows));
        TRY(ensure(a, a->dbs[1], (size_t)n * 6, &node));
        TRY(ensure(a, a->dbs[2], (size_t)n, &mask));
        TRY(ensure(a, a->dbs[3], (size_t)1, &st));
        int32_t *word = node, *rep = node + n, *m = node + 2 * n, *Mx = node + 3 * n;
        uint32_t* start = (uint32_t*)(node + 4 * n);
        uint32_t* number = (uint32_t*)(node + 5 * n);
        int32_t *dl, *dd;
        TRY(out_slot(a, labels, (size_t)n, mem_kind, a->stage[1], &dl));
        TRY(out_slot(a, degrees, (size_t)n, mem_kind, a->stage[2], &dd));
        TRY(launch_knn_normals<4>(a, k, r2, (float*)rows, nullptr, (float4*)word));
        HIPCHK(a, hipMemsetAsync(st, 0, sizeof(DbscanState), a->stream));
        const int nb = blocks_for(n);
        dbscan_init<<<nb, 256, 0, a->stream>>>(n, rep, m, Mx);
        dbscan_hook<<<nb, 256, 0, a->stream>>>(rows, word, n, k, min_points, rep);
        dbscan_flatten<<<nb, 256, 0, a->stream>>>(n, rep);
        dbscan_classify<<<nb, 256, 0, a->stream>>>(rows, word, rep, n, k, min_points, mask, st);
        KCHK(a);
        for (int batch = 6;; batch = 16) {
            for (int r = 0; r < batch; ++r) {
                dbscan_round<<<nb, 256, 0, a->stream>>>(rows, mask, rep, n, k, m, Mx, st);
                dbscan_step<<<1, 64, 0, a->stream>>>(st);
            }
            dbscan_starts<<<nb, 256, 0, a->stream>>>(word, rep, m, n, min_points, st, start);
            TRY(scan_into(a, start, number, n, &total));
            dbscan_labels<<<nb, 256, 0, a->stream>>>(word, rep, m, Mx, start, number, n, st, dl, dd);
            KCHK(a);
            HIPCHK(a, hipMemcpyAsync(a->u_host, st, sizeof(DbscanState), hipMemcpyDeviceToHost, a->stream));
            TRY(read_total(a, total, 4));
            TRY(from_device(a, (const int32_t*)dl, labels, (size_t)n, mem_kind));
            TRY(from_device(a, (const int32_t*)dd, degrees, (size_t)n, mem_kind));
            HIPCHK(a, hipStreamSynchronize(a->stream));
            DbscanState s;
            std::memcpy(&s, a->u_host, sizeof(s));
            if (s.phase == 2u) {
                *n_clusters = (int64_t)a->u_host[4];
                return MI_ICP_OK;
            }
            // each phase settles within (one-way edges) rounds that change something and one that does not
            if ((uint64_t)s.rounds >= 2ull * ((uint64_t)s.oneway + 1ull))
                return fail(a, MI_ICP_ERR_STATE, "the one-way edges did not settle in %u rounds", s.rounds);
        }
    });
}

int mi_icp_cluster_dbscan(mi_icp_ctx* c, const float* xyz, int64_t n, float eps, int64_t min_points, int max_edges,
                          int32_t* labels, int32_t* degrees, int64_t* n_clusters, int mem_kind) {
    const char* what = "cluster_dbscan";
    // (its own preamble: the count is n_clusters, and the message says so)
    TRY(check_ctx(c, mem_kind, what));
    if (!n_clusters) return fail(c, MI_ICP_ERR_INVALID, "%s: n_clusters is null", what);
    *n_clusters = 0;
    TRY(count_ok(c, what, n));
    if (n > 0 && (!xyz || !labels)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    if (!(eps > 0.0f) || !(eps * eps < INFINITY))
        return fail(c, MI_ICP_ERR_INVALID, "%s: eps must be positive, and finite when squared", what);
    if (min_points < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: min_points must not be negative", what);
    if (max_edges < 0 || max_edges > kKnnLimit)
        return fail(c, MI_ICP_ERR_INVALID, "%s: max_edges outside [0, %d] (knn::NUM_MAX_NN)", what, kKnnLimit);
    if (n == 0) return MI_ICP_OK;
    // (a degree is at most max_edges + 1: every larger threshold means "no core point")
    const int mp = (int)std::min<int64_t>(min_points, kKnnLimit + 2);
    return dbscan_impl(c, xyz, n, eps * eps, mp, max_edges, labels, degrees, n_clusters, mem_kind);
}

// ---------------------------------------------------------------------------
// geometry::keypoint::ComputeISSKeypoints (geometry/iss_keypoints.cu:108-172; iss.h).  The cloud gets a tree in the
// private scratch context, once; the model resolution (when a radius is 0) is knn_normals_kernel<2> at k = 2 summed in
// fp64, and its one scalar is the call's first wait; iss_kernel<0> and <1> follow on the same tree, and the count -- the
// total of the scan select.h compacts with -- comes back with the second wait, together with whatever the caller asked for.
static int iss_impl(mi_icp_ctx* c, const char* what, const float* xyz, int64_t n, float rs, float rn, IssGates gates,
                    int k, uint8_t* mask_out, float* saliency_out, float* eig_out, int32_t* counts_out, float* radii_out,
                    int64_t* m, int mem_kind) {
    return in_scratch(c, what, [&](mi_icp_ctx* a) -> int {
        const float* pts;
        TRY(to_device(a, xyz, (size_t)n * 3, mem_kind, a->stage[0], &pts));
        TRY(mi_icp_set_target(a, pts, nullptr, nullptr, n, MI_ICP_DEVICE));
        hipStream_t s = a->stream;
        if (rs == 0.0f || rn == 0.0f) {  // ComputeModelResolution (iss_keypoints.cu:37-49): both radii replaced
            float* half_d2;
            double *part, *sum;
            const int blocks = std::min(kOutlierBlocks, blocks_for(n));
            TRY(ensure(a, a->stage[3], (size_t)n, &half_d2));
            TRY(ensure(a, a->partial, (size_t)kOutlierBlocks * 4, &part));
            TRY(ensure(a, a->sys_dev, (size_t)kSysSize, &sum));
            TRY(launch_knn_normals<2>(a, 2, INFINITY, half_d2, nullptr, nullptr));
            outlier_stats_partial<<<blocks, 256, 0, s>>>(half_d2, n, part);
            iss_resolution_sum<<<1, 64, 0, s>>>(part, blocks, sum);
            KCHK(a);
            HIPCHK(a, hipMemcpyAsync(a->sys_host, sum, sizeof(double), hipMemcpyDeviceToHost, s));
            HIPCHK(a, hipStreamSynchronize(s));
            const float resolution = (float)std::sqrt(a->sys_host[0] / (double)n);
            rs = 6.0f * resolution;
            rn = 4.0f * resolution;
        }
        if (radii_out) {
            radii_out[0] = rs;
            radii_out[1] = rn;
        }
        if (!(rs * rs < INFINITY) || !(rn * rn < INFINITY)) return fail(a, MI_ICP_ERR_INVALID, "a radius is not finite when squared");
        float *sal, *eig;
        int32_t* cnt;
        uint8_t* mask;
        uint32_t *flags, *pos;
        const uint32_t* total;
        TRY(out_slot(a, saliency_out, (size_t)n, mem_kind, a->stage[1], &sal));
        if (!sal) TRY(ensure(a, a->stage[1], (size_t)n, &sal));  // (the caller does not want it; pass 1 does)
        TRY(out_slot(a, eig_out, (size_t)n * 3, mem_kind, a->stage[2], &eig));
        TRY(out_slot(a, counts_out, (size_t)n, mem_kind, a->stage[3], &cnt));
        TRY(out_slot(a, mask_out, (size_t)n, mem_kind, a->stage[4], &mask));
        TRY(ensure(a, a->flags, (size_t)n, &flags));
        const uint32_t nblocks = (uint32_t)((a->nleaf + 7) / 8);
        auto pass = [&](auto which, float r2) -> int {
            return knn_launch(a, k, nblocks, [](auto kc) { return iss_kernel<decltype(which)::value, decltype(kc)::value>; },
                              (const float*)a->nodes.p, (const float*)a->tblk.p, (const int32_t*)a->tidx.p, a->leaf_first,
                              a->nts, a->nleaf, k, r2, pts, gates, sal, eig, cnt, mask, flags);
        };
        TRY(pass(Cap<0>(), rs * rs));
        TRY(pass(Cap<1>(), rn * rn));
        TRY(scan_flags(a, flags, n, &pos, &total));
        TRY(read_total(a, total));
        TRY(from_device(a, (const float*)sal, saliency_out, (size_t)n, mem_kind));
        TRY(from_device(a, (const float*)eig, eig_out, (size_t)n * 3, mem_kind));
        TRY(from_device(a, (const int32_t*)cnt, counts_out, (size_t)n, mem_kind));
        TRY(from_device(a, (const uint8_t*)mask, mask_out, (size_t)n, mem_kind));
        HIPCHK(a, hipStreamSynchronize(s));
        *m = (int64_t)a->u_host[0];
        return MI_ICP_OK;
    });
}

int mi_icp_iss_keypoints(mi_icp_ctx* c, const float* xyz, int64_t n, float salient_radius, float non_max_radius,
                         float gamma_21, float gamma_32, int min_neighbors, int max_neighbors, uint8_t* mask_out,
                         float* saliency_out, float* eig_out, int32_t* counts_out, float* radii_out, int64_t* m,
                         int mem_kind) {
    const char* what = "iss_keypoints";
    // (its own preamble: radii_out is filled in between m and the size)
    TRY(check_ctx(c, mem_kind, what));
    if (!m) return fail(c, MI_ICP_ERR_INVALID, "%s: m is null", what);
    *m = 0;
    if (radii_out) {
        radii_out[0] = salient_radius;
        radii_out[1] = non_max_radius;
    }
    TRY(count_ok(c, what, n));
    if (n > 0 && (!xyz || !mask_out)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    if (!(salient_radius >= 0.0f) || !(non_max_radius >= 0.0f) || !(salient_radius * salient_radius < INFINITY) ||
        !(non_max_radius * non_max_radius < INFINITY))
        return fail(c, MI_ICP_ERR_INVALID, "%s: the radii must not be negative, and finite when squared", what);
    if (max_neighbors < 1 || max_neighbors > kKnnLimit)
        return fail(c, MI_ICP_ERR_INVALID, "%s: max_neighbors outside [1, %d] (knn::NUM_MAX_NN)", what, kKnnLimit);
    if (n == 0) return MI_ICP_OK;
    return iss_impl(c, what, xyz, n, salient_radius, non_max_radius, IssGates{min_neighbors, gamma_21, gamma_32},
                    max_neighbors, mask_out, saliency_out, eig_out, counts_out, radii_out, m, mem_kind);
}

// ---------------------------------------------------------------------------
// PointCloud::GaussianFilter (geometry/pointcloud.cu:56-106, 387-434; gaussian_filter.h): one tree of the cloud in the
// private scratch context, one launch, one wait.
int mi_icp_gaussian_filter(mi_icp_ctx* c, const float* xyz, const float* normals, const float* colors, int64_t n,
                           float search_radius, float sigma2, int num_max_search_points, float* out_xyz,
                           float* out_normals, float* out_colors, int mem_kind) {
    const char* what = "gaussian_filter";
    TRY(check_ctx(c, mem_kind, what));
    TRY(count_ok(c, what, n));
    if (!(search_radius > 0.0f) || !(search_radius * search_radius < INFINITY))
        return fail(c, MI_ICP_ERR_INVALID, "%s: search_radius must be positive, and finite when squared", what);
    if (!(sigma2 > 0.0f) || !(sigma2 < INFINITY)) return fail(c, MI_ICP_ERR_INVALID, "%s: sigma2 must be positive and finite", what);
    if (num_max_search_points < 1 || num_max_search_points > kKnnLimit)
        return fail(c, MI_ICP_ERR_INVALID, "%s: num_max_search_points outside [1, %d] (knn::NUM_MAX_NN)", what, kKnnLimit);
    if (n == 0) return MI_ICP_OK;
    Cloud cl{{xyz, normals, colors}, {out_xyz, out_normals, out_colors}};
    TRY(cloud_check(c, what, cl));
    const int k = num_max_search_points;
    return in_scratch(c, what, [&](mi_icp_ctx* a) -> int {
        TRY(cloud_upload(a, &cl, n, mem_kind, a->stage));
        const float* const* in = cl.in;
        TRY(mi_icp_set_target(a, in[0], nullptr, nullptr, n, MI_ICP_DEVICE));
        float* dst[3];  // (not cloud_emit: the launch itself can fail)
        TRY(cloud_out(a, in, cl.out, n, mem_kind, a->stage + 3, dst));
        TRY(knn_launch(a, k, (uint32_t)((a->nleaf + 7) / 8), [](auto kc) { return gaussian_kernel<decltype(kc)::value>; },
                       (const float*)a->nodes.p, (const float*)a->tblk.p, (const int32_t*)a->tidx.p, a->leaf_first, a->nts,
                       a->nleaf, k, search_radius * search_radius, sigma2, in[0], in[1], in[2], dst[0], dst[1], dst[2]));
        TRY(cloud_out_back(a, dst, cl.out, n, mem_kind));
        HIPCHK(a, hipStreamSynchronize(a->stream));
        return MI_ICP_OK;
    });
}

// ---------------------------------------------------------------------------
// knn::KDTreeFlann::SearchKNN / SearchRadius (knn/kdtree_flann.inl:46-122)
int mi_icp_search_knn(mi_icp_ctx* c, const float* queries, int64_t nq, int knn, float radius, int32_t* idx_out,
                      float* d2_out, int64_t* found, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "search_knn"));
    if (found) *found = 0;
    if (nq < 0 || knn < 0 || (nq > 0 && (!queries || !idx_out || !d2_out)))
        return fail(c, MI_ICP_ERR_INVALID, "search_knn: bad arguments");
    if (knn > kKnnLimit) return fail(c, MI_ICP_ERR_INVALID, "search_knn: more than %d neighbours (knn::NUM_MAX_NN) are not supported", kKnnLimit);
    if (c->nt <= 0) return fail(c, MI_ICP_ERR_STATE, "search_knn: no target cloud (mi_icp_set_target)");
    if (nq == 0 || knn == 0) return MI_ICP_OK;
    // the queries are staged exactly like an ICP source (Morton-ordered SoA + permutation)
    TRY(mi_icp_set_source(c, queries, nullptr, nullptr, nq, mem_kind));
    int32_t* d_idx;
    float* d_d2;
    TRY(out_slot(c, idx_out, (size_t)nq * knn, mem_kind, c->stage[4], &d_idx));
    TRY(out_slot(c, d2_out, (size_t)nq * knn, mem_kind, c->stage[5], &d_d2));
    unsigned long long* cnt;
    TRY(ensure(c, c->flags, 1, (unsigned long long**)&cnt));
    HIPCHK(c, hipMemsetAsync(cnt, 0, sizeof(unsigned long long), c->stream));
    TRY(knn_launch(c, knn, (uint32_t)((nq + 63) / 64), [](auto kc) { return knn_search_kernel<decltype(kc)::value>; },
                   (const float*)c->nodes.p, (const float*)c->tblk.p, (const int32_t*)c->tidx.p, c->leaf_first,
                   (const float*)c->sx.p, (const float*)c->sy.p, (const float*)c->sz.p, (const int32_t*)c->sperm.p, (int)nq,
                   c->nleaf, knn, radius > 0.0f ? radius * radius : INFINITY, d_idx, d_d2, cnt));
    TRY(from_device(c, (const int32_t*)d_idx, idx_out, (size_t)nq * knn, mem_kind));
    TRY(from_device(c, (const float*)d_d2, d2_out, (size_t)nq * knn, mem_kind));
    HIPCHK(c, hipMemcpyAsync(c->sys_host, cnt, sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (found) *found = (int64_t) * reinterpret_cast<unsigned long long*>(c->sys_host);
    return MI_ICP_OK;
}

int mi_icp_compute_color_gradients(mi_icp_ctx* c, float radius, int max_nn, float* gradients_out, int mem_kind) {
    TRY(check_ctx(c, mem_kind, "compute_color_gradients"));
    c->t_has_grad = false;
    if (c->nt <= 0) return MI_ICP_OK;
    if (!c->t_has_nrm || !c->t_has_int)
        return fail(c, MI_ICP_ERR_STATE, "compute_color_gradients: the target needs normals and colours");
    if (max_nn > kKnnLimit)
        return fail(c, MI_ICP_ERR_INVALID, "compute_color_gradients: more than %d neighbours (knn::NUM_MAX_NN) are not supported", kKnnLimit);
    const int64_t n = c->nt;
    float4* tgrad;
    TRY(ensure(c, c->tgrad, (size_t)c->nts, &tgrad));
    float* dg;
    TRY(out_slot(c, gradients_out, (size_t)n * 3, mem_kind, c->stage[1], &dg));
    TRY(launch_knn_normals<1>(c, max_nn, radius * radius, dg, (const float4*)c->tnrm.p, tgrad));
    c->t_has_grad = true;
    if (gradients_out) {
        TRY(from_device(c, (const float*)dg, gradients_out, (size_t)n * 3, mem_kind));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return MI_ICP_OK;
}

int mi_icp_registration_colored_icp(mi_icp_ctx* c, float max_distance, const float* init,
                                    const mi_icp_params* params, float lambda_geometric, mi_icp_result* out) {
    TRY(check_ctx(c));
    TRY(mi_icp_set_lambda_geometric(c, lambda_geometric));
    // colored_icp.cu:337-338: gradients over KDTreeSearchParamRadius(max_distance * 2, 30)
    if (c->nt > 0 && c->t_has_nrm && c->t_has_int)
        TRY(mi_icp_compute_color_gradients(c, max_distance * 2.0f, 30, nullptr, MI_ICP_DEVICE));
    return mi_icp_registration_icp(c, kEstColored, max_distance, init, params, out);
}

}  // extern "C"
