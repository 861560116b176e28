// mi_feature.hip -- registration::Feature matching (knn::BruteForceNN in feature space), CorrespondencesFromFeatures and
// registration::FastGlobalRegistration (one translation unit of libmi_icp.so; csrc/ctx.h lists them)
#include "ctx.h"
#include "feature_kernels.h"

using namespace mi;
using namespace mi::eng;

// ---------------------------------------------------------------------------
// The contract is in include/mi_icp.h ("feature matching and FastGlobalRegistration"), the kernels in
// feature_kernels.h, the rules host and device share in fgr_rules.h.  Every buffer is the caller's DEVICE memory; the
// work runs in the private scratch context `a` (ctx.h in_scratch), whose fgr[] buffers hold what a call needs beyond
// its arguments: [0] the two key arrays, [1] the reciprocal pairs, [2] the cut tuple list, [3] / [4] the normalised
// clouds, [5] the optimiser's moving target points, [6] the words below, [7] neighbour lists.
namespace {

struct FgrWords {        // fgr[6]
    double partial[kFgrSumBlocks * 4];
    double sums[27];
    float mean[2][4];    // source, target
    float scales[2];     // scale_global, the largest norm
    float trans[16];     // the optimiser's result, normalised frame
    float T[16];         // ... mapped back
    float par;
    uint32_t max_bits;
    uint32_t n_corr;     // the cut list's length
};

int dims_ok(mi_icp_ctx* c, const char* what, int64_t nq, int64_t nr, int dim) {
    if (dim < 1 || dim > MI_ICP_FEATURE_MAX_DIM) return fail(c, MI_ICP_ERR_INVALID, "%s: dim must be in [1, %d]", what, MI_ICP_FEATURE_MAX_DIM);
    if (nq < 1 || nr < 1 || nq > 0x7fffffffll || nr > 0x7fffffffll) return fail(c, MI_ICP_ERR_INVALID, "%s: sizes must be in [1, 2^31)", what);
    return MI_ICP_OK;
}

// qkey[nq], rkey[nr] in a->fgr[0]: both directions' minima from one pass
int run_match(mi_icp_ctx* a, const float* q, int64_t nq, const float* r, int64_t nr, int dim, unsigned long long** qkey,
              unsigned long long** rkey) {
    unsigned long long* keys;
    TRY(ensure(a, a->fgr[0], (size_t)nq + (size_t)nr, &keys));
    HIPCHK(a, hipMemsetAsync(keys, 0xff, ((size_t)nq + (size_t)nr) * sizeof(unsigned long long), a->stream));
    const int64_t tiles_q = (nq + kFmTile - 1) / kFmTile, tiles_r = (nr + kFmTile - 1) / kFmTile, tiles = tiles_q * tiles_r;
    const int grid = (int)std::min<int64_t>(tiles, kFmMaxBlocks);
    feature_match_kernel<<<grid, 256, 0, a->stream>>>(q, nq, r, nr, dim, tiles_r, tiles, keys, keys + nq);
    KCHK(a);
    *qkey = keys;
    *rkey = keys + nq;
    return MI_ICP_OK;
}

// the rows of s_idx that have a neighbour (and, reciprocal, whose neighbour points back) -> pairs, ascending; one wait
int run_pairs(mi_icp_ctx* a, const int32_t* s_idx, int64_t ns, const int32_t* t_idx, int64_t nt, int reciprocal, int32_t* pairs,
              int64_t* n_pairs) {
    uint32_t *flags, *pos;
    const uint32_t* total;
    TRY(ensure(a, a->flags, (size_t)ns, &flags));
    fgr_recip_flags<<<blocks_for(ns), 256, 0, a->stream>>>(s_idx, ns, t_idx, nt, reciprocal, flags);
    KCHK(a);
    TRY(scan_flags(a, flags, ns, &pos, &total));
    fgr_recip_list<<<blocks_for(ns), 256, 0, a->stream>>>(s_idx, ns, flags, pos, pairs);
    KCHK(a);
    TRY(read_total(a, total));
    HIPCHK(a, hipStreamSynchronize(a->stream));
    *n_pairs = (int64_t)a->u_host[0];
    return MI_ICP_OK;
}

// the cut tuple list of `ncorr` pairs -> corr, its length -> *n_dev (device word); no wait
int run_tuples(mi_icp_ctx* a, const int32_t* pairs, int64_t ncorr, const float* src, int64_t ns, const float* tgt, int64_t nt,
               float tuple_scale, int64_t max_corr, uint64_t seed, int32_t* corr, uint32_t* n_dev) {
    const int64_t trials = 100 * ncorr;
    if (trials > kMaxCount) return fail(a, MI_ICP_ERR_INVALID, "fgr: more than %lld trials are not supported", (long long)kMaxCount);
    if (trials == 0 || max_corr <= 0) {
        HIPCHK(a, hipMemsetAsync(n_dev, 0, sizeof(uint32_t), a->stream));
        return MI_ICP_OK;
    }
    uint32_t *flags, *pos;
    const uint32_t* total;
    TRY(ensure(a, a->flags, (size_t)trials, &flags));
    const float s2 = tuple_scale * tuple_scale;
    fgr_trial_flags<<<blocks_for(trials), 256, 0, a->stream>>>(pairs, ncorr, src, ns, tgt, nt, seed, s2, trials, flags);
    KCHK(a);
    TRY(scan_flags(a, flags, trials, &pos, &total));
    fgr_trial_emit<<<blocks_for(trials), 256, 0, a->stream>>>(pairs, ncorr, seed, trials, flags, pos, total, max_corr, corr, n_dev);
    KCHK(a);
    return MI_ICP_OK;
}

int64_t corr_room(int64_t ns, int64_t nt, int64_t max_corr) {  // entries the cut list can reach
    return std::max<int64_t>(0, std::min<int64_t>(max_corr, 300 * std::min(ns, nt)));
}

int option_ok(mi_icp_ctx* c, const char* what, const mi_icp_fgr_option* o) {
    if (!o) return fail(c, MI_ICP_ERR_INVALID, "%s: option is null", what);
    if (o->iteration_number < 0 || o->maximum_tuple_count < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: negative iteration_number or maximum_tuple_count", what);
    return MI_ICP_OK;
}

int launch_optimize(mi_icp_ctx* a, const float* src, int64_t ns, const float* tgt, int64_t nt, const int32_t* corr, int64_t count_host,
                    const uint32_t* count_dev, float par_host, const float* par_dev, const mi_icp_fgr_option* o, int64_t room, float* T16,
                    double* sums27, float* par_out) {
    float* qwork;
    TRY(ensure(a, a->fgr[5], (size_t)std::max<int64_t>(room, 1) * 3, &qwork));
    fgr_optimize_kernel<<<1, 256, 0, a->stream>>>(src, ns, tgt, nt, corr, count_host, count_dev, par_host, par_dev, o->iteration_number,
                                                  o->decrease_mu, o->maximum_correspondence_distance, o->division_factor, qwork, T16, sums27,
                                                  par_out);
    KCHK(a);
    return MI_ICP_OK;
}

// centred (and, unless absolute, scaled) copies of both clouds; means, scales in w
int run_normalize(mi_icp_ctx* a, FgrWords* w, const float* src, int64_t ns, const float* tgt, int64_t nt, int use_absolute_scale, float** nsrc,
                  float** ntgt) {
    TRY(ensure(a, a->fgr[3], (size_t)ns * 3, nsrc));
    TRY(ensure(a, a->fgr[4], (size_t)nt * 3, ntgt));
    hipStream_t s = a->stream;
    HIPCHK(a, hipMemsetAsync(&w->max_bits, 0, sizeof(uint32_t), s));
    const float* in[2] = {src, tgt};
    float* out[2] = {*nsrc, *ntgt};
    const int64_t n[2] = {ns, nt};
    for (int k = 0; k < 2; ++k) {
        const int nb = std::min(kFgrSumBlocks, blocks_for(n[k]));
        fgr_sum_partial<<<nb, 256, 0, s>>>(in[k], n[k], w->partial);
        fgr_mean_final<<<1, 64, 0, s>>>(w->partial, nb, n[k], w->mean[k]);
        fgr_center_max<<<blocks_for(n[k]), 256, 0, s>>>(in[k], n[k], w->mean[k], out[k], &w->max_bits);
    }
    fgr_scales<<<1, 1, 0, s>>>(&w->max_bits, use_absolute_scale, w->scales);
    if (!use_absolute_scale)  // (a division by 1 changes nothing)
        for (int k = 0; k < 2; ++k) fgr_divide<<<blocks_for(n[k] * 3), 256, 0, s>>>(out[k], n[k] * 3, w->scales);
    KCHK(a);
    return MI_ICP_OK;
}

}  // namespace

extern "C" {

int mi_icp_feature_match(mi_icp_ctx* c, const float* q, int64_t nq, const float* r, int64_t nr, int dim, int32_t* q_idx, float* q_d,
                         int32_t* r_idx, float* r_d) {
    const char* what = "feature_match";
    TRY(check_ctx(c));
    TRY(dims_ok(c, what, nq, nr, dim));
    if (!q || !r) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    return in_scratch(c, what, [&](mi_icp_ctx* a) -> int {
        unsigned long long *qkey, *rkey;
        TRY(run_match(a, q, nq, r, nr, dim, &qkey, &rkey));
        if (q_idx || q_d) fm_decode<<<blocks_for(nq), 256, 0, a->stream>>>(qkey, nq, q_idx, q_d);
        if (r_idx || r_d) fm_decode<<<blocks_for(nr), 256, 0, a->stream>>>(rkey, nr, r_idx, r_d);
        KCHK(a);
        return MI_ICP_OK;
    });
}

int mi_icp_fgr_correspondences(mi_icp_ctx* c, const int32_t* s_idx, int64_t ns, const int32_t* t_idx, int64_t nt, const float* src_xyz,
                               const float* tgt_xyz, float tuple_scale, int64_t maximum_tuple_count, uint64_t seed, int32_t* pairs,
                               int64_t* n_pairs, int32_t* corr, int64_t* n_corr) {
    const char* what = "fgr_correspondences";
    TRY(check_ctx(c));
    if (!n_pairs || !n_corr) return fail(c, MI_ICP_ERR_INVALID, "%s: a count is null", what);
    *n_pairs = *n_corr = 0;
    if (ns < 1 || nt < 1 || ns > kMaxCount || nt > kMaxCount) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    if (maximum_tuple_count < 0) return fail(c, MI_ICP_ERR_INVALID, "%s: negative maximum_tuple_count", what);
    if (!s_idx || !t_idx || !src_xyz || !tgt_xyz || !pairs || (!corr && corr_room(ns, nt, maximum_tuple_count) > 0))
        return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    return in_scratch(c, what, [&](mi_icp_ctx* a) -> int {
        FgrWords* w;
        TRY(ensure(a, a->fgr[6], 1, &w));
        TRY(run_pairs(a, s_idx, ns, t_idx, nt, 1, pairs, n_pairs));
        TRY(run_tuples(a, pairs, *n_pairs, src_xyz, ns, tgt_xyz, nt, tuple_scale, maximum_tuple_count, seed, corr, &w->n_corr));
        HIPCHK(a, hipMemcpyAsync(a->u_host, &w->n_corr, sizeof(uint32_t), hipMemcpyDeviceToHost, a->stream));
        HIPCHK(a, hipStreamSynchronize(a->stream));
        *n_corr = (int64_t)a->u_host[0];
        return MI_ICP_OK;
    });
}

int mi_icp_fgr_optimize(mi_icp_ctx* c, const float* src_xyz, int64_t ns, const float* tgt_xyz, int64_t nt, const int32_t* corr,
                        int64_t n_corr, float par_start, const mi_icp_fgr_option* option, float* T16, double* sums27, float* par_out) {
    const char* what = "fgr_optimize";
    TRY(check_ctx(c));
    TRY(option_ok(c, what, option));
    if (ns < 1 || nt < 1 || ns > kMaxCount || nt > kMaxCount || n_corr < 0 || n_corr > kMaxCount) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    if (!src_xyz || !tgt_xyz || !T16 || (n_corr > 0 && !corr)) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    return in_scratch(c, what, [&](mi_icp_ctx* a) -> int {
        return launch_optimize(a, src_xyz, ns, tgt_xyz, nt, corr, n_corr, nullptr, par_start, nullptr, option, n_corr, T16, sums27, par_out);
    });
}

int mi_icp_correspondences_from_features(mi_icp_ctx* c, const float* src_feat, int64_t ns, const float* tgt_feat, int64_t nt, int dim,
                                         int mutual_filter, float mutual_consistency_ratio, int32_t* corr, int64_t* n_corr) {
    const char* what = "correspondences_from_features";
    TRY(check_ctx(c));
    if (!n_corr) return fail(c, MI_ICP_ERR_INVALID, "%s: n_corr is null", what);
    *n_corr = 0;
    TRY(dims_ok(c, what, ns, nt, dim));
    if (ns > kMaxCount || nt > kMaxCount) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    if (!src_feat || !tgt_feat || !corr) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    return in_scratch(c, what, [&](mi_icp_ctx* a) -> int {
        unsigned long long *qkey, *rkey;
        int32_t* idx;
        TRY(ensure(a, a->fgr[7], (size_t)ns + (size_t)nt, &idx));
        TRY(run_match(a, src_feat, ns, tgt_feat, nt, dim, &qkey, &rkey));
        fm_decode<<<blocks_for(ns), 256, 0, a->stream>>>(qkey, ns, idx, nullptr);
        fm_decode<<<blocks_for(nt), 256, 0, a->stream>>>(rkey, nt, idx + ns, nullptr);
        KCHK(a);
        TRY(run_pairs(a, idx, ns, idx + ns, nt, mutual_filter ? 1 : 0, corr, n_corr));
        if (mutual_filter && (float)*n_corr < mutual_consistency_ratio * (float)ns)  // too few: the unfiltered list
            TRY(run_pairs(a, idx, ns, idx + ns, nt, 0, corr, n_corr));
        return MI_ICP_OK;
    });
}

int mi_icp_fast_global_registration(mi_icp_ctx* c, const float* src_xyz, const float* src_feat, int64_t ns, const float* tgt_xyz,
                                    const float* tgt_feat, int64_t nt, int dim, const mi_icp_fgr_option* option, uint64_t seed,
                                    mi_icp_result* out) {
    const char* what = "fast_global_registration";
    TRY(check_ctx(c));
    if (!out) return fail(c, MI_ICP_ERR_INVALID, "%s: out is null", what);
    std::memset(out, 0, sizeof(*out));
    TRY(option_ok(c, what, option));
    TRY(dims_ok(c, what, ns, nt, dim));
    if (ns > kMaxCount || nt > kMaxCount) return fail(c, MI_ICP_ERR_INVALID, "%s: bad size", what);
    if (!src_xyz || !src_feat || !tgt_xyz || !tgt_feat) return fail(c, MI_ICP_ERR_INVALID, "%s: null buffer", what);
    float T[16];
    TRY(in_scratch(c, what, [&](mi_icp_ctx* a) -> int {
        FgrWords* w;
        unsigned long long *qkey, *rkey;
        int32_t *idx, *pairs, *corr;
        float *nsrc, *ntgt;
        const int64_t room = corr_room(ns, nt, option->maximum_tuple_count);
        TRY(ensure(a, a->fgr[6], 1, &w));
        TRY(ensure(a, a->fgr[7], (size_t)ns + (size_t)nt, &idx));
        TRY(ensure(a, a->fgr[1], (size_t)std::min(ns, nt) * 2, &pairs));
        TRY(ensure(a, a->fgr[2], (size_t)std::max<int64_t>(room, 1) * 2, &corr));
        TRY(run_match(a, src_feat, ns, tgt_feat, nt, dim, &qkey, &rkey));
        fm_decode<<<blocks_for(ns), 256, 0, a->stream>>>(qkey, ns, idx, nullptr);
        fm_decode<<<blocks_for(nt), 256, 0, a->stream>>>(rkey, nt, idx + ns, nullptr);
        KCHK(a);
        int64_t ncorr = 0;
        TRY(run_pairs(a, idx, ns, idx + ns, nt, 1, pairs, &ncorr));  // (the call's first wait: the trials' count)
        TRY(run_tuples(a, pairs, ncorr, src_xyz, ns, tgt_xyz, nt, option->tuple_scale, option->maximum_tuple_count, seed, corr, &w->n_corr));
        TRY(run_normalize(a, w, src_xyz, ns, tgt_xyz, nt, option->use_absolute_scale, &nsrc, &ntgt));
        // (the reference hands scale_global to the optimiser's scale_start: kept)
        TRY(launch_optimize(a, nsrc, ns, ntgt, nt, corr, 0, &w->n_corr, 0.0f, &w->scales[0], option, room, w->trans, w->sums, &w->par));
        fgr_finish<<<1, 1, 0, a->stream>>>(w->trans, w->mean[0], w->mean[1], w->scales, w->T);
        KCHK(a);
        HIPCHK(a, hipMemcpyAsync(a->f_host, w->T, sizeof(float) * 16, hipMemcpyDeviceToHost, a->stream));
        HIPCHK(a, hipStreamSynchronize(a->stream));  // (the second)
        std::memcpy(T, a->f_host, sizeof(T));
        return MI_ICP_OK;
    }));
    // EvaluateRegistration(source, target, maximum_correspondence_distance, T) on the caller's context: the clouds are
    // loaded there, so mi_icp_get_correspondences gives the result's correspondence_set
    TRY(mi_icp_set_target(c, tgt_xyz, nullptr, nullptr, nt, MI_ICP_DEVICE));
    TRY(mi_icp_set_source(c, src_xyz, nullptr, nullptr, ns, MI_ICP_DEVICE));
    return mi_icp_evaluate_registration(c, option->maximum_correspondence_distance, T, out);
}

}  // extern "C"
