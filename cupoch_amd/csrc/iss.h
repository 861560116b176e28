// iss.h -- geometry::keypoint::ComputeISSKeypoints (geometry/iss_keypoints.cu:37-172): Intrinsic Shape Signatures.
//
// The reference: SearchRadius(salient_radius, max_nn) with N x max_nn indices and distances written out, a reduce_by_key
// over N x max_nn cumulant tuples, FastEigen3x3Val per point, a second SearchRadius(non_max_radius, max_nn) written
// out, and a transform over its rows.  Here both passes are phases A/B of knn_normals.h on the cloud's own tree -- the
// lists ordered by (d2, ORIGINAL index), KnnList<KCAP, true>, so a truncated row holds exactly the reference's points --
// and a phase C that never hands a row out:
//   PASS 0  (saliency)  the nine cumulants of q = p_j - p_i over the lane's row, in registers; covariance, the zero
//           test, the eigenvalues alone (eigen3.h fast_eigen3x3_val), the two ratio gates; saliency[orig] and, for
//           callers who want them, the three eigenvalues and the row's length.
//   PASS 1  (non-maximum suppression)  the lane gathers saliency[l] over its row; mask byte and compaction flag at
//           [orig].  A point whose saliency is negative cannot be a keypoint and does not search.
// The contract is stated in include/mi_icp.h (mi_icp_iss_keypoints).  The row's entries are original indices, so the
// neighbours' coordinates come from the cloud in the caller's order (`pts`), not from the tree's leaves.
#pragma once
#include "knn_normals.h"

namespace mi {

struct IssGates {
    int min_neighbors;
    float gamma_21, gamma_32;
};

// ---- phases A and B of knn_normals_kernel for the lane's own point, restated (that kernel's text is left as it is:
// factoring these lines out of it changed its register allocation).  knn_own_query: the coordinates and ORIGINAL index
// (-1: a padding slot, or past the end) of sorted position pkt * 64 + lane.  knn_own_neighbours: the list seeded from
// the Morton neighbourhood of the packet's leaves, then the walk.
__device__ __forceinline__ void knn_own_query(const float* tblk_g, const int32_t* tidx_g, int64_t n, uint32_t pkt,
                                              float& qx, float& qy, float& qz, int32_t& orig) {
    const int64_t i = (int64_t)pkt * 64 + lane_id();
    qx = qy = qz = 0.0f;
    orig = -1;
    if (i < n) {  // n = sorted positions; padding slots carry original index -1
        const float* line = tblk_g + (i >> 3) * kLeafFloats + (i & 7);
        qx = line[0];
        qy = line[8];
        qz = line[16];
        orig = tidx_g[i];
    }
}
template <class List>
__device__ __forceinline__ void knn_own_neighbours(const float* records_g, const float* tblk_g, uint32_t leaf_first,
                                                   int nleaf, uint32_t pkt, bool active, float qx, float qy, float qz,
                                                   List& l) {
    const cfloat_p tblk = (cfloat_p)(uintptr_t)tblk_g;
    const int leaf0 = (int)pkt * 8;
    const int seed_lo = max(0, leaf0 - kKnnSeedBefore);
    const int seed_hi = min(nleaf, leaf0 + kKnnSeedAfter);
    for (int L = seed_lo; L < seed_hi; ++L) {
        const LeafXYZ p = load_leaf(tblk, L);
#pragma unroll
        for (int t = 0; t < kLeaf; ++t)
            l.offer(sq3(qx - p.x[t], qy - p.y[t], qz - p.z[t]), L * kLeaf + t);  // padding points have d2 = +inf
    }
    knn_walk<true>(records_g, tblk_g, leaf_first, active, qx, qy, qz, (uint32_t)seed_lo, (uint32_t)seed_hi, l);
}

constexpr float kIssZero = 1.0e-5f;  // Eigen's isZero() at fp32: every |c_ij| <= 1e-5, absolute (iss_keypoints.cu:64)

// ---- C of pass 0: saliency of the lane's point q from its row; ev[3] = the eigenvalues it was decided on, ascending
// ((-1, -1, -1): too few neighbours, or a zero covariance, as ComputeThirdEigenValue returns then)
template <int KCAP>
__device__ __forceinline__ float iss_saliency(const float* __restrict__ pts, float qx, float qy, float qz,
                                              const KnnList<KCAP, true>& l, const IssGates& g, float* ev) {
    ev[0] = ev[1] = ev[2] = -1.0f;
    const int count = l.st.count;
    if (count < g.min_neighbors) return -1.0f;
    float cum[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = 0; t < count; ++t) {
        const float* p = pts + (int64_t)l.kidx[t * 64 + l.lane] * 3;
        const float x = p[0] - qx, y = p[1] - qy, z = p[2] - qz;
        cum[0] += x;
        cum[1] += y;
        cum[2] += z;
        cum[3] += x * x;
        cum[4] += x * y;
        cum[5] += x * z;
        cum[6] += y * y;
        cum[7] += y * z;
        cum[8] += z * z;
    }
    const float cnt = (float)count;
#pragma unroll
    for (int e = 0; e < 9; ++e) cum[e] = cum[e] / cnt;
    M3 A;
    A.m[0][0] = cum[3] - cum[0] * cum[0];
    A.m[1][1] = cum[6] - cum[1] * cum[1];
    A.m[2][2] = cum[8] - cum[2] * cum[2];
    A.m[0][1] = A.m[1][0] = cum[4] - cum[0] * cum[1];
    A.m[0][2] = A.m[2][0] = cum[5] - cum[0] * cum[2];
    A.m[1][2] = A.m[2][1] = cum[7] - cum[1] * cum[2];
    const bool zero = fabsf(A.m[0][0]) <= kIssZero && fabsf(A.m[1][1]) <= kIssZero && fabsf(A.m[2][2]) <= kIssZero &&
                      fabsf(A.m[0][1]) <= kIssZero && fabsf(A.m[0][2]) <= kIssZero && fabsf(A.m[1][2]) <= kIssZero;
    if (zero) return -1.0f;
    fast_eigen3x3_val(A, ev);
    return (ev[2] > 0.0f && ev[1] / ev[2] < g.gamma_21 && ev[0] / ev[1] < g.gamma_32) ? ev[0] : -1.0f;
}

// ---- C of pass 1: is the lane's point (saliency s >= 0) a maximum of its row?  Strict: tied neighbours both stay.
template <int KCAP>
__device__ __forceinline__ bool iss_is_maximum(const float* __restrict__ saliency, float s, const KnnList<KCAP, true>& l) {
    bool keep = s >= 0.0f;
    for (int t = 0; t < l.st.count; ++t) keep = keep && !(s < saliency[l.kidx[t * 64 + l.lane]]);
    return keep;
}

// PASS 0: saliency[n] written, eig_out[n][3] and cnt_out[n] when not null.  PASS 1: saliency[n] read, mask_out[n]
// (bytes, 0 / 1) and flags[n] (words, for the compaction's scan) written.  Everything at the points' original indices.
template <int PASS, int KCAP = kMaxKnn>
__global__ __launch_bounds__(64) void iss_kernel(
        const float* __restrict__ records_g, const float* __restrict__ tblk_g, const int32_t* __restrict__ tidx_g,
        uint32_t leaf_first, int64_t n, int nleaf, int k, float r2, const float* __restrict__ pts, IssGates gates,
        float* __restrict__ saliency, float* __restrict__ eig_out, int32_t* __restrict__ cnt_out,
        uint8_t* __restrict__ mask_out, uint32_t* __restrict__ flags, uint32_t nblocks, KnnSlab slab) {
    knn_wave<KCAP>(nblocks, slab, [&](uint32_t pkt, float* kd2, int32_t* kidx) {
        float qx, qy, qz;
        int32_t orig;
        knn_own_query(tblk_g, tidx_g, n, pkt, qx, qy, qz, orig);
        const bool valid = orig >= 0;
        float s = -1.0f;
        if (PASS == 1 && valid) s = saliency[orig];
        const bool active = valid && k > 0 && (PASS == 0 || s >= 0.0f);
        KnnList<KCAP, true> l(kd2, kidx, k, active ? r2 : -1.0f, tidx_g);
        knn_own_neighbours(records_g, tblk_g, leaf_first, nleaf, pkt, active, qx, qy, qz, l);

        if (!valid) return;
        if constexpr (PASS == 0) {
            float ev[3];
            saliency[orig] = iss_saliency(pts, qx, qy, qz, l, gates, ev);
            if (eig_out) {
                eig_out[(int64_t)orig * 3] = ev[0];
                eig_out[(int64_t)orig * 3 + 1] = ev[1];
                eig_out[(int64_t)orig * 3 + 2] = ev[2];
            }
            if (cnt_out) cnt_out[orig] = l.st.count;
        } else {
            const bool keep = iss_is_maximum(saliency, s, l);
            mask_out[orig] = keep ? (uint8_t)1 : (uint8_t)0;
            flags[orig] = keep ? 1u : 0u;
        }
    });
}

// One wave: the model resolution's sum.  partial[b][4] are select.h's per-block fp64 sums of knn_mean_d2 at k = 2 --
// (0 + d2 of the nearest other entry) / 2 per point, exact -- so twice their total is the sum of the squared nearest
// distances.  Lane l adds blocks l, l + 64, ... in order, wave_sum the lanes in its fixed order.
static __global__ __launch_bounds__(64) void iss_resolution_sum(const double* __restrict__ partial, int nblocks,
                                                               double* __restrict__ sum_out) {
    const int lane = lane_id();
    double s = 0.0;
    for (int b = lane; b < nblocks; b += 64) s += partial[b * 4];
    s = wave_sum(s);
    if (lane == kWaveSumLane) *sum_out = 2.0 * s;
}

}  // namespace mi
