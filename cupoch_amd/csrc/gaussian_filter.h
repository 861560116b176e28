// gaussian_filter.h -- PointCloud::GaussianFilter (geometry/pointcloud.cu:56-106, 387-434).
//
// The reference: SearchRadius(search_radius, max_nn) with N x max_nn indices and distances written out, then a transform
// that reads them back and forms the weighted means.  Here it is iss.h's pass 0 with another phase C: phases A and B on
// the cloud's own tree leave the lane's row -- ordered by (d2, ORIGINAL index), KnnList<KCAP, true>, so a truncated row
// holds exactly the reference's points -- in its LDS distance column and its slab index column, and phase C adds
// w = exp(-0.5 * d2 / sigma2) and w * (point, normal, colour) over the row in registers and writes 12 to 36 bytes at the
// point's original index.  No row reaches memory.  The contract is stated in include/mi_icp.h (mi_icp_gaussian_filter).
#pragma once
#include "iss.h"

namespace mi {

__device__ __forceinline__ void gauss_add(const float* __restrict__ a, int64_t j, float w, float* s) {
    s[0] += w * a[j * 3];
    s[1] += w * a[j * 3 + 1];
    s[2] += w * a[j * 3 + 2];
}
__device__ __forceinline__ void gauss_put(float* __restrict__ out, int64_t i, const float* s, float total) {
    out[i * 3] = s[0] / total;
    out[i * 3 + 1] = s[1] / total;
    out[i * 3 + 2] = s[2] / total;
}

// pts / nrm / col: the cloud in the caller's order (nrm, col and their outputs may be null).  The row's d2 are the ones
// the search compared -- sq3 of the fp32 differences -- so the weights are a function of the row alone.
template <int KCAP = kMaxKnn>
__global__ __launch_bounds__(64) void gaussian_kernel(
        const float* __restrict__ records_g, const float* __restrict__ tblk_g, const int32_t* __restrict__ tidx_g,
        uint32_t leaf_first, int64_t n, int nleaf, int k, float r2, float sigma2, const float* __restrict__ pts,
        const float* __restrict__ nrm, const float* __restrict__ col, float* __restrict__ out_p, float* __restrict__ out_n,
        float* __restrict__ out_c, uint32_t nblocks, KnnSlab slab) {
    knn_wave<KCAP>(nblocks, slab, [&](uint32_t pkt, float* kd2, int32_t* kidx) {
        float qx, qy, qz;
        int32_t orig;
        knn_own_query(tblk_g, tidx_g, n, pkt, qx, qy, qz, orig);
        const bool valid = orig >= 0;
        KnnList<KCAP, true> l(kd2, kidx, k, valid ? r2 : -1.0f, tidx_g);
        knn_own_neighbours(records_g, tblk_g, leaf_first, nleaf, pkt, valid, qx, qy, qz, l);
        if (!valid) return;
        float total = 0.0f;
        float sp[3] = {0, 0, 0}, sn[3] = {0, 0, 0}, sc[3] = {0, 0, 0};
        for (int t = 0; t < l.st.count; ++t) {
            const int64_t j = l.kidx[t * 64 + l.lane];
            const float w = expf(-0.5f * l.kd2[t * 64 + l.lane] / sigma2);
            total += w;
            gauss_add(pts, j, w, sp);
            if (nrm) gauss_add(nrm, j, w, sn);
            if (col) gauss_add(col, j, w, sc);
        }
        // (an empty row -- a point with a non-finite coordinate finds nothing, itself included -- gives 0 / 0 = NaN)
        gauss_put(out_p, orig, sp, total);
        if (nrm) gauss_put(out_n, orig, sn, total);
        if (col) gauss_put(out_c, orig, sc, total);
    });
}

}  // namespace mi
