// fgr_rules.h -- the rules of FastGlobalRegistration that host and device share (include/mi_icp.h "feature matching
// and FastGlobalRegistration"): the sampler, the tuple test and the schedule of the line-process parameter.  Plain C++:
// the kernels (feature_kernels.h, segment_plane.h), the launcher (mi_feature.hip) and a stand-alone host program
// include it.  Compile with -ffp-contract=off: every product and sum below is one fp32 rounding.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MI_FGR_HD __host__ __device__ inline
#else
#define MI_FGR_HD inline
#endif

namespace mi {
namespace fgr {

// ---- the sampler: u(j) = output j of splitmix64 seeded with `seed` (SegmentPlane draws its triples from it too) ----
MI_FGR_HD uint64_t stream_u(uint64_t seed, uint64_t j) {
    uint64_t z = seed + (j + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// floor(u * m / 2^64): u mapped into [0, m)
MI_FGR_HD uint64_t below(uint64_t u, uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(u, m);
#else
    return (uint64_t)(((unsigned __int128)u * (unsigned __int128)m) >> 64);
#endif
}

// pair number m = 0, 1, 2 of trial t among ncorr reciprocal pairs
MI_FGR_HD uint64_t trial_pair(uint64_t seed, uint64_t t, int m, uint64_t ncorr) {
    return below(stream_u(seed, 3ull * t + (uint64_t)m), ncorr);
}

// squared length of a - b
MI_FGR_HD float side2(const float* a, const float* b) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// The tuple test on the caller's coordinates: p0, p1, p2 source points, q0, q1, q2 the target points paired with them,
// s2 = tuple_scale * tuple_scale.  Multiplications and comparisons only; a repeated pair (a zero side) fails by itself.
MI_FGR_HD bool tuple_ok(const float* p0, const float* p1, const float* p2, const float* q0, const float* q1, const float* q2,
                        float s2) {
    const float li[3] = {side2(p0, p1), side2(p1, p2), side2(p2, p0)};
    const float lj[3] = {side2(q0, q1), side2(q1, q2), side2(q2, q0)};
    bool ok = true;
    for (int k = 0; k < 3; ++k) ok = ok && (li[k] * s2 < lj[k]) && (lj[k] * s2 < li[k]);
    return ok;
}

// the line-process parameter after iteration `itr` (fast_global_registration.cu:365-369)
MI_FGR_HD float par_next(float par, int itr, bool decrease_mu, float maximum_correspondence_distance, float division_factor) {
    if (decrease_mu && itr % 4 == 0 && par > maximum_correspondence_distance) par = par / division_factor;
    return par;
}

// how many of `passing` accepted trials the cut list of `maximum_tuple_count` correspondences holds entries from
MI_FGR_HD int64_t cut_count(int64_t passing, int64_t maximum_tuple_count) {
    const int64_t all = 3 * passing;
    return all < maximum_tuple_count ? all : (maximum_tuple_count < 0 ? 0 : maximum_tuple_count);
}

}  // namespace fgr
}  // namespace mi
