// collision_predicates.h -- the collision family's predicates (include/mi_icp.h, "collision"): cell boxes, cell-cell,
// segment-cell, sphere-cell, box-cell, capsule-cell, the primitives' bounding boxes.  Plain C++ that hipcc compiles for
// the device and any host compiler compiles for a test (tests/cpp/test_collision_predicates.cpp), as edt_envelope.h is.
// Everything is fp32 in exactly the order written; the build passes -ffp-contract=off, so no product is fused.
// tests/collision_exact.py restates every function here in numpy.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "../../include/mi_icp.h"

#if defined(__HIPCC__)
#define COL_HD __host__ __device__ inline
#else
#define COL_HD inline
#endif

namespace mi {
namespace col {

COL_HD bool finite(float x) { return x - x == 0.0f; }
COL_HD float fmax2(float a, float b) { return a > b ? a : b; }  // (no NaN reaches these: the callers check first)
COL_HD float fmin2(float a, float b) { return a < b ? a : b; }

// the box of the voxel with key k along one axis: [lo, hi] = [(float)k * vs + origin, (float)(k + 1) * vs + origin].
// Both are non-decreasing in k (a rounding is monotone), which is what the candidate ranges rest on.
COL_HD float cell_lo(int32_t k, float vs, float origin) { return (float)k * vs + origin; }
COL_HD float cell_hi(int32_t k, float vs, float origin) { return (float)((int64_t)k + 1) * vs + origin; }  // (k + 1 in 64 bits)

// cell-cell, closed: per axis a.lo <= b.hi && b.lo <= a.hi (a: already inflated) -- as a range of b's keys, cell_range
// below; no kernel evaluates it cell by cell

// segment-cell: LineSegmentAABB (intersection_test.inl:93-118) on the box [lo, hi] (already inflated)
COL_HD bool segment_cell(const float* p0, const float* p1, const float* lo, const float* hi) {
    float ext[3], mid[3], dst[3], ad[3];
    for (int i = 0; i < 3; ++i) {
        const float center = (lo[i] + hi[i]) * 0.5f;
        ext[i] = hi[i] - center;
        const float m = (p0[i] + p1[i]) * 0.5f;
        dst[i] = p1[i] - m;
        mid[i] = m - center;
    }
    for (int i = 0; i < 3; ++i) {
        ad[i] = fabsf(dst[i]);
        if (fabsf(mid[i]) > ext[i] + ad[i]) return false;
    }
    for (int i = 0; i < 3; ++i) ad[i] = ad[i] + FLT_EPSILON;
    if (fabsf(mid[1] * dst[2] - mid[2] * dst[1]) > ext[1] * ad[2] + ext[2] * ad[1]) return false;
    if (fabsf(mid[2] * dst[0] - mid[0] * dst[2]) > ext[2] * ad[0] + ext[0] * ad[2]) return false;
    if (fabsf(mid[0] * dst[1] - mid[1] * dst[0]) > ext[0] * ad[1] + ext[1] * ad[0]) return false;
    return true;
}

// the squared distance of q to the box [lo, hi]: e_i = max(max(lo_i - q_i, q_i - hi_i), 0), (e0^2 + e1^2) + e2^2
COL_HD float point_cell_d2(const float* q, const float* lo, const float* hi) {
    const float e0 = fmax2(fmax2(lo[0] - q[0], q[0] - hi[0]), 0.0f);
    const float e1 = fmax2(fmax2(lo[1] - q[1], q[1] - hi[1]), 0.0f);
    const float e2 = fmax2(fmax2(lo[2] - q[2], q[2] - hi[2]), 0.0f);
    return (e0 * e0 + e1 * e1) + e2 * e2;
}

// box-cell: the fifteen separating axes.  rot[j][i] = transform[i * 4 + j] is the primitive's rotation (column-major
// storage); the box's axes are its columns, so R[i][j] = rot[j][i] = transform[i * 4 + j].  cb: the box's centre, ea: its
// half lengths; cc / eb: the cell's centre and half extent (margin included).
COL_HD bool box_cell(const float* transform, const float* ea, const float* cc, const float* eb) {
    float R[3][3], A[3][3], t[3];
    const float dc0 = cc[0] - transform[12], dc1 = cc[1] - transform[13], dc2 = cc[2] - transform[14];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            R[i][j] = transform[i * 4 + j];
            A[i][j] = fabsf(R[i][j]) + FLT_EPSILON;
        }
        t[i] = (R[i][0] * dc0 + R[i][1] * dc1) + R[i][2] * dc2;
    }
    for (int i = 0; i < 3; ++i)
        if (fabsf(t[i]) > ea[i] + ((eb[0] * A[i][0] + eb[1] * A[i][1]) + eb[2] * A[i][2])) return false;
    for (int j = 0; j < 3; ++j)
        if (fabsf((t[0] * R[0][j] + t[1] * R[1][j]) + t[2] * R[2][j]) > ((ea[0] * A[0][j] + ea[1] * A[1][j]) + ea[2] * A[2][j]) + eb[j])
            return false;
    for (int i = 0; i < 3; ++i) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3;
        for (int j = 0; j < 3; ++j) {
            const int j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            if (fabsf(t[i2] * R[i1][j] - t[i1] * R[i2][j]) > (ea[i1] * A[i2][j] + ea[i2] * A[i1][j]) + (eb[j1] * A[i][j2] + eb[j2] * A[i][j1]))
                return false;
        }
    }
    return true;
}

// the squared distance of the segment p + t * d, t in [0, 1], to the box [lo, hi]: the minimum of point_cell_d2 over 34
// parameters -- 0, 1, the six slab crossings, the 26 stationary points of the pieces of the (C1, convex) distance
COL_HD float segment_cell_d2(const float* p, const float* d, const float* lo, const float* hi) {
    float best = 0.0f;
    for (int s = 0; s < 34; ++s) {
        float t;
        if (s == 0) t = 0.0f;
        else if (s == 1) t = 1.0f;
        else if (s < 8) {
            const int a = (s - 2) >> 1;
            const float b = ((s - 2) & 1) ? hi[a] : lo[a];
            t = (b - p[a]) / d[a];
        } else {
            const int code = s - 7;  // 1 .. 26: digits (axis 0, axis 1, axis 2) in base 3; 0 inactive, 1 lo, 2 hi
            const int c[3] = {code / 9, (code / 3) % 3, code % 3};
            float num = 0.0f, den = 0.0f;
            for (int a = 0; a < 3; ++a) {
                if (c[a] == 0) continue;
                const float b = c[a] == 1 ? lo[a] : hi[a];
                num = num + d[a] * (p[a] - b);
                den = den + d[a] * d[a];
            }
            t = -num / den;
        }
        t = finite(t) ? fmin2(fmax2(t, 0.0f), 1.0f) : 0.0f;
        const float q[3] = {p[0] + t * d[0], p[1] + t * d[1], p[2] + t * d[2]};
        const float d2 = point_cell_d2(q, lo, hi);
        if (s == 0 || d2 < best) best = d2;
    }
    return best;
}

COL_HD bool primitive_finite(const mi_icp_primitive& P) {
    bool ok = true;
    for (int k = 0; k < 16; ++k) ok = ok && finite(P.transform[k]);
    for (int k = 0; k < 3; ++k) ok = ok && finite(P.param[k]);
    return ok;
}

// how far a box primitive's rotation may be from orthonormal (max |rot^T rot - I|) and still collide: the conservative
// bounds below, which pick the candidate cells, hold for such rotations only
constexpr float kBoxOrthoTol = 1.0e-4f;

COL_HD bool box_rotation_ok(const float* T) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const float g = (T[i * 4] * T[j * 4] + T[i * 4 + 1] * T[j * 4 + 1]) + T[i * 4 + 2] * T[j * 4 + 2];
            if (!(fabsf(g - (i == j ? 1.0f : 0.0f)) <= kBoxOrthoTol)) return false;
        }
    return true;
}

// can this primitive collide at all?  Box, Sphere or Capsule, every field finite, a box's rotation orthonormal
COL_HD bool primitive_live(const mi_icp_primitive& P) {
    if (P.type != MI_ICP_PRIMITIVE_BOX && P.type != MI_ICP_PRIMITIVE_SPHERE && P.type != MI_ICP_PRIMITIVE_CAPSULE) return false;
    if (!primitive_finite(P)) return false;
    return P.type != MI_ICP_PRIMITIVE_BOX || box_rotation_ok(P.transform);
}

// a live primitive against the cell [lo, hi]
COL_HD bool primitive_cell(const mi_icp_primitive& P, const float* lo, const float* hi, float margin) {
    const float* T = P.transform;
    if (P.type == MI_ICP_PRIMITIVE_SPHERE) {
        const float rr = P.param[0] + margin;
        return point_cell_d2(T + 12, lo, hi) <= rr * rr;
    }
    if (P.type == MI_ICP_PRIMITIVE_CAPSULE) {
        const float rr = P.param[0] + margin, hh = 0.5f * P.param[1];
        const float p[3] = {T[12] - hh * T[8], T[13] - hh * T[9], T[14] - hh * T[10]};
        const float d[3] = {P.param[1] * T[8], P.param[1] * T[9], P.param[1] * T[10]};
        return segment_cell_d2(p, d, lo, hi) <= rr * rr;
    }
    float cc[3], eb[3], ea[3];
    for (int k = 0; k < 3; ++k) {
        cc[k] = (lo[k] + hi[k]) * 0.5f;
        eb[k] = (hi[k] - cc[k]) + margin;
        ea[k] = P.param[k] * 0.5f;
    }
    return box_cell(T, ea, cc, eb);
}

// GetAxisAlignedBoundingBox (collision/primitives.h): Box |rot| * (lengths / 2) about the translation; Sphere the radius;
// Capsule the end points +- radius; Cylinder the reference's formula with max in the max bound.  Other types: zeros.
COL_HD void primitive_aabb(const mi_icp_primitive& P, float* mn, float* mx) {
    const float* T = P.transform;
    for (int k = 0; k < 3; ++k) mn[k] = mx[k] = 0.0f;
    if (P.type == MI_ICP_PRIMITIVE_BOX) {
        for (int k = 0; k < 3; ++k) {
            const float h = (fabsf(T[k]) * (0.5f * P.param[0]) + fabsf(T[4 + k]) * (0.5f * P.param[1])) + fabsf(T[8 + k]) * (0.5f * P.param[2]);
            mn[k] = -fabsf(h) + T[12 + k];
            mx[k] = fabsf(h) + T[12 + k];
        }
    } else if (P.type == MI_ICP_PRIMITIVE_SPHERE) {
        for (int k = 0; k < 3; ++k) {
            mn[k] = -P.param[0] + T[12 + k];
            mx[k] = P.param[0] + T[12 + k];
        }
    } else if (P.type == MI_ICP_PRIMITIVE_CAPSULE) {
        for (int k = 0; k < 3; ++k) {
            const float pa = T[8 + k] * (0.5f * P.param[1]), pb = -pa;
            mn[k] = (fmin2(pa, pb) - P.param[0]) + T[12 + k];
            mx[k] = (fmax2(pa, pb) + P.param[0]) + T[12 + k];
        }
    } else if (P.type == MI_ICP_PRIMITIVE_CYLINDER) {
        float pa[3], a[3];
        for (int k = 0; k < 3; ++k) {
            pa[k] = T[8 + k] * (0.5f * P.param[1]);
            a[k] = -pa[k] - pa[k];
        }
        const float n2 = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2];
        for (int k = 0; k < 3; ++k) {
            const float e = P.param[0] * sqrtf(1.0f - a[k] * a[k] / n2);
            mn[k] = fmin2(pa[k] - e, -pa[k] - e) + T[12 + k];
            mx[k] = fmax2(pa[k] + e, -pa[k] + e) + T[12 + k];
        }
    }
}

// THE CANDIDATE CELLS.  An element (a segment, a primitive) reaches the cells whose box meets its bounds [blo, bhi],
// margin included, widened by slack(M) with M the largest magnitude among the bounds: every predicate above opens with
// axis tests that are a bounds overlap computed in fp32 through at most a dozen roundings of values no larger than
// M + the cell's own coordinates, that is below 2e-6 of them; the slack is 1e-5 of M plus 1e-30 (so that it is not
// zero at the origin), five times that.  A box primitive's bounds are further widened by 1 % for kBoxOrthoTol.
// The cells that meet [blo - s, bhi + s] are then found exactly: cell_hi(k) >= blo - s holds from some k on and
// cell_lo(k) <= bhi + s up to some k (both are monotone in k), and a binary search finds each end (cell_range below),
// so no slack is needed for the cells' own rounding.  Voxel queries need no slack at all: their predicate is this test.
// This covers an element's WHOLE bounds only.  What a segment can reach inside one x-slab is narrower and needs the
// further terms of segment_slab_cells below, because segment_cell's cross-axis tests are lenient by FLT_EPSILON.
COL_HD float slack(float M) { return 1.0e-5f * M + 1.0e-30f; }

// the keys k in [klo, khi] with cell_hi(k) >= a && cell_lo(k) <= b: [*k0, *k1], empty when *k0 > *k1
COL_HD void cell_range(float a, float b, float vs, float origin, int32_t klo, int32_t khi, int32_t* k0, int32_t* k1) {
    int64_t lo = klo, hi = (int64_t)khi + 1;  // the first k in [klo, khi + 1) with cell_hi(k) >= a
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (cell_hi((int32_t)mid, vs, origin) >= a) hi = mid;
        else lo = mid + 1;
    }
    *k0 = (int32_t)lo;
    lo = (int64_t)klo - 1;
    hi = khi;  // the last k in (klo - 1, khi] with cell_lo(k) <= b
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (cell_lo((int32_t)mid, vs, origin) <= b) lo = mid;
        else hi = mid - 1;
    }
    *k1 = (int32_t)lo;
}

// ---- a segment against the cells of a lattice (vs, origin[3]), one x-slab at a time
// segment_cells: the box of keys r0..r1 inside klo..khi that the segment's bounds, margin and slack s[a] included, meet --
// the three opening rejects of segment_cell are this overlap.  false: none (or an end point is not finite).
COL_HD bool segment_cells(const float* p0, const float* p1, float margin, float vs, const float* origin, const int32_t* klo,
                          const int32_t* khi, float* s, int32_t* r0, int32_t* r1) {
    for (int a = 0; a < 3; ++a) {
        if (!(finite(p0[a]) && finite(p1[a])) || klo[a] > khi[a]) return false;
        const float mn = fmin2(p0[a], p1[a]), mx = fmax2(p0[a], p1[a]);
        s[a] = slack(fmax2(fabsf(mn), fabsf(mx)) + margin);
        cell_range((mn - margin) - s[a], (mx + margin) + s[a], vs, origin[a], klo[a], khi[a], &r0[a], &r1[a]);
        if (r0[a] > r1[a]) return false;
    }
    return true;
}

// segment_slab_cells: the keys y0..y1, z0..z1 (k0[1..2], k1[1..2]; inside r0..r1) of the cells with key x that
// segment_cell can accept.  With t0..t1 the parameters at which the segment is inside the slab's x range (margin and
// s[0] included, widened by dt for the division's rounding), its y / z there span [min, max](p + t * d).  A cell the
// cross-axis tests (2,0) / (0,1) accept lies within that span widened by
//   margin + s[a]                               the inflated cell, and the rounding of mid and center (below 2e-6 * M)
//   w1 = FLT_EPSILON * (ext_0 + ext_a) / |dst_0| the tests add FLT_EPSILON to |dst|: the line may pass that far from the
//                                               cell; ext <= vs / 2 + margin and |dst_0| = |dx| / 2, so w1 <=
//                                               2 * FLT_EPSILON * (vs + 2 margin) / |dx|; twice that is taken
//   w2 = 3 * FLT_EPSILON * (|mid_a| + |mid_0| * |dst_a| / |dst_0|)   the roundings of the two products and their
//                                               difference, |mid| <= ext + |dst|: below 16 * FLT_EPSILON * ((vs + 2 margin)
//                                               * |d_a| / |dx| + |d_a| + vs + margin)
// (an error of mid_0 moves the line by that times |d_a| / |dx|, which s[0] in the slab's x range covers as it covers
// 2e-6 * M).  A segment whose |dx| is below 1e-5 of its |x| -- where dst_0 itself is rounding -- takes its whole y / z
// range; so does one for which a term above is not finite.  The result is cut to r0..r1, the segment's own bounds,
// which the opening rejects enforce whatever the cross-axis tests admit.
COL_HD bool segment_slab_cells(const float* p0, const float* p1, float margin, const float* s, float vs, const float* origin,
                               int32_t x, const int32_t* r0, const int32_t* r1, int32_t* k0, int32_t* k1) {
    const float dx = p1[0] - p0[0], adx = fabsf(dx);
    const float xa = (cell_lo(x, vs, origin[0]) - margin) - s[0], xb = (cell_hi(x, vs, origin[0]) + margin) + s[0];
    const float ta = (xa - p0[0]) / dx, tb = (xb - p0[0]) / dx;
    const float dt = 8.0f * FLT_EPSILON * ((fabsf(p0[0]) + fmax2(fabsf(xa), fabsf(xb))) + adx) / adx;
    float t0 = fmin2(ta, tb) - dt, t1 = fmax2(ta, tb) + dt;
    const bool whole = !(finite(t0) && finite(t1)) || !(adx > 1.0e-5f * (fabsf(p0[0]) + fabsf(p1[0])));
    t0 = whole ? 0.0f : fmin2(fmax2(t0, 0.0f), 1.0f);
    t1 = whole ? 1.0f : fmin2(fmax2(t1, 0.0f), 1.0f);
    k0[0] = k1[0] = x;
    for (int a = 1; a < 3; ++a) {
        const float d = p1[a] - p0[a], qa = p0[a] + t0 * d, qb = p0[a] + t1 * d, ad = fabsf(d);
        const float cell = vs + 2.0f * margin;
        float w = (4.0f * FLT_EPSILON * cell) / adx * (1.0f + 4.0f * ad) + 16.0f * FLT_EPSILON * (ad + cell);
        float blo = -INFINITY, bhi = INFINITY;
        if (!whole && finite(w) && finite(qa) && finite(qb)) {
            blo = ((fmin2(qa, qb) - margin) - s[a]) - w;
            bhi = ((fmax2(qa, qb) + margin) + s[a]) + w;
        }
        cell_range(blo, bhi, vs, origin[a], r0[a], r1[a], &k0[a], &k1[a]);
        if (k0[a] > k1[a]) return false;
    }
    return true;
}

// a live primitive's conservative bounds against cells of size vs, margin and slack included.  Sphere and capsule: the
// axis (a point, a segment) +- |radius + margin|.  Box: |rot| * half lengths + margin, and 1e-3 of the largest such half
// width, cell included, for a rotation that is orthonormal only within kBoxOrthoTol (the cell-axis tests then bound
// |dc_j| by the half widths + 3 * kBoxOrthoTol * max |dc|).
COL_HD void primitive_reach(const mi_icp_primitive& P, float margin, float vs, float* blo, float* bhi) {
    const float* T = P.transform;
    float h[3];
    if (P.type == MI_ICP_PRIMITIVE_BOX) {
        float hm = 0.0f;
        for (int k = 0; k < 3; ++k) {
            h[k] = (fabsf(T[k] * (0.5f * P.param[0])) + fabsf(T[4 + k] * (0.5f * P.param[1]))) + fabsf(T[8 + k] * (0.5f * P.param[2])) + fabsf(margin);
            hm = fmax2(hm, h[k]);
        }
        for (int k = 0; k < 3; ++k) h[k] = h[k] + 1.0e-3f * (hm + vs);
    } else {
        const float rr = fabsf(P.param[0] + margin);
        for (int k = 0; k < 3; ++k) h[k] = (P.type == MI_ICP_PRIMITIVE_CAPSULE ? fabsf(T[8 + k] * (0.5f * P.param[1])) : 0.0f) + rr;
    }
    for (int k = 0; k < 3; ++k) {
        const float c = T[12 + k], s = slack(fabsf(c) + h[k]);
        blo[k] = (c - h[k]) - s;
        bhi[k] = (c + h[k]) + s;
    }
}

}  // namespace col
}  // namespace mi
