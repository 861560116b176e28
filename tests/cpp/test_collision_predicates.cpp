// The collision predicates of csrc/collision_predicates.h on the host, for tests/test_collision_cpu.py: reads cases from
// argv[1], writes per case eight floats to argv[2].  A case is 34 floats:
//   [0] kind (0 segment-cell, 1 primitive-cell, 2 bounding box + live, 3 cell_range, 4 the slab rule), [1] margin,
//   [2..4] lo, [5..7] hi, [8..10] p0, [11..13] p1, [14] primitive type, [15..30] transform (column-major), [31..33] param
// Kind 4 walks a segment through the lattice of origin lo, voxel size hi[0], keys -hi[1] .. hi[1] per axis as the line
// kernel does (segment_cells, then segment_slab_cells per x) and holds it against segment_cell on every cell of that
// lattice: out = accepted cells, accepted cells the walk did not visit, visited cells, cells of the segment's box.
// Built stand-alone (with the sanitizers) and run directly; it includes nothing but that header.
#include "collision_predicates.h"

#include <cstdio>
#include <vector>

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) return 3;
    std::vector<float> in;
    float buf[34];
    while (std::fread(buf, sizeof(float), 34, f) == 34) in.insert(in.end(), buf, buf + 34);
    std::fclose(f);
    const size_t n = in.size() / 34;
    std::vector<float> out(n * 8, 0.0f);
    for (size_t i = 0; i < n; ++i) {
        const float* c = &in[i * 34];
        float* o = &out[i * 8];
        const int kind = (int)c[0];
        const float margin = c[1];
        const float* lo = c + 2;
        const float* hi = c + 5;
        mi_icp_primitive P;
        P.type = (int32_t)c[14];
        for (int k = 0; k < 16; ++k) P.transform[k] = c[15 + k];
        for (int k = 0; k < 3; ++k) P.param[k] = c[31 + k];
        if (kind == 0) {
            const float ilo[3] = {lo[0] - margin, lo[1] - margin, lo[2] - margin}, ihi[3] = {hi[0] + margin, hi[1] + margin, hi[2] + margin};
            o[0] = mi::col::segment_cell(c + 8, c + 11, ilo, ihi) ? 1.0f : 0.0f;
        } else if (kind == 1) {
            o[0] = (mi::col::primitive_live(P) && mi::col::primitive_cell(P, lo, hi, margin)) ? 1.0f : 0.0f;
        } else if (kind == 2) {
            mi::col::primitive_aabb(P, o, o + 3);
            o[6] = mi::col::primitive_live(P) ? 1.0f : 0.0f;
        } else if (kind == 4) {
            const float vs = hi[0];
            const int32_t K = (int32_t)hi[1];
            const int32_t klo[3] = {-K, -K, -K}, khi[3] = {K, K, K};
            const float *p0 = c + 8, *p1 = c + 11;
            float s[3];
            int32_t r0[3], r1[3], k0[3], k1[3];
            const bool live = mi::col::segment_cells(p0, p1, margin, vs, lo, klo, khi, s, r0, r1);
            if (live) o[3] = ((float)(r1[0] - r0[0] + 1) * (float)(r1[1] - r0[1] + 1)) * (float)(r1[2] - r0[2] + 1);
            for (int32_t x = -K; x <= K; ++x) {
                const bool any = live && x >= r0[0] && x <= r1[0] && mi::col::segment_slab_cells(p0, p1, margin, s, vs, lo, x, r0, r1, k0, k1);
                if (any) o[2] += (float)(k1[1] - k0[1] + 1) * (float)(k1[2] - k0[2] + 1);
                for (int32_t y = -K; y <= K; ++y)
                    for (int32_t z = -K; z <= K; ++z) {
                        const int32_t k[3] = {x, y, z};
                        float ilo[3], ihi[3];
                        for (int a = 0; a < 3; ++a) {
                            ilo[a] = mi::col::cell_lo(k[a], vs, lo[a]) - margin;
                            ihi[a] = mi::col::cell_hi(k[a], vs, lo[a]) + margin;
                        }
                        if (!mi::col::segment_cell(p0, p1, ilo, ihi)) continue;
                        o[0] += 1.0f;
                        if (!(any && y >= k0[1] && y <= k1[1] && z >= k0[2] && z <= k1[2])) o[1] += 1.0f;
                    }
            }
        } else {  // the keys in [p0.x, p0.y] whose cells of size margin at origin p0.z meet [lo.x, hi.x]
            int32_t k0, k1;
            mi::col::cell_range(lo[0], hi[0], margin, c[10], (int32_t)c[8], (int32_t)c[9], &k0, &k1);
            o[0] = (float)k0;
            o[1] = (float)k1;
        }
    }
    f = std::fopen(argv[2], "wb");
    if (!f) return 4;
    std::fwrite(out.data(), sizeof(float), out.size(), f);
    std::fclose(f);
    std::puts("ok");
    return 0;
}
