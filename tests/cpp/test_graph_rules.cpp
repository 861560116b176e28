// Host-side check of csrc/graph_rules.h, the rules the graph kernels share with the launcher: built with
// -fsanitize=address,undefined by tests/test_graph_cpu.py and held against vectors the numpy restatement writes.
// stdin:  "L rx ry rz"        -> the edge count, then the first edge of every node in node order
//         "T du dv w" (hex bit patterns of three floats) -> tier1 tier2 (0 / 1) with sum = (float)(du + w)
#include "graph_rules.h"

#include <cstdio>
#include <cstring>

static float from_bits(unsigned u) {
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

int main() {
    char op;
    while (std::scanf(" %c", &op) == 1) {
        if (op == 'L') {
            long long rx, ry, rz;
            if (std::scanf("%lld %lld %lld", &rx, &ry, &rz) != 3) return 2;
            std::printf("%lld", (long long)mi::graph::lattice_edge_count(rx, ry, rz));
            for (long long x = 0; x < rx; ++x)
                for (long long y = 0; y < ry; ++y)
                    for (long long z = 0; z < rz; ++z) std::printf(" %lld", (long long)mi::graph::lattice_edge_offset(x, y, z, rx, ry, rz));
            std::printf("\n");
        } else if (op == 'T') {
            unsigned a, b, c;
            if (std::scanf("%x %x %x", &a, &b, &c) != 3) return 2;
            const float du = from_bits(a), dv = from_bits(b), w = from_bits(c);
            const float sum = du + w;
            std::printf("%d %d\n", mi::graph::tier1_ok(du, dv, sum) ? 1 : 0, mi::graph::tier2_ok(du, dv, sum) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
