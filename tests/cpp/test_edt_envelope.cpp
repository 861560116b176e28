// The per-line routine of the distance transform (csrc/edt_envelope.h: build the lower envelope, sweep it) against an
// O(n^2) minimum.  Includes nothing but that header; built with AddressSanitizer and UBSan and run directly
// (tests/test_edt_cpu.py).  The cross-multiplication as written in the header peaks at (2 * 1023^2 + 1023^2 - 1022^2) *
// 1022 = 2 141 195 266 for the g a pass can meet, a hair inside int32 (other ways of writing it reach three times that),
// so the lines "past the passes' range" below go on to g = 2^33: with the test in `int` UBSan stops this program there.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "edt_envelope.h"

namespace {

struct Node {
    int64_t g;
    int link;
};

// a line over plain arrays: g < 0 means that the cell has seen no site
struct HostLine {
    const int64_t* gin;
    Node* nodes;
    int* out;  // the minimiser of every cell, -1: none
    int n;
    int pushes = 0;

    int64_t load(int j) const { return gin[j]; }
    bool none(int64_t w) const { return w < 0; }
    int64_t g(int64_t w) const { return w; }
    int64_t g(const Node& nd) const { return nd.g; }
    void push(int j, int64_t w, int prev) {
        if (j < 0 || j >= n || prev >= j) std::abort();
        nodes[j] = Node{w, prev};
        ++pushes;
    }
    Node node(int j) const {
        if (j < 0 || j >= n) std::abort();
        return nodes[j];
    }
    int link(const Node& nd) const { return nd.link; }
    void emit(int i, int j, const Node&) { out[i] = j; }
    void emit_none(int i) { out[i] = -1; }
};

int failures = 0;

void check_line(const std::vector<int64_t>& g, const char* what) {
    const int n = (int)g.size();
    std::vector<Node> nodes(n, Node{-7, -7});
    std::vector<int> out(n, -2);
    HostLine line{g.data(), nodes.data(), out.data(), n};
    const int top = mi::edt_build(line, n);
    mi::edt_sweep(line, n, top);
    for (int i = 0; i < n; ++i) {
        int64_t best = -1;
        for (int j = 0; j < n; ++j) {
            if (g[j] < 0) continue;
            const int64_t f = (int64_t)(i - j) * (i - j) + g[j];
            if (best < 0 || f < best) best = f;
        }
        const int j = out[i];
        bool ok;
        if (best < 0) {
            ok = j == -1;
        } else {
            ok = j >= 0 && j < n && g[j] >= 0 && (int64_t)(i - j) * (i - j) + g[j] == best;
        }
        if (!ok) {
            if (failures < 10) std::printf("FAIL %s n=%d cell %d: minimiser %d, minimum %lld\n", what, n, i, j, (long long)best);
            ++failures;
            return;
        }
    }
}

uint64_t rng_state = 0x9e3779b97f4a7c15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

}  // namespace

int main() {
    const int sizes[] = {2, 3, 64, 65, 1023, 1024};
    const int64_t gmax = 2ll * 1023 * 1023;
    for (int n : sizes) {
        std::vector<int64_t> g(n);
        // random g: every cell, half of them, a few; small values and the whole range
        for (int rep = 0; rep < 12; ++rep) {
            const int64_t range = (rep & 1) ? gmax + 1 : 50;
            const int keep = rep % 3;  // 0: all, 1: every second at random, 2: one in sixteen
            for (int j = 0; j < n; ++j) {
                const bool site = keep == 0 || (keep == 1 ? (rnd() & 1) : (rnd() & 15) == 0);
                g[j] = site ? (int64_t)(rnd() % (uint64_t)range) : -1;
            }
            check_line(g, "random");
        }
        // all none
        for (int j = 0; j < n; ++j) g[j] = -1;
        check_line(g, "all none");
        // one site, at each end and in the middle, near and far
        for (int at : {0, n / 2, n - 1}) {
            for (int64_t v : {(int64_t)0, gmax}) {
                for (int j = 0; j < n; ++j) g[j] = -1;
                g[at] = v;
                check_line(g, "one site");
            }
        }
        // every cell a site: g = 0 everywhere, then the largest value everywhere
        for (int64_t v : {(int64_t)0, gmax}) {
            for (int j = 0; j < n; ++j) g[j] = v;
            check_line(g, "every cell");
        }
        // the extremes of the cross-multiplication: the largest g next to 0, in both orders and alternating
        for (int j = 0; j < n; ++j) g[j] = (j & 1) ? gmax : 0;
        check_line(g, "alternating");
        for (int j = 0; j < n; ++j) g[j] = (j & 1) ? 0 : gmax;
        check_line(g, "alternating'");
        for (int j = 0; j < n; ++j) g[j] = gmax;
        g[n - 1] = 0;
        check_line(g, "far then near");
        g[n - 1] = gmax;
        g[0] = 0;
        check_line(g, "near then far");
        // sites only at both ends, near and far
        for (int j = 0; j < n; ++j) g[j] = -1;
        g[0] = 0;
        g[n - 1] = gmax;
        check_line(g, "both ends");
        g[0] = gmax;
        g[n - 1] = gmax;
        check_line(g, "both ends far");
        g[0] = gmax;
        g[n - 1] = 0;
        check_line(g, "both ends'");
        // a parabola-shaped g (every site stays on the envelope) and its negative (only the ends do)
        for (int j = 0; j < n; ++j) g[j] = (int64_t)j * j % (gmax + 1);
        check_line(g, "convex");
        for (int j = 0; j < n; ++j) g[j] = gmax - (int64_t)j * (n - j);
        check_line(g, "concave");
    }
    // past the passes' range: the routine is exact for any g that leaves the products inside 64 bits
    for (int n : sizes) {
        std::vector<int64_t> g(n);
        const int64_t big = 1ll << 33;
        for (int j = 0; j < n; ++j) g[j] = (j & 1) ? big : 0;
        check_line(g, "alternating 2^33");
        for (int j = 0; j < n; ++j) g[j] = big - (int64_t)j * 4099;
        check_line(g, "falling from 2^33");
        for (int j = 0; j < n; ++j) g[j] = (rnd() & 3) ? -1 : (int64_t)(rnd() % (uint64_t)big);
        check_line(g, "random below 2^33");
    }
    // the dominance test at its largest operands
    if (!mi::edt_hidden(0, 0, 1, gmax, 1023, 0) || mi::edt_hidden(0, gmax, 1, 0, 1023, gmax)) {
        std::printf("FAIL edt_hidden at the extremes\n");
        ++failures;
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
