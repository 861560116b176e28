// edt_envelope.h -- one line of a pass of the exact Euclidean distance transform (edt_kernels.h): the lower envelope of
// the parabolas F_j(i) = (i - j)^2 + g_j over the cells j of the line that have seen a site, then the sweep that gives
// every cell i its minimiser.  Integer arithmetic only, the products in 64 bits.  No HIP, no context: the same text runs
// in the pass kernels and in tests/cpp/test_edt_envelope.cpp, which includes nothing but this header.
//
// A Line says where the cells are:
//   In  load(j)                 the cell of the planes done so far;   bool none(In)   no site seen there
//   int64_t g(In)               its squared distance so far
//   void push(j, In, prev)      cell j enters the stack above cell prev (-1: it is the bottom): a NODE is written
//   Node node(j)                a node read back;   int64_t g(Node), int link(Node) (-1: the bottom)
//   void emit(i, j, Node)       cell i's nearest site is the one node j carries;   void emit_none(i)
// The stack is a linked list through the nodes (each cell is pushed at most once, so a node lives at its own cell).
// emit may overwrite what load read -- the sweep reads nodes only -- but not the nodes.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MI_EDT_HD __host__ __device__ __forceinline__
#else
#define MI_EDT_HD inline
#endif

namespace mi {

// a < b < c: is parabola b nowhere below both a and c?  With f = g + j^2, F_a <= F_b exactly for i <= s_ab =
// (f_b - f_a) / (2 (b - a)); b shows between s_ab and s_bc, so it is hidden iff s_ab >= s_bc, cross-multiplied.
// f reaches 3 * 1023^2 and the products 2.14e9 on a line of 1024: a hair inside int32 as written here, past it written
// almost any other way (the reference's form overflows from a resolution of about 710) -- hence 64 bits throughout.
MI_EDT_HD bool edt_hidden(int a, int64_t ga, int b, int64_t gb, int c, int64_t gc) {
    const int64_t fa = ga + (int64_t)a * a, fb = gb + (int64_t)b * b, fc = gc + (int64_t)c * c;
    return (fb - fa) * (int64_t)(c - b) >= (fc - fb) * (int64_t)(b - a);
}

MI_EDT_HD int64_t edt_at(int i, int j, int64_t gj) { return (int64_t)(i - j) * (i - j) + gj; }

// the envelope of the line's n cells as a stack of nodes; returns its top (-1: the line has seen no site)
template <class Line>
MI_EDT_HD int edt_build(Line& line, int n) {
    int t1 = -1, t2 = -1, t3 = -1;  // the top, the one below, and the one below that
    int64_t g1 = 0, g2 = 0;
    for (int j = 0; j < n; ++j) {
        const auto w = line.load(j);
        if (line.none(w)) continue;
        const int64_t g = line.g(w);
        while (t2 >= 0 && edt_hidden(t2, g2, t1, g1, j, g)) {
            t1 = t2;
            g1 = g2;
            t2 = t3;
            if (t2 >= 0) {
                const auto nd = line.node(t2);
                g2 = line.g(nd);
                t3 = line.link(nd);
            }
        }
        line.push(j, w, t1);
        t3 = t2;
        t2 = t1;
        g2 = g1;
        t1 = j;
        g1 = g;
    }
    return t1;
}

// every cell's minimiser, from the last cell down: the minimiser never moves up as i goes down, so the stack is popped
// while the node below is at least as good (a tie goes to the lower cell)
template <class Line>
MI_EDT_HD void edt_sweep(Line& line, int n, int top) {
    if (top < 0) {
        for (int i = 0; i < n; ++i) line.emit_none(i);
        return;
    }
    int t1 = top;
    auto n1 = line.node(t1);
    int64_t g1 = line.g(n1), g2 = 0;
    int t2 = line.link(n1);
    auto n2 = n1;
    if (t2 >= 0) {
        n2 = line.node(t2);
        g2 = line.g(n2);
    }
    for (int i = n - 1; i >= 0; --i) {
        while (t2 >= 0 && edt_at(i, t2, g2) <= edt_at(i, t1, g1)) {
            t1 = t2;
            n1 = n2;
            g1 = g2;
            t2 = line.link(n1);
            if (t2 >= 0) {
                n2 = line.node(t2);
                g2 = line.g(n2);
            }
        }
        line.emit(i, t1, n1);
    }
}

}  // namespace mi
