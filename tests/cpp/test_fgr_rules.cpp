// Host-side check of csrc/fgr_rules.h, the rules FastGlobalRegistration's kernels share with the launcher: built with
// -fsanitize=address,undefined by tests/test_fgr_cpu.py and held against the decisions of the numpy restatement.
// stdin:  "B seed t ncorr"                       -> the three pair numbers of trial t
//         "A s2 p0 p1 p2 q0 q1 q2" (19 hex float bit patterns) -> 1 if the tuple test passes, else 0
//         "P par itr decrease_mu max_dist division_factor" (floats as hex bit patterns) -> the next par's bit pattern
//         "C passing maximum_tuple_count"        -> the cut list's length
#include "fgr_rules.h"

#include <cinttypes>
#include <cstdio>
#include <cstring>

static float from_bits(unsigned u) {
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}

static unsigned to_bits(float f) {
    unsigned u;
    std::memcpy(&u, &f, sizeof(u));
    return u;
}

int main() {
    char op;
    while (std::scanf(" %c", &op) == 1) {
        if (op == 'B') {
            uint64_t seed, t, ncorr;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64, &seed, &t, &ncorr) != 3) return 2;
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", mi::fgr::trial_pair(seed, t, 0, ncorr), mi::fgr::trial_pair(seed, t, 1, ncorr),
                        mi::fgr::trial_pair(seed, t, 2, ncorr));
        } else if (op == 'A') {
            unsigned w[19];
            for (int k = 0; k < 19; ++k)
                if (std::scanf("%x", &w[k]) != 1) return 2;
            float v[18];
            for (int k = 0; k < 18; ++k) v[k] = from_bits(w[k + 1]);
            std::printf("%d\n", mi::fgr::tuple_ok(v, v + 3, v + 6, v + 9, v + 12, v + 15, from_bits(w[0])) ? 1 : 0);
        } else if (op == 'P') {
            unsigned par, maxd, div;
            int itr, dec;
            if (std::scanf("%x %d %d %x %x", &par, &itr, &dec, &maxd, &div) != 5) return 2;
            std::printf("%08x\n", to_bits(mi::fgr::par_next(from_bits(par), itr, dec != 0, from_bits(maxd), from_bits(div))));
        } else if (op == 'C') {
            long long passing, maxc;
            if (std::scanf("%lld %lld", &passing, &maxc) != 2) return 2;
            std::printf("%lld\n", (long long)mi::fgr::cut_count(passing, maxc));
        } else {
            return 2;
        }
    }
    return 0;
}
