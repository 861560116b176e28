// The registration loop's host policy (cupoch_amd/csrc/loop_policy.h), rule by rule, on the CPU: the chunk schedule, the
// halo decision, the re-location arming, the search skip's gate and the form a search launch takes.  The expectations
// are those of the code before the rules moved into the header.  Prints "ok"; exits non-zero at the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "loop_policy.h"

using namespace mi::eng;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

// the chunks of a call with `budget`; the first `singles` of them are asked to be single iterations
static std::vector<int> chunks_of(int budget, int singles = 0) {
    ChunkSchedule s;
    std::vector<int> out;
    while (budget > 0) {
        const int n = s.plan(budget, (int)out.size() < singles);
        CHECK(n >= 1 && n <= budget);
        out.push_back(n);
        budget -= n;
        s.ran(n);
    }
    return out;
}

static void test_chunks() {
    CHECK(kChunkStart == 8 && kChunkCap == 32);
    CHECK(chunks_of(12) == std::vector<int>({12}));
    CHECK(chunks_of(13) == std::vector<int>({8, 5}));
    CHECK(chunks_of(30) == std::vector<int>({8, 22}));
    CHECK(chunks_of(100) == std::vector<int>({8, 16, 32, 44}));
    const std::vector<int> c = chunks_of(1000);
    CHECK(c[0] == 8 && c[1] == 16);
    int sum = 24;
    for (size_t i = 2; i + 1 < c.size(); ++i) {
        CHECK(c[i] == 32);
        sum += 32;
    }
    CHECK(c.back() <= 48 && c.back() > 16 && sum + c.back() == 1000);
    CHECK(chunks_of(30, 2) == std::vector<int>({1, 1, 8, 20}));  // (the single chunks do not grow the size)
    // a remainder that rides along does not grow the size either: 8 + 4 asked of a schedule at 8 leaves it at 8
    ChunkSchedule s;
    CHECK(s.plan(12, false) == 12);
    s.ran(12);
    CHECK(s.chunk == 8);
}

// one look of an undecided loop: `executed` iterations, `asked` lanes of `ns`
static HaloAction look(HaloPolicy& h, uint32_t& counter, int64_t asked, int executed, int64_t ns) {
    CHECK(h.wants_look(true));
    h.account(executed);
    counter += (uint32_t)asked;
    return h.observe(counter, executed, ns, !h.declined);
}

static void test_halo_undecided() {
    CHECK(kLarge == 500000);
    for (int executed : {1, 8}) {
        const int64_t ns = 1000000, e = executed;
        for (int at = 1; at <= 2; ++at) {  // the 1/32 test is strict, at any look
            HaloPolicy h;
            h.on_loop_begin();
            uint32_t counter = 0;
            if (at == 2) CHECK(look(h, counter, 31251 * e, executed, ns) == HaloAction::Nothing);
            CHECK(look(h, counter, 31250 * e, executed, ns) == HaloAction::Declined);
            CHECK(h.declined && !h.sticky);
        }
        {
            HaloPolicy h;
            h.on_loop_begin();
            uint32_t counter = 0;
            CHECK(look(h, counter, 31251 * e, executed, ns) == HaloAction::Nothing);
            CHECK(!h.declined && !h.sticky && h.looks == 1);  // still undecided
            CHECK(look(h, counter, 31251 * e, executed, ns) == HaloAction::BuildAndWait);
            CHECK(h.sticky && !h.declined && h.looks == 2);
        }
        {
            HaloPolicy h;
            h.on_loop_begin();
            uint32_t counter = 0;
            CHECK(look(h, counter, 400000 * e, executed, ns) == HaloAction::Nothing);
            CHECK(!h.sticky);
        }
        {
            HaloPolicy h;
            h.on_loop_begin();
            uint32_t counter = 0;
            CHECK(look(h, counter, 400000 * e + 1, executed, ns) == HaloAction::BuildAndWait);
            CHECK(h.sticky);
        }
    }
    {   // executed 0 (the loop was done before the chunk) counts as one iteration
        HaloPolicy h;
        h.on_loop_begin();
        uint32_t counter = 0;
        CHECK(look(h, counter, 400001, 0, 1000000) == HaloAction::BuildAndWait);
    }
    for (int64_t asked : {3126, 3125}) {  // a small source decides at its first look
        HaloPolicy h;
        h.on_loop_begin();
        uint32_t counter = 0;
        CHECK(look(h, counter, asked, 1, 100000) == (asked == 3126 ? HaloAction::BuildAndWait : HaloAction::Declined));
        CHECK(h.sticky == (asked == 3126) && h.declined == (asked == 3125));
    }
    // who runs single-iteration chunks
    CHECK(HaloPolicy::single_iteration(true, 500000, false));
    CHECK(!HaloPolicy::single_iteration(true, 499999, false));
    CHECK(!HaloPolicy::single_iteration(false, 500000, false));
    CHECK(!HaloPolicy::single_iteration(true, 500000, true));
}

static void test_halo_declined() {
    CHECK(kHaloLongRun == 40 && kHaloVeryLongRun == 1000);
    {   // the look at every eighth chunk only, lanes at looks only, iters at every chunk
        const int64_t ns = 1000;
        HaloPolicy h;
        h.on_loop_begin();
        h.declined = true;
        CHECK(!h.wants_look(false) && h.chunks == 0);  // (halos there or on their way: no count, no look)
        for (int chunk = 1; chunk <= 24; ++chunk) {
            const bool l = h.wants_look(true);
            CHECK(l == (chunk % 8 == 0));
            h.account(2);
            CHECK(h.iters == 2 * chunk);
            if (l) CHECK(h.observe(0u, 2, ns, false) == HaloAction::Nothing);
            CHECK(h.lanes == ns * 16 * (chunk / 8));
            CHECK(h.iters_unseen == 2 * (chunk % 8));
        }
        CHECK(h.declined && h.asked == 0);
    }
    // the two background rules, over iters x asked; lanes = 1000 per iteration
    const int64_t ns = 1000;
    for (int64_t iters : {1, 39, 40, 41, 999, 1000, 1001}) {
        for (int64_t asked : {(int64_t)0, (int64_t)1, iters * 10 - 1, iters * 10, iters * 1000}) {
            if (asked < 0) continue;
            HaloPolicy h;
            h.on_loop_begin();
            h.declined = true;
            h.account((int)iters);
            const HaloAction a = h.observe((uint32_t)asked, 8, ns, false);
            CHECK(h.iters == iters && h.asked == asked && h.lanes == ns * iters);
            const bool want = (iters >= 40 && asked * 100 >= ns * iters) || (iters >= 1000 && asked > 0);
            CHECK(a == (want ? HaloAction::BuildInBackgroundIfMemory : HaloAction::Nothing));
            CHECK(h.declined && !h.sticky);  // (in the background: the loop stays declined, the context does not turn sticky)
        }
    }
    {   // 39 iterations with every lane asking: nothing; 1000 with nobody asking: nothing
        HaloPolicy h;
        h.declined = true;
        h.account(39);
        CHECK(h.observe(39000u, 8, ns, false) == HaloAction::Nothing);
        HaloPolicy g;
        g.declined = true;
        g.account(1000);
        CHECK(g.observe(0u, 8, ns, false) == HaloAction::Nothing);
    }
    CHECK(HaloPolicy::bytes_needed(1000) == 368000);
    CHECK(HaloPolicy::bytes_needed(20000000) == 7360000000ll);  // (past 2^32)
}

static void test_halo_counter_and_resets() {
    {   // the counter wraps between two looks
        HaloPolicy h;
        h.on_loop_begin();
        h.declined = true;
        h.account(1);
        (void)h.observe(0xFFFFFF00u, 1, 1000, false);
        const int64_t before = h.asked;
        CHECK(before == 0xFFFFFF00ll);
        h.account(1);
        (void)h.observe(0x00000010u, 1, 1000, false);
        CHECK(h.asked - before == 0x110);
    }
    HaloPolicy h;
    h.sticky = h.ran_loop = h.declined = true;
    h.iters = 5, h.asked = 6, h.lanes = 7, h.iters_unseen = 8, h.chunks = 9, h.want_seen = 10, h.looks = 11;
    h.on_new_target();
    CHECK(h.iters == 0 && h.asked == 0 && h.lanes == 0);
    CHECK(h.sticky && h.ran_loop && h.declined && h.iters_unseen == 8 && h.chunks == 9 && h.want_seen == 10 && h.looks == 11);
    h.iters = 5, h.asked = 6, h.lanes = 7, h.ran_loop = false;
    h.on_loop_begin();
    CHECK(!h.declined && h.looks == 0 && h.want_seen == 0 && h.iters_unseen == 0 && h.chunks == 0 && h.ran_loop);
    CHECK(h.sticky && h.iters == 5 && h.asked == 6 && h.lanes == 7);
    // start_ahead: all of ran_loop, sticky, links allowed, and a target below kHaloAheadMax
    CHECK(kHaloAheadMax == 2000000);
    for (int m = 0; m < 16; ++m) {
        HaloPolicy s;
        s.ran_loop = m & 1, s.sticky = m & 2;
        const bool allowed = m & 4, small = m & 8;
        CHECK(s.start_ahead(small ? kHaloAheadMax - 1 : kHaloAheadMax, allowed) == (m == 15));
    }
}

static void test_relocation() {
    Relocation r;
    CHECK(!r.armed && !r.possible);
    r.on_loop_begin(true);
    CHECK(r.armed && r.possible);
    r.after_chunk(true, true, 500000);  // carried, and one was needed: stays armed
    CHECK(r.armed);
    r.after_chunk(false, false, 500000);  // armed but not carried (no halos): unchanged
    CHECK(r.armed);
    r.after_chunk(false, true, 500000);
    CHECK(r.armed);
    r.after_chunk(true, false, 500000);  // carried and never needed: disarmed
    CHECK(!r.armed && r.possible);
    r.after_chunk(false, false, 500000);  // no re-location counted: stays disarmed
    CHECK(!r.armed);
    r.after_chunk(false, true, 499999);  // not a large source
    CHECK(!r.armed);
    r.after_chunk(false, true, 500000);  // a large source whose step grew again
    CHECK(r.armed);
    r.on_loop_begin(false);
    CHECK(!r.armed && !r.possible);
    r.after_chunk(false, true, 500000);  // the step does not size itself: never armed
    CHECK(!r.armed);
}

static void test_skip() {
    CHECK(skip_live_shift(0) == 0 && skip_live_shift(1) == 0);
    CHECK(skip_live_shift(64 * 127) == 0);
    CHECK(skip_live_shift(64 * 127 + 1) == 1);  // (128 packets)
    CHECK(skip_live_shift(64 * 128) == 1);
    CHECK(skip_live_shift(64 * 255) == 1 && skip_live_shift(64 * 256) == 2);
    CHECK(skip_live_shift(10000000) == 11);  // 156250 packets: 76 samples at shift 11
    uint8_t live[64] = {};
    for (int k = 0; k < 15; ++k) live[4 * k] = 1;
    CHECK(!skip_pays(live, 64 * 64));  // 15 of 64 held
    live[63] = 1;
    CHECK(skip_pays(live, 64 * 64));  // 16 of 64
    CHECK(skip_pays(live, 10000000));
    CHECK(!skip_pays(live, 0) && !skip_pays(live, -1) && !skip_pays(nullptr, 64 * 64));
    // a small source has min(64, packets >> shift) samples: only the first of them count
    uint8_t few[64] = {};
    few[0] = 1;
    CHECK(skip_pays(few, 4 * 64));       // 1 of 4
    CHECK(skip_pays(few, 3 * 64 + 1));   // 4 packets, the last one short
    CHECK(!skip_pays(few, 5 * 64));      // 1 of 5
    few[0] = 0, few[4] = 1;
    CHECK(!skip_pays(few, 4 * 64));      // (the fifth sample is not one of a 4-packet source's)
    CHECK(skip_pays(few, 1) == false);
    uint8_t one[64] = {1};
    CHECK(skip_pays(one, 1));
}

static void test_plan_search() {
    const uint32_t kRun = 8;
    uint8_t all[64], none[64] = {};
    for (uint8_t& v : all) v = 1;
    for (int m = 0; m < (1 << 11); ++m) {
        const bool in_loop = m & 1, seed = m & 2, nn_valid = m & 4, stats = m & 8, halos = m & 16, planes = m & 32,
                   large = m & 64, has_expiry = m & 128, expiry_live = m & 256, same_r2 = m & 512, pays = m & 1024;
        const SearchPlan p = plan_search(in_loop, seed, nn_valid, stats, large ? 65536 : 65535, 65536, halos, planes, has_expiry,
                                         expiry_live, same_r2 ? 0.25f : 0.5f, 0.25f, pays ? all : none, kRun);
        // the expressions of launch_nn before the move
        const bool use_seed = seed && nn_valid;
        const bool self_seeded = !use_seed && !stats && large && halos && planes;
        const bool limits = in_loop && (use_seed || self_seeded) && !stats && has_expiry;
        const bool may_skip = limits && use_seed && expiry_live && same_r2;
        const uint32_t run = (may_skip && pays) ? kRun : 1u;
        CHECK(p.use_seed == use_seed && p.self_seeded == self_seeded && p.limits == limits && p.may_skip == may_skip);
        CHECK(p.run == run);
        CHECK(p.kind == (use_seed ? 1 : (self_seeded ? 2 : 0)));
        // ... and what they amount to
        if (stats) CHECK(!p.self_seeded && !p.limits && !p.may_skip && p.run == 1u);
        if (p.may_skip) CHECK(in_loop && p.use_seed && has_expiry && expiry_live && same_r2);
        CHECK((p.run == kRun) == (p.may_skip && pays));
        CHECK(!(p.use_seed && p.self_seeded));
        CHECK(p.kind == 0 || p.kind == 1 || p.kind == 2);
    }
    // no radius on record (NaN) never equals this search's; live[] is never read unless may_skip holds, and without a
    // sample the gate does not pay
    const auto in_loop_seeded = [&](float skip_r2, const uint8_t* live) {
        return plan_search(true, true, true, false, 100000, 65536, false, false, true, true, skip_r2, 0.25f, live, kRun);
    };
    SearchPlan p = in_loop_seeded(__builtin_nanf(""), all);
    CHECK(p.limits && !p.may_skip && p.run == 1u);
    p = in_loop_seeded(0.25f, all);
    CHECK(p.may_skip && p.run == kRun);
    p = in_loop_seeded(0.25f, nullptr);
    CHECK(p.may_skip && p.run == 1u);
    p = plan_search(false, false, true, false, 100000, 65536, true, true, true, true, 0.25f, 0.25f, nullptr, kRun);
    CHECK(p.kind == 2 && !p.limits && p.run == 1u);  // (a one-shot search from its own seeds keeps no limits)
}

int main() {
    test_chunks();
    test_halo_undecided();
    test_halo_declined();
    test_halo_counter_and_resets();
    test_relocation();
    test_skip();
    test_plan_search();
    std::printf("ok\n");
    return 0;
}
