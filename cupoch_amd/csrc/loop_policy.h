// loop_policy.h -- the host's policy for the device-resident registration loop: the chunks, the halo decision, the
// re-location arming, the form of a search launch.  State and rules only -- no HIP, no context, no environment: the callers
// hand in plain values.  tests/cpp/test_loop_policy.cpp pins every rule; the measurements: DESIGN.md 4.1, 4.3, EXPERIMENTS.md.
#pragma once
#include <algorithm>
#include <cstdint>

namespace mi::eng {

// a call's chunks grow 8, 16, 32, 32 ...: a look at the loop is ~30 us, two iterations of a 100k-point loop; one enqueued past the end ~3 us
constexpr int kChunkStart = 8, kChunkCap = 32;
// large sources: a stale seed's climb, or a walk for want of a halo, costs a 10M-point search milliseconds, a 100k-point one less than a synchronisation
constexpr int64_t kLarge = 500000;
// "many" lanes ask for a halo: more than 1/32 (~3 %) of them per iteration; "most": more than 2/5
constexpr int64_t kHaloManyOneIn = 32, kHaloMostNum = 2, kHaloMostDen = 5;
// a declined loop looks at the 4-KB counter every eighth chunk: the copy is ~1 us per iteration of an 8-way shard's 36-us step
constexpr uint32_t kHaloDeclinedLookEvery = 8;
// a background build (2.2 ms, 1.6 GB at 10M points) saves a clean loop 2-3 us per iteration: from 1 % of the lanes asking after 40, anybody after 1000
constexpr int64_t kHaloLongRun = 40, kHaloVeryLongRun = 1000, kHaloBackgroundPercent = 1;
// ... and twice what the halos and their build's scratch take (~128 + ~56 bytes per slot) free on the device
constexpr int64_t kHaloBytesPerSlot = 368;
// smaller targets get their halos behind the tree on a context whose loops have asked; a larger build would fight the staging of the source
constexpr int64_t kHaloAheadMax = 2000000;
// live[] (loop.h) samples one packet in 2^shift, 64 at most; the gate costs a search that skips nothing 3-12 %, a quarter skipped saves a quarter
constexpr int64_t kSkipSamples = 64, kSkipPaysOneIn = 4;

// Every rank enqueues alike -- by the budget alone; single_iteration: one rank only: an RCCL all-reduce is a host-side call per evaluation
struct ChunkSchedule {
    int chunk = kChunkStart;
    // evaluations to enqueue now (a short remainder rides along: one host synchronisation less than it would cost)
    int plan(int budget, bool single_iteration) const { return single_iteration ? 1 : (budget <= chunk + chunk / 2) ? budget : chunk; }
    void ran(int n) { chunk = (n == chunk) ? std::min(chunk * 2, kChunkCap) : chunk; }  // only a whole regular chunk grows the next
};

enum class HaloAction { Nothing, Declined, BuildAndWait, BuildInBackgroundIfMemory };
// Halos are built when a loop's searches ask (nn_search.h counts the lanes one would serve); the rules: DESIGN.md 4.3's table.
struct HaloPolicy {
    bool sticky = false, ran_loop = false;  // a loop of this context has asked: the next one builds with the loop; it has registered before
    bool declined = false;                  // this loop's searches have been looked at and did not ask ...
    int looks = 0;                          // ... after so many looks while undecided
    int64_t iters = 0, asked = 0, lanes = 0;  // seeded iterations against this target, the lanes that asked in them, out of so many looked at
    int64_t iters_unseen = 0;               // iterations since the counter was last looked at
    uint32_t chunks = 0, want_seen = 0;     // chunks of a declined loop; the counter's sum at the last look (zeroed when a loop begins)
    void on_new_target() { iters = asked = lanes = 0; }
    void on_loop_begin() { declined = false, ran_loop = true, want_seen = 0, looks = 0, iters_unseen = 0, chunks = 0; }
    bool start_ahead(int64_t n_target, bool links_allowed) const { return ran_loop && sticky && links_allowed && n_target < kHaloAheadMax; }
    static bool single_iteration(bool undecided, int64_t ns, bool several_ranks) { return undecided && ns >= kLarge && !several_ranks; }
    // is the counter copied back behind this chunk?  no_halo: the target has none, none are on the way, it may have them
    bool wants_look(bool no_halo) { return no_halo && (!declined || (++chunks % kHaloDeclinedLookEvery) == 0); }
    void account(int executed) { iters += executed, iters_unseen += executed; }  // every chunk
    // every look: the counter's words sum to `counter_sum`, 32 bits that keep counting: differenced modulo 2^32, a wrap costs nothing
    HaloAction observe(uint32_t counter_sum, int executed, int64_t ns, bool undecided) {
        const int64_t now = (int64_t)(uint32_t)(counter_sum - want_seen);  // asked by the iterations since the last look
        want_seen = counter_sum;
        asked += now;
        lanes += ns * std::max<int64_t>(iters_unseen, 0);
        iters_unseen = 0;
        if (undecided) {  // (a registration's first seeded iteration is still displaced and asks whatever the data: hence the second look)
            ++looks;
            const int64_t per = std::max(executed, 1);
            const bool many = now * kHaloManyOneIn > ns * per, most = now * kHaloMostDen > kHaloMostNum * ns * per;
            if (!many) declined = true;
            else if (most || looks >= 2 || ns < kLarge) sticky = true;
            else return HaloAction::Nothing;
            return many ? HaloAction::BuildAndWait : HaloAction::Declined;
        }
        // (in the background: `declined` stays, nothing waits; the caller asks for the free memory only now)
        const bool earned = (iters >= kHaloLongRun && asked * 100 >= lanes * kHaloBackgroundPercent) || (iters >= kHaloVeryLongRun && asked > 0);
        return earned ? HaloAction::BuildInBackgroundIfMemory : HaloAction::Nothing;
    }
    static int64_t bytes_needed(int64_t target_slots) { return target_slots * kHaloBytesPerSlot; }
};

// RE-LOCATION (loop.h): a gated launch ahead of a seeded search replaces every seed once a step moved the source by about a leaf's width
struct Relocation {
    bool armed = false, possible = false;  // the next chunk carries the gated launches; the step sizes its displacement (loop_begin): they may be armed again
    void on_loop_begin(bool can_locate) { armed = possible = can_locate; }
    // carried: the chunk's iterations carried the launches (armed, and the halos were there); relocated: one was needed
    void after_chunk(bool carried, bool relocated, int64_t ns) {
        if (carried && !relocated) armed = false;  // the steps have become small, and they only shrink
        // ... or grow again (point-to-plane sliding, an escape from a plateau): the step sizes itself with or without the launches
        else if (!armed && possible && ns >= kLarge && relocated) armed = true;
    }
};

inline uint32_t skip_live_shift(int64_t ns) {
    uint32_t shift = 0;
    while ((((ns + 63) / 64) >> (shift + 1)) >= kSkipSamples) ++shift;
    return shift;
}
// Does gating the loop's next seeded search pay?  By live[] as of the host's last look at the loop state.
inline bool skip_pays(const uint8_t* live, int64_t ns) {
    if (!live || ns <= 0) return false;
    const int64_t samples = std::min<int64_t>(kSkipSamples, ((ns + 63) / 64) >> skip_live_shift(ns));
    int64_t held = 0;
    for (int64_t k = 0; k < samples; ++k) held += live[k] ? 1 : 0;
    return samples > 0 && held * kSkipPaysOneIn >= samples;
}

// The form a search launch takes (launch_nn).  seed, nn_valid: seeds wanted, matches there to seed from; stats: counters
// wanted; has_expiry, expiry_live, skip_r2: the per-packet limits' array exists, may hold limits, measured at this squared radius
struct SearchPlan {
    bool use_seed, self_seeded, limits, may_skip;
    uint32_t run;  // packets per workgroup: skip_run for the gated launch (may_skip, and it pays), else 1
    int kind;      // mi_icp_debug_last_search_kind: 0 from the root, 1 from the previous matches, 2 from its own seeds
};
inline SearchPlan plan_search(bool in_loop, bool seed, bool nn_valid, bool stats, int64_t ns, int64_t coarse_min, bool halos, bool planes,
                              bool has_expiry, bool expiry_live, float skip_r2, float r2, const uint8_t* live, uint32_t skip_run) {
    SearchPlan p;
    p.use_seed = seed && nn_valid;
    // no previous matches, but the halos are there: a large source's queries take the leaf they fall into as seed (without halos
    // most packets would walk up from it: 10M points 3.9 against 1.2 ms from the root)
    p.self_seeded = !p.use_seed && !stats && ns >= coarse_min && halos && planes;
    // THE SKIP (nn_search.h): a seeded search of the loop leaves a limit per packet and may skip by those on record from such a
    // search at this radius; every other search rewrites matches the limits know nothing of: the caller drops them first
    p.limits = in_loop && (p.use_seed || p.self_seeded) && !stats && has_expiry;
    p.may_skip = p.limits && p.use_seed && expiry_live && skip_r2 == r2;
    p.run = (p.may_skip && skip_pays(live, ns)) ? skip_run : 1u;
    p.kind = p.use_seed ? 1 : (p.self_seeded ? 2 : 0);
    return p;
}

}  // namespace mi::eng
