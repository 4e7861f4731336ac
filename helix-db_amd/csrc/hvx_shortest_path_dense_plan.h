// hvx_shortest_path_dense_plan.h -- the round plan of hvx_shortest_path_batch_dense (hvx_shortest_path_dense.hip): host arithmetic only.
// The b requests of a batch are cut into groups of 64 (one bit of a u64 word each).  Per group and node the scratch holds three u64 words
// (seen, cur, next) and 64 level bytes = 88 bytes; the groups run in rounds of as many as the budget holds, and a budget that does not hold
// one group is refused.  Every product is 64-bit: n x 64 x groups passes 2^32 at n = 2^20 with 64 groups.  No HIP in here:
// tests/native/sp_dense_plan_probe.cpp compiles this header alone.
#pragma once
#include <cstdint>

namespace hvx_spd {

constexpr uint32_t kGroup = 64;                          // requests per group: the bits of a word
constexpr uint64_t kNodeGroupBytes = 3 * 8 + kGroup;     // seen, cur, next + one level byte per request
constexpr uint64_t kDefaultScratch = 1ull << 30;         // scratch_bytes == 0

// Scratch of one round of G groups, from its start: seen [G][n] u64 | cur [G][n] u64 | next [G][n] u64 | lvl [G][n][64] u8
struct RoundPlan {
    uint64_t groups;            // ceil(b / 64)
    uint64_t groups_per_round;  // min(groups, budget / (n x 88)), at least 1
    uint64_t rounds;            // ceil(groups / groups_per_round)
    uint64_t words;             // u64 words of each of the three word arrays = n x groups_per_round
    uint64_t seen_off, cur_off, next_off, lvl_off; // byte offsets
    uint64_t bytes;             // n x 88 x groups_per_round
};

// false: the budget does not hold one group (nothing is written).  b >= 1; n < 2^32, so n x 88 x 1 024 groups stays below 2^49.
inline bool plan_rounds(uint64_t n, uint32_t b, uint64_t scratch_bytes, RoundPlan *p) {
    const uint64_t budget = scratch_bytes ? scratch_bytes : kDefaultScratch;
    const uint64_t group_bytes = (n ? n : 1) * kNodeGroupBytes;
    const uint64_t fit = budget / group_bytes;
    if (fit == 0) return false;
    p->groups = ((uint64_t)b + kGroup - 1) / kGroup;
    p->groups_per_round = fit < p->groups ? fit : p->groups;
    if (p->groups_per_round == 0) p->groups_per_round = 1;
    p->rounds = (p->groups + p->groups_per_round - 1) / p->groups_per_round;
    p->words = n * p->groups_per_round;
    p->seen_off = 0;
    p->cur_off = p->words * 8;
    p->next_off = p->words * 16;
    p->lvl_off = p->words * 24;
    p->bytes = p->lvl_off + p->words * kGroup;
    return true;
}

// round r of the plan: its first group, its groups, its first request and its requests
struct Round { uint64_t group0, n_groups; uint32_t request0, n_requests; };
inline Round round_of(const RoundPlan &p, uint32_t b, uint64_t r) {
    Round o;
    o.group0 = r * p.groups_per_round;
    o.n_groups = p.groups - o.group0 < p.groups_per_round ? p.groups - o.group0 : p.groups_per_round;
    o.request0 = (uint32_t)(o.group0 * kGroup);
    const uint64_t left = (uint64_t)b - o.request0, full = o.n_groups * kGroup;
    o.n_requests = (uint32_t)(left < full ? left : full);
    return o;
}

} // namespace hvx_spd
