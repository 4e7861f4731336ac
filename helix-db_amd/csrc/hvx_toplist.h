// hvx_toplist.h -- the k <= 64 smallest (score, row) pairs offered to ONE wavefront, kept sorted in a register pair per lane (round 6).
//
// Candidate order (crates/db/src/search/vector/model.rs:55-61): score ascending, then id ascending -- rows are numbered in id order, so
// (score, row) sorts like (score, id).  Lane l holds the l-th smallest pair; unused lanes hold (+inf, kSentinel), so that the rank of a
// new pair is one ballot without a length test.  An insertion = two ballots + one DPP wave shift; a pair whose row is already in the
// list is dropped (RestrictedVectorCandidates is a set, restricted.rs:303-371: a duplicate candidate id counts once).  Shared by the
// one-launch restricted scan (hvx_restricted_exact.hip) and the exact tail of the small-batch scan (hvx_flat_tail.hip).
#pragma once
#include "hvx_beam.h"

namespace hvx {

struct TopList {
    float sc;
    uint32_t id;
    uint32_t count; // uniform
    float thr_s;    // the k-th pair once the list holds k (else +inf / all ones): only pairs before it are admitted
    uint32_t thr_i;
    __device__ __forceinline__ void init() {
        sc = __uint_as_float(0x7F800000u);
        id = kSentinel;
        count = 0;
        thr_s = __uint_as_float(0x7F800000u);
        thr_i = 0xFFFFFFFFu;
    }
    __device__ __forceinline__ bool admits(float d, uint32_t row) const { return d < thr_s || (d == thr_s && row < thr_i); }
    // (d, row) wave-uniform, d finite
    __device__ __forceinline__ void insert(float d, uint32_t row, uint32_t k, int lane) {
        const bool less = (sc < d) | ((sc == d) & (id < row));
        const unsigned long long before = __ballot(less);
        if (__ballot(id == row)) return; // the same candidate twice: a set holds it once
        const uint32_t p = (uint32_t)__builtin_popcountll(before);
        if (p >= k) return;
        const uint32_t ss = shr1(__float_as_uint(sc), 0u), si = shr1(id, 0u);
        const bool at = (uint32_t)lane == p, after = (uint32_t)lane > p;
        sc = at ? d : (after ? __uint_as_float(ss) : sc);
        id = at ? row : (after ? si : id);
        count += count < 64u ? 1u : 0u;
        if (count >= k) {
            thr_s = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(sc), (int)(k - 1u)));
            thr_i = __builtin_amdgcn_readlane(id, (int)(k - 1u));
        }
    }
    // every lane holding a pair with take == true offers it, in lane order
    __device__ __forceinline__ void offer(bool take, float d, uint32_t row, uint32_t k, int lane) {
        unsigned long long m = __ballot(take);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1ull;
            const float dd = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(d), l));
            const uint32_t rr = __builtin_amdgcn_readlane(row, l);
            if (admits(dd, rr)) insert(dd, rr, k, lane);
        }
    }
    // the pair this lane holds, padded
    __device__ __forceinline__ float lane_score() const { return sc; }
    __device__ __forceinline__ uint32_t lane_row() const { return id; }
};

// The same list over R registers per lane: 64 R pairs, entry e in register e / 64 of lane e % 64 (the layout of Beam<R>, hvx_beam.h), for
// result counts up to MAX_RESTRICTED_RESULT_COUNT = 800 (restricted.rs:55: R = 13).  Unused entries hold (+inf, kSentinel), so the rank
// needs no length test.  Against Beam<R>: a row already in the list is rejected (the ballot covers all R registers), the admission
// threshold is the k-th pair (register (k - 1) / 64, lane (k - 1) % 64: a chain of selects, no indexed register array), and there is no
// expanded bit.  The lane-63 -> lane-0 carry between registers is Beam::insert's.
template <int R> struct TopListWide {
    static constexpr uint32_t CAP = 64u * R;
    float sc[R];
    uint32_t id[R];
    uint32_t count; // uniform
    float thr_s;
    uint32_t thr_i;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int r = 0; r < R; ++r) { sc[r] = __uint_as_float(0x7F800000u); id[r] = kSentinel; }
        count = 0;
        thr_s = __uint_as_float(0x7F800000u);
        thr_i = 0xFFFFFFFFu;
    }
    __device__ __forceinline__ bool admits(float d, uint32_t row) const { return d < thr_s || (d == thr_s && row < thr_i); }
    // entry `pos` (uniform) of one of the two register rows: R readlanes + scalar selects
    __device__ __forceinline__ uint32_t bcast(const uint32_t (&v)[R], uint32_t pos) const {
        uint32_t out = __builtin_amdgcn_readlane(v[0], pos & 63u);
#pragma unroll
        for (int r = 1; r < R; ++r) {
            const uint32_t t = __builtin_amdgcn_readlane(v[r], pos & 63u);
            out = (pos >> 6) == (uint32_t)r ? t : out;
        }
        return out;
    }
    __device__ __forceinline__ void set_threshold(uint32_t k) {
        if (count < k) return;
        uint32_t bits[R];
#pragma unroll
        for (int r = 0; r < R; ++r) bits[r] = __float_as_uint(sc[r]);
        thr_s = __uint_as_float(bcast(bits, k - 1u));
        thr_i = bcast(id, k - 1u);
    }
    // (d, row) wave-uniform, d finite
    __device__ __forceinline__ void insert(float d, uint32_t row, uint32_t k, int lane) {
        uint32_t p = 0;
        unsigned long long same = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const bool less = (sc[r] < d) | ((sc[r] == d) & (id[r] < row));
            p += (uint32_t)__builtin_popcountll(__ballot(less));
            same |= __ballot(id[r] == row);
        }
        if (same) return; // the same candidate twice: a set holds it once
        if (p >= k) return;
#pragma unroll
        for (int r = R - 1; r >= 0; --r) {
            if (p > (uint32_t)r * 64u + 63u) continue; // (uniform: the registers before the insertion point stay)
            const uint32_t e = (uint32_t)r * 64u + (uint32_t)lane;
            uint32_t cs = 0, ci = 0;
            if (r > 0) {
                cs = __builtin_amdgcn_readlane(__float_as_uint(sc[r - 1]), 63);
                ci = __builtin_amdgcn_readlane(id[r - 1], 63);
            }
            const uint32_t ss = shr1(__float_as_uint(sc[r]), cs), si = shr1(id[r], ci);
            const bool at = e == p, after = e > p;
            sc[r] = at ? d : (after ? __uint_as_float(ss) : sc[r]);
            id[r] = at ? row : (after ? si : id[r]);
        }
        count += count < CAP ? 1u : 0u;
        set_threshold(k);
    }
    // every lane holding a pair with take == true offers it, in lane order
    __device__ __forceinline__ void offer(bool take, float d, uint32_t row, uint32_t k, int lane) {
        unsigned long long m = __ballot(take);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1ull;
            const float dd = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(d), l));
            const uint32_t rr = __builtin_amdgcn_readlane(row, l);
            if (admits(dd, rr)) insert(dd, rr, k, lane);
        }
    }
    // the registers were filled with a sorted, padded list of distinct rows: count it and set the threshold
    __device__ __forceinline__ void adopt(uint32_t k) {
        count = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) count += (uint32_t)__builtin_popcountll(__ballot(id[r] != kSentinel));
        thr_s = __uint_as_float(0x7F800000u);
        thr_i = 0xFFFFFFFFu;
        set_threshold(k);
    }
};

} // namespace hvx
