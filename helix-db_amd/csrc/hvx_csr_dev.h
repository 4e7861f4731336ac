// hvx_csr_dev.h -- the device pieces every graph kernel shares, each defined once: the label test, the row split (rows of
// at most kLightRow arcs by their own lane, longer ones by a whole wavefront), the wave-aggregated append and the LDS node set of the
// per-request kernels.  Callers pass lambdas; nothing here knows which kernel is calling.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hvx_csr_view.h"

namespace hvx {

__device__ __forceinline__ bool label_ok(uint32_t lab, const uint32_t *allowed, uint32_t n_allowed) {
    if (n_allowed == 0) return true; // empty allow-set means every label (traversal.rs:53)
    for (uint32_t i = 0; i < n_allowed; ++i)
        if (allowed[i] == lab) return true;
    return false;
}

constexpr uint32_t kLightRow = 16; // rows up to this long are walked one arc per step by their node's own lane (64 nodes per wavefront)

// One place per flagged lane behind *counter (LDS or global): ONE counter update per wavefront.  Returns at once, wave-uniformly, with
// any == false when no lane is flagged (the caller's step has nothing to place); pos means something in flagged lanes only.
struct WavePlace { bool any; uint32_t pos; };
__device__ __forceinline__ WavePlace wave_append(bool flag, uint32_t *counter, uint32_t lane) {
    const unsigned long long m = __ballot(flag);
    if (m == 0ull) return {false, 0u};
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(counter, (uint32_t)__builtin_popcountll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    return {true, base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u))}; // + flagged lanes below this one
}

__device__ __forceinline__ uint32_t wave_max(uint32_t steps) {
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)steps, sh, 64); steps = o > steps ? o : steps; }
    return steps;
}

// One adjacency row of `node`: pass 0 = outgoing, pass 1 = incoming.  False when `direction` skips the pass.  A lane without a node
// gets an empty row; the arc count saturates at 32 bits (the chain entry points refuse graphs with a row of 2^31 arcs anyway).
struct AdjRow {
    const uint32_t *tgt, *lab;
    uint64_t a0;
    uint32_t deg;
};
__device__ __forceinline__ bool adj_pass(const CsrView &g, uint32_t direction, int pass, bool have, uint32_t node, AdjRow *r) {
    const bool use_out = pass == 0;
    if (use_out && direction == 1u) return false;  // In only
    if (!use_out && direction == 0u) return false; // Out only
    const uint64_t *off = use_out ? g.out_off : g.in_off;
    r->tgt = use_out ? g.out_tgt : g.in_tgt;
    r->lab = use_out ? g.out_lab : g.in_lab;
    const uint64_t a0 = have ? off[node] : 0ull, a1 = have ? off[node + 1] : 0ull;
    r->a0 = a0;
    r->deg = (uint32_t)((a1 - a0) < 0xFFFFFFFFull ? (a1 - a0) : 0xFFFFFFFFull);
    return true;
}

// Long rows: the whole wavefront strides over the arcs of one flagged lane's row at a time.  arc(active, at) sees one arc per lane;
// keep_going() is wave-uniform and asked before every step.  (Rows stay below 2^32 - 64 arcs: the callers' entry points see to it.)
template <typename KeepGoing, typename Arc>
__device__ __forceinline__ void walk_heavy_rows(bool is_heavy, uint64_t a0, uint32_t deg, KeepGoing keep_going, Arc arc) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long heavy = __ballot(is_heavy);
    while (heavy && keep_going()) {
        const int l = __builtin_ctzll(heavy);
        heavy &= heavy - 1ull;
        const uint64_t h0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(a0 >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)a0, l);
        const uint32_t hdeg = (uint32_t)__builtin_amdgcn_readlane((int)deg, l);
        for (uint32_t j = 0; j < hdeg && keep_going(); j += 64u) arc(j + lane < hdeg, h0 + j + lane);
    }
}

// Both passes over the rows of one node per lane, each wavefront on its own: the light rows one arc per step, then the heavy ones.
// arc(active, tgt, lab, at).
template <typename KeepGoing, typename Arc>
__device__ __forceinline__ void walk_rows_per_wave(const CsrView &g, uint32_t direction, bool have, uint32_t node, KeepGoing keep_going, Arc arc) {
    for (int pass = 0; pass < 2; ++pass) {
        AdjRow r;
        if (!adj_pass(g, direction, pass, have, node, &r)) continue;
        const bool light = r.deg <= kLightRow;
        const uint32_t steps = wave_max(light ? r.deg : 0u);
        for (uint32_t i = 0; i < steps && keep_going(); ++i) arc(light && i < r.deg, r.tgt, r.lab, r.a0 + i);
        walk_heavy_rows(have && !light, r.a0, r.deg, keep_going, [&](bool active, uint64_t at) __attribute__((always_inline)) { arc(active, r.tgt, r.lab, at); });
    }
}

// The per-workgroup open-addressing set of u32 node numbers in dynamic LDS (path_lists_kernel, repeat_lists_kernel, shortest_path_kernel).  kNodeSetCtlWords
// control words sit in front of the table; word [0] counts the nodes in the set.
constexpr uint32_t kNodeSetCtlWords = 32;
struct LdsNodeSet {
    static constexpr uint32_t kEmpty = 0xFFFFFFFFu; // (hvx_csr_import keeps the node count below it)
    uint32_t *tab;
    uint32_t slots, shift;
    __device__ __forceinline__ void clear(uint32_t tid) const {
        for (uint32_t i = tid; i < slots; i += 1024u) tab[i] = kEmpty;
    }
    // test-and-set of v; a full table answers "seen" (only a set past max_frontier gets there: its request is over)
    __device__ __forceinline__ bool insert(uint32_t v) const {
        uint32_t h = (v * 0x9E3779B1u) >> shift;
        for (uint32_t probe = 0; probe < slots; ++probe) {
            const uint32_t old = atomicCAS(&tab[h], kEmpty, v);
            if (old == kEmpty) return true;
            if (old == v) return false;
            h = (h + 1u) & (slots - 1u);
        }
        return false;
    }
    // insert that also says where: the slot that holds v, *fresh = this call put it there; `slots` (and not fresh) for a full table
    __device__ __forceinline__ uint32_t insert_slot(uint32_t v, bool *fresh) const {
        uint32_t h = (v * 0x9E3779B1u) >> shift;
        *fresh = false;
        for (uint32_t probe = 0; probe < slots; ++probe) {
            const uint32_t old = atomicCAS(&tab[h], kEmpty, v);
            if (old == kEmpty) { *fresh = true; return h; }
            if (old == v) return h;
            h = (h + 1u) & (slots - 1u);
        }
        return slots;
    }
    // read-only probe, for a phase in which nothing inserts: the slot that holds v, or `slots` when v is not in the set
    __device__ __forceinline__ uint32_t find(uint32_t v) const {
        uint32_t h = (v * 0x9E3779B1u) >> shift;
        for (uint32_t probe = 0; probe < slots; ++probe) {
            const uint32_t at = tab[h];
            if (at == v) return h;
            if (at == kEmpty) break;
            h = (h + 1u) & (slots - 1u);
        }
        return slots;
    }
    // wave-uniform: the set, counted in *size, has outgrown `max`.  A wavefront asks before EVERY step, so at most 16 x 64 insertions
    // are in flight when the size crosses `max` and the table cannot fill.
    __device__ __forceinline__ static bool over(const uint32_t *size, uint32_t max) {
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(size, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) > max;
    }
};

// slots of the table for sets of up to max_frontier nodes: a power of two >= 2 x max_frontier
inline uint32_t node_set_slots(uint32_t max_frontier) {
    uint32_t slots = 4096u; // the floor keeps max_frontier + 1 024 below the slot count for small slots
    while (slots < 2u * max_frontier) slots <<= 1;
    return slots;
}

// One 1 024-thread workgroup per request, the table sized from args.max_frontier (Args carries max_frontier, slots, hash_shift).
template <typename Args>
hipError_t launch_node_set_kernel(void (*kernel)(Args), const Args &args, uint32_t b, hipStream_t s) {
    if (b == 0) return hipSuccess;
    Args a = args;
    a.slots = node_set_slots(a.max_frontier);
    a.hash_shift = 32u - (uint32_t)__builtin_ctz(a.slots);
    const size_t lds = (size_t)(kNodeSetCtlWords + a.slots) * 4u;
    if (lds > 48 * 1024) { // (a workgroup above 48 KiB asks for it)
        hipError_t e = hipFuncSetAttribute((const void *)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(b), dim3(1024), lds, s, a);
    return hipGetLastError();
}

} // namespace hvx
