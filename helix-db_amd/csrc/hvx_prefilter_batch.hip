// hvx_prefilter_batch.hip -- chains of `expand` hops for a BATCH of requests, every request from its own start nodes
// (hvx_expand_path_lists / hvx_prefilter_path_search_lists_params; the entry points live in hvx_prefilter.hip beside the graph handle).
//
// Reference: one stored query such as g().n(user).out("follows").out("likes").vector_search(..) runs once per request: the compiled plan
// (hop directions, edge labels, Filter step) is the same, the bind parameters (start nodes) and the query vector are the request's own
// (crates/db/src/execution/interpreter/access/expand.rs:16-80, access/search/storage.rs:140-163, search/vector/restricted.rs:303-371).
//
// The chains of different requests are independent, so nothing orders two workgroups: ONE launch, one 1 024-thread workgroup per request,
// which walks all hops of its own chain.  Semantics per request are hvx_expand_path_filter's: F0 = the seeds, F(i + 1) = the union of the
// neighbours of F(i) under hop i's direction and allow-set, no visited exclusion, a node without arcs drops out.
//   * The union is a per-workgroup open-addressing hash set in LDS (u32 node numbers, empty = 0xFFFFFFFF -- hvx_csr_import keeps the node
//     count below that), insertion = one atomicCAS test-and-set per probe, cleared between the hops.  Slots = a power of two >= 2 x
//     max_frontier and >= 4 096: a wavefront looks at the set's size before every step, so at most 16 x 64 insertions are in flight when the
//     size crosses max_frontier, and the table cannot fill.  The probe loop is bounded by the slot count all the same.
//     max_frontier <= 16 384: 32 768 slots = 128 KiB of the CU's 160 KiB, + 128 bytes of counters.
//   * Frontier lists ping-pong between two HBM slots of max_frontier u32 per request.  The workgroup that writes them reads them: the
//     workgroup barrier (and the fence it carries) orders that, no agent-scope operation is needed.
//   * Row work is split as in path_hop_kernel: rows of at most 16 arcs by their own lane, longer ones by a whole wavefront, one at a time.
//     Append positions cost one LDS counter update per wavefront step (ballot + popcount).
//   * The first hop whose set exceeds max_frontier ends the chain: its size is reported as max_frontier + 1, later hops as 0, the request
//     is marked HVX_ERR_CANDIDATE_LIMIT and its list length is 0 (the scan behind it reads lens[q] ids of a slot of max_frontier).
//   * The last hop writes the set as u64 ids, ANDed with the optional node mask, into the request's slot of the one-launch scan
//     (hvx_restricted_exact.hip: per-query lists in fixed slots), in whatever order the wavefronts get there: the scan orders by (score, id).
// Algorithmic bytes per request: the adjacency rows of every frontier node once (offsets 16 B + 4 B per arc, + 4 B per arc when labelled)
// + 8 B per frontier node written and read back.  The kernel is latency-bound (dependent offset -> target -> LDS probe chains), not HBM-bound.
#include <hip/hip_runtime.h>

#include "hvx_host.h"

using namespace hvx;

namespace {

constexpr uint32_t kEmpty = 0xFFFFFFFFu;
constexpr uint32_t kLight = 16;    // rows up to this long are walked by their own lane
constexpr uint32_t kCtlWords = 32; // LDS words in front of the table: [0] size of the set under construction, [1] ids written by the last hop, [8 ..) hop sizes

__device__ __forceinline__ bool lists_label_ok(uint32_t lab, const uint32_t *allowed, uint32_t n_allowed) {
    if (n_allowed == 0) return true; // an empty allow-set means every label (traversal.rs:53)
    for (uint32_t i = 0; i < n_allowed; ++i)
        if (allowed[i] == lab) return true;
    return false;
}

__global__ __launch_bounds__(1024) void path_lists_kernel(PathListsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *ctl = reinterpret_cast<uint32_t *>(smem);
    uint32_t *tab = ctl + kCtlWords;
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t mf = a.max_frontier, slot_mask = a.slots - 1u;
    const unsigned long long below = (1ull << lane) - 1ull;

    // test-and-set of v in the table; a full table answers "seen" (only a set past max_frontier gets there: its chain is over)
    auto insert = [&](uint32_t v) __attribute__((always_inline)) -> bool {
        uint32_t h = (v * 0x9E3779B1u) >> a.hash_shift;
        for (uint32_t probe = 0; probe < a.slots; ++probe) {
            const uint32_t old = atomicCAS(&tab[h], kEmpty, v);
            if (old == kEmpty) return true;
            if (old == v) return false;
            h = (h + 1u) & slot_mask;
        }
        return false;
    };
    // wave-uniform: the set under construction has outgrown the slot
    auto over = [&]() __attribute__((always_inline)) -> bool {
        return (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(&ctl[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) > mf;
    };

    if (tid < kCtlWords) ctl[tid] = 0u;
    const uint32_t s0 = a.seed_off[q];
    uint32_t n_cur = a.seed_off[q + 1] - s0; // (the host has seen it at most max_frontier)
    const uint32_t *cur = a.seeds + s0;
    uint32_t *slot[2] = {a.front + (size_t)q * 2u * mf, a.front + (size_t)q * 2u * mf + mf};
    unsigned long long *ids_out = a.out_ids + (size_t)q * mf;
    bool overflow = false;

    for (uint32_t hop = 0; hop < a.n_hops && n_cur != 0u; ++hop) {
        const bool last = hop + 1u == a.n_hops;
        for (uint32_t i = tid; i < a.slots; i += 1024u) tab[i] = kEmpty;
        if (tid == 0) ctl[0] = 0u;
        __syncthreads();
        uint32_t *dst = slot[hop & 1u];
        const uint32_t direction = a.direction[hop];
        const uint32_t *allowed = a.labels + a.label_off[hop];
        const uint32_t n_allowed = a.label_off[hop + 1] - a.label_off[hop];
        // one arc of every lane: fresh targets take a place in the next frontier (the last hop: in the scan's slot, behind the mask)
        auto take = [&](bool active, const uint32_t *tgt, const uint32_t *lab, uint64_t at) __attribute__((always_inline)) {
            uint32_t v = 0;
            bool fresh = false;
            if (active && (!lab || lists_label_ok(lab[at], allowed, n_allowed))) {
                v = tgt[at];
                fresh = insert(v);
            }
            const unsigned long long fm = __ballot(fresh);
            if (fm == 0ull) return;
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&ctl[0], (uint32_t)__builtin_popcountll(fm));
            base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
            uint32_t pos = base + (uint32_t)__builtin_popcountll(fm & below);
            if (!last) {
                if (fresh && pos < mf) dst[pos] = v;
                return;
            }
            bool keep = fresh;
            if (a.mask) {
                keep = fresh && ((a.mask[v >> 5] >> (v & 31u)) & 1u) != 0u;
                const unsigned long long km = __ballot(keep);
                if (km == 0ull) return;
                if (lane == 0) base = atomicAdd(&ctl[1], (uint32_t)__builtin_popcountll(km));
                base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
                pos = base + (uint32_t)__builtin_popcountll(km & below);
            }
            if (keep && pos < mf) ids_out[pos] = (unsigned long long)v;
        };
        for (uint32_t c0 = 0; c0 < n_cur; c0 += 1024u) {
            const bool have = c0 + tid < n_cur;
            const uint32_t node = have ? cur[c0 + tid] : 0u;
            for (int pass = 0; pass < 2; ++pass) {
                const bool use_out = pass == 0;
                if (use_out && direction == 1u) continue;  // In only
                if (!use_out && direction == 0u) continue; // Out only
                const uint64_t *off = use_out ? a.out_off : a.in_off;
                const uint32_t *tgt = use_out ? a.out_tgt : a.in_tgt;
                const uint32_t *lab = use_out ? a.out_lab : a.in_lab;
                const uint64_t a0 = have ? off[node] : 0ull, a1 = have ? off[node + 1] : 0ull;
                const uint32_t deg = (uint32_t)(a1 - a0); // (the entry points refuse graphs with a row of 2^31 arcs)
                const bool light = deg <= kLight;
                uint32_t steps = light ? deg : 0u;
#pragma unroll
                for (int sh = 32; sh > 0; sh >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)steps, sh, 64); steps = o > steps ? o : steps; }
                for (uint32_t i = 0; i < steps && !over(); ++i) take(light && i < deg, tgt, lab, a0 + i);
                unsigned long long heavy = __ballot(have && !light); // long rows: the whole wavefront strides over the arcs of one node at a time
                while (heavy && !over()) {
                    const int l = __builtin_ctzll(heavy);
                    heavy &= heavy - 1ull;
                    const uint64_t h0 = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(a0 >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)a0, l);
                    const uint32_t hdeg = (uint32_t)__builtin_amdgcn_readlane((int)deg, l);
                    for (uint32_t j = 0; j < hdeg && !over(); j += 64u) take(j + lane < hdeg, tgt, lab, h0 + j + lane);
                }
            }
        }
        __syncthreads(); // the hop's set is complete, its list visible to the whole workgroup
        const uint32_t size = ctl[0];
        __syncthreads(); // (every thread has read it before the next hop starts from zero)
        overflow = size > mf;
        if (tid == 0) ctl[8 + hop] = overflow ? mf + 1u : size;
        if (overflow) break; // (uniform: every thread read the same word between the two barriers)
        cur = dst;
        n_cur = size;
    }
    __syncthreads();
    if (tid < a.n_hops) a.hop_sizes[(size_t)q * 16u + tid] = ctl[8 + tid];
    if (tid == 0) {
        // a chain that ran dry before its last hop wrote no id; one that reached it left ctl[0] (no mask) or ctl[1] ids in the slot
        const bool reached = !overflow && n_cur != 0u;
        a.lens[q] = reached ? (a.mask ? ctl[1] : ctl[0]) : 0u;
        a.status[q] = overflow ? (uint32_t)HVX_ERR_CANDIDATE_LIMIT : (uint32_t)HVX_OK;
    }
}

} // namespace

namespace hvx {

hipError_t launch_path_lists(const PathListsArgs &args, uint32_t b, hipStream_t s) {
    if (b == 0) return hipSuccess;
    PathListsArgs a = args;
    a.slots = 4096u; // the floor keeps max_frontier + 1 024 below the slot count for small slots
    while (a.slots < 2u * a.max_frontier) a.slots <<= 1;
    a.hash_shift = 32u - (uint32_t)__builtin_ctz(a.slots);
    const size_t lds = (size_t)(kCtlWords + a.slots) * 4u;
    if (lds > 48 * 1024) { // (a workgroup above 48 KiB asks for it)
        hipError_t e = hipFuncSetAttribute((const void *)path_lists_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(path_lists_kernel, dim3(b), dim3(1024), lds, s, a);
    return hipGetLastError();
}

} // namespace hvx
