// hvx_prefilter_batch.hip -- chains of `expand` hops for a BATCH of requests, every request from its own start nodes
// (hvx_expand_path_lists / hvx_prefilter_path_search_lists_params; the entry points live in hvx_prefilter.hip, the graph handle in hvx_csr.h, the row walker and the node set in hvx_csr_dev.h).
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

#include "hvx_csr_dev.h"
#include "hvx_host.h"

using namespace hvx;

namespace {

// LDS control words in front of the table: [0] size of the set under construction, [1] ids written by the last hop, [8 ..) hop sizes
__global__ __launch_bounds__(1024) void path_lists_kernel(PathListsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *ctl = reinterpret_cast<uint32_t *>(smem);
    const LdsNodeSet set{ctl + kNodeSetCtlWords, a.slots, a.hash_shift};
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t mf = a.max_frontier;
    auto room = [&]() __attribute__((always_inline)) -> bool { return !LdsNodeSet::over(&ctl[0], mf); };

    if (tid < kNodeSetCtlWords) ctl[tid] = 0u;
    const uint32_t s0 = a.seed_off[q];
    uint32_t n_cur = a.seed_off[q + 1] - s0; // (the host has seen it at most max_frontier)
    const uint32_t *cur = a.seeds + s0;
    uint32_t *slot[2] = {a.front + (size_t)q * 2u * mf, a.front + (size_t)q * 2u * mf + mf};
    unsigned long long *ids_out = a.out_ids + (size_t)q * mf;
    bool overflow = false;

    for (uint32_t hop = 0; hop < a.n_hops && n_cur != 0u; ++hop) {
        const bool last = hop + 1u == a.n_hops;
        set.clear(tid);
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
            if (active && (!lab || label_ok(lab[at], allowed, n_allowed))) {
                v = tgt[at];
                fresh = set.insert(v);
            }
            WavePlace p = wave_append(fresh, &ctl[0], lane);
            if (!p.any) return;
            if (!last) {
                if (fresh && p.pos < mf) dst[p.pos] = v;
                return;
            }
            bool keep = fresh;
            if (a.mask) {
                keep = fresh && ((a.mask[v >> 5] >> (v & 31u)) & 1u) != 0u;
                p = wave_append(keep, &ctl[1], lane);
                if (!p.any) return;
            }
            if (keep && p.pos < mf) ids_out[p.pos] = (unsigned long long)v;
        };
        for (uint32_t c0 = 0; c0 < n_cur; c0 += 1024u) {
            const bool have = c0 + tid < n_cur;
            walk_rows_per_wave(a.g, direction, have, have ? cur[c0 + tid] : 0u, room, take);
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

hipError_t launch_path_lists(const PathListsArgs &args, uint32_t b, hipStream_t s) { return launch_node_set_kernel(path_lists_kernel, args, b, s); }

} // namespace hvx
