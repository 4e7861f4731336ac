// hvx_shortest_path.hip -- shortest_path for a BATCH of (source, target) requests that share direction, label allow-set and max_depth
// (hvx_shortest_path_batch), and the reference's literal loop on the host (hvx_shortest_path_host, hvx_shortest_path_host.h).
//
// Reference: crates/db/src/execution/interpreter/shortest_path.rs:16-96 -- a breadth-first search from the source, a node's neighbours its
// distinct allowed neighbours in ascending id order, the first discoverer in queue order the predecessor, the search over when the target
// is discovered.  Queue order inside a level is the lexicographic order of the nodes' predecessor chains, so that path is the
// lexicographically smallest of all shortest paths (DESIGN 4.4f has the argument, tests/test_shortest_path_host.py holds the literal loop
// to it).  Which node discovers which inside a level therefore does not matter; only every node's LEVEL does:
//   Phase A  levels from the TARGET over the reversed arcs, level-synchronous, until the source is in the set (that level completes), a
//            level comes up empty, max_depth levels are done or the set outgrows max_reach.  One append-only list of max_reach u32 per
//            request holds the set in discovery order (level k is a slice of it); the lane whose insert wins writes the node's level into
//            a byte per TABLE SLOT in HBM.
//   Phase B  from c = source at level d, d times: walk c's FORWARD row with all sixteen wavefronts, look every allowed target up in the set
//            (read-only), keep the smallest one whose level is level(c) - 1 (wavefront min, then one LDS atomicMin per wavefront).
// The kernel has repeat_lists_kernel's shape (hvx_prefilter_repeat.hip): one launch, one 1 024-thread workgroup per request, the set an
// LdsNodeSet in dynamic LDS sized by node_set_slots(max_reach), rows of at most 16 arcs by their own lane and longer ones by a wavefront in
// Phase A, append positions by wave_append on an LDS counter, every store guarded by position < max_reach, LdsNodeSet::over asked before
// every step so the table cannot fill.  The workgroup that writes the list and the level bytes is the one that reads them, behind a
// workgroup barrier: there is no agent-scope fence or atomic.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "hvx_csr.h"
#include "hvx_shortest_path_host.h"

using namespace hvx;

namespace {

constexpr uint32_t kNoNode = 0xFFFFFFFFu; // an endpoint that resolved to nothing; also "no candidate" in Phase B (node numbers stay below it)

// LDS control words in front of the table: [0] nodes in the reach set, [2] the source was seen, [4] [5] Phase B's minimum (steps alternate)
__global__ __launch_bounds__(1024) void shortest_path_kernel(ShortestPathArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *ctl = reinterpret_cast<uint32_t *>(smem);
    const LdsNodeSet set{ctl + kNodeSetCtlWords, a.slots, a.hash_shift};
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t mr = a.max_frontier, md = a.max_depth;
    const uint32_t src = a.src[q], dst = a.dst[q];
    unsigned long long *path = a.out_paths + (size_t)q * (md + 1u);
    uint32_t *sizes = a.level_sizes + (size_t)q * md;
    if (src == kNoNode || dst == kNoNode || src == dst) { // (uniform) nothing to search
        const uint32_t same = (src == dst && src != kNoNode) ? 1u : 0u;
        for (uint32_t i = tid; i < md; i += 1024u) sizes[i] = same; // the reach set is the target alone / there is none
        if (tid == 0) {
            if (same) path[0] = (unsigned long long)src;
            a.lens[q] = same;
            a.status[q] = (uint32_t)HVX_OK;
        }
        return;
    }
    uint32_t *order = a.order + (size_t)q * mr;
    uint8_t *level = a.level + (size_t)q * a.slots;
    auto room = [&]() __attribute__((always_inline)) -> bool { return !LdsNodeSet::over(&ctl[0], mr); };

    if (tid < kNodeSetCtlWords) ctl[tid] = tid == 4u || tid == 5u ? kNoNode : 0u;
    set.clear(tid);
    __syncthreads();
    if (tid == 0) { // level 0 = the target (max_reach >= 1: it fits)
        bool fresh;
        level[set.insert_slot(dst, &fresh)] = 0;
        order[0] = dst;
        ctl[0] = 1u;
    }
    __syncthreads();

    // Phase A
    const uint32_t back = a.direction == (uint32_t)HVX_DIR_OUT ? (uint32_t)HVX_DIR_IN : a.direction == (uint32_t)HVX_DIR_IN ? (uint32_t)HVX_DIR_OUT : (uint32_t)HVX_DIR_BOTH;
    bool overflow = false;
    uint32_t r0 = 0, n_cur = 1, reached = 1; // the level being expanded = order[r0 .. r0 + n_cur); nodes in the set when it was complete
    uint32_t ran = 0, dist = 0;
    for (uint32_t d = 1; d <= md && n_cur != 0u; ++d) {
        bool hit = false;
        // one arc of every lane
        auto arc = [&](bool active, const uint32_t *tgt, const uint32_t *lab, uint64_t at) __attribute__((always_inline)) {
            uint32_t v = 0, slot = 0;
            bool fresh = false;
            if (active && (!lab || label_ok(lab[at], a.allowed, a.n_allowed))) {
                v = tgt[at];
                hit = hit || v == src;
                slot = set.insert_slot(v, &fresh);
            }
            const WavePlace p = wave_append(fresh, &ctl[0], lane);
            if (!p.any) return;
            if (fresh) {
                level[slot] = (uint8_t)d; // (a fresh insert has a slot inside the table)
                if (p.pos < mr) order[p.pos] = v;
            }
        };
        for (uint32_t c0 = 0; c0 < n_cur; c0 += 1024u) {
            const bool have = c0 + tid < n_cur;
            const uint32_t node = have ? order[r0 + c0 + tid] : 0u;
            walk_rows_per_wave(a.g, back, have, node, room, arc);
        }
        if (hit) ctl[2] = 1u;
        __syncthreads(); // the level is complete: its slice of the list, its level bytes and the flag are visible to the whole workgroup
        const uint32_t reach = ctl[0];
        const bool found = ctl[2] != 0u;
        __syncthreads(); // (every thread has read both before the next level moves them)
        overflow = reach > mr;
        ran = d;
        if (tid == 0) sizes[d - 1u] = overflow ? mr + 1u : reach;
        if (overflow) break; // (uniform: every thread read the same words between the two barriers)
        r0 = reached;
        n_cur = reach - reached; // an empty new level ends the loop
        reached = reach;
        if (found) { dist = d; break; } // the level completed first: whether it overflowed does not depend on who saw the source when
    }
    // levels the loop never ran keep the size at its end; after an overflow they report 0
    for (uint32_t i = ran + tid; i < md; i += 1024u) sizes[i] = overflow ? 0u : reached;

    // Phase B: nothing inserts any more; the last level's barrier has made every level byte visible
    bool broken = false;
    if (dist != 0u) {
        uint32_t c = src;
        for (uint32_t i = 0; i < dist; ++i) {
            if (tid == 0) path[i] = (unsigned long long)c;
            const uint32_t want = dist - 1u - i;
            uint32_t best = kNoNode;
            for (int pass = 0; pass < 2; ++pass) {
                AdjRow r;
                if (!adj_pass(a.g, a.direction, pass, true, c, &r)) continue;
                for (uint64_t j = tid; j < r.deg; j += 1024u) {
                    const uint64_t at = r.a0 + j;
                    if (r.lab && !label_ok(r.lab[at], a.allowed, a.n_allowed)) continue;
                    const uint32_t v = r.tgt[at];
                    if (v >= best) continue;
                    const uint32_t s = set.find(v); // absent: not on a shortest path
                    if (s < a.slots && level[s] == (uint8_t)want) best = v;
                }
            }
#pragma unroll
            for (int sh = 32; sh > 0; sh >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)best, sh, 64); best = o < best ? o : best; }
            uint32_t *mn = &ctl[4u + (i & 1u)];
            if (lane == 0 && best != kNoNode) atomicMin(mn, best);
            __syncthreads();
            const uint32_t next = *mn;
            if (tid == 0) ctl[4u + ((i + 1u) & 1u)] = kNoNode; // the other word: last read before the previous step's second barrier
            __syncthreads();
            if (next >= a.g.n) { broken = true; break; } // (uniform; a node at level k > 0 has an arc to level k - 1, so this does not happen)
            c = next;
        }
        if (tid == 0 && !broken) path[dist] = (unsigned long long)c;
    }
    if (tid == 0) {
        a.lens[q] = (overflow || broken || dist == 0u) ? 0u : dist + 1u;
        a.status[q] = overflow ? (uint32_t)HVX_ERR_CANDIDATE_LIMIT : broken ? (uint32_t)HVX_ERR_INVARIANT : (uint32_t)HVX_OK;
    }
}

constexpr uint32_t kMaxReach = 16384; // 32 768 table slots x 4 B = 128 KiB of a CU's 160 KiB of LDS
constexpr uint32_t kMaxBatch = 65535;
constexpr uint32_t kMaxDepth = 255;   // a level is a byte

} // namespace

namespace hvx {

int shortest_path_plan_check(uint32_t max_depth, uint32_t direction, const uint32_t *allowed_label_ids, uint32_t n_labels) {
    if (direction > HVX_DIR_BOTH) return fail(HVX_ERR_INVARIANT, "bad direction %u", direction);
    if (max_depth == 0) return fail(HVX_ERR_INVARIANT, "shortest_path searches at least one level");
    if (n_labels && !allowed_label_ids) return fail(HVX_ERR_INVARIANT, "null labels");
    return HVX_OK;
}

hipError_t launch_shortest_path(const ShortestPathArgs &args, uint32_t b, hipStream_t s) { return launch_node_set_kernel(shortest_path_kernel, args, b, s); }

} // namespace hvx

extern "C" int hvx_shortest_path_batch(const hvx_csr *cg, uint32_t b, const uint64_t *sources, const uint64_t *targets, uint32_t max_depth,
                                       uint32_t direction, const uint32_t *allowed_label_ids, uint32_t n_labels, uint32_t max_reach,
                                       uint64_t *out_paths, uint32_t *out_lens, uint32_t *out_status, uint64_t *out_level_sizes) {
    if (!cg || !out_paths || !out_lens || !out_status || (b && (!sources || !targets))) return fail(HVX_ERR_INVARIANT, "null argument");
    hvx_csr *g = const_cast<hvx_csr *>(cg);
    int rc = shortest_path_plan_check(max_depth, direction, allowed_label_ids, n_labels);
    if (rc) return rc;
    if (max_depth > kMaxDepth) return fail(HVX_ERR_UNSUPPORTED, "shortest_path on the device searches at most %u levels, not %u", kMaxDepth, max_depth);
    if (max_reach == 0 || max_reach > kMaxReach)
        return fail(HVX_ERR_UNSUPPORTED, "a request's reach set holds 1 .. %u nodes (max_reach %u): larger searches take hvx_traverse_ordered", kMaxReach, max_reach);
    if (b > kMaxBatch) return fail(HVX_ERR_UNSUPPORTED, "a batch of shortest-path requests holds at most %u", kMaxBatch);
    for (uint32_t q = 0; q < b; ++q)
        for (const uint64_t v : {sources[q], targets[q]})
            if (v >= g->n && v != UINT64_MAX) return fail(HVX_ERR_INVARIANT, "unknown node %llu in request %u", (unsigned long long)v, q);
    if (b == 0) return HVX_OK;

    std::lock_guard<std::mutex> lock(g->mu);
    HIP_TRY(hipSetDevice(g->device));
    hipStream_t s = g->stream;
    if ((rc = seeds_reserve(g, 2 * (size_t)b, nullptr))) return rc;
    uint32_t *h_src = g->h_seeds, *h_dst = g->h_seeds + b;
    for (uint32_t q = 0; q < b; ++q) {
        h_src[q] = sources[q] == UINT64_MAX ? kNoNode : (uint32_t)sources[q];
        h_dst[q] = targets[q] == UINT64_MAX ? kNoNode : (uint32_t)targets[q];
    }
    if ((rc = upload_labels(g, allowed_label_ids, n_labels, s))) return rc;
    // [b][max_depth + 1] u64 paths | [b] lengths | [b] statuses | [b][max_depth] sizes || [b][max_reach] u32 order | [b][slots] u8 levels
    const uint32_t slots = node_set_slots(max_reach);
    const size_t path_words = (size_t)b * (max_depth + 1u), ctl_words = (size_t)b * (2u + max_depth), back_bytes = path_words * 8 + ctl_words * 4;
    if ((rc = csr_reserve(g, &g->sp_buf, &g->sp_cap, back_bytes + (size_t)b * max_reach * 4 + (size_t)b * slots))) return rc;
    ShortestPathArgs a;
    memset(&a, 0, sizeof(a));
    a.g = csr_view(g);
    a.src = h_src; a.dst = h_dst;
    a.max_depth = max_depth; a.direction = direction; a.n_allowed = n_labels;
    a.allowed = g->labels;
    a.max_frontier = max_reach;
    a.out_paths = static_cast<unsigned long long *>(g->sp_buf);
    uint32_t *ctl = reinterpret_cast<uint32_t *>(a.out_paths + path_words);
    a.lens = ctl; a.status = ctl + b; a.level_sizes = ctl + 2 * (size_t)b;
    a.order = ctl + ctl_words;
    a.level = reinterpret_cast<uint8_t *>(a.order + (size_t)b * max_reach);
    hipError_t e = launch_shortest_path(a, b, s);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        return fail(HVX_ERR_DEVICE, "shortest_path_kernel: %s", hipGetErrorString(e));
    }
    // one copy back: the paths and the control words lie back to back
    std::vector<uint64_t> back((back_bytes + 7) / 8);
    HIP_TRY(hipMemcpyAsync(back.data(), g->sp_buf, back_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint32_t *h_ctl = reinterpret_cast<const uint32_t *>(back.data() + path_words);
    for (uint32_t q = 0; q < b; ++q) {
        out_lens[q] = h_ctl[q];
        out_status[q] = h_ctl[b + q];
        memcpy(out_paths + (size_t)q * (max_depth + 1u), back.data() + (size_t)q * (max_depth + 1u), (size_t)out_lens[q] * 8);
        if (out_level_sizes)
            for (uint32_t i = 0; i < max_depth; ++i) out_level_sizes[(size_t)q * max_depth + i] = h_ctl[2 * (size_t)b + (size_t)q * max_depth + i];
    }
    return HVX_OK;
}

extern "C" int hvx_shortest_path_host(uint64_t n_nodes, uint64_t n_edges, const uint64_t *out_offsets, const uint64_t *out_targets,
                                      const uint32_t *edge_labels, uint64_t source, uint64_t target, uint32_t max_depth, uint32_t direction,
                                      const uint32_t *allowed_label_ids, uint32_t n_labels, uint64_t *out_path, uint32_t *out_len) {
    if (!out_offsets || (n_edges && !out_targets) || !out_path || !out_len) return fail(HVX_ERR_INVARIANT, "null argument");
    *out_len = 0;
    int rc = shortest_path_plan_check(max_depth, direction, allowed_label_ids, n_labels);
    if (rc) return rc;
    for (const uint64_t v : {source, target})
        if (v >= n_nodes && v != UINT64_MAX) return fail(HVX_ERR_INVARIANT, "unknown node %llu", (unsigned long long)v);
    hvx_sp::HostGraph g;
    if (const uint64_t bad = hvx_sp::build_incoming(n_nodes, n_edges, out_offsets, out_targets, edge_labels, &g))
        return fail(HVX_ERR_INVARIANT, "the arrays are no CSR of %llu nodes (arc %llu)", (unsigned long long)n_nodes, (unsigned long long)(bad - 1));
    if (source == UINT64_MAX || target == UINT64_MAX) return HVX_OK;
    const std::vector<uint64_t> path = hvx_sp::shortest_path(g, source, target, max_depth, direction, allowed_label_ids, n_labels);
    // (a path has at most max_depth + 1 nodes)
    if (!path.empty()) memcpy(out_path, path.data(), path.size() * 8);
    *out_len = (uint32_t)path.size();
    return HVX_OK;
}
