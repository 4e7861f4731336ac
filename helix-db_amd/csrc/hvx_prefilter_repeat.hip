// hvx_prefilter_repeat.hip -- repeat(expand).times(n).emit() for a BATCH of requests, every request from its own start nodes
// (hvx_expand_repeat_lists / hvx_prefilter_repeat_search_lists_params; the entry points live in hvx_prefilter.hip, the graph handle in hvx_csr.h, the row walker and the node set in hvx_csr_dev.h).
//
// Reference: g().n(user).repeat(out("follows")).times(3).emit().vector_search(..) runs once per request; the loop is
// crates/db/src/execution/interpreter/control/repeat.rs:24-99.  On sets, per request:
//   cur = the distinct seeds; emitted = {}
//   for i in 1 .. times:  BEFORE / ALL: emitted |= cur;  nxt = N(cur);  AFTER / ALL: emitted |= nxt;  stop = nxt meets `until`;
//                         cur = nxt;  if cur is empty or stop: break
// N(.) has no visited exclusion.  The kernel computes the same sets as a breadth-first walk WITH exclusion (DESIGN 4.4d has the argument,
// tests/test_prefilter_repeat_host.py holds the literal loop, tests/test_gpu_prefilter_repeat.py compares):
//   * ONE visited set per request, never cleared between the iterations; iteration i expands only the nodes first reached at i - 1.
//   * BEFORE / ALL insert the distinct seeds first (level 0, duplicates collapse there).  AFTER does not: a seed that an arc reaches is
//     emitted -- and expanded once more -- when it is reached.
//   * AFTER / ALL emit a node when it is first inserted (ALL: the seeds as well); BEFORE emits a level's list when that level is expanded.
//   * `until` is tested on EVERY arc target of the expanded nodes, fresh or not: a pre-inserted seed that comes back must stop the loop.
//     The iteration in which it fires completes; then the loop ends.
// The kernel has path_lists_kernel's shape (hvx_prefilter_batch.hip): one launch, one 1 024-thread workgroup per request, the visited set an
// open-addressing u32 hash set in dynamic LDS (atomicCAS per probe, linear probing, empty = 0xFFFFFFFF), slots = a power of two >= 2 x
// max_frontier and >= 4 096 (at most 128 KiB + 128 bytes of control words), level lists ping-pong between two HBM slots of max_frontier u32
// per request, rows of at most 16 arcs by their own lane and longer ones by a wavefront, append positions by ballot + popcount with one LDS
// counter update per wavefront step.  A wavefront looks at the set's size before every step, so at most 16 x 64 insertions are in flight
// when the size crosses max_frontier and the table cannot fill.  The workgroup that writes a level list is the one that reads it: the
// workgroup barrier orders that, there is no agent-scope fence or atomic.
// max_frontier bounds the REACH set (what the table holds): the first iteration that outgrows it ends the request with
// HVX_ERR_CANDIDATE_LIMIT, length 0, that iteration's size max_frontier + 1, later ones 0 and stop depth 0.
// The kernel is latency-bound (dependent offset -> target -> LDS probe chains), not HBM-bound.
#include <hip/hip_runtime.h>

#include "hvx_csr_dev.h"
#include "hvx_host.h"

using namespace hvx;

namespace {

// LDS control words in front of the table: [0] nodes in the visited set, [1] ids written behind the mask, [2] `until` fired, [8 ..) sizes
__global__ __launch_bounds__(1024) void repeat_lists_kernel(RepeatListsArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *ctl = reinterpret_cast<uint32_t *>(smem);
    const LdsNodeSet set{ctl + kNodeSetCtlWords, a.slots, a.hash_shift};
    const uint32_t q = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t mf = a.max_frontier;
    const bool emit_before = a.emit == (uint32_t)HVX_REPEAT_EMIT_BEFORE, emit_after = a.emit == (uint32_t)HVX_REPEAT_EMIT_AFTER;
    auto room = [&]() __attribute__((always_inline)) -> bool { return !LdsNodeSet::over(&ctl[0], mf); };

    unsigned long long *ids_out = a.out_ids + (size_t)q * mf;
    // one emitted node of every lane into the scan's slot, behind the mask.  `pos` = its place when nothing filters and the caller has one
    // (the node's number in the visited set); `counted`: take the place from the slot's own counter whatever the mask
    auto put = [&](bool keep, uint32_t v, uint32_t pos, bool counted) __attribute__((always_inline)) {
        if (a.mask) keep = keep && ((a.mask[v >> 5] >> (v & 31u)) & 1u) != 0u;
        if (a.mask || counted) {
            const WavePlace p = wave_append(keep, &ctl[1], lane);
            if (!p.any) return;
            pos = p.pos;
        }
        if (keep && pos < mf) ids_out[pos] = (unsigned long long)v;
    };
    // one node of every lane: fresh ones take a place in the level under construction (`r0` = the set's size when the level began)
    auto take = [&](bool valid, uint32_t v, uint32_t *dst, uint32_t r0, bool emit_fresh) __attribute__((always_inline)) {
        const bool fresh = valid && set.insert(v);
        const WavePlace p = wave_append(fresh, &ctl[0], lane);
        if (!p.any) return;
        const uint32_t idx = p.pos;
        if (fresh && idx < mf) dst[idx - r0] = v; // (idx >= r0: the counter only grows)
        if (emit_fresh) put(fresh, v, idx, false);
    };

    if (tid < kNodeSetCtlWords) ctl[tid] = 0u;
    set.clear(tid); // once: the set lives as long as the request
    __syncthreads();
    const uint32_t s0 = a.seed_off[q];
    uint32_t n_cur = a.seed_off[q + 1] - s0; // (the host has seen it at most max_frontier)
    const uint32_t *cur = a.seeds + s0;
    uint32_t *slot[2] = {a.front + (size_t)q * 2u * mf, a.front + (size_t)q * 2u * mf + mf};
    uint32_t r0 = 0; // nodes in the visited set when the current level was complete
    if (!emit_after) {
        // level 0 = the distinct seeds (at most max_frontier of them: this pass cannot overflow); ALL emits them here
        for (uint32_t c0 = 0; c0 < n_cur; c0 += 1024u) {
            const bool have = c0 + tid < n_cur;
            take(have, have ? cur[c0 + tid] : 0u, slot[1], 0u, !emit_before);
        }
        __syncthreads();
        r0 = ctl[0];
        __syncthreads();
        cur = slot[1];
        n_cur = r0;
    }

    bool overflow = false;
    uint32_t ran = 0, final_size = 0, stop_depth = 0;
    for (uint32_t it = 0; it < a.times && n_cur != 0u; ++it) {
        uint32_t *dst = slot[it & 1u];
        bool hit = false;
        // one arc of every lane
        auto arc = [&](bool active, const uint32_t *tgt, const uint32_t *lab, uint64_t at) __attribute__((always_inline)) {
            uint32_t v = 0;
            bool valid = false;
            if (active && (!lab || label_ok(lab[at], a.allowed, a.n_allowed))) {
                v = tgt[at];
                valid = true;
                if (a.until) hit = hit || ((a.until[v >> 5] >> (v & 31u)) & 1u) != 0u; // every target, fresh or not
            }
            take(valid, v, dst, r0, !emit_before);
        };
        for (uint32_t c0 = 0; c0 < n_cur; c0 += 1024u) {
            const bool have = c0 + tid < n_cur;
            const uint32_t node = have ? cur[c0 + tid] : 0u;
            if (emit_before) put(have, node, 0u, true); // the level is emitted as it is expanded
            // walk_rows_per_wave's loop, kept in the kernel: passed through that helper it costs this kernel 6 more SGPR spills
            for (int pass = 0; pass < 2; ++pass) {
                AdjRow r;
                if (!adj_pass(a.g, a.direction, pass, have, node, &r)) continue;
                const bool light = r.deg <= kLightRow;
                const uint32_t steps = wave_max(light ? r.deg : 0u);
                for (uint32_t i = 0; i < steps && room(); ++i) arc(light && i < r.deg, r.tgt, r.lab, r.a0 + i);
                walk_heavy_rows(have && !light, r.a0, r.deg, room, [&](bool active, uint64_t at) __attribute__((always_inline)) { arc(active, r.tgt, r.lab, at); });
            }
        }
        if (hit) ctl[2] = 1u;
        __syncthreads(); // the iteration's level is complete, its list visible to the whole workgroup
        const uint32_t reach = ctl[0];
        const bool stop = ctl[2] != 0u;
        __syncthreads(); // (every thread has read both before the next iteration moves them)
        overflow = reach > mf;
        ran = it + 1u;
        // |emitted| after this iteration: BEFORE has emitted the levels up to the one just expanded, AFTER / ALL everything reached
        const uint32_t size = emit_before ? r0 : reach;
        if (tid == 0) ctl[8 + it] = overflow ? mf + 1u : size;
        if (overflow) break; // (uniform: every thread read the same words between the two barriers)
        final_size = size;
        if (stop) { stop_depth = it + 1u; break; }
        cur = dst;
        n_cur = reach - r0; // an empty new level ends the loop
        r0 = reach;
    }
    __syncthreads();
    // iterations the loop never ran keep the size at its end; after an overflow they report 0
    if (tid < a.times) a.emit_sizes[(size_t)q * 16u + tid] = tid < ran ? ctl[8 + tid] : (overflow ? 0u : final_size);
    if (tid == 0) {
        // AFTER / ALL without a mask placed every id by its number in the visited set; the other forms counted in ctl[1]
        a.lens[q] = overflow ? 0u : ((a.mask || emit_before) ? ctl[1] : ctl[0]);
        a.status[q] = overflow ? (uint32_t)HVX_ERR_CANDIDATE_LIMIT : (uint32_t)HVX_OK;
        a.stop_depth[q] = overflow ? 0u : stop_depth;
    }
}

} // namespace

namespace hvx {

hipError_t launch_repeat_lists(const RepeatListsArgs &args, uint32_t b, hipStream_t s) { return launch_node_set_kernel(repeat_lists_kernel, args, b, s); }

} // namespace hvx
