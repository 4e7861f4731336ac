// hvx_shortest_path_dense.hip -- shortest_path for a BATCH of requests whose backward reach may be the whole graph
// (hvx_shortest_path_batch_dense): the sibling of hvx_shortest_path.hip without max_reach.
//
// The requests of a batch share direction, allow-set and max_depth, and only every node's LEVEL from the target matters for the reference's
// path (hvx_shortest_path.hip).  So the levels of 64 requests are found by ONE bit-parallel sweep: request q of a group is bit
// q of a u64 word per node.  Per group and node the scratch holds three words -- seen (reached so far), cur (reached in the last level),
// next (being reached) -- and 64 level bytes, which are never cleared: a byte is read only behind its seen bit.  Groups run in rounds of as
// many as the scratch budget holds (hvx_shortest_path_dense_plan.h); one launch serves every group of a round (blockIdx.y).
//   init     clear the words; per request set its bit in seen and cur at its target, level byte 0, its bit in the group's `active` word
//   per level, three launches back to back:
//     push   every node u with cur[u] & active walks its rows in the mirrored direction; per allowed arc to v the bits v has not seen
//            are OR-ed into next[v] (relaxed agent-scope fetch-or, result unused).  seen does not change in this launch.
//     commit per node w = next & ~seen & active; seen |= w, cur = w, next = 0, a level byte per bit of w; the OR of all w and (when sizes
//            are asked for) the per-request counts are reduced per wavefront, then per workgroup in LDS: one atomic per word and workgroup
//     check  per request, in this order: its bit in cur[source] = found at this level; its bit missing in `grew` = no path; either way it
//            leaves `active`.  A request still active sets a pinned word the host reads after a run of kRun levels.
//   walk out one workgroup per request: hvx_shortest_path.hip's Phase B over seen and the level bytes.
// Kernel boundaries on one stream are the only ordering between workgroups: no spin, no cooperative launch, no fence.  A launch whose group
// has nothing active returns at once.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "hvx_csr.h"
#include "hvx_shortest_path_dense_plan.h"

using namespace hvx;

namespace {

constexpr uint32_t kNoNode = 0xFFFFFFFFu; // an endpoint that resolved to nothing; also "no candidate" in the walk out
constexpr uint32_t kMaxBatch = 65535;
constexpr uint32_t kMaxDepth = 255;       // a level is a byte
// Levels enqueued between two host looks at the pinned word.  A level is three launches (~4 us each when its groups have ended, since they
// return at once); a host wait costs about as much as a run of four such levels, so a batch that ends early wastes at most one wait's worth
// of empty launches and a batch that runs to max_depth waits ceil(max_depth / 4) times instead of max_depth times.
constexpr uint32_t kRun = 4;
constexpr uint32_t kMaxRuns = (kMaxDepth + kRun - 1) / kRun;

typedef unsigned long long u64w;

struct DenseArgs {
    CsrView g;
    uint32_t max_depth, direction, n_allowed;
    const uint32_t *allowed;          // (n_allowed == 0: every label)
    uint32_t request0, n_requests;    // the round's requests within the batch
    uint32_t group0, groups;          // the round's first group; groups of the whole batch
    uint32_t level;                   // the level this launch produces (push, commit, check)
    uint32_t want_sizes;
    u64w *seen, *cur, *next;          // [groups of the round][n]
    uint8_t *lvl;                     // [groups of the round][n][64]
    const uint32_t *src, *dst;        // [b]; 0xFFFFFFFF = the endpoint resolved to no node
    uint32_t *dist, *cnt, *ran;       // [b] arcs of the path (0: none), nodes reached, levels the request was active in
    u64w *active, *grew;              // [groups], [2][groups] (by level parity: check clears the other one)
    uint32_t *still;                  // nullable, pinned: someone is still active after this level
    u64w *out_paths;                  // [b][max_depth + 1]
    uint32_t *lens, *status, *level_sizes; // [b], [b], [b][max_depth]
};

__global__ __launch_bounds__(256) void sp_dense_init_kernel(DenseArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_requests) return;
    const uint32_t q = a.request0 + i, gl = i >> 6;
    const u64w bit = 1ull << (i & 63u);
    const uint32_t src = a.src[q], dst = a.dst[q];
    const bool none = src == kNoNode || dst == kNoNode;
    a.dist[q] = 0u;
    a.ran[q] = 0u;
    a.cnt[q] = none ? 0u : 1u; // the target alone
    if (none || src == dst) return;
    const size_t at = (size_t)gl * a.g.n + dst;
    atomicOr(&a.seen[at], bit); // targets repeat within a group
    atomicOr(&a.cur[at], bit);
    a.lvl[at * 64u + (i & 63u)] = 0;
    atomicOr(&a.active[a.group0 + gl], bit);
}

__device__ __forceinline__ u64w readlane64(u64w x, int l) {
    return ((u64w)(uint32_t)__builtin_amdgcn_readlane((int)(x >> 32), l) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, l);
}

__global__ __launch_bounds__(256) void sp_dense_push_kernel(DenseArgs a) {
    const uint32_t gl = blockIdx.y, lane = threadIdx.x & 63u;
    const u64w act = a.active[a.group0 + gl];
    if (act == 0ull) return; // (uniform) every request of the group has ended
    const uint32_t n = a.g.n, node = blockIdx.x * 256u + threadIdx.x;
    const u64w *seen = a.seen + (size_t)gl * n;
    u64w *next = a.next + (size_t)gl * n;
    const u64w w = node < n ? a.cur[(size_t)gl * n + node] & act : 0ull;
    const bool have = w != 0ull;
    if (__ballot(have) == 0ull) return; // (per wavefront; there is no barrier below)
    const uint32_t back = a.direction == (uint32_t)HVX_DIR_OUT ? (uint32_t)HVX_DIR_IN : a.direction == (uint32_t)HVX_DIR_IN ? (uint32_t)HVX_DIR_OUT : (uint32_t)HVX_DIR_BOTH;
    auto always = []() __attribute__((always_inline)) -> bool { return true; };
    // one arc per lane; `word` is the frontier word of the node whose row the arc belongs to
    auto relax = [&](bool on, const uint32_t *tgt, const uint32_t *lab, uint64_t at, u64w word) __attribute__((always_inline)) {
        if (!on || (lab && !label_ok(lab[at], a.allowed, a.n_allowed))) return;
        const uint32_t v = tgt[at];
        const u64w add = word & ~seen[v]; // exact: seen does not change during this launch
        if (add != 0ull) (void)__hip_atomic_fetch_or(&next[v], add, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    for (int pass = 0; pass < 2; ++pass) {
        AdjRow r;
        if (!adj_pass(a.g, back, pass, have, node, &r)) continue;
        const bool light = r.deg <= kLightRow;
        // the light rows by their own lanes, one arc per step (walk_rows_per_wave's loop: its long rows would lose the row's word) ...
        const uint32_t steps = wave_max(light ? r.deg : 0u);
        for (uint32_t i = 0; i < steps; ++i) relax(light && i < r.deg, r.tgt, r.lab, r.a0 + i, w);
        // ... the long ones by the whole wavefront, one row at a time with its node's word broadcast
        unsigned long long heavy = __ballot(have && !light);
        while (heavy) {
            const int l = __builtin_ctzll(heavy);
            heavy &= heavy - 1ull;
            const u64w wl = readlane64(w, l);
            walk_heavy_rows((int)lane == l, r.a0, r.deg, always, [&](bool on, uint64_t at) __attribute__((always_inline)) { relax(on, r.tgt, r.lab, at, wl); });
        }
    }
}

__global__ __launch_bounds__(1024) void sp_dense_commit_kernel(DenseArgs a) {
    __shared__ uint32_t s_cnt[64];
    __shared__ u64w s_or;
    const uint32_t gl = blockIdx.y, tid = threadIdx.x, lane = tid & 63u;
    const u64w act = a.active[a.group0 + gl];
    if (act == 0ull) return; // (uniform)
    if (tid < 64u) s_cnt[tid] = 0u;
    if (tid == 64u) s_or = 0ull;
    __syncthreads();
    const uint32_t n = a.g.n, v = blockIdx.x * 1024u + tid;
    u64w w = 0ull;
    if (v < n) {
        const size_t at = (size_t)gl * n + v;
        const u64w nx = a.next[at];
        if (nx != 0ull) {
            const u64w sn = a.seen[at];
            w = nx & ~sn & act;
            a.next[at] = 0ull;
            if (w != 0ull) a.seen[at] = sn | w;
        }
        a.cur[at] = w;
        uint8_t *lv = a.lvl + at * 64u;
        for (u64w m = w; m != 0ull; m &= m - 1ull) lv[__builtin_ctzll(m)] = (uint8_t)a.level;
    }
    u64w any = w;
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)any, sh, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(any >> 32), sh, 64);
        any |= ((u64w)hi << 32) | lo;
    }
    if (any != 0ull) { // (per wavefront)
        if (lane == 0) atomicOr(&s_or, any);
        if (a.want_sizes)
            for (u64w m = any; m != 0ull; m &= m - 1ull) {
                const int q = __builtin_ctzll(m);
                const uint32_t c = (uint32_t)__builtin_popcountll(__ballot((w >> q) & 1ull));
                if (lane == 0) atomicAdd(&s_cnt[q], c);
            }
    }
    __syncthreads();
    if (tid < 64u && s_cnt[tid] != 0u) atomicAdd(&a.cnt[a.request0 + gl * 64u + tid], s_cnt[tid]); // (a bit past the batch's end is never active)
    if (tid == 64u && s_or != 0ull) atomicOr(&a.grew[(size_t)(a.level & 1u) * a.groups + a.group0 + gl], s_or);
}

__global__ __launch_bounds__(256) void sp_dense_check_kernel(DenseArgs a) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= a.n_requests) return;
    const uint32_t q = a.request0 + i, gl = i >> 6, group = a.group0 + gl;
    if ((i & 63u) == 0u) a.grew[(size_t)((a.level + 1u) & 1u) * a.groups + group] = 0ull; // the word the next level's commit ORs into
    const u64w bit = 1ull << (i & 63u);
    if ((a.active[group] & bit) == 0ull) return; // (only this thread ever clears this bit)
    const bool found = (a.cur[(size_t)gl * a.g.n + a.src[q]] & bit) != 0ull;
    const bool grew = (a.grew[(size_t)(a.level & 1u) * a.groups + group] & bit) != 0ull;
    a.ran[q] = a.level;
    if (a.want_sizes) a.level_sizes[(size_t)q * a.max_depth + (a.level - 1u)] = a.cnt[q];
    if (found) a.dist[q] = a.level; // found before empty: the level that reaches the source completes
    if (found || !grew) atomicAnd(&a.active[group], ~bit);
    else if (a.still) *a.still = 1u;
}

// LDS: the minimum of the step (steps alternate between two words)
__global__ __launch_bounds__(1024) void sp_dense_walk_out_kernel(DenseArgs a) {
    __shared__ uint32_t s_min[2];
    const uint32_t i = blockIdx.x, tid = threadIdx.x, lane = tid & 63u;
    const uint32_t q = a.request0 + i, gl = i >> 6, bitno = i & 63u, md = a.max_depth;
    const uint32_t src = a.src[q], dst = a.dst[q], dist = a.dist[q];
    u64w *path = a.out_paths + (size_t)q * (md + 1u);
    if (a.want_sizes) { // levels the request was not active in keep the size at its loop's end
        const uint32_t reach = a.cnt[q];
        for (uint32_t k = a.ran[q] + tid; k < md; k += 1024u) a.level_sizes[(size_t)q * md + k] = reach;
    }
    if (dist == 0u) { // (uniform) no path, a sentinel, or source == target
        if (tid == 0) {
            const uint32_t same = (src == dst && src != kNoNode) ? 1u : 0u;
            if (same) path[0] = (u64w)src;
            a.lens[q] = same;
            a.status[q] = (uint32_t)HVX_OK;
        }
        return;
    }
    const u64w *seen = a.seen + (size_t)gl * a.g.n;
    const uint8_t *lvl = a.lvl + (size_t)gl * a.g.n * 64u;
    if (tid < 2u) s_min[tid] = kNoNode;
    __syncthreads();
    bool broken = false;
    uint32_t c = src;
    for (uint32_t step = 0; step < dist; ++step) {
        if (tid == 0) path[step] = (u64w)c;
        const uint32_t want = dist - 1u - step;
        uint32_t best = kNoNode;
        for (int pass = 0; pass < 2; ++pass) {
            AdjRow r;
            if (!adj_pass(a.g, a.direction, pass, true, c, &r)) continue;
            for (uint64_t j = tid; j < r.deg; j += 1024u) {
                const uint64_t at = r.a0 + j;
                if (r.lab && !label_ok(r.lab[at], a.allowed, a.n_allowed)) continue;
                const uint32_t v = r.tgt[at];
                if (v >= best) continue;
                if (((seen[v] >> bitno) & 1ull) && lvl[(size_t)v * 64u + bitno] == (uint8_t)want) best = v;
            }
        }
#pragma unroll
        for (int sh = 32; sh > 0; sh >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)best, sh, 64); best = o < best ? o : best; }
        uint32_t *mn = &s_min[step & 1u];
        if (lane == 0 && best != kNoNode) atomicMin(mn, best);
        __syncthreads();
        const uint32_t nxt = *mn;
        if (tid == 0) s_min[(step + 1u) & 1u] = kNoNode; // the other word: last read before the previous step's second barrier
        __syncthreads();
        if (nxt >= a.g.n) { broken = true; break; } // (uniform; a node at level k > 0 has an arc to level k - 1, so this does not happen)
        c = nxt;
    }
    if (tid == 0) {
        if (!broken) path[dist] = (u64w)c;
        a.lens[q] = broken ? 0u : dist + 1u;
        a.status[q] = broken ? (uint32_t)HVX_ERR_INVARIANT : (uint32_t)HVX_OK;
    }
}

} // namespace

extern "C" int hvx_shortest_path_batch_dense(const hvx_csr *cg, uint32_t b, const uint64_t *sources, const uint64_t *targets, uint32_t max_depth,
                                             uint32_t direction, const uint32_t *allowed_label_ids, uint32_t n_labels, uint64_t scratch_bytes,
                                             uint64_t *out_paths, uint32_t *out_lens, uint32_t *out_status, uint64_t *out_level_sizes) {
    if (!cg || !out_paths || !out_lens || !out_status || (b && (!sources || !targets))) return fail(HVX_ERR_INVARIANT, "null argument");
    hvx_csr *g = const_cast<hvx_csr *>(cg);
    int rc = shortest_path_plan_check(max_depth, direction, allowed_label_ids, n_labels);
    if (rc) return rc;
    if (max_depth > kMaxDepth) return fail(HVX_ERR_UNSUPPORTED, "shortest_path on the device searches at most %u levels, not %u", kMaxDepth, max_depth);
    if (b > kMaxBatch) return fail(HVX_ERR_UNSUPPORTED, "a batch of shortest-path requests holds at most %u", kMaxBatch);
    for (uint32_t q = 0; q < b; ++q)
        for (const uint64_t v : {sources[q], targets[q]})
            if (v >= g->n && v != UINT64_MAX) return fail(HVX_ERR_INVARIANT, "unknown node %llu in request %u", (unsigned long long)v, q);
    if (b == 0) return HVX_OK;
    hvx_spd::RoundPlan plan;
    if (!hvx_spd::plan_rounds(g->n, b, scratch_bytes, &plan))
        return fail(HVX_ERR_UNSUPPORTED, "scratch_bytes %llu does not hold one group of 64 requests: %llu nodes x %llu bytes", (unsigned long long)scratch_bytes,
                    (unsigned long long)g->n, (unsigned long long)hvx_spd::kNodeGroupBytes);

    std::lock_guard<std::mutex> lock(g->mu);
    HIP_TRY(hipSetDevice(g->device));
    hipStream_t s = g->stream;
    // pinned: [b] sources | [b] targets | [kMaxRuns] "someone is still active" words, one per run of a round
    if ((rc = seeds_reserve(g, 2 * (size_t)b + kMaxRuns, nullptr))) return rc;
    uint32_t *h_src = g->h_seeds, *h_dst = g->h_seeds + b, *h_still = g->h_seeds + 2 * (size_t)b;
    for (uint32_t q = 0; q < b; ++q) {
        h_src[q] = sources[q] == UINT64_MAX ? kNoNode : (uint32_t)sources[q];
        h_dst[q] = targets[q] == UINT64_MAX ? kNoNode : (uint32_t)targets[q];
    }
    if ((rc = upload_labels(g, allowed_label_ids, n_labels, s))) return rc;
    // [b][max_depth + 1] u64 paths | [b] lengths | [b] statuses | [b][max_depth] sizes || [b] x 5 request words | [groups] active | [2][groups] grew || the round
    const size_t path_words = (size_t)b * (max_depth + 1u), ctl_words = (size_t)b * (2u + max_depth), back_bytes = path_words * 8 + ctl_words * 4;
    const size_t req_off = (back_bytes + 7) / 8 * 8, group_off = (req_off + (size_t)b * 5 * 4 + 7) / 8 * 8;
    const size_t round_off = (group_off + (size_t)plan.groups * 3 * 8 + 255) / 256 * 256;
    if ((rc = csr_reserve(g, &g->spd_buf, &g->spd_cap, round_off + (size_t)plan.bytes))) return rc;
    char *base = static_cast<char *>(g->spd_buf);
    DenseArgs a;
    memset(&a, 0, sizeof(a));
    a.g = csr_view(g);
    a.max_depth = max_depth; a.direction = direction; a.n_allowed = n_labels;
    a.allowed = g->labels;
    a.groups = (uint32_t)plan.groups;
    a.want_sizes = out_level_sizes ? 1u : 0u;
    a.out_paths = reinterpret_cast<u64w *>(base);
    uint32_t *ctl = reinterpret_cast<uint32_t *>(a.out_paths + path_words);
    a.lens = ctl; a.status = ctl + b; a.level_sizes = ctl + 2 * (size_t)b;
    uint32_t *req = reinterpret_cast<uint32_t *>(base + req_off);
    a.src = req; a.dst = req + b; a.dist = req + 2 * (size_t)b; a.cnt = req + 3 * (size_t)b; a.ran = req + 4 * (size_t)b;
    a.active = reinterpret_cast<u64w *>(base + group_off);
    a.grew = a.active + plan.groups;
    a.seen = reinterpret_cast<u64w *>(base + round_off + plan.seen_off);
    a.lvl = reinterpret_cast<uint8_t *>(base + round_off + plan.lvl_off);
    HIP_TRY(hipMemcpyAsync(req, h_src, 2 * (size_t)b * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(a.active, 0, (size_t)plan.groups * 3 * 8, s));

    auto failed = [&](const char *what) {
        const hipError_t e = hipGetLastError();
        if (e == hipSuccess) return false;
        (void)hipStreamSynchronize(s);
        fail(HVX_ERR_DEVICE, "%s: %s", what, hipGetErrorString(e));
        return true;
    };
    std::vector<uint64_t> back((back_bytes + 7) / 8);
    for (uint64_t r = 0; r < plan.rounds; ++r) {
        const hvx_spd::Round rd = hvx_spd::round_of(plan, b, r);
        a.request0 = rd.request0; a.n_requests = rd.n_requests; a.group0 = (uint32_t)rd.group0;
        bool live = false; // a request of the round searches at all
        for (uint32_t q = rd.request0; q < rd.request0 + rd.n_requests && !live; ++q) live = h_src[q] != kNoNode && h_dst[q] != kNoNode && h_src[q] != h_dst[q];
        const dim3 per_request((rd.n_requests + 255u) / 256u);
        // the three word arrays of the round's groups lie back to back at the front of the plan's word area (a last, shorter round uses less of it)
        const size_t words = (size_t)g->n * rd.n_groups;
        a.cur = a.seen + words; a.next = a.cur + words;
        if (live) HIP_TRY(hipMemsetAsync(a.seen, 0, words * 24, s));
        a.level = 0; a.still = nullptr;
        hipLaunchKernelGGL(sp_dense_init_kernel, per_request, dim3(256), 0, s, a);
        if (failed("sp_dense_init_kernel")) return HVX_ERR_DEVICE;
        memset(h_still, 0, kMaxRuns * 4); // (every launch that wrote them has been waited for)
        uint32_t level = 0, run = 0;
        while (live && level < max_depth) {
            const uint32_t end = level + kRun < max_depth ? level + kRun : max_depth;
            while (level < end) {
                a.level = ++level;
                a.still = (level == end && end < max_depth) ? h_still + run : nullptr;
                hipLaunchKernelGGL(sp_dense_push_kernel, dim3((g->n + 255u) / 256u, (uint32_t)rd.n_groups), dim3(256), 0, s, a);
                hipLaunchKernelGGL(sp_dense_commit_kernel, dim3((g->n + 1023u) / 1024u, (uint32_t)rd.n_groups), dim3(1024), 0, s, a);
                hipLaunchKernelGGL(sp_dense_check_kernel, per_request, dim3(256), 0, s, a);
            }
            if (failed("shortest-path sweep")) return HVX_ERR_DEVICE;
            if (level == max_depth) break;
            HIP_TRY(hipStreamSynchronize(s));
            live = h_still[run++] != 0u;
        }
        hipLaunchKernelGGL(sp_dense_walk_out_kernel, dim3(rd.n_requests), dim3(1024), 0, s, a);
        if (failed("sp_dense_walk_out_kernel")) return HVX_ERR_DEVICE;
        // one copy back behind the last round: the paths and the control words lie back to back
        if (r + 1 == plan.rounds) HIP_TRY(hipMemcpyAsync(back.data(), g->spd_buf, back_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s)); // at most ceil(max_depth / kRun) + 1 waits a round
    }
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
