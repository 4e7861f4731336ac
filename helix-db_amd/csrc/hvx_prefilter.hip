// hvx_prefilter.hip -- the restricted (prefiltered) vector search entry point and the fused prefilter searches: candidate bitmap ->
// row list pipeline, one-hop expand, chains of hops, per-query chains and repeats.  The graph handle is hvx_csr.h, the traversals
// hvx_traverse.hip, the shared device pieces hvx_csr_dev.h.
//
// Reference: crates/db/src/execution/interpreter/access/expand.rs:16-80,
// crates/db/src/search/vector/restricted.rs:196-260,303-371,426-453,529-613,753-835.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "hvx_csr.h"

using namespace hvx;

// ---------------------------------------------------------------------------------------------
// Restricted (prefiltered) search: search_restricted_observed_with_beam_percent
// (restricted.rs:529-613).  Plan `Exact` is the reference's restricted_exact_scan; candidate sets
// above the exact thresholds are ALSO scanned exactly on the device (a gathered flat scan over the
// allowed rows): on MI355X a 100k x 1536 f32 candidate set is 0.6 GB = ~0.1 ms of HBM, and the
// result is the exact answer that the reference's ACORN-style walk (restricted.rs:837-1148)
// approximates (recall gate >= 0.92/0.95).  See DESIGN.md "restricted search".
// ---------------------------------------------------------------------------------------------
extern "C" int hvx_search_restricted_batch(const hvx_index *cix, const float *queries, uint32_t b, uint32_t k,
                                           uint32_t ef, const uint64_t *allowed_ids, const uint64_t *allowed_offsets,
                                           uint64_t n_allowed, uint64_t *out_ids, float *out_scores,
                                           uint32_t *out_counts, uint32_t *out_status, hvx_stats *stats) {
    if (!cix) return fail(HVX_ERR_INVARIANT, "null index");
    hvx_index *ix = const_cast<hvx_index *>(cix);
    if (k == 0) return fail(HVX_ERR_K_RANGE, "result count must be non-zero");
    if (ef < k) return fail(HVX_ERR_K_RANGE, "search beam width %u is below the result count %u", ef, k);
    if (b == 0) return HVX_OK;
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->sync_rewrites();
    HIP_TRY(hipSetDevice(ix->device));
    hvx_restricted_params rp; // this entry point answers every candidate-set size with the exact gathered scan
    memset(&rp, 0, sizeof(rp));
    rp.k = k;
    rp.ef = ef;
    rp.strategy = HVX_RESTRICTED_EXACT;
    return restricted_search_host(ix, queries, b, rp, allowed_ids, allowed_offsets, n_allowed, out_ids, out_scores, out_counts, out_status, nullptr, stats);
}

// ---------------------------------------------------------------------------------------------
// Fused prefilter + restricted kNN: the candidate bitmap never leaves the device.
// ---------------------------------------------------------------------------------------------
namespace {

// external node id -> internal row of the index (ids ascending), kSentinel when the node holds no vector
// (or whose vector has been deleted: `dead` = the image's deleted-row bitmap, NULL while nothing has been deleted)
__device__ __forceinline__ uint32_t find_row(const uint64_t *ids, uint32_t n, uint64_t id, bool contiguous, const uint32_t *dead) {
    if (n == 0) return kSentinel;
    uint32_t row;
    if (contiguous) {
        if (!(id >= ids[0] && id - ids[0] < n)) return kSentinel;
        row = (uint32_t)(id - ids[0]);
    } else {
        uint32_t lo = 0, hi = n;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (ids[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        if (!(lo < n && ids[lo] == id)) return kSentinel;
        row = lo;
    }
    if (dead && ((dead[row >> 5] >> (row & 31u)) & 1u)) return kSentinel;
    return row;
}

// pass 1: per 256-word block, how many set bits map to an indexed row (restricted.rs:615-659: ids that are not
// indexed are omitted) and how many bits are set at all (the RestrictedVectorCandidates population, :356-371)
__global__ __launch_bounds__(256) void bitmap_count_kernel(const uint32_t *bitmap, uint32_t n_words, const uint64_t *ids, uint32_t n,
                                                           uint32_t contiguous, const uint32_t *dead, uint32_t *block_rows, uint32_t *total_bits, uint32_t *block_bits) {
    __shared__ uint32_t s_rows, s_bits;
    if (threadIdx.x == 0) { s_rows = 0; s_bits = 0; }
    __syncthreads();
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    uint32_t word = w < n_words ? bitmap[w] : 0u, rows = 0;
    const uint32_t bits = (uint32_t)__builtin_popcount(word);
    while (word) {
        const uint32_t b = (uint32_t)__builtin_ctz(word);
        word &= word - 1u;
        rows += find_row(ids, n, (uint64_t)w * 32u + b, contiguous != 0u, dead) != kSentinel ? 1u : 0u;
    }
    if (rows) atomicAdd(&s_rows, rows);
    if (bits) atomicAdd(&s_bits, bits);
    __syncthreads();
    if (threadIdx.x == 0) {
        block_rows[blockIdx.x] = s_rows;
        if (block_bits) block_bits[blockIdx.x] = s_bits; // for the deterministic sample: ranks count every candidate id
        if (s_bits) atomicAdd(total_bits, s_bits);
    }
}

// exclusive scan of the block counts (one block; n_blocks <= a few thousand), total into block_rows[n_blocks]
__global__ __launch_bounds__(1024) void block_scan_kernel(uint32_t *block_rows, uint32_t n_blocks) {
    __shared__ uint32_t part[1024];
    const uint32_t per = (n_blocks + 1023u) / 1024u, t = threadIdx.x;
    uint32_t sum = 0;
    for (uint32_t i = t * per; i < (t + 1) * per && i < n_blocks; ++i) sum += block_rows[i];
    part[t] = sum;
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (uint32_t i = 0; i < 1024; ++i) { const uint32_t v = part[i]; part[i] = run; run += v; }
        block_rows[n_blocks] = run;
    }
    __syncthreads();
    uint32_t run = part[t];
    for (uint32_t i = t * per; i < (t + 1) * per && i < n_blocks; ++i) { const uint32_t v = block_rows[i]; block_rows[i] = run; run += v; }
}

// pass 2: rows of the set bits, ascending id order (thread order inside a block by an LDS scan of the per-word counts)
__global__ __launch_bounds__(256) void bitmap_compact_kernel(const uint32_t *bitmap, uint32_t n_words, const uint64_t *ids, uint32_t n,
                                                             uint32_t contiguous, const uint32_t *dead, const uint32_t *block_base, uint32_t *subset) {
    __shared__ uint32_t cnt[256];
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    const uint32_t word0 = w < n_words ? bitmap[w] : 0u;
    uint32_t word = word0, rows = 0;
    while (word) {
        const uint32_t b = (uint32_t)__builtin_ctz(word);
        word &= word - 1u;
        rows += find_row(ids, n, (uint64_t)w * 32u + b, contiguous != 0u, dead) != kSentinel ? 1u : 0u;
    }
    cnt[threadIdx.x] = rows;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) { // Hillis-Steele inclusive scan
        const uint32_t v = threadIdx.x >= off ? cnt[threadIdx.x - off] : 0u;
        __syncthreads();
        cnt[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t out = block_base[blockIdx.x] + cnt[threadIdx.x] - rows;
    word = word0;
    while (word) {
        const uint32_t b = (uint32_t)__builtin_ctz(word);
        word &= word - 1u;
        const uint32_t r = find_row(ids, n, (uint64_t)w * 32u + b, contiguous != 0u, dead);
        if (r != kSentinel) subset[out++] = r;
    }
}

// deterministic_sample_ids (restricted.rs:321-342) on the device: the candidate with rank ranks[t] in the ascending id order
// of the bitmap, as an index row (kSentinel when that id holds no vector).  bits_prefix = exclusive scan of the per-block counts.
__global__ __launch_bounds__(64) void bitmap_select_kernel(const uint32_t *bitmap, uint32_t n_words, const uint32_t *bits_prefix, uint32_t n_blocks,
                                                           const uint64_t *ids, uint32_t n, uint32_t contiguous, const uint32_t *dead, const uint32_t *ranks,
                                                           uint32_t n_ranks, uint32_t *out_rows) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_ranks) return;
    const uint32_t r = ranks[t];
    uint32_t lo = 0, hi = n_blocks; // last block whose prefix is <= r
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (bits_prefix[mid] <= r) lo = mid;
        else hi = mid;
    }
    uint32_t rem = r - bits_prefix[lo], row = kSentinel;
    for (uint32_t w = lo * 256u; w < n_words && w < (lo + 1u) * 256u; ++w) {
        uint32_t word = bitmap[w];
        const uint32_t pc = (uint32_t)__builtin_popcount(word);
        if (rem >= pc) { rem -= pc; continue; }
        while (rem--) word &= word - 1u;
        row = find_row(ids, n, (uint64_t)w * 32u + (uint32_t)__builtin_ctz(word), contiguous != 0u, dead);
        break;
    }
    out_rows[t] = row;
}

// Round 6: one `expand` hop (expand.rs:16-80) straight into the scan's row list.  One wavefront per seed, lanes over its arcs: a target
// whose bit was clear joins the candidate population (a bitmap test-and-set makes the union a set) and, when it holds a live vector, the
// row list -- in whatever order the wavefronts get there: the one-launch scan (hvx_restricted_exact.hip) orders by (score, row) itself.
// counters[0] = rows of the list, counters[1] = candidate population.  Replaces the level kernel + count + scan + compact sequence and
// the host read-back between them for plans that are exact whatever the population turns out to be.
__global__ __launch_bounds__(1024) void expand_collect_kernel(CsrView g, const uint32_t *seeds, uint32_t n_seeds, uint32_t direction, const uint32_t *allowed,
                                                             uint32_t n_allowed, uint32_t *visited, const uint64_t *ids, uint32_t n, uint32_t contiguous,
                                                             const uint32_t *dead, uint32_t *rows_out, uint32_t rows_cap, uint32_t *counters) {
    const uint32_t lane = threadIdx.x & 63u;
    // one arc -> (joined the population, row of its target)
    auto visit = [&](bool active, const uint32_t *tgt, const uint32_t *lab, uint64_t at, bool *fresh) __attribute__((always_inline)) -> uint32_t {
        uint32_t row = kSentinel;
        *fresh = false;
        if (active && (!lab || label_ok(lab[at], allowed, n_allowed))) {
            const uint32_t v = tgt[at];
            const uint32_t bit = 1u << (v & 31u);
            *fresh = (atomicOr(&visited[v >> 5], bit) & bit) == 0u;
            if (*fresh) row = find_row(ids, n, (uint64_t)v, contiguous != 0u, dead);
        }
        return row;
    };
    // Round 6 (second build): the sixteen wavefronts of a workgroup walk their light rows in lock step and share ONE pair of counter updates per
    // step (a group of 100 000 sources with one edge each was still 3 126 updates of two words -- same-address atomics serialise at the
    // memory side: 121 us of a 0.43-ms call)
    __shared__ uint32_t s_f[16], s_r[16], s_base, s_steps;
    const uint32_t wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    for (uint32_t c0 = blockIdx.x * blockDim.x; c0 < n_seeds; c0 += gridDim.x * blockDim.x) {
        const uint32_t s0 = c0 + wave * 64u;
        const bool have = s0 + lane < n_seeds;
        const uint32_t node = have ? seeds[s0 + lane] : 0u;
        for (int pass = 0; pass < 2; ++pass) {
            AdjRow r;
            if (!adj_pass(g, direction, pass, have, node, &r)) continue;
            const bool light = r.deg <= kLightRow;
            const uint32_t steps = wave_max(light ? r.deg : 0u);
            if (threadIdx.x == 0) s_steps = 0u;
            __syncthreads();
            if (lane == 0 && steps) atomicMax(&s_steps, steps);
            __syncthreads();
            const uint32_t wg_steps = s_steps;
            for (uint32_t i = 0; i < wg_steps; ++i) {
                bool fresh;
                const uint32_t row = visit(light && i < r.deg, r.tgt, r.lab, r.a0 + i, &fresh);
                const unsigned long long fm = __ballot(fresh), rm = __ballot(row != kSentinel);
                if (lane == 0) { s_f[wave] = (uint32_t)__builtin_popcountll(fm); s_r[wave] = (uint32_t)__builtin_popcountll(rm); }
                __syncthreads();
                if (threadIdx.x == 0) {
                    uint32_t tf = 0, tr = 0;
                    for (uint32_t w = 0; w < waves; ++w) { tf += s_f[w]; tr += s_r[w]; }
                    if (tf) atomicAdd(&counters[1], tf);
                    s_base = tr ? atomicAdd(&counters[0], tr) : 0u;
                }
                __syncthreads();
                if (row != kSentinel) {
                    uint32_t pos = s_base + (uint32_t)__builtin_popcountll(rm & ((1ull << lane) - 1ull));
                    for (uint32_t w = 0; w < wave; ++w) pos += s_r[w];
                    if (pos < rows_cap) rows_out[pos] = row;
                }
                __syncthreads(); // (the next step writes s_f / s_r again)
            }
            // long rows (hubs): the wavefront's arcs of one step share ONE pair of counter updates (a where_() group of 10 000 sources with one
            // edge each was 20 000 atomics on two words with a wavefront per seed: 0.25 ms of a 0.34 ms call)
            walk_heavy_rows(have && !light, r.a0, r.deg, [] { return true; }, [&](bool active, uint64_t at) __attribute__((always_inline)) {
                bool fresh;
                const uint32_t row = visit(active, r.tgt, r.lab, at, &fresh);
                const unsigned long long fm = __ballot(fresh);
                if (fm == 0ull) return;
                if (lane == 0) atomicAdd(&counters[1], (uint32_t)__builtin_popcountll(fm));
                const WavePlace p = wave_append(row != kSentinel, &counters[0], lane);
                if (p.any && row != kSentinel && p.pos < rows_cap) rows_out[p.pos] = row;
            });
        }
    }
}

// ---------------------------------------------------------------------------------------------
// A chain of `expand` hops (hvx_expand_path_filter / hvx_prefilter_path_search_batch_params): hop i's frontier is the bitmap hop i - 1
// wrote, so no frontier crosses PCIe and the host never learns a frontier's size between two hops.  Kernel boundaries order the hops.
// ---------------------------------------------------------------------------------------------
struct PathHopArgs {
    CsrView g;
    const uint32_t *front;   // hop 0: the seed list (pinned host memory), n_front entries; hops >= 1: the bitmap of the frontier,
    uint32_t n_front;        // n_front = the graph's node count
    uint32_t direction;
    const uint32_t *allowed; // this hop's allow-set
    uint32_t n_allowed;
    uint32_t *dst;           // the bitmap of the next frontier (cleared on the stream before the launch)
    uint32_t *hop_size;      // += bits this launch set in dst: |F(i + 1)|
    // the last hop of the lean route only (kCollect): rows of the fresh nodes that pass the mask and hold a live vector -> rows_out,
    // counters[0] = rows of the list, counters[1] = candidate population (fresh AND mask), as expand_collect_kernel leaves them
    const uint32_t *mask;    // nullable
    const uint64_t *ids;
    uint32_t n, contiguous;
    const uint32_t *dead;
    uint32_t *rows_out;
    uint32_t rows_cap;
    uint32_t *counters;
};

// One hop.  kBitmap: a wavefront takes 64 consecutive node numbers (two words of the frontier's bitmap), one node per lane where the bit
// is set; otherwise 64 entries of the seed list.  The row work is split as in expand_collect_kernel: rows of at most 16 arcs by their
// own lane, longer ones by the whole wavefront, one at a time.  What a thread sets in dst it counts in a register: the hop's size (and
// the population) cost ONE update per workgroup, at its end.  Only the row list needs a position per step (kCollect): there the light
// rows are walked in lock step across the workgroup and share one update of counters[0] per step.
template <bool kBitmap, bool kCollect>
__global__ __launch_bounds__(1024) void path_hop_kernel(PathHopArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    __shared__ uint32_t s_r[16], s_base, s_steps, s_fresh, s_pop;
    uint32_t n_fresh = 0, n_pop = 0;
    // one arc: test-and-set its target in dst; kCollect: the row of a fresh target that passes the mask (kSentinel otherwise)
    auto visit = [&](bool active, const uint32_t *tgt, const uint32_t *lab, uint64_t at) __attribute__((always_inline)) -> uint32_t {
        uint32_t row = kSentinel;
        if (active && (!lab || label_ok(lab[at], a.allowed, a.n_allowed))) {
            const uint32_t v = tgt[at];
            const uint32_t bit = 1u << (v & 31u);
            if ((atomicOr(&a.dst[v >> 5], bit) & bit) == 0u) {
                ++n_fresh;
                if (kCollect && (!a.mask || (a.mask[v >> 5] & bit))) {
                    ++n_pop;
                    row = find_row(a.ids, a.n, (uint64_t)v, a.contiguous != 0u, a.dead);
                }
            }
        }
        return row;
    };
    auto always = [] { return true; };
    for (uint32_t c0 = blockIdx.x * blockDim.x; c0 < a.n_front; c0 += gridDim.x * blockDim.x) {
        const uint32_t s0 = c0 + wave * 64u;
        bool have;
        uint32_t node;
        if (kBitmap) {
            // (the bitmap holds whole pairs of words: s0 < n_front keeps the read inside it, and a set bit is a node of the graph)
            const uint32_t word = s0 < a.n_front ? a.front[(s0 >> 5) + (lane >> 5)] : 0u;
            have = ((word >> (lane & 31u)) & 1u) != 0u;
            node = s0 + lane;
        } else {
            have = s0 + lane < a.n_front;
            node = have ? a.front[s0 + lane] : 0u;
        }
        if (!kCollect) {
            walk_rows_per_wave(a.g, a.direction, have, node, always, [&](bool active, const uint32_t *tgt, const uint32_t *lab, uint64_t at)
                               __attribute__((always_inline)) { (void)visit(active, tgt, lab, at); });
            continue;
        }
        // the row list needs a position per step: light rows in lock step across the workgroup, one update of counters[0] per step
        for (int pass = 0; pass < 2; ++pass) {
            AdjRow r;
            if (!adj_pass(a.g, a.direction, pass, have, node, &r)) continue;
            const bool light = r.deg <= kLightRow;
            const uint32_t steps = wave_max(light ? r.deg : 0u);
            if (threadIdx.x == 0) s_steps = 0u;
            __syncthreads();
            if (lane == 0 && steps) atomicMax(&s_steps, steps);
            __syncthreads();
            const uint32_t wg_steps = s_steps;
            for (uint32_t i = 0; i < wg_steps; ++i) {
                const uint32_t row = visit(light && i < r.deg, r.tgt, r.lab, r.a0 + i);
                const unsigned long long rm = __ballot(row != kSentinel);
                if (lane == 0) s_r[wave] = (uint32_t)__builtin_popcountll(rm);
                __syncthreads();
                if (threadIdx.x == 0) {
                    uint32_t tr = 0;
                    for (uint32_t w = 0; w < waves; ++w) tr += s_r[w];
                    s_base = tr ? atomicAdd(&a.counters[0], tr) : 0u;
                }
                __syncthreads();
                if (row != kSentinel) {
                    uint32_t pos = s_base + (uint32_t)__builtin_popcountll(rm & ((1ull << lane) - 1ull));
                    for (uint32_t w = 0; w < wave; ++w) pos += s_r[w];
                    if (pos < a.rows_cap) a.rows_out[pos] = row;
                }
                __syncthreads(); // (the next step writes s_r again)
            }
            walk_heavy_rows(have && !light, r.a0, r.deg, always, [&](bool active, uint64_t at) __attribute__((always_inline)) {
                const uint32_t row = visit(active, r.tgt, r.lab, at);
                const WavePlace p = wave_append(row != kSentinel, &a.counters[0], lane);
                if (p.any && row != kSentinel && p.pos < a.rows_cap) a.rows_out[p.pos] = row;
            });
        }
    }
    // the workgroup's share of the hop's size (and of the population): one update each
#pragma unroll
    for (int sh = 32; sh > 0; sh >>= 1) {
        n_fresh += (uint32_t)__shfl_xor((int)n_fresh, sh, 64);
        if (kCollect) n_pop += (uint32_t)__shfl_xor((int)n_pop, sh, 64);
    }
    if (threadIdx.x == 0) { s_fresh = 0u; s_pop = 0u; }
    __syncthreads();
    if (lane == 0) {
        if (n_fresh) atomicAdd(&s_fresh, n_fresh);
        if (kCollect && n_pop) atomicAdd(&s_pop, n_pop);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_fresh) atomicAdd(a.hop_size, s_fresh);
        if (kCollect && s_pop) atomicAdd(&a.counters[1], s_pop);
    }
}

// the Filter step on the bitmap route: final frontier AND node mask
__global__ __launch_bounds__(256) void bitmap_and_kernel(uint32_t *bitmap, const uint32_t *mask, uint32_t n_words) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w < n_words) bitmap[w] &= mask[w];
}

} // namespace

static int prefilter_search_impl(const hvx_index *cix, const hvx_csr *cg, const float *queries, uint32_t b, const hvx_restricted_params &rp,
                                 uint32_t mode, const uint64_t *seeds, uint32_t n_seeds, uint32_t max_depth, uint32_t direction,
                                 const uint32_t *allowed_label_ids, uint32_t n_labels, uint32_t hub_degree, uint32_t include_seeds,
                                 uint64_t *out_ids, float *out_scores, uint32_t *out_counts, uint32_t *out_status, uint64_t *out_candidates,
                                 hvx_restricted_stats *rstats, hvx_stats *stats);

static int prefilter_bitmap_route(hvx_index *ix, hvx_csr *g, const uint32_t *bitmap, const float *queries, uint32_t b, const hvx_restricted_params &rp,
                                  uint64_t *out_ids, float *out_scores, uint32_t *out_counts, uint32_t *out_status, uint64_t *out_candidates,
                                  hvx_restricted_stats *rstats, hvx_stats *stats);

// The lean route of the fused calls: the hops, the row list and the one-launch scan behind ONE host wait.  Taken when the plan is exact
// WHATEVER the hops reach -- `bound` = what they can reach at most -- and the one-launch scan serves the shape.
static bool lean_route(hvx_index *ix, const hvx_restricted_params &rp, uint32_t b, uint64_t bound) {
    const uint32_t k = rp.k;
    // (k > 64: one query per tile over the shared set -- that shape lost to the pipeline at 10 000 ids, and the hop in front of it has not
    // been measured: the lean route takes it when forced or when the pipeline would refuse)
    if (ix->opt[HVX_OPT_RESTRICTED_DIRECT] == 1u || rp.explicit_budgets ||
        !(k <= 64u || ix->opt[HVX_OPT_RESTRICTED_DIRECT] == 2u || !restricted_older_serves(ix, k)) || !restricted_direct_supported(ix, k) || ix->dev.n == 0u)
        return false;
    RestrictedPlan plan;
    const bool exact_any = bound == 0 || (bound <= 1000000ull && restricted_make_plan(rp, bound, ix->dev.dim, &plan, ix) == HVX_OK && plan.strategy == HVX_RESTRICTED_EXACT &&
                                         (rp.strategy != HVX_RESTRICTED_REFERENCE_PLAN || bound <= 256)); // (a plan is monotone in the population)
    const uint64_t work = (uint64_t)b * std::min<uint64_t>(bound, ix->dev.n) * ix->dev.dim;
    // (the other path costs ~0.2 ms of host round trips more: the one-launch scan is the better choice up to 2^28 here, not 2^26)
    return exact_any && bound != 0 && b <= ix->max_batch && (work <= (1ull << 28) || ix->opt[HVX_OPT_RESTRICTED_DIRECT] == 2u);
}

// its row list of rows_cap rows and the two counters in front of the scan (zeroed on `s`)
static int lean_reserve(hvx_index *ix, uint32_t rows_cap, hipStream_t s) {
    int rc;
    if (rows_cap > ix->cap_subset) {
        if ((rc = ix->regrow((void **)&ix->f_subset, (size_t)std::max<uint32_t>(rows_cap, 1u) * 4))) return rc;
        ix->cap_subset = rows_cap;
    }
    if (ix->cap_pf_blocks < 4) {
        if ((rc = ix->regrow((void **)&ix->pf_blocks, 64))) return rc;
        ix->cap_pf_blocks = 16;
    }
    HIP_TRY(hipMemsetAsync(ix->pf_blocks, 0, 8, s));
    return HVX_OK;
}

// One hop + exact scan with ONE host wait (round 6; the reference issues one query per call, index_lifecycle_scale.rs:1893-1912: the
// latency of this call is what a request sees).  Taken when the plan is exact WHATEVER the hop reaches -- strategy EXACT, or a planned
// strategy whose bound on the population (seeds x the largest adjacency row) is inside the plan's exact region -- and the one-launch scan
// serves the shape.  Everything is enqueued on the index's stream: clear the bitmap, expand_collect_kernel (seeds read out of the pinned
// staging buffer), queries copied + validated, the scan with its row count read ON THE DEVICE, results into mapped host rows.
static int prefilter_expand_lean(hvx_index *ix, hvx_csr *g, const float *queries, uint32_t b, const hvx_restricted_params &rp, const uint64_t *seeds,
                                 uint32_t n_seeds, uint32_t direction, const uint32_t *allowed_label_ids, uint32_t n_labels, uint64_t bound,
                                 uint64_t *out_ids, float *out_scores, uint32_t *out_counts, uint32_t *out_status, uint64_t *out_candidates,
                                 hvx_restricted_stats *rstats, hvx_stats *stats) {
    int rc;
    const uint32_t k = rp.k;
    hipStream_t s = ix->stream;
    if ((rc = seeds_reserve(g, n_seeds, s))) return rc;
    for (uint32_t i = 0; i < n_seeds; ++i) {
        if (seeds[i] >= g->n) return fail(HVX_ERR_INVARIANT, "unknown node %llu", (unsigned long long)seeds[i]);
        g->h_seeds[i] = (uint32_t)seeds[i];
    }
    if ((rc = upload_labels(g, allowed_label_ids, n_labels))) return rc; // (on g->stream: ordered below)
    if (n_labels) {
        if (!g->done) HIP_TRY(hipEventCreateWithFlags(&g->done, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(g->done, g->stream));
        HIP_TRY(hipStreamWaitEvent(s, g->done, 0));
    }
    const uint32_t rows_cap = (uint32_t)std::min<uint64_t>(bound, ix->dev.n);
    if ((rc = lean_reserve(ix, rows_cap, s))) return rc;
    const size_t words32 = ((g->n + 63) / 64) * 2;
    HIP_TRY(hipMemsetAsync(g->visited, 0, std::max<size_t>(words32, 2) * 4, s));
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(512, ((uint64_t)n_seeds + 1023) / 1024); // (a wavefront takes 64 seeds at a time, a workgroup 1 024)
    hipLaunchKernelGGL(expand_collect_kernel, dim3(std::max(blocks, 1u)), dim3(1024), 0, s, csr_view(g), g->h_seeds, n_seeds, direction, g->labels, n_labels, g->visited,
                       ix->dev.ids, ix->dev.n, ix->contiguous ? 1u : 0u, ix->dev.dead, ix->f_subset, rows_cap, ix->pf_blocks);
    HIP_TRY(hipGetLastError());
    return restricted_direct_shared_devcount(ix, queries, b, k, ix->f_subset, rows_cap, ix->pf_blocks, out_ids, out_scores, out_counts, out_status,
                                             out_candidates, rstats, stats);
}

extern "C" int hvx_prefilter_search_batch(const hvx_index *cix, const hvx_csr *cg, const float *queries, uint32_t b, uint32_t k,
                                          uint32_t ef, uint32_t mode, const uint64_t *seeds, uint32_t n_seeds, uint32_t max_depth,
                                          uint32_t direction, const uint32_t *allowed_label_ids, uint32_t n_labels,
                                          uint32_t hub_degree, uint32_t include_seeds, uint64_t *out_ids, float *out_scores,
                                          uint32_t *out_counts, uint32_t *out_status, uint64_t *out_candidates, hvx_stats *stats) {
    hvx_restricted_params rp;
    memset(&rp, 0, sizeof(rp));
    rp.k = k;
    rp.ef = ef;
    rp.strategy = HVX_RESTRICTED_EXACT; // this entry point answers every candidate-set size with the exact gathered scan
    return prefilter_search_impl(cix, cg, queries, b, rp, mode, seeds, n_seeds, max_depth, direction, allowed_label_ids, n_labels, hub_degree,
                                 include_seeds, out_ids, out_scores, out_counts, out_status, out_candidates, nullptr, stats);
}

extern "C" int hvx_prefilter_search_batch_params(const hvx_index *cix, const hvx_csr *cg, const float *queries, uint32_t b,
                                                 const hvx_restricted_params *params, uint32_t mode, const uint64_t *seeds, uint32_t n_seeds,
                                                 uint32_t max_depth, uint32_t direction, const uint32_t *allowed_label_ids, uint32_t n_labels,
                                                 uint32_t hub_degree, uint32_t include_seeds, uint64_t *out_ids, float *out_scores,
                                                 uint32_t *out_counts, uint32_t *out_status, uint64_t *out_candidates,
                                                 hvx_restricted_stats *out_restricted_stats, hvx_stats *stats) {
    if (!params) return fail(HVX_ERR_INVARIANT, "null argument");
    if (params->strategy > HVX_RESTRICTED_REFERENCE_PLAN) return fail(HVX_ERR_INVARIANT, "unknown restricted strategy %u", params->strategy);
    return prefilter_search_impl(cix, cg, queries, b, *params, mode, seeds, n_seeds, max_depth, direction, allowed_label_ids, n_labels, hub_degree,
                                 include_seeds, out_ids, out_scores, out_counts, out_status, out_candidates, out_restricted_stats, stats);
}

static int prefilter_search_impl(const hvx_index *cix, const hvx_csr *cg, const float *queries, uint32_t b, const hvx_restricted_params &rp,
                                 uint32_t mode, const uint64_t *seeds, uint32_t n_seeds, uint32_t max_depth, uint32_t direction,
                                 const uint32_t *allowed_label_ids, uint32_t n_labels, uint32_t hub_degree, uint32_t include_seeds,
                                 uint64_t *out_ids, float *out_scores, uint32_t *out_counts, uint32_t *out_status, uint64_t *out_candidates,
                                 hvx_restricted_stats *rstats, hvx_stats *stats) {
    const uint32_t k = rp.k, ef = rp.ef;
    if (!cix || !cg) return fail(HVX_ERR_INVARIANT, "null argument");
    hvx_index *ix = const_cast<hvx_index *>(cix);
    hvx_csr *g = const_cast<hvx_csr *>(cg);
    if (k == 0) return fail(HVX_ERR_K_RANGE, "result count must be non-zero");
    if (ef < k) return fail(HVX_ERR_K_RANGE, "search beam width %u is below the result count %u", ef, k);
    if (mode > HVX_PREFILTER_TRAVERSE) return fail(HVX_ERR_INVARIANT, "bad prefilter mode");
    if (ix->device != g->device) return fail(HVX_ERR_INVARIANT, "index and graph live on different devices");
    if (out_candidates) *out_candidates = 0;
    for (uint32_t q = 0; q < b; ++q) {
        out_counts[q] = 0;
        if (out_status) out_status[q] = HVX_OK;
        if (rstats) memset(&rstats[q], 0, sizeof(hvx_restricted_stats));
    }
    if (b == 0) return HVX_OK;
    if (mode == HVX_PREFILTER_EXPAND && n_seeds == 0) return HVX_OK; // an empty stream expands to nothing
    std::lock_guard<std::mutex> glock(g->mu);
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->sync_rewrites();
    // (the collect kernel counts the arcs of one row in 32 bits: a graph with a row of 2^31 arcs takes the level kernel below)
    if (mode == HVX_PREFILTER_EXPAND && direction <= HVX_DIR_BOTH && std::max(g->max_out_deg, g->max_in_deg) < (1ull << 31)) {
        // what one hop can reach at most: seeds x the largest adjacency row (both rows for direction Both), never more than the graph
        const uint64_t per_seed = (direction != HVX_DIR_IN ? g->max_out_deg : 0) + (direction != HVX_DIR_OUT ? g->max_in_deg : 0);
        const uint64_t bound = std::min<uint64_t>((uint64_t)n_seeds * per_seed, g->n);
        if (lean_route(ix, rp, b, bound))
            return prefilter_expand_lean(ix, g, queries, b, rp, seeds, n_seeds, direction, allowed_label_ids, n_labels, bound, out_ids, out_scores, out_counts,
                                         out_status, out_candidates, rstats, stats);
    }
    int rc = run_bfs_locked(g, seeds, n_seeds, mode == HVX_PREFILTER_EXPAND ? 1u : max_depth, direction, allowed_label_ids, n_labels,
                            mode == HVX_PREFILTER_EXPAND ? 0u : hub_degree, mode == HVX_PREFILTER_EXPAND ? 0u : include_seeds,
                            mode == HVX_PREFILTER_EXPAND, nullptr, nullptr, ix->stream);
    if (rc) return rc; // (the index's stream waits for the traversal: the bitmap is complete before anything below reads it)
    return prefilter_bitmap_route(ix, g, g->visited, queries, b, rp, out_ids, out_scores, out_counts, out_status, out_candidates, rstats, stats);
}

// The bitmap route of the fused calls: `bitmap` (a candidate bitmap of g, complete on ix->stream) -> count / scan / compact -> the plan.
static int prefilter_bitmap_route(hvx_index *ix, hvx_csr *g, const uint32_t *bitmap, const float *queries, uint32_t b, const hvx_restricted_params &rp,
                                  uint64_t *out_ids, float *out_scores, uint32_t *out_counts, uint32_t *out_status, uint64_t *out_candidates,
                                  hvx_restricted_stats *rstats, hvx_stats *stats) {
    const uint32_t k = rp.k;
    int rc;
    const uint32_t n_words = ((g->n + 63u) / 64u) * 2u, n_blocks = (n_words + 255u) / 256u;
    if (2 * (n_blocks + 2) > ix->cap_pf_blocks) {
        if ((rc = ix->regrow((void **)&ix->pf_blocks, (size_t)2 * (n_blocks + 2) * 4))) return rc;
        ix->cap_pf_blocks = 2 * (n_blocks + 2);
    }
    uint32_t *d_total_bits = ix->pf_blocks + n_blocks + 1;
    uint32_t *d_block_bits = ix->pf_blocks + n_blocks + 2; // [n_blocks + 1]: per-block candidate counts, then their scan
    HIP_TRY(hipMemsetAsync(d_total_bits, 0, 4, ix->stream));
    hipLaunchKernelGGL(bitmap_count_kernel, dim3(n_blocks), dim3(256), 0, ix->stream, bitmap, n_words, ix->dev.ids, ix->dev.n,
                       ix->contiguous ? 1u : 0u, ix->dev.dead, ix->pf_blocks, d_total_bits, d_block_bits);
    hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(1024), 0, ix->stream, ix->pf_blocks, n_blocks);
    HIP_TRY(hipGetLastError());
    if ((rc = ix->pin(64))) return rc;
    uint32_t *totals = reinterpret_cast<uint32_t *>(ix->h_pin); // rows to scan, candidate population (read back through the pinned mirror)
    HIP_TRY(hipMemcpyAsync(totals, ix->pf_blocks + n_blocks, 8, hipMemcpyDeviceToHost, ix->stream));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    const uint32_t n_rows = totals[0], population = totals[1];
    if (out_candidates) *out_candidates = population;
    // RestrictedVectorCandidates::from_ids (restricted.rs:356-371) / RestrictedResultCount::try_new (:200-213)
    if (population > 1000000) return fail(HVX_ERR_CANDIDATE_LIMIT, "restricted vector search accepts at most 1000000 unique candidates");
    if (population == 0) return HVX_OK;
    const uint32_t kk = std::min<uint32_t>(k, population);
    if (kk > 800) return fail(HVX_ERR_K_RANGE, "restricted vector search result count %u is above the maximum 800", kk);
    if (n_rows > ix->cap_subset) {
        if ((rc = ix->regrow((void **)&ix->f_subset, (size_t)n_rows * 4))) return rc;
        ix->cap_subset = n_rows;
    }
    if (n_rows)
        hipLaunchKernelGGL(bitmap_compact_kernel, dim3(n_blocks), dim3(256), 0, ix->stream, bitmap, n_words, ix->dev.ids, ix->dev.n,
                           ix->contiguous ? 1u : 0u, ix->dev.dead, ix->pf_blocks, ix->f_subset);
    HIP_TRY(hipGetLastError());
    // restricted_execution_plan_with_beam_percent (restricted.rs:426-453) over the candidate population
    RestrictedPlan plan;
    if ((rc = restricted_make_plan(rp, population, ix->dev.dim, &plan, ix))) return rc;
    (void)kk;
    const uint32_t *d_samples = nullptr;
    if (plan.strategy == HVX_RESTRICTED_FILTERED && plan.p.n_sample) {
        // the deterministic seeds: ranks into the candidate population, resolved against the bitmap on the device
        std::vector<uint64_t> ranks64;
        restricted_sample_ranks(population, plan.p.n_sample, ranks64);
        std::vector<uint32_t> ranks(ranks64.begin(), ranks64.end());
        const uint32_t ns = plan.p.n_sample;
        if ((size_t)2 * ns * 4 > ix->cap_w_samples) {
            if ((rc = ix->regrow((void **)&ix->w_samples, (size_t)2 * ns * 4))) return rc;
            ix->cap_w_samples = (size_t)2 * ns * 4;
        }
        HIP_TRY(hipMemcpyAsync(ix->w_samples + ns, ranks.data(), (size_t)ns * 4, hipMemcpyHostToDevice, ix->stream));
        hipLaunchKernelGGL(block_scan_kernel, dim3(1), dim3(1024), 0, ix->stream, d_block_bits, n_blocks);
        hipLaunchKernelGGL(bitmap_select_kernel, dim3((ns + 63u) / 64u), dim3(64), 0, ix->stream, bitmap, n_words, d_block_bits, n_blocks,
                           ix->dev.ids, ix->dev.n, ix->contiguous ? 1u : 0u, ix->dev.dead, ix->w_samples + ns, ns, ix->w_samples);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(ix->stream)); // `ranks` lives on this frame
        d_samples = ix->w_samples;
    }
    return restricted_run_plan(ix, queries, b, k, plan, ix->f_subset, n_rows, d_samples, out_ids, out_scores, out_counts, out_status, rstats, stats);
}

// ---------------------------------------------------------------------------------------------
// Chains of expand hops: Access -> Expand -> ... -> Expand -> optional Filter -> VectorSearch (expand.rs:16-80, node output).
// ---------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t kMaxPathHops = 16;

struct PathPlan {
    uint32_t n_hops = 0, n_labels = 0;
    const uint32_t *direction = nullptr, *label_off = nullptr, *labels = nullptr;
    uint32_t lab0(uint32_t i) const { return label_off ? label_off[i] : 0u; }
    uint32_t lab_n(uint32_t i) const { return label_off ? label_off[i + 1] - label_off[i] : 0u; }
};

// the argument rules of both entry points: nothing is enqueued, nothing of the graph is touched
int path_check(const hvx_csr *g, const uint64_t *seeds, uint32_t n_seeds, uint32_t n_hops, const uint32_t *hop_direction,
               const uint32_t *hop_label_offsets, const uint32_t *hop_labels, PathPlan *p) {
    if (n_hops == 0 || n_hops > kMaxPathHops) return fail(HVX_ERR_INVARIANT, "a chain has 1 .. %u hops, not %u", kMaxPathHops, n_hops);
    if (!hop_direction) return fail(HVX_ERR_INVARIANT, "null argument");
    if (std::max(g->max_out_deg, g->max_in_deg) >= (1ull << 31)) // (the hop kernel counts the arcs of one row in 32 bits)
        return fail(HVX_ERR_UNSUPPORTED, "a chain of hops serves adjacency rows below 2^31 arcs");
    for (uint32_t i = 0; i < n_hops; ++i)
        if (hop_direction[i] > HVX_DIR_BOTH) return fail(HVX_ERR_INVARIANT, "bad direction on hop %u", i);
    if (hop_label_offsets) {
        for (uint32_t i = 0; i < n_hops; ++i)
            if (hop_label_offsets[i + 1] < hop_label_offsets[i]) return fail(HVX_ERR_INVARIANT, "label offsets do not ascend at hop %u", i);
        if (hop_label_offsets[n_hops] != 0 && !hop_labels) return fail(HVX_ERR_INVARIANT, "null labels");
    }
    if (n_seeds && !seeds) return fail(HVX_ERR_INVARIANT, "null seeds");
    for (uint32_t i = 0; i < n_seeds; ++i)
        if (seeds[i] >= g->n) return fail(HVX_ERR_INVARIANT, "unknown node %llu", (unsigned long long)seeds[i]);
    p->n_hops = n_hops;
    p->direction = hop_direction;
    p->label_off = hop_label_offsets;
    p->labels = hop_labels;
    p->n_labels = hop_label_offsets ? hop_label_offsets[n_hops] : 0u;
    return HVX_OK;
}

// min(n_nodes, n_seeds x the product of every hop's largest row), saturating: what the chain can reach at most
uint64_t path_bound(const hvx_csr *g, uint32_t n_seeds, const PathPlan &p) {
    uint64_t bound = n_seeds;
    for (uint32_t i = 0; i < p.n_hops; ++i) {
        const uint64_t per = (p.direction[i] != HVX_DIR_IN ? g->max_out_deg : 0) + (p.direction[i] != HVX_DIR_OUT ? g->max_in_deg : 0);
        if (per == 0 || bound == 0) return 0;
        bound = bound > g->n / per ? g->n : std::min<uint64_t>(bound * per, g->n); // (bound * per >= n whenever bound > n / per)
    }
    return bound;
}

// caller holds g->mu: the chain's buffers, the seeds in the pinned buffer, labels and mask uploads enqueued on `s`
int path_stage(hvx_csr *g, hipStream_t s, const uint64_t *seeds, uint32_t n_seeds, const PathPlan &p, const uint64_t *node_mask_words) {
    HIP_TRY(hipSetDevice(g->device));
    int rc;
    const size_t words32 = std::max<size_t>(((g->n + 63) / 64) * 2, 2);
    if (!g->visited2) {
        if ((rc = csr_alloc(g, (void **)&g->visited2, words32 * 4))) return rc;
        if ((rc = csr_alloc(g, (void **)&g->hop_cnt, kMaxPathHops * 4))) return rc;
    }
    if (!g->h_hops && hipHostMalloc((void **)&g->h_hops, kMaxPathHops * 4, hipHostMallocDefault) != hipSuccess)
        return fail(HVX_ERR_DEVICE, "hipHostMalloc hop sizes");
    if ((rc = seeds_reserve(g, n_seeds, s))) return rc;
    for (uint32_t i = 0; i < n_seeds; ++i) g->h_seeds[i] = (uint32_t)seeds[i]; // (path_check has seen every one below n)
    if ((rc = upload_labels(g, p.labels, p.n_labels, s))) return rc;
    if (node_mask_words && (rc = stage_bitmap(g, s, node_mask_words, &g->mask_dev, &g->h_mask))) return rc;
    HIP_TRY(hipMemsetAsync(g->hop_cnt, 0, kMaxPathHops * 4, s));
    return HVX_OK;
}

// Enqueues hops [0, n_run) of the chain on `s`; the bitmap of F(n_hops) lands in g->visited whatever the hop count's parity.
// `collect` != NULL: the last hop is the lean route's (rows and counters filled in by the caller).
int path_enqueue(hvx_csr *g, hipStream_t s, uint32_t n_seeds, const PathPlan &p, const PathHopArgs *collect) {
    const size_t words32 = std::max<size_t>(((g->n + 63) / 64) * 2, 2);
    const uint32_t grid_cap = 512; // (a workgroup takes 1 024 seeds or node numbers per pass)
    for (uint32_t i = 0; i < p.n_hops; ++i) {
        const bool last = i + 1 == p.n_hops;
        uint32_t *dst = ((p.n_hops - 1 - i) & 1u) ? g->visited2 : g->visited, *src = dst == g->visited ? g->visited2 : g->visited;
        PathHopArgs a;
        memset(&a, 0, sizeof(a));
        if (last && collect) a = *collect;
        a.g = csr_view(g);
        a.front = i == 0 ? g->h_seeds : src;
        a.n_front = i == 0 ? n_seeds : g->n;
        a.direction = p.direction[i];
        a.allowed = g->labels + p.lab0(i);
        a.n_allowed = p.lab_n(i);
        a.dst = dst;
        a.hop_size = g->hop_cnt + i;
        HIP_TRY(hipMemsetAsync(dst, 0, words32 * 4, s));
        const uint32_t blocks = std::max<uint32_t>(1u, (uint32_t)std::min<uint64_t>(grid_cap, ((uint64_t)a.n_front + 1023) / 1024));
        if (i == 0) {
            if (last && collect) hipLaunchKernelGGL((path_hop_kernel<false, true>), dim3(blocks), dim3(1024), 0, s, a);
            else hipLaunchKernelGGL((path_hop_kernel<false, false>), dim3(blocks), dim3(1024), 0, s, a);
        } else {
            if (last && collect) hipLaunchKernelGGL((path_hop_kernel<true, true>), dim3(blocks), dim3(1024), 0, s, a);
            else hipLaunchKernelGGL((path_hop_kernel<true, false>), dim3(blocks), dim3(1024), 0, s, a);
        }
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(g->h_hops, g->hop_cnt, kMaxPathHops * 4, hipMemcpyDeviceToHost, s));
    return HVX_OK;
}

void path_sizes_out(const hvx_csr *g, uint32_t n_hops, uint64_t *out_hop_sizes) {
    if (out_hop_sizes)
        for (uint32_t i = 0; i < n_hops; ++i) out_hop_sizes[i] = g->h_hops[i];
}

} // namespace

extern "C" int hvx_expand_path_filter(const hvx_csr *cg, const uint64_t *seeds, uint32_t n_seeds, uint32_t n_hops, const uint32_t *hop_direction,
                                      const uint32_t *hop_label_offsets, const uint32_t *hop_labels, uint64_t *out_bitmap_words,
                                      uint64_t *out_hop_sizes) {
    if (!cg || !out_bitmap_words) return fail(HVX_ERR_INVARIANT, "null argument");
    hvx_csr *g = const_cast<hvx_csr *>(cg);
    PathPlan p;
    int rc = path_check(g, seeds, n_seeds, n_hops, hop_direction, hop_label_offsets, hop_labels, &p);
    if (rc) return rc;
    const size_t bytes = (size_t)((g->n + 63) / 64) * 8;
    if (n_seeds == 0) { // an empty stream expands to nothing
        memset(out_bitmap_words, 0, bytes);
        if (out_hop_sizes) memset(out_hop_sizes, 0, (size_t)n_hops * 8);
        return HVX_OK;
    }
    std::lock_guard<std::mutex> lock(g->mu);
    if ((rc = path_stage(g, g->stream, seeds, n_seeds, p, nullptr))) return rc;
    if ((rc = path_enqueue(g, g->stream, n_seeds, p, nullptr))) return rc;
    if (bytes) HIP_TRY(hipMemcpyAsync(out_bitmap_words, g->visited, bytes, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    path_sizes_out(g, n_hops, out_hop_sizes);
    return HVX_OK;
}

extern "C" int hvx_prefilter_path_search_batch_params(const hvx_index *cix, const hvx_csr *cg, const float *queries, uint32_t b,
                                                      const hvx_restricted_params *params, const uint64_t *seeds, uint32_t n_seeds, uint32_t n_hops,
                                                      const uint32_t *hop_direction, const uint32_t *hop_label_offsets, const uint32_t *hop_labels,
                                                      const uint64_t *node_mask_words, uint64_t *out_ids, float *out_scores, uint32_t *out_counts,
                                                      uint32_t *out_status, uint64_t *out_candidates, uint64_t *out_hop_sizes,
                                                      hvx_restricted_stats *rstats, hvx_stats *stats) {
    if (!cix || !cg || !params) return fail(HVX_ERR_INVARIANT, "null argument");
    if (params->strategy > HVX_RESTRICTED_REFERENCE_PLAN) return fail(HVX_ERR_INVARIANT, "unknown restricted strategy %u", params->strategy);
    const hvx_restricted_params &rp = *params;
    hvx_index *ix = const_cast<hvx_index *>(cix);
    hvx_csr *g = const_cast<hvx_csr *>(cg);
    const uint32_t k = rp.k;
    if (k == 0) return fail(HVX_ERR_K_RANGE, "result count must be non-zero");
    if (rp.ef < k) return fail(HVX_ERR_K_RANGE, "search beam width %u is below the result count %u", rp.ef, k);
    if (ix->device != g->device) return fail(HVX_ERR_INVARIANT, "index and graph live on different devices");
    PathPlan p;
    int rc = path_check(g, seeds, n_seeds, n_hops, hop_direction, hop_label_offsets, hop_labels, &p);
    if (rc) return rc;
    if (out_candidates) *out_candidates = 0;
    if (out_hop_sizes) memset(out_hop_sizes, 0, (size_t)n_hops * 8);
    for (uint32_t q = 0; q < b; ++q) {
        out_counts[q] = 0;
        if (out_status) out_status[q] = HVX_OK;
        if (rstats) memset(&rstats[q], 0, sizeof(hvx_restricted_stats));
    }
    if (b == 0 || n_seeds == 0) return HVX_OK; // an empty stream expands to nothing
    std::lock_guard<std::mutex> glock(g->mu);
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->sync_rewrites();
    hipStream_t s = ix->stream;
    const uint64_t bound = path_bound(g, n_seeds, p);
    const bool lean = lean_route(ix, rp, b, bound); // prefilter_search_impl's rule, over the chain's bound
    // (a refusal below leaves nothing of this call on the stream: hvx_csr_apply_edges relies on every reader having drained when it gives up g->mu)
    auto drained = [&](int code) { (void)hipStreamSynchronize(s); return code; };
    if ((rc = path_stage(g, s, seeds, n_seeds, p, node_mask_words))) return drained(rc);
    if (lean) { // every hop, the row list and the scan behind one host wait
        const uint32_t rows_cap = (uint32_t)std::min<uint64_t>(bound, ix->dev.n);
        if ((rc = lean_reserve(ix, rows_cap, s))) return drained(rc);
        PathHopArgs c;
        memset(&c, 0, sizeof(c));
        c.mask = node_mask_words ? g->mask_dev : nullptr;
        c.ids = ix->dev.ids;
        c.n = ix->dev.n;
        c.contiguous = ix->contiguous ? 1u : 0u;
        c.dead = ix->dev.dead;
        c.rows_out = ix->f_subset;
        c.rows_cap = rows_cap;
        c.counters = ix->pf_blocks;
        if ((rc = path_enqueue(g, s, n_seeds, p, &c))) return drained(rc);
        rc = restricted_direct_shared_devcount(ix, queries, b, k, ix->f_subset, rows_cap, ix->pf_blocks, out_ids, out_scores, out_counts, out_status,
                                               out_candidates, rstats, stats);
    } else {
        if ((rc = path_enqueue(g, s, n_seeds, p, nullptr))) return drained(rc);
        if (node_mask_words) {
            const uint32_t n_words = ((g->n + 63u) / 64u) * 2u;
            hipLaunchKernelGGL(bitmap_and_kernel, dim3((n_words + 255u) / 256u), dim3(256), 0, s, g->visited, g->mask_dev, n_words);
            HIP_TRY(hipGetLastError());
        }
        rc = prefilter_bitmap_route(ix, g, g->visited, queries, b, rp, out_ids, out_scores, out_counts, out_status, out_candidates, rstats, stats);
    }
    if (rc != HVX_OK && rc != HVX_ERR_CANDIDATE_LIMIT && rc != HVX_ERR_K_RANGE) (void)hipStreamSynchronize(s); // (a refusal in front of the route's wait)
    path_sizes_out(g, n_hops, out_hop_sizes);
    return rc;
}

// ---------------------------------------------------------------------------------------------
// Chains with per-query seeds: the same plan (hops, labels, Filter step) for every request of a batch, each request from its own start
// nodes -- the batching operator's prefiltered branch (storage.rs:140-163) with the traversal in front of it.  One launch of
// path_lists_kernel (hvx_prefilter_batch.hip) runs every chain and leaves query q's final set in slot q of the one-launch scan.
// ---------------------------------------------------------------------------------------------
namespace {

constexpr uint32_t kMaxListFrontier = 16384; // 32 768 table slots x 4 B = 128 KiB of a CU's 160 KiB of LDS
constexpr uint32_t kMaxListBatch = 65535;    // (seed offsets and slot positions stay inside 32 bits)

// the argument rules of both entry points: nothing is enqueued, nothing of the graph is touched
int lists_check(const hvx_csr *g, uint32_t b, const uint64_t *seeds, const uint64_t *seed_offsets, uint32_t n_hops, const uint32_t *hop_direction,
                const uint32_t *hop_label_offsets, const uint32_t *hop_labels, uint32_t max_frontier, PathPlan *p) {
    int rc = path_check(g, nullptr, 0, n_hops, hop_direction, hop_label_offsets, hop_labels, p);
    if (rc) return rc;
    if (!seed_offsets) return fail(HVX_ERR_INVARIANT, "null argument");
    if (max_frontier == 0 || max_frontier > kMaxListFrontier)
        return fail(HVX_ERR_UNSUPPORTED, "per-query chains keep sets of 1 .. %u nodes (max_frontier %u): larger sets take the shared-seed call", kMaxListFrontier, max_frontier);
    if (b > kMaxListBatch) return fail(HVX_ERR_UNSUPPORTED, "a batch of per-query chains holds at most %u queries", kMaxListBatch);
    for (uint32_t q = 0; q < b; ++q) {
        if (seed_offsets[q + 1] < seed_offsets[q]) return fail(HVX_ERR_INVARIANT, "seed offsets do not ascend at query %u", q);
        if (seed_offsets[q + 1] - seed_offsets[q] > max_frontier)
            return fail(HVX_ERR_INVARIANT, "query %u starts from %llu seeds, its slot holds %u", q, (unsigned long long)(seed_offsets[q + 1] - seed_offsets[q]), max_frontier);
    }
    if (b && seed_offsets[b] != seed_offsets[0] && !seeds) return fail(HVX_ERR_INVARIANT, "null seeds");
    for (uint64_t i = b ? seed_offsets[0] : 0; b && i < seed_offsets[b]; ++i)
        if (seeds[i] >= g->n) return fail(HVX_ERR_INVARIANT, "unknown node %llu", (unsigned long long)seeds[i]);
    return HVX_OK;
}

// the carved g->lists_buf: [b][max_frontier] u64 scan slots | [b][2][max_frontier] u32 frontier lists | control words, which begin
// [b] lengths | [b] statuses | [b][16] sizes (the repeat adds [b] stop depths)
struct ListsView { uint64_t *ids; uint32_t *front, *ctl; size_t ctl_words; };

// caller holds g->mu; b != 0.  Every query's seeds and the [b + 1] offsets into them, as u32, in the pinned buffer a kernel reads them from.
int lists_stage_seeds(hvx_csr *g, hipStream_t s, uint32_t b, const uint64_t *seeds, const uint64_t *seed_offsets, const uint32_t **h_off, const uint32_t **h_seed) {
    const uint64_t first = seed_offsets[0], total = seed_offsets[b] - first;
    int rc = seeds_reserve(g, (size_t)b + 1 + total, s);
    if (rc) return rc;
    uint32_t *off = g->h_seeds, *seed = g->h_seeds + b + 1;
    for (uint32_t q = 0; q <= b; ++q) off[q] = (uint32_t)(seed_offsets[q] - first);
    for (uint64_t i = 0; i < total; ++i) seed[i] = (uint32_t)seeds[first + i]; // (the argument check has seen every one below n)
    *h_off = off;
    *h_seed = seed;
    return HVX_OK;
}

// g->lists_buf of at least `bytes` (every call that used the old one has waited for its stream)
int lists_reserve(hvx_csr *g, size_t bytes) {
    if (bytes <= g->lists_cap) return HVX_OK;
    if (g->lists_buf) {
        g->allocs.erase(std::remove(g->allocs.begin(), g->allocs.end(), g->lists_buf), g->allocs.end());
        (void)hipFree(g->lists_buf);
        g->lists_buf = nullptr;
        g->lists_cap = 0;
    }
    int rc = csr_alloc(g, &g->lists_buf, bytes);
    if (rc) return rc;
    g->lists_cap = bytes;
    return HVX_OK;
}

// Reserves and carves g->lists_buf for b queries with ctl_per_query control words each, and fills in what the two per-query kernels'
// arguments share: the CSR, the staged seeds, the mask, the slots.
template <typename Args>
int lists_carve(hvx_csr *g, uint32_t b, uint32_t max_frontier, uint32_t ctl_per_query, const uint32_t *h_off, const uint32_t *h_seed,
                const uint64_t *node_mask_words, ListsView *view, Args *a) {
    const size_t slots = (size_t)b * max_frontier;
    view->ctl_words = (size_t)b * ctl_per_query;
    int rc = lists_reserve(g, slots * 8 + slots * 2 * 4 + view->ctl_words * 4);
    if (rc) return rc;
    view->ids = static_cast<uint64_t *>(g->lists_buf);
    view->front = reinterpret_cast<uint32_t *>(view->ids + slots);
    view->ctl = view->front + slots * 2;
    memset(a, 0, sizeof(*a));
    a->g = csr_view(g);
    a->seeds = h_seed; a->seed_off = h_off;
    a->mask = node_mask_words ? g->mask_dev : nullptr;
    a->max_frontier = max_frontier;
    a->front = view->front;
    a->out_ids = reinterpret_cast<unsigned long long *>(view->ids);
    a->lens = view->ctl; a->status = view->ctl + b;
    return HVX_OK;
}

// caller holds g->mu; b != 0.  Seeds and offsets into the pinned buffer, labels and mask uploads and the chain kernel enqueued on `s`.
int lists_enqueue(hvx_csr *g, hipStream_t s, uint32_t b, const uint64_t *seeds, const uint64_t *seed_offsets, const PathPlan &p,
                  const uint64_t *node_mask_words, uint32_t max_frontier, ListsView *view) {
    HIP_TRY(hipSetDevice(g->device));
    int rc;
    const uint32_t *h_off, *h_seed;
    if ((rc = lists_stage_seeds(g, s, b, seeds, seed_offsets, &h_off, &h_seed))) return rc;
    if ((rc = upload_labels(g, p.labels, p.n_labels, s))) return rc;
    if (node_mask_words && (rc = stage_bitmap(g, s, node_mask_words, &g->mask_dev, &g->h_mask))) return rc;
    PathListsArgs a;
    if ((rc = lists_carve(g, b, max_frontier, 2 + kMaxPathHops, h_off, h_seed, node_mask_words, view, &a))) return rc;
    a.n_hops = p.n_hops;
    for (uint32_t i = 0; i < p.n_hops; ++i) { a.direction[i] = p.direction[i]; a.label_off[i] = p.lab0(i); a.label_off[i + 1] = p.lab0(i) + p.lab_n(i); }
    a.labels = g->labels;
    a.hop_sizes = view->ctl + 2 * (size_t)b;
    HIP_TRY(launch_path_lists(a, b, s));
    return HVX_OK;
}

void lists_sizes_out(const uint32_t *ctl, uint32_t b, uint32_t n_hops, uint64_t *out_hop_sizes) {
    if (!out_hop_sizes) return;
    for (uint32_t q = 0; q < b; ++q)
        for (uint32_t i = 0; i < n_hops; ++i) out_hop_sizes[(size_t)q * n_hops + i] = ctl[2 * (size_t)b + (size_t)q * kMaxPathHops + i];
}

// the read-back of the two hvx_expand_*_lists calls: every slot, the control words into *ctl, lengths and statuses out of them
int lists_readback(hvx_csr *g, const ListsView &v, uint32_t b, uint32_t max_frontier, uint64_t *out_ids, uint32_t *out_lens, uint32_t *out_status,
                   std::vector<uint32_t> *ctl) {
    ctl->resize(v.ctl_words);
    HIP_TRY(hipMemcpyAsync(ctl->data(), v.ctl, v.ctl_words * 4, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(out_ids, v.ids, (size_t)b * max_frontier * 8, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    for (uint32_t q = 0; q < b; ++q) { out_lens[q] = (*ctl)[q]; out_status[q] = (*ctl)[b + q]; }
    return HVX_OK;
}

// The fused per-query calls around their kernel: the argument rules (`check` = the graph side's own), both locks, the plan, then
// `run(ix, g)` under the locks.  These calls ARE the exact scan (as hvx_batcher_new_restricted): a plan that would walk a set of
// max_frontier ids is not served.  `what`: "chains" / "repeats".
template <typename Check, typename Run>
int lists_search_admit(const hvx_index *cix, const hvx_csr *cg, const float *queries, uint32_t b, const hvx_restricted_params *params, const void *out_ids,
                       const void *out_scores, const void *out_counts, const void *out_status, uint32_t max_frontier, const char *what, Check check, Run run) {
    if (!cix || !cg || !params || !out_ids || !out_scores || !out_counts || !out_status || (b && !queries)) return fail(HVX_ERR_INVARIANT, "null argument");
    if (params->strategy > HVX_RESTRICTED_REFERENCE_PLAN) return fail(HVX_ERR_INVARIANT, "unknown restricted strategy %u", params->strategy);
    hvx_index *ix = const_cast<hvx_index *>(cix);
    hvx_csr *g = const_cast<hvx_csr *>(cg);
    const uint32_t k = params->k;
    if (k == 0) return fail(HVX_ERR_K_RANGE, "result count must be non-zero");
    if (params->ef < k) return fail(HVX_ERR_K_RANGE, "search beam width %u is below the result count %u", params->ef, k);
    if (ix->device != g->device) return fail(HVX_ERR_INVARIANT, "index and graph live on different devices");
    int rc = check();
    if (rc) return rc;
    if (b > ix->max_batch) return fail(HVX_ERR_UNSUPPORTED, "batch %u exceeds max_batch %u given at import", b, ix->max_batch);
    std::lock_guard<std::mutex> glock(g->mu);
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->sync_rewrites();
    RestrictedPlan plan;
    if (params->strategy == HVX_RESTRICTED_FILTERED || params->strategy == HVX_RESTRICTED_REFERENCE_PLAN || params->explicit_budgets ||
        restricted_make_plan(*params, max_frontier, ix->dev.dim, &plan, ix) != HVX_OK || plan.strategy != HVX_RESTRICTED_EXACT)
        return fail(HVX_ERR_UNSUPPORTED, "per-query %s are answered by the exact scan: strategy EXACT, or AUTO with max_frontier x row bytes within the "
                    "device plan's limit, and no explicit budgets", what);
    if (!restricted_direct_supported(ix, k))
        return fail(HVX_ERR_UNSUPPORTED, "the one-launch restricted scan serves k <= 800 over f32 / bf16 rows of a non-empty image");
    return b == 0 ? HVX_OK : run(ix, g);
}

// the graph side's word over the scan's: candidates per query, and a request that outgrew its slot keeps that status whatever the scan
// made of the query vector
void lists_overlay(const uint32_t *ctl, uint32_t b, uint64_t *out_candidates, uint32_t *out_status, uint32_t *out_counts) {
    for (uint32_t q = 0; q < b; ++q) {
        if (out_candidates) out_candidates[q] = ctl[q];
        if (ctl[b + q] != HVX_OK) {
            out_status[q] = ctl[b + q];
            out_counts[q] = 0;
        }
    }
}

} // namespace

extern "C" int hvx_expand_path_lists(const hvx_csr *cg, uint32_t b, const uint64_t *seeds, const uint64_t *seed_offsets, uint32_t n_hops,
                                     const uint32_t *hop_direction, const uint32_t *hop_label_offsets, const uint32_t *hop_labels,
                                     const uint64_t *node_mask_words, uint32_t max_frontier, uint64_t *out_ids, uint32_t *out_lens,
                                     uint32_t *out_status, uint64_t *out_hop_sizes) {
    if (!cg || !out_ids || !out_lens || !out_status) return fail(HVX_ERR_INVARIANT, "null argument");
    hvx_csr *g = const_cast<hvx_csr *>(cg);
    PathPlan p;
    int rc = lists_check(g, b, seeds, seed_offsets, n_hops, hop_direction, hop_label_offsets, hop_labels, max_frontier, &p);
    if (rc) return rc;
    if (b == 0) return HVX_OK;
    std::lock_guard<std::mutex> lock(g->mu);
    ListsView v;
    if ((rc = lists_enqueue(g, g->stream, b, seeds, seed_offsets, p, node_mask_words, max_frontier, &v))) {
        (void)hipStreamSynchronize(g->stream);
        return rc;
    }
    std::vector<uint32_t> ctl;
    if ((rc = lists_readback(g, v, b, max_frontier, out_ids, out_lens, out_status, &ctl))) return rc;
    lists_sizes_out(ctl.data(), b, n_hops, out_hop_sizes);
    return HVX_OK;
}

extern "C" int hvx_prefilter_path_search_lists_params(const hvx_index *cix, const hvx_csr *cg, const float *queries, uint32_t b,
                                                      const hvx_restricted_params *params, const uint64_t *seeds, const uint64_t *seed_offsets,
                                                      uint32_t n_hops, const uint32_t *hop_direction, const uint32_t *hop_label_offsets,
                                                      const uint32_t *hop_labels, const uint64_t *node_mask_words, uint32_t max_frontier,
                                                      uint64_t *out_ids, float *out_scores, uint32_t *out_counts, uint32_t *out_status,
                                                      uint64_t *out_candidates, uint64_t *out_hop_sizes, hvx_stats *stats) {
    PathPlan p;
    return lists_search_admit(cix, cg, queries, b, params, out_ids, out_scores, out_counts, out_status, max_frontier, "chains", [&] {
        return lists_check(cg, b, seeds, seed_offsets, n_hops, hop_direction, hop_label_offsets, hop_labels, max_frontier, &p);
    }, [&](hvx_index *ix, hvx_csr *g) -> int {
        hipStream_t s = ix->stream;
        ListsView v;
        int rc;
        if ((rc = lists_enqueue(g, s, b, seeds, seed_offsets, p, node_mask_words, max_frontier, &v)) ||
            (rc = restricted_direct_lists_devlens(ix, queries, b, params->k, v.ids, max_frontier, v.ctl, v.ctl_words, out_ids, out_scores, out_counts,
                                                  out_status, stats))) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        lists_overlay(ix->h_flags, b, out_candidates, out_status, out_counts);
        lists_sizes_out(ix->h_flags, b, n_hops, out_hop_sizes);
        return HVX_OK;
    });
}

// ---------------------------------------------------------------------------------------------
// repeat(expand).times(n).emit() with per-query seeds (control/repeat.rs:24-99): the same loop (body hop, times, emit mode, `until`
// predicate, Filter step) for every request of a batch, each request from its own start nodes.  One launch of repeat_lists_kernel
// (hvx_prefilter_repeat.hip) runs every loop and leaves query q's emitted set in slot q of the one-launch scan.
// ---------------------------------------------------------------------------------------------
namespace {

// the argument rules of both entry points: nothing is enqueued, nothing of the graph is touched
int repeat_check(const hvx_csr *g, uint32_t b, const uint64_t *seeds, const uint64_t *seed_offsets, uint32_t times, uint32_t emit, uint32_t direction,
                 const uint32_t *allowed_label_ids, uint32_t n_labels, uint32_t max_frontier) {
    if (times == 0 || times > kMaxPathHops) return fail(HVX_ERR_INVARIANT, "repeat runs 1 .. %u times, not %u", kMaxPathHops, times);
    if (emit < HVX_REPEAT_EMIT_BEFORE || emit > HVX_REPEAT_EMIT_ALL)
        return fail(HVX_ERR_INVARIANT, "emit mode %u: BEFORE, AFTER or ALL (emit None is the chain of hvx_expand_path_lists)", emit);
    if (n_labels && !allowed_label_ids) return fail(HVX_ERR_INVARIANT, "null labels");
    PathPlan body; // the seed and slot rules are the chain's, over a plan of the one body hop
    return lists_check(g, b, seeds, seed_offsets, 1, &direction, nullptr, nullptr, max_frontier, &body);
}

// caller holds g->mu; b != 0.  Seeds and offsets into the pinned buffer, label and bitmap uploads and the repeat kernel enqueued on `s`.
int repeat_enqueue(hvx_csr *g, hipStream_t s, uint32_t b, const uint64_t *seeds, const uint64_t *seed_offsets, uint32_t times, uint32_t emit,
                   uint32_t direction, const uint32_t *allowed_label_ids, uint32_t n_labels, const uint64_t *until_mask_words,
                   const uint64_t *node_mask_words, uint32_t max_frontier, ListsView *view) {
    HIP_TRY(hipSetDevice(g->device));
    int rc;
    const uint32_t *h_off, *h_seed;
    if ((rc = lists_stage_seeds(g, s, b, seeds, seed_offsets, &h_off, &h_seed))) return rc;
    if ((rc = upload_labels(g, allowed_label_ids, n_labels, s))) return rc;
    if (until_mask_words && (rc = stage_bitmap(g, s, until_mask_words, &g->until_dev, &g->h_until))) return rc;
    if (node_mask_words && (rc = stage_bitmap(g, s, node_mask_words, &g->mask_dev, &g->h_mask))) return rc;
    RepeatListsArgs a; // the chain's buffer, with one more control word per query
    if ((rc = lists_carve(g, b, max_frontier, 3 + kMaxPathHops, h_off, h_seed, node_mask_words, view, &a))) return rc;
    a.times = times; a.emit = emit; a.direction = direction; a.n_allowed = n_labels;
    a.allowed = g->labels;
    a.until = until_mask_words ? g->until_dev : nullptr;
    a.emit_sizes = view->ctl + 2 * (size_t)b;
    a.stop_depth = view->ctl + (2 + kMaxPathHops) * (size_t)b;
    HIP_TRY(launch_repeat_lists(a, b, s));
    return HVX_OK;
}

void repeat_ctl_out(const uint32_t *ctl, uint32_t b, uint32_t times, uint32_t *out_stop_depth, uint64_t *out_emit_sizes) {
    lists_sizes_out(ctl, b, times, out_emit_sizes);
    if (out_stop_depth)
        for (uint32_t q = 0; q < b; ++q) out_stop_depth[q] = ctl[(2 + kMaxPathHops) * (size_t)b + q];
}

} // namespace

extern "C" int hvx_expand_repeat_lists(const hvx_csr *cg, uint32_t b, const uint64_t *seeds, const uint64_t *seed_offsets, uint32_t times,
                                       uint32_t emit, uint32_t direction, const uint32_t *allowed_label_ids, uint32_t n_labels,
                                       const uint64_t *until_mask_words, const uint64_t *node_mask_words, uint32_t max_frontier,
                                       uint64_t *out_ids, uint32_t *out_lens, uint32_t *out_status, uint32_t *out_stop_depth,
                                       uint64_t *out_emit_sizes) {
    if (!cg || !out_ids || !out_lens || !out_status) return fail(HVX_ERR_INVARIANT, "null argument");
    hvx_csr *g = const_cast<hvx_csr *>(cg);
    int rc = repeat_check(g, b, seeds, seed_offsets, times, emit, direction, allowed_label_ids, n_labels, max_frontier);
    if (rc) return rc;
    if (b == 0) return HVX_OK;
    std::lock_guard<std::mutex> lock(g->mu);
    ListsView v;
    if ((rc = repeat_enqueue(g, g->stream, b, seeds, seed_offsets, times, emit, direction, allowed_label_ids, n_labels, until_mask_words,
                             node_mask_words, max_frontier, &v))) {
        (void)hipStreamSynchronize(g->stream);
        return rc;
    }
    std::vector<uint32_t> ctl;
    if ((rc = lists_readback(g, v, b, max_frontier, out_ids, out_lens, out_status, &ctl))) return rc;
    repeat_ctl_out(ctl.data(), b, times, out_stop_depth, out_emit_sizes);
    return HVX_OK;
}

extern "C" int hvx_prefilter_repeat_search_lists_params(const hvx_index *cix, const hvx_csr *cg, const float *queries, uint32_t b,
                                                        const hvx_restricted_params *params, const uint64_t *seeds, const uint64_t *seed_offsets,
                                                        uint32_t times, uint32_t emit, uint32_t direction, const uint32_t *allowed_label_ids,
                                                        uint32_t n_labels, const uint64_t *until_mask_words, const uint64_t *node_mask_words,
                                                        uint32_t max_frontier, uint64_t *out_ids, float *out_scores, uint32_t *out_counts,
                                                        uint32_t *out_status, uint64_t *out_candidates, uint32_t *out_stop_depth,
                                                        uint64_t *out_emit_sizes, hvx_stats *stats) {
    return lists_search_admit(cix, cg, queries, b, params, out_ids, out_scores, out_counts, out_status, max_frontier, "repeats", [&] {
        return repeat_check(cg, b, seeds, seed_offsets, times, emit, direction, allowed_label_ids, n_labels, max_frontier);
    }, [&](hvx_index *ix, hvx_csr *g) -> int {
        hipStream_t s = ix->stream;
        ListsView v;
        int rc;
        if ((rc = repeat_enqueue(g, s, b, seeds, seed_offsets, times, emit, direction, allowed_label_ids, n_labels, until_mask_words, node_mask_words,
                                 max_frontier, &v)) ||
            (rc = restricted_direct_lists_devlens(ix, queries, b, params->k, v.ids, max_frontier, v.ctl, v.ctl_words, out_ids, out_scores, out_counts,
                                                  out_status, stats))) {
            (void)hipStreamSynchronize(s);
            return rc;
        }
        lists_overlay(ix->h_flags, b, out_candidates, out_status, out_counts);
        repeat_ctl_out(ix->h_flags, b, times, out_stop_depth, out_emit_sizes);
        return HVX_OK;
    });
}
