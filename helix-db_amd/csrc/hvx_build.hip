// hvx_build.hip -- GPU-assisted HNSW build: the reference's insert path
// (crates/db/src/search/vector/mutation.rs:642-895 insert_with_mutation_cache / insert_hnsw) for BATCHES of nodes on
// the device, over an index image whose rows are already resident in HBM.
//
// Per batch of B new nodes (consecutive ids; every node of a batch sees the graph as of the batch start):
//   1. search   hnsw_wave_kernel<BUILD> -- greedy descent above min(level, max_layer), search_layer_beam
//               (mutation.rs:904-1005) on every layer from there to 0; per layer the first 2*Mmax entries of W
//   2. select   build_select_kernel    -- select_neighbors_heuristic (mutation.rs:1072-1097) = select_diverse
//               (mod.rs:809-856) over those hydrated candidates, backfill; writes the new node's canonical row
//   3. link     build_link_kernel / build_link_wg_kernel -- add_bidirectional_link (mutation.rs:1498-1583) for every selected neighbour IN
//               SELECTION ORDER: append, and when the row exceeds Mmax rank its neighbours by distance to the row's owner,
//               select_diverse + backfill, canonical row (neighbor_set.rs:1-9), remove the reverse edge of every dropped
//               neighbour (mutation.rs:1890-1908).  One wavefront per new node; a row is changed under its owner's lock.
// With B = 1 this IS the reference's sequential insertion: rows equal the oracle's row for row (tests).  With B > 1 the
// nodes of one batch do not see each other and the order in which concurrent links reach a shared neighbour is not
// defined; the result is a valid (symmetric, degree-bounded, canonical) HNSW graph whose recall / work match the
// sequential one (bench.py graph_equivalence).  A node whose level exceeds the current top layer always forms its own
// batch (it becomes the entry point, mutation.rs:769-772).
//
// Every distance is the reference-order f32 distance of hvx_device.h (group_distance), so `dist(c,s) < dist(c,q)` decisions
// are the CPU path's.  Served shapes: f32 rows of any dimension, L2 / cosine / Manhattan, every summation tree (the unrolled
// search builds for L2 / cosine + AVX+FMA + dim in {128,...,1536} + ef_construction <= 352, the GENERIC build of the same kernel
// otherwise; select / link kernels per metric and tree), m0 <= 64 (m <= 32), ef_construction <= 800.  The kernels of THIS file hold one id
// per lane and 64-bit masks: degree limits up to 32.  Limits up to 64 (the reference's scale fixture, M 32 / M0 64) run the kernels of
// hvx_build_wide.hip -- two ids per lane, 128-bit masks, 128 search candidates per layer and node;
// their one-node steps are the two many-workgroup kernels of hvx_build_wide_seq.hip (f32 and bf16 rows; link_mode = 1: the one-wavefront
// kernels); their batches hold half the fraction and do not overlap search and link.
// bf16 images (hvx_index_build with dtype bf16, inserts, upserts, hvx_index_link_rows): the same loop over the packed rows.  The build search
// takes the batch's rows widened to f32 as its queries (decode_rows_bf16_kernel), the BF builds of the select / link kernels widen bf16 rows
// on their way into LDS (stage_row<BF>; build_link_wg_kernel<.., BF> in hvx_build_link_wg.h, instantiated in hvx_build_bf16.hip), the one-node
// steps read them in place (pair_distance<.., BF>): every distance is the reference's on the ROUNDED vectors, bit for bit.
// WHICH of these kernels a batch runs, with what grids and LDS, is decided on the host by plan_write_batch() in hvx_build_plan.h, next to the
// degree limits and their defaults, the refusals, the link workgroups' geometry, the batch sizes and the scratch layout; insert_range below
// is a loop over those plans and launch_write_batch the one switch that maps a plan to launches.
// Round 3: the batched link step runs one WORKGROUP per link with the prune evaluated from LDS (build_link_wg_kernel below) and
// the search side two wavefronts per SIMD for batches > 1 024 nodes: 1M x 768 in 4.1 s (round 2: 10.0 s).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hvx_host.h"
#include "hvx_graph_dev.h"
#include "hvx_build_plan.h"
#include "hvx_build_link_wg.h"

using namespace hvx;

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(HVX_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

namespace hvx {


// ---- step 2: the new node's own neighbour lists ----
template <uint32_t METRIC, bool FUSED, bool BF> __global__ __launch_bounds__(64) void build_select_kernel(BuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DevIndex &ix = a.ix;
    const uint32_t q = blockIdx.x, layer = blockIdx.y;
    const int lane = (int)threadIdx.x;
    const uint32_t node = a.nodes[q];
    const uint32_t lv = ix.level[node];
    const uint32_t top = lv < a.layers - 1u ? lv : a.layers - 1u; // min(node level, old max_layer)
    if (layer > top) return; // layers above the old top stay empty rows (mutation.rs:883-894)
    BuildLds L = carve_build(smem, ix.ld);
    const uint32_t maxn = layer == 0u ? a.m0 : a.m;
    const size_t slot = (size_t)layer * a.b + q;
    const uint32_t cnt = a.cand_cnt[slot];
    const uint32_t hyd = cnt < 2u * maxn ? cnt : 2u * maxn; // select_neighbors_heuristic hydrates the first 2*Mmax only
    if ((uint32_t)lane < hyd) {
        L.cid[lane] = (uint32_t)a.cand_ids[slot * kCand + lane];
        L.csc[lane] = a.cand_sc[slot * kCand + lane];
    }
    __syncthreads();
    const uint32_t ns = select_diverse_dev<METRIC, FUSED, BF>(ix, L, hyd, maxn, lane);
    if ((uint32_t)lane < ns) a.sel[slot * 32u + lane] = L.kept[lane];
    if (lane == 0) a.sel_cnt[slot] = ns;
    uint32_t stride;
    uint32_t *row = row_ptr(a, node, layer, stride);
    store_canonical(row, stride, L.kept, ns, lane, false); // nobody else can reach this row before the link step
}

// remove `victim` from the row of `owner` on `layer` (mutation.rs:1890-1908), under owner's lock
__device__ __forceinline__ void remove_edge_dev(const BuildArgs &a, uint32_t layer, uint32_t owner, uint32_t victim, int lane) {
    lock_row(a.locks, owner, lane);
    uint32_t stride;
    uint32_t *row = row_ptr(a, owner, layer, stride);
    const uint32_t v = (uint32_t)lane < stride ? ld_row(row + lane) : kSentinel;
    const bool keep = v != kSentinel && v != victim;
    const unsigned long long km = __ballot(keep);
    const uint32_t pos = (uint32_t)__builtin_popcountll(km & ((1ull << lane) - 1ull));
    const uint32_t nk = (uint32_t)__builtin_popcountll(km);
    __syncthreads();
    if (keep) st_row(row + pos, v);
    if ((uint32_t)lane >= nk && (uint32_t)lane < stride) st_row(row + lane, kSentinel);
    unlock_row(a.locks, owner, lane);
}

// ---- step 3: bidirectional links of the new node, in selection order, top layer first ----
template <uint32_t METRIC, bool FUSED, bool BF> __global__ __launch_bounds__(64) void build_link_kernel(BuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DevIndex &ix = a.ix;
    const uint32_t q = blockIdx.x;
    const int lane = (int)threadIdx.x, grp = lane >> 3, j = lane & 7;
    const uint32_t me = a.nodes[q];
    const uint32_t lv = ix.level[me];
    const uint32_t top = lv < a.layers - 1u ? lv : a.layers - 1u;
    BuildLds L = carve_build(smem, ix.ld);
    for (int32_t layer = (int32_t)top; layer >= 0; --layer) {
        const uint32_t maxn = layer == 0 ? a.m0 : a.m;
        const size_t slot = (size_t)layer * a.b + q;
        const uint32_t ns = a.sel_cnt[slot];
        for (uint32_t s = 0; s < ns; ++s) {
            const uint32_t to = a.sel[slot * 32u + s];
            // add_bidirectional_link(from = me, to) (mutation.rs:1498-1583)
            lock_row(a.locks, to, lane);
            uint32_t stride;
            uint32_t *row = row_ptr(a, to, (uint32_t)layer, stride);
            uint32_t v = (uint32_t)lane < stride ? ld_row(row + lane) : kSentinel;
            uint32_t deg = (uint32_t)__builtin_popcountll(__ballot(v != kSentinel));
            const bool present = __ballot(v == me) != 0ull;
            if (!present) {
                if (deg >= 64u) { if (lane == 0) *a.err = 1u; unlock_row(a.locks, to, lane); continue; }
                if ((uint32_t)lane == deg) v = me; // rows are canonical: the valid ids occupy lanes 0..deg-1
                ++deg;
            }
            const uint32_t nc = deg;
            uint32_t dropped_id = kSentinel; // per lane: a candidate this prune removed
            if (nc > maxn) {
                // rank the row's neighbours by distance to its owner, select_diverse with the owner as the reference point
                stage_row<BF>(ix, L.qv, to, lane);
                const float thdr = ix.hdr[to];
                __syncthreads();
                if ((uint32_t)lane < nc) L.kept[lane] = v; // scratch: unsorted candidate ids
                __syncthreads();
                for (uint32_t p0 = 0; p0 < nc; p0 += 8) {
                    const uint32_t g = p0 + (uint32_t)grp;
                    const uint32_t other = L.kept[g < nc ? g : nc - 1u];
                    const float d = staged_distance<METRIC, FUSED, BF>(ix, L.qv, thdr, other, j);
                    if (g < nc && j == 0) L.dtmp[g] = d;
                }
                __syncthreads();
                const float dmine = (uint32_t)lane < nc ? L.dtmp[lane] : 0.f;
                uint32_t rank = 0;
                for (uint32_t t = 0; t < nc; ++t) { // Candidate order: score, then id (model.rs:55-61)
                    const float dt = L.dtmp[t];
                    const uint32_t it = L.kept[t];
                    rank += (dt < dmine || (dt == dmine && it < v)) ? 1u : 0u;
                }
                __syncthreads();
                if ((uint32_t)lane < nc) { L.cid[rank] = v; L.csc[rank] = dmine; }
                __syncthreads();
                const uint32_t keepn = select_diverse_dev<METRIC, FUSED, BF>(ix, L, nc, maxn, lane);
                bool kept_mine = false;
                for (uint32_t t = 0; t < keepn; ++t) kept_mine |= L.kept[t] == v;
                if ((uint32_t)lane < nc && !kept_mine) dropped_id = v;
                store_canonical(row, stride, L.kept, keepn, lane, true);
            } else if (!present) {
                __syncthreads();
                if ((uint32_t)lane < nc) L.kept[lane] = v;
                __syncthreads();
                store_canonical(row, stride, L.kept, nc, lane, true);
            }
            unlock_row(a.locks, to, lane);
            // every neighbour dropped by the prune loses its edge to `to` as well: the graph stays symmetric
            unsigned long long dm = __ballot(dropped_id != kSentinel);
            while (dm) {
                const uint32_t src = (uint32_t)__builtin_ctzll(dm);
                dm &= dm - 1ull;
                const uint32_t x = __builtin_amdgcn_readlane(dropped_id, src);
                remove_edge_dev(a, (uint32_t)layer, x, to, lane);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// ONE node at a time (sequential mode = the reference's order exactly; every upsert; promotions): round 6.  build_select_kernel and
// build_link_kernel evaluate select_diverse lazily on one wavefront -- a chain of dependent row gathers per candidate: 0.33 ms + 2.0 ms of
// a 2.9-ms insert at 600 000 x 768 (profiles/r06o_seq_insert_kernel_stats.csv).  The two kernels below evaluate the distance matrices of
// ALL prunes of a step up front, spread over the layer's workgroups (one 8-lane group per pair, reference summation order), and the last
// workgroup to deliver replays the decisions from registers (hvx_graph_dev.h: replay_rows) -- as the delete steps do (hvx_delete.hip):
//   build_select_seq_kernel   the node's own lists: <= 64 search candidates per layer, 2 016 pairs, one replay per layer;
//   build_link_seq_kernel     add_bidirectional_link for its <= 32 selected neighbours per layer IN SELECTION ORDER.  A link reads the
//                             neighbour's row as earlier links of the same node left it -- and the only thing an earlier link can do to it
//                             is REMOVE an id (a neighbour its prune dropped loses the reverse edge).  So: every link's list (row + the
//                             node) and its matrix are taken from the rows as the kernel finds them -- a superset of what the link will
//                             see --, sixteen wavefronts replay the links speculatively in parallel, and one wavefront then walks them in
//                             order: a link whose row an earlier link has touched is replayed again over the ids that are still there
//                             (replay_rows' `alive` mask), everything else stands.  The removals (row of the dropped id loses the
//                             neighbour) go out last, all victims of a row at once.
// Same distances, same comparisons, same order of decisions as the one-wavefront kernels: tests/test_gpu_build.py holds both to the oracle
// row for row (hvx_build_params.link_mode = 1 selects the one-wavefront kernels).
// ---------------------------------------------------------------------------------------------------------------------------------

template <uint32_t METRIC, bool FUSED, bool BF> __global__ __launch_bounds__(256) void build_select_seq_kernel(BuildArgs a) {
    __shared__ uint32_t s_cid[64], s_wsc[128], s_last;
    const DevIndex &ix = a.ix;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t L, g, G;
    if (blockIdx.x < a.g0) { L = 0u; g = blockIdx.x; G = a.g0; }
    else { L = 1u + (blockIdx.x - a.g0) / a.gu; g = (blockIdx.x - a.g0) % a.gu; G = a.gu; }
    const uint32_t node = a.nodes[0];
    const uint32_t lv = ix.level[node];
    const uint32_t top = lv < a.layers - 1u ? lv : a.layers - 1u; // min(node level, old max_layer)
    if (L > top) return; // layers above the old top stay empty rows (mutation.rs:883-894)
    const uint32_t maxn = L == 0u ? a.m0 : a.m;
    const size_t slot = (size_t)L * a.b;
    const uint32_t cnt = a.cand_cnt[slot];
    const uint32_t hyd = cnt < 2u * maxn ? cnt : 2u * maxn; // select_neighbors_heuristic hydrates the first 2*Mmax only
    float *gl = a.gdm + (size_t)L * kSeqLayerDm;
    if (tid < hyd) s_cid[tid] = (uint32_t)a.cand_ids[slot * kCand + tid];
    __syncthreads();
    bool last = g == 0u;
    const uint32_t npairs = hyd * (hyd - (hyd ? 1u : 0u)) / 2u;
    if (npairs != 0u) {
        if (g == 0u && tid < hyd) st_agent(gl + hyd * 64u + tid, a.cand_sc[slot * kCand + tid]); // the owner's row: the search's scores
        const int j = (int)(lane & 7u);
        for (uint32_t q = g * 32u + (tid >> 3); q < npairs; q += G * 32u) {
            uint32_t i, jj;
            pair_of(q, i, jj); // 0 <= jj < i < hyd
            const uint32_t ni = s_cid[i], nj = s_cid[jj];
            const float d = pair_distance<METRIC, FUSED, BF>(ix, ni, nj, j);
            if (j == 0) { st_agent(gl + i * 64u + jj, d); st_agent(gl + jj * 64u + i, d); }
        }
        last = last_workgroup(a.tick, L, G, &s_last, true); // (hvx_handoff.h; the ticket goes back to zero)
    }
    if (!last || wave != 0u) return;
    const WaveScratch W{s_wsc, s_wsc + 64};
    uint32_t ns = hyd;
    bool bad = false;
    if (hyd >= 2u) ns = replay_rows<64>(gl, s_cid, hyd, maxn, lane, W, &bad);
    else if (lane < hyd) W.kept[lane] = s_cid[lane];
    lds_order();
    const uint32_t kf = lane < ns ? W.kept[lane] : kSentinel;
    if (lane < ns) a.sel[slot * 32u + lane] = kf;
    if (lane == 0) a.sel_cnt[slot] = ns;
    uint32_t stride;
    uint32_t *row = row_ptr(a, node, L, stride);
    store_canonical_reg(row, stride, kf, ns, lane); // nobody else can reach this row before the link step
}

struct SeqLds {
    uint32_t *rcur, *rkept;   // [32][kSeqRS] a link's list (row + the node) / what stays of it
    uint32_t *rdeg, *rkn;     // [32] ids in the list (0: nothing to do) / ids that stay
    uint32_t *rdlo, *rdhi;    // [32] dropped ids by list position
    uint32_t *to;             // [32] the selected neighbours, selection order
    uint32_t *px, *pv;        // [kSeqPairs] removals: row px loses pv
    uint32_t *pbase;          // [34]
    uint32_t *wsc;            // [16][128]
};
__device__ __forceinline__ SeqLds carve_seq(char *smem) {
    SeqLds S;
    uint32_t *p = reinterpret_cast<uint32_t *>(smem);
    S.rcur = p; p += 32 * kSeqRS;
    S.rkept = p; p += 32 * kSeqRS;
    S.rdeg = p; p += 32; S.rkn = p; p += 32; S.rdlo = p; p += 32; S.rdhi = p; p += 32; S.to = p; p += 32;
    S.px = p; p += kSeqPairs; S.pv = p; p += kSeqPairs;
    S.pbase = p; p += 36;
    S.wsc = p;
    return S;
}

template <uint32_t METRIC, bool FUSED, bool BF> __global__ __launch_bounds__(1024) void build_link_seq_kernel(BuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ uint32_t s_err, s_last, s_np;
    const DevIndex &ix = a.ix;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t L, g, G;
    if (blockIdx.x < a.g0) { L = 0u; g = blockIdx.x; G = a.g0; }
    else { L = 1u + (blockIdx.x - a.g0) / a.gu; g = (blockIdx.x - a.g0) % a.gu; G = a.gu; }
    const uint32_t me = a.nodes[0];
    const uint32_t lv = ix.level[me];
    const uint32_t top = lv < a.layers - 1u ? lv : a.layers - 1u;
    if (L > top) return;
    const uint32_t maxn = L == 0u ? a.m0 : a.m;
    const size_t slot = (size_t)L * a.b;
    const uint32_t ns = a.sel_cnt[slot];
    if (ns == 0u) return;
    const SeqLds S = carve_seq(smem);
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (tid == 0) s_err = 0u;
    if (tid < ns) S.to[tid] = a.sel[slot * 32u + tid];
    __syncthreads();
    // ---- the links' lists, from the rows as they are now (every workgroup of the layer arrives at the same lists) ----
    for (uint32_t t = wave; t < ns; t += 16u) {
        const uint32_t to = S.to[t];
        uint32_t stride;
        const uint32_t *row = row_ptr(a, to, L, stride);
        uint32_t v = lane < stride ? ld_row(row + lane) : kSentinel;
        uint32_t deg = (uint32_t)__builtin_popcountll(__ballot(v != kSentinel));
        const bool present = __ballot(v == me) != 0ull;
        if (!present) {
            if (deg + 1u > kSeqRow) { if (lane == 0) s_err = 1u; deg = 0u; }
            else { if (lane == deg) v = me; ++deg; } // rows are canonical: the valid ids occupy lanes 0..deg-1
        } else if (deg > kSeqRow) { if (lane == 0) s_err = 1u; deg = 0u; }
        if (lane < deg) S.rcur[t * kSeqRS + lane] = v;
        if (lane == 0) S.rdeg[t] = deg;
    }
    __syncthreads();
    if (s_err) { if (g == 0u && tid == 0) *a.err = 1u; return; }
    if (wave == 0) { // first pair of every link's prune (a list within its limit needs no matrix)
        const uint32_t rd = lane < ns ? S.rdeg[lane] : 0u;
        const uint32_t np = rd > maxn ? (rd + 1u) * rd / 2u : 0u;
        uint32_t incl = np;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            const uint32_t o = __shfl_up(incl, sft, 64);
            if ((int)lane >= sft) incl += o;
        }
        if (lane < 32u) S.pbase[lane] = incl - np;
        if (lane == 31u) S.pbase[32] = incl;
    }
    __syncthreads();
    const uint32_t total = S.pbase[32];
    float *gl = a.gdm + (size_t)L * kSeqLayerDm + kSeqSelDm;
    pair_sweep<METRIC, FUSED, BF, 1024>(ix, S.pbase, ns, total, g, G, [&](uint32_t t) __attribute__((always_inline)) {
        return PairTask{S.rcur + t * kSeqRS, S.rdeg[t], S.to[t], gl + (size_t)t * kSeqLinkDm, kSeqRS};
    });
    // (the ticket is taken even when no list needs a matrix: the last workgroup rewrites rows the others are still reading their lists from)
    if (!last_workgroup(a.tick, a.layers + L, G, &s_last, true)) return;
    // ---- the last workgroup: every link replayed on its list as found (sixteen at a time) ...
    const WaveScratch W{S.wsc + wave * 128u, S.wsc + wave * 128u + 64u};
    bool bad = false; // (a distance that is no valid score: add_bidirectional_link does not look, neither does the one-wavefront kernel)
    for (uint32_t t = wave; t < ns; t += 16u) {
        const uint32_t deg = S.rdeg[t];
        const uint32_t *rc = S.rcur + t * kSeqRS;
        uint32_t kn = deg;
        unsigned long long dropped = 0ull;
        if (deg > maxn) kn = replay_rows<(int)kSeqRS>(gl + (size_t)t * kSeqLinkDm, rc, deg, maxn, lane, W, &bad, ~0ull, &dropped);
        else if (lane < deg) W.kept[lane] = rc[lane];
        lds_order();
        if (lane < kn) S.rkept[t * kSeqRS + lane] = W.kept[lane];
        if (lane == 0) { S.rkn[t] = kn; S.rdlo[t] = (uint32_t)dropped; S.rdhi[t] = (uint32_t)(dropped >> 32); }
        lds_order();
    }
    if (tid == 0) s_np = 0u;
    __syncthreads();
    // ---- ... then in selection order: a link whose row an earlier link has taken an id from is replayed over the ids still there
    if (wave == 0) {
        uint32_t np = 0;
        for (uint32_t s = 0; s < ns; ++s) {
            const uint32_t to = S.to[s], deg = S.rdeg[s];
            if (deg == 0u) continue;
            const uint32_t *rc = S.rcur + s * kSeqRS;
            const uint32_t mine = lane < deg ? rc[lane] : kSentinel;
            bool gone = false; // my id has been removed from this row by an earlier link
            for (uint32_t i = 0; i < np; ++i) gone |= S.px[i] == to && S.pv[i] == mine;
            const unsigned long long alive = __ballot(lane < deg && !gone);
            unsigned long long dropped = ((unsigned long long)S.rdhi[s] << 32) | S.rdlo[s];
            if (alive != (deg >= 64u ? ~0ull : (1ull << deg) - 1ull)) {
                const uint32_t nlive = (uint32_t)__builtin_popcountll(alive);
                uint32_t kn;
                dropped = 0ull;
                if (nlive > maxn) {
                    kn = replay_rows<(int)kSeqRS>(gl + (size_t)s * kSeqLinkDm, rc, deg, maxn, lane, W, &bad, alive, &dropped);
                } else {
                    if ((alive >> lane) & 1ull) W.kept[(uint32_t)__builtin_popcountll(alive & lt)] = mine;
                    kn = nlive;
                    lds_order();
                }
                if (lane < kn) S.rkept[s * kSeqRS + lane] = W.kept[lane];
                if (lane == 0) S.rkn[s] = kn;
                lds_order();
            }
            // every neighbour dropped by the prune loses its edge to `to` as well: the graph stays symmetric (mutation.rs:1890-1908)
            const bool drop_mine = ((dropped >> lane) & 1ull) != 0ull;
            const uint32_t at = np + (uint32_t)__builtin_popcountll(dropped & lt);
            if (drop_mine && at < kSeqPairs) { S.px[at] = mine; S.pv[at] = to; }
            np += (uint32_t)__builtin_popcountll(dropped);
            if (np > kSeqPairs) { if (lane == 0) *a.err = 1u; np = kSeqPairs; }
            lds_order();
        }
        if (lane == 0) s_np = np;
    }
    __syncthreads();
    // ---- the rows.  Every neighbour dropped by a prune loses its edge back (mutation.rs:1890-1908): a neighbour row (a link's own row) gets
    // its removals before it is stored -- one store per row, nothing in this kernel reads a row it has written --, every other row that
    // loses edges (the node's own among them) is read, compacted and stored by the first removal that names it
    const uint32_t np = s_np;
    for (uint32_t t = wave; t < ns; t += 16u) {
        if (S.rdeg[t] == 0u) continue;
        const uint32_t kn = S.rkn[t], to = S.to[t];
        const uint32_t v = lane < kn ? S.rkept[t * kSeqRS + lane] : kSentinel;
        bool victim = false;
        for (uint32_t k2 = 0; k2 < np; ++k2) victim |= S.px[k2] == to && S.pv[k2] == v;
        const bool keep = v != kSentinel && !victim;
        const unsigned long long km = __ballot(keep);
        const uint32_t nk = (uint32_t)__builtin_popcountll(km);
        // (compact: the ids that stay move to the low lanes)
        const uint32_t src = (uint32_t)__builtin_amdgcn_ds_permute((int)(((keep ? (uint32_t)__builtin_popcountll(km & lt) : 63u - (uint32_t)__builtin_popcountll(~km & lt))) << 2), (int)v);
        uint32_t stride;
        uint32_t *row = row_ptr(a, to, L, stride);
        if (nk > stride) { if (lane == 0) *a.err = 1u; continue; }
        store_canonical_reg(row, stride, lane < nk ? src : kSentinel, nk, lane);
    }
    for (uint32_t i = wave; i < np; i += 16u) {
        const uint32_t x = S.px[i];
        bool first = true;
        for (uint32_t k2 = 0; k2 < i; ++k2) first &= S.px[k2] != x;
        for (uint32_t t = 0; t < ns; ++t) first &= S.to[t] != x; // (a link's row: done above)
        if (!first) continue;
        uint32_t stride;
        uint32_t *row = row_ptr(a, x, L, stride);
        const uint32_t v = lane < stride ? ld_row(row + lane) : kSentinel;
        bool victim = false;
        for (uint32_t k2 = i; k2 < np; ++k2) victim |= S.px[k2] == x && S.pv[k2] == v;
        const bool keep = v != kSentinel && !victim;
        const unsigned long long km = __ballot(keep);
        const uint32_t pos = (uint32_t)__builtin_popcountll(km & lt), nk = (uint32_t)__builtin_popcountll(km);
        if (keep) st_row(row + pos, v); // every lane holds its id in a register: the order of the stores does not matter
        if (lane >= nk && lane < stride) st_row(row + lane, kSentinel);
    }
}

template <typename K> static hipError_t launch_step(K kern, const StepGeom &g, const BuildArgs &a, hipStream_t s) {
    if (g.lds > 48 * 1024) { // (46 KB at <= 33 candidate rows: only larger Mmax would need it; the attribute is per function AND device)
        const hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(g.gx, g.gy), dim3(g.threads), g.lds, s, a);
    return hipGetLastError();
}

// insertion order: position i inserts row (i * stride) mod n; stride 1 = id order, a stride coprime with n = a permutation that puts
// the nodes of a batch far apart in id space (hvx_build_params.scatter)
__global__ void iota_kernel(uint32_t *p, uint32_t count, uint32_t first, uint32_t stride, uint32_t mod) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < count) p[i] = stride == 1u ? first + i : (uint32_t)(((unsigned long long)(first + i) * stride) % mod);
}

// the build searches of a bf16 batch read the nodes' ROUNDED vectors as f32 queries: rows nodes[0 .. count) of the image, widened into
// out[count][dim] in plain order, one 16-byte piece per thread
__global__ void decode_rows_bf16_kernel(const uint16_t *vecb, const uint32_t *nodes, uint32_t count, uint32_t dim, float *out) {
    const uint32_t ppr = dim >> 3; // pieces per row
    const size_t e = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (e >= (size_t)count * ppr) return;
    const uint32_t i = (uint32_t)(e / ppr), t = (uint32_t)(e - (size_t)i * ppr);
    const uint4 x = reinterpret_cast<const uint4 *>(vecb + (size_t)nodes[i] * dim)[t];
    const uint32_t w[4] = {x.x, x.y, x.z, x.w};
    float lo[4], hi[4];
    bf16_piece_widen(w, lo, hi);
    float *dst = out + (size_t)i * dim + bf16_piece_dst(t);
    *reinterpret_cast<float4 *>(dst) = make_float4(lo[0], lo[1], lo[2], lo[3]);
    *reinterpret_cast<float4 *>(dst + 32) = make_float4(hi[0], hi[1], hi[2], hi[3]);
}

// one instantiation per (metric, summation tree): the reference picks both per index (spaces/*.rs, distance/*.rs)
struct BuildKernels {
    BuildKernel select, link, link_wg; // link_wg: null where the workgroup kernel has no instantiation (Manhattan)
    BuildKernel select_seq, link_seq;  // one node per step
};
template <uint32_t METRIC, bool FUSED> static BuildKernels build_kernels_of() {
    BuildKernels k{build_select_kernel<METRIC, FUSED, false>, build_link_kernel<METRIC, FUSED, false>, nullptr, build_select_seq_kernel<METRIC, FUSED, false>,
                   build_link_seq_kernel<METRIC, FUSED, false>};
    if constexpr (METRIC != kL1) k.link_wg = build_link_wg_kernel<METRIC, FUSED, false>;
    return k;
}
// bf16 images (L2 / cosine, the AVX+FMA tree: what the import accepts): every step reads the interleaved bf16 rows in place
template <uint32_t METRIC> static BuildKernels build_kernels_bf16() {
    return BuildKernels{build_select_kernel<METRIC, true, true>, build_link_kernel<METRIC, true, true>, build_link_wg_bf16_kernel(METRIC),
                        build_select_seq_kernel<METRIC, true, true>, build_link_seq_kernel<METRIC, true, true>};
}
static BuildKernels pick_build_kernels(uint32_t metric, bool fused, bool bf16 = false) {
    if (bf16) return metric == kL2 ? build_kernels_bf16<kL2>() : build_kernels_bf16<kCosine>();
    if (metric == kL2) return fused ? build_kernels_of<kL2, true>() : build_kernels_of<kL2, false>();
    if (metric == kCosine) return fused ? build_kernels_of<kCosine, true>() : build_kernels_of<kCosine, false>();
    return fused ? build_kernels_of<kL1, true>() : build_kernels_of<kL1, false>();
}

// a device temporary that lives as long as its scope
struct DevTemp {
    void *p = nullptr;
    DevTemp() = default;
    DevTemp(const DevTemp &) = delete;
    DevTemp &operator=(const DevTemp &) = delete;
    ~DevTemp() { if (p) (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

// the select and link launches of one batch, as planned (plan_write_batch, hvx_build_plan.h)
static hipError_t launch_write_batch(const WriteBatchPlan &p, const WriteCtx &c, const BuildKernels &kern, BuildArgs ba, hipStream_t s) {
    const bool fused = kernel_fused(ba.ix.fkernel);
    hipError_t e = hipSuccess;
    switch (p.select) {
    case SelectStep::narrow_wave: e = launch_step(kern.select, p.sel, ba, s); break;
    case SelectStep::narrow_eager:
        ba.g0 = p.sel.g0; ba.gu = p.sel.gu;
        hipLaunchKernelGGL(kern.select_seq, dim3(p.sel.gx), dim3(p.sel.threads), p.sel.lds, s, ba);
        ba.g0 = p.lnk.g0; ba.gu = p.lnk.gu;
        hipLaunchKernelGGL(kern.link_seq, dim3(p.lnk.gx), dim3(p.lnk.threads), p.lnk.lds, s, ba);
        e = hipGetLastError();
        break;
    case SelectStep::wide_wave: e = launch_build_select_wide(ba, fused, c.bf16, dim3(p.sel.gx, p.sel.gy), s); break;
    case SelectStep::wide_eager: // (both take their grids from wide_seq_geom, as the plan does)
        e = launch_build_select_wide_seq(ba, fused, c.bf16, s);
        if (e == hipSuccess) e = launch_build_link_wide_seq(ba, fused, c.bf16, s);
        break;
    }
    if (e != hipSuccess) return e;
    const LinkGeom &lg = p.link == LinkStep::wide_wg ? c.wide_link : c.link;
    ba.ldp = lg.ldp;
    ba.ncmax = lg.ncmax;
    ba.link_ck = lg.link_ck;
    switch (p.link) {
    case LinkStep::none: break;
    case LinkStep::narrow_wave: e = launch_step(kern.link, p.lnk, ba, s); break;
    case LinkStep::narrow_wg: e = launch_step(kern.link_wg, p.lnk, ba, s); break;
    case LinkStep::wide_wave: e = launch_build_link_wide(ba, fused, c.bf16, p.lnk.gx, s); break;
    case LinkStep::wide_wg: e = launch_build_link_wide_wg(ba, fused, p.lnk.gy, p.lnk.lds, s); break;
    }
    return e;
}

} // namespace hvx

extern "C" uint32_t hvx_index_last_write_path(const hvx_index *ix) { return ix ? ix->last_write_path : 0u; }
extern "C" uint32_t hvx_index_last_write_tie_overflows(const hvx_index *ix) { return ix ? ix->last_write_tie_overflows : 0u; }

extern "C" void hvx_build_params_default(hvx_build_params *p) {
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->ef_construction = 200; // DEFAULT_EF_CONSTRUCTION (mod.rs:702-708)
    p->max_batch = 2048;
    p->batch_divisor = 32;
}

// a refusal of write_refusal() in the caller's words: "device build" "s", "device inserts" ""
static int refuse_write(WriteRefusal r, const char *noun, const char *verb_s) {
    switch (r) {
    case kRefuseDegrees: return fail(HVX_ERR_UNSUPPORTED, "%s serve%s m0 <= 64 (m <= 32)", noun, verb_s);
    case kRefuseRowsNarrow: return fail(HVX_ERR_UNSUPPORTED, "the image's neighbour rows are narrower than the degree limits (build it with hvx_index_build)");
    case kRefuseRowsOver64: return fail(HVX_ERR_UNSUPPORTED, "%s with m0 > 32 serve%s neighbour rows of <= 64 ids", noun, verb_s);
    case kRefuseEf: return fail(HVX_ERR_UNSUPPORTED, "device build serves ef_construction <= 800");
    default: return HVX_OK;
    }
}

// The rows an insert_range call links: insertion positions [first, first + count) of an image that already holds their vectors, levels
// and (empty) neighbour rows.  Position p inserts row (p * stride) mod `mod` (stride 1: row p).
struct WriteRows {
    uint64_t first, count;
    uint32_t stride;
    uint64_t mod;
    const uint16_t *levels; // levels[0] is the level of row level_row0; null: every node on layer 0 only
    uint64_t level_row0;
    // bf16 images: the nodes' ROUNDED vectors as f32 [count][dim] on the device -- the queries of their build searches; null: every
    // batch's rows are widened from the image into the call's scratch on the search stream
    const float *build_q;
    uint64_t row_at(uint64_t pos) const { return stride == 1 ? pos : (pos * stride) % mod; }
    uint16_t level_at(uint64_t pos) const { return levels ? levels[row_at(pos) - level_row0] : 0; }
};

// insert_hnsw (mutation.rs:787-895) for the rows of `r`: batches of nodes searched on the handle's stream while the previous batch is
// selected and linked on a second one.  hvx_index_build runs it over a whole image (positions 0 .. n - 1, optionally scattered);
// hvx_index_insert_batch over the rows it has just appended (id order).  Every batch runs what plan_write_batch (hvx_build_plan.h) says.
// The handle is private to the caller for the duration (its lock is held or it has not been returned yet).
static int insert_range(hvx_index *ix, const WriteRows &r, const hvx_build_params *params, hvx_build_stats *stats) {
    if (r.count == 0) return HVX_OK;
    const uint64_t first = r.first, end = r.first + r.count;
    DevIndex &d = ix->dev;
    uint32_t top_level = d.has_entry ? d.max_layer : 0u;
    for (uint64_t p = first; p < end; ++p) top_level = std::max<uint32_t>(top_level, r.level_at(p));
    HIP_TRY(hipSetDevice(ix->device));
    hipStream_t s = ix->stream;
    const uint32_t layers_max = top_level + 1u;
    const WriteCtx ctx = write_ctx(d, ix->desc, *params, ix->max_batch, layers_max);
    const WriteDegrees &g = ctx.g;
    // degree limits above 32: twice the candidates and selected neighbours per layer and node, and the kernels of hvx_build_wide.hip
    const WriteRefusal refused = write_refusal(g, d.s0, d.su, kRefuseDegrees | (g.wide ? kRefuseRowsNarrow | kRefuseRowsOver64 : 0u));
    if (refused == kRefuseDegrees) return refuse_write(refused, "device build", "s");
    if (refused) return fail(HVX_ERR_UNSUPPORTED, "device build with m0 > 32 serves neighbour rows of m0 .. 64 ids");
    // Round 6: the scratch, the link stream and its events stay with the handle (a one-node insert / upsert paid nine hipMalloc + hipFree --
    // each a device synchronisation --, a stream and four events per call: ~2 ms of a 6.4-ms upsert).  Only tuning buffers are per call.
    // Round 4: the search of batch i + 1 runs on the handle's stream WHILE batch i is selected and linked on a second stream.  Batch i + 1
    // then does not see batch i -- which it tolerates exactly as the nodes of one batch tolerate not seeing each other: rows are only ever
    // read as stale-or-current (agent-scope stores by the link step, immutable vectors), never torn into invalid ids.  Candidate /
    // selection buffers are double-buffered; a promotion (new top layer = new entry point), a one-node batch and sequential mode do not overlap.
    int rc;
    const WriteScratch w = write_scratch(ctx, r.count, layers_max, d.dim, !r.build_q);
    if (w.need > ix->ins_cap) {
        ix->ins_cap = 0;
        if ((rc = ix->regrow(&ix->ins_scratch, w.need + w.need / 4))) return rc;
        if (hipMemsetAsync(ix->ins_scratch, 0, w.need + w.need / 4, s) != hipSuccess) return fail(HVX_ERR_DEVICE, "memset");
        ix->ins_cap = w.need + w.need / 4;
    }
    char *const base = reinterpret_cast<char *>(ix->ins_scratch);
    uint32_t *const d_tick = reinterpret_cast<uint32_t *>(base + w.tick), *const d_iota = reinterpret_cast<uint32_t *>(base + w.iota);
    uint64_t *const d_cids = reinterpret_cast<uint64_t *>(base + w.cids);
    float *const d_csc = reinterpret_cast<float *>(base + w.csc), *const d_gdm = reinterpret_cast<float *>(base + w.gdm);
    uint32_t *const d_cnt = reinterpret_cast<uint32_t *>(base + w.cnt), *const d_selcnt = reinterpret_cast<uint32_t *>(base + w.selcnt);
    uint32_t *const d_sel = reinterpret_cast<uint32_t *>(base + w.sel), *const d_status = reinterpret_cast<uint32_t *>(base + w.status);
    uint32_t *const d_err = reinterpret_cast<uint32_t *>(base + w.err);
    float *const d_bq = w.has_bq ? reinterpret_cast<float *>(base + w.bq) : nullptr;
    const uint64_t lock_rows = std::max<uint64_t>(std::max<uint64_t>(end, r.mod), ix->cap_rows);
    if (lock_rows > ix->ins_locks_rows) { // one lock per row the image can hold: all zero between calls (every lock taken is released)
        ix->ins_locks_rows = 0;
        if ((rc = ix->regrow((void **)&ix->ins_locks, lock_rows * 4))) return rc;
        if (hipMemsetAsync(ix->ins_locks, 0, lock_rows * 4, s) != hipSuccess) return fail(HVX_ERR_DEVICE, "memset");
        ix->ins_locks_rows = lock_rows;
    }
    if (!ix->ins_stream && hipStreamCreateWithFlags(&ix->ins_stream, hipStreamNonBlocking) != hipSuccess) return fail(HVX_ERR_DEVICE, "stream creation failed");
    for (int i = 0; i < 4; ++i)
        if (!ix->ins_ev[i] && hipEventCreateWithFlags(&ix->ins_ev[i], hipEventDisableTiming) != hipSuccess) return fail(HVX_ERR_DEVICE, "event creation failed");
    hipStream_t s2 = ix->ins_stream;
    hipEvent_t ev_search[2] = {ix->ins_ev[0], ix->ins_ev[1]}, ev_link[2] = {ix->ins_ev[2], ix->ins_ev[3]};
    bool link_pending[2] = {false, false};
    auto bail = [&](int code) { // (a failed call may leave locks / tickets set: the next call starts from fresh scratch)
        (void)hipStreamSynchronize(s);
        (void)hipStreamSynchronize(s2);
        ix->ins_cap = 0;
        ix->ins_locks_rows = 0;
        return code;
    };
    DevTemp dbg;
    if (tuning_env("HVX_BUILD_DEBUG")) {
        if (dbg.alloc(32) != hipSuccess) return bail(fail(HVX_ERR_DEVICE, "hipMalloc(32) build scratch"));
        if (hipMemsetAsync(dbg.p, 0, 32, s) != hipSuccess) return bail(fail(HVX_ERR_DEVICE, "memset"));
    }
    hipLaunchKernelGGL(iota_kernel, dim3((uint32_t)((r.count + 255) / 256)), dim3(256), 0, s, d_iota, (uint32_t)r.count, (uint32_t)first, r.stride, (uint32_t)std::max<uint64_t>(r.mod, 1));
    uint32_t *d_ties = d_err + 1; // nodes whose build search stayed flagged (the word next to the error word: one read for both)
    if (hipMemsetAsync(d_err, 0, 8, s) != hipSuccess) return bail(fail(HVX_ERR_DEVICE, "memset"));

    const BuildKernels kern = pick_build_kernels(d.metric, kernel_fused(d.fkernel), ctx.bf16);
    uint64_t done = first, batches = 0, singles = 0;
    if (!d.has_entry) { // the first node of an index: the entry point with empty rows on its layers (mutation.rs:706-739)
        d.has_entry = 1;
        d.entry = (uint32_t)r.row_at(first);
        d.max_layer = r.level_at(first);
        done = first + 1;
        singles = 1;
    }
    bool prev_serial = true; // the previous batch must be complete before the next search starts
    // the iota / lock / err initialisation above ran on `s`: the link stream starts behind it
    if (hipEventRecord(ev_search[0], s) != hipSuccess || hipStreamWaitEvent(s2, ev_search[0], 0) != hipSuccess)
        return bail(fail(HVX_ERR_DEVICE, "stream ordering failed"));
    while (done < end) {
        const uint16_t lv0 = r.level_at(done);
        const bool promotes = lv0 > d.max_layer;
        const uint32_t bsz = write_batch_size(ctx, done, end, promotes, [&](uint64_t pos) { return r.level_at(pos) > d.max_layer; });
        const uint32_t layers = d.max_layer + 1u; // old max_layer + 1
        const WriteBatchPlan plan = plan_write_batch(ctx, bsz, promotes, layers);
        const uint32_t pb = (uint32_t)(batches & 1u); // buffer set of this batch
        // the buffers of set pb were last read by the link step of batch - 2; and a serial batch (or the batch behind one) starts
        // only when everything before it is in the graph
        if (link_pending[pb] && hipStreamWaitEvent(s, ev_link[pb], 0) != hipSuccess) return bail(fail(HVX_ERR_DEVICE, "stream ordering failed"));
        if ((plan.serial || prev_serial) && link_pending[pb ^ 1u] && hipStreamWaitEvent(s, ev_link[pb ^ 1u], 0) != hipSuccess)
            return bail(fail(HVX_ERR_DEVICE, "stream ordering failed"));
        uint64_t *b_cids = d_cids + (size_t)pb * w.sz_cids;
        float *b_csc = d_csc + (size_t)pb * w.sz_cids;
        uint32_t *b_cnt = d_cnt + (size_t)pb * w.sz_cnt, *b_sel = d_sel + (size_t)pb * w.sz_sel, *b_selcnt = d_selcnt + (size_t)pb * w.sz_cnt;
        HnswArgs a{};
        a.ix = d;
        a.bitmap = ix->d_bitmap;
        a.words_per_query = ix->words_per_query;
        a.k = g.kc; // the first 2 * Mmax entries of W (mutation.rs:1072-1097)
        a.ef = g.ef0;
        a.build_ef_upper = g.efu;
        a.out_ids = b_cids;
        a.out_scores = b_csc;
        a.out_counts = b_cnt;
        a.out_status = d_status;
        a.tie_flags = ix->d_tie;
        a.tie_count = d_ties; // (a flagged build search is counted, never repeated: hvx_index_last_write_tie_overflows)
        a.build_nodes = d_iota + (done - first);
        if (ctx.bf16 && r.build_q) a.queries = r.build_q + (size_t)(done - first) * d.dim;
        else if (ctx.bf16) {
            hipLaunchKernelGGL(decode_rows_bf16_kernel, dim3((uint32_t)(((size_t)bsz * (d.dim >> 3) + 255u) / 256u)), dim3(256), 0, s, d.vecb, d_iota + (done - first), bsz, d.dim, d_bq);
            if (hipGetLastError() != hipSuccess) return bail(fail(HVX_ERR_DEVICE, "launch of the bf16 query rows failed"));
            a.queries = d_bq;
        }
        a.occupancy = plan.occupancy;
        if (launch_hnsw_wave(a, bsz, s) != hipSuccess) return bail(fail(HVX_ERR_DEVICE, "build search launch failed: %s", hipGetErrorString(hipGetLastError())));
        if (hipEventRecord(ev_search[pb], s) != hipSuccess || hipStreamWaitEvent(s2, ev_search[pb], 0) != hipSuccess)
            return bail(fail(HVX_ERR_DEVICE, "stream ordering failed"));
        BuildArgs ba{};
        ba.ix = d;
        ba.l0 = const_cast<uint32_t *>(d.l0);
        ba.up = const_cast<uint32_t *>(d.up);
        ba.locks = ix->ins_locks;
        ba.nodes = d_iota + (done - first);
        ba.b = bsz;
        ba.layers = layers;
        ba.cand_ids = b_cids;
        ba.cand_sc = b_csc;
        ba.cand_cnt = b_cnt;
        ba.sel = b_sel;
        ba.sel_cnt = b_selcnt;
        ba.m = g.m;
        ba.m0 = g.m0;
        ba.err = d_err;
        ba.dbg = dbg.as<uint32_t>();
        ba.gdm = d_gdm;
        ba.tick = d_tick;
        ba.kc = g.kc;
        ba.selw = g.selw;
        const hipError_t e = launch_write_batch(plan, ctx, kern, ba, s2);
        ix->last_write_path |= plan.path;
        if (e != hipSuccess) return bail(fail(HVX_ERR_DEVICE, "build launch failed: %s", hipGetErrorString(e)));
        if (hipEventRecord(ev_link[pb], s2) != hipSuccess) return bail(fail(HVX_ERR_DEVICE, "stream ordering failed"));
        link_pending[pb] = true;
        prev_serial = plan.serial;
        if (promotes) { // mutation.rs:769-772
            d.entry = (uint32_t)r.row_at(done);
            d.max_layer = lv0;
        }
        done += bsz;
        batches += 1;
        singles += bsz == 1 ? 1 : 0;
        if ((batches & 63u) == 0u && (hipStreamSynchronize(s) != hipSuccess || hipStreamSynchronize(s2) != hipSuccess)) // bound the launch queues
            return bail(fail(HVX_ERR_DEVICE, "build kernels failed: %s", hipGetErrorString(hipGetLastError())));
    }
    if (hipStreamSynchronize(s2) != hipSuccess) return bail(fail(HVX_ERR_DEVICE, "build did not complete: %s", hipGetErrorString(hipGetLastError())));
    uint32_t words[2] = {0u, 0u}; // the error word, the flagged nodes
    if (hipMemcpyAsync(words, d_err, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return bail(fail(HVX_ERR_DEVICE, "build did not complete: %s", hipGetErrorString(hipGetLastError())));
    ix->last_write_tie_overflows += words[1];
    if (dbg.p) {
        uint32_t h[8] = {0};
        (void)hipMemcpy(h, dbg.p, 32, hipMemcpyDeviceToHost);
        fprintf(stderr, "[hvx build] link step: lock spins %u, prunes %u, reverse-edge removals %u, plain appends %u\n", h[0], h[1], h[2], h[3]);
    }
    if (words[0]) return fail(HVX_ERR_INVARIANT, "a neighbour row overflowed its stride during the build");
    if (stats) {
        stats->batches += batches;
        stats->single_node_batches += singles;
        stats->nodes += r.count;
    }
    return HVX_OK;
}

// a completed write becomes the handle's description and the image's visible generation
static void publish_write(hvx_index *ix, bool bump = true) {
    ix->desc.has_entry = 1;
    ix->desc.entry_point = ix->ids_ref()[ix->dev.entry];
    ix->desc.max_layer = ix->dev.max_layer;
    ix->publish_view(bump);
}

// Rows on their way into an image: `count` rows of `vectors` (row stride dim) are uploaded to vdst with the image's ld (zero padded),
// rounded in place for bf16 images (the index IS the rounded vectors: validation and headers see them) and validated as rows of the image,
// their headers written to hdr_dst.  The first invalid row fails the call with its status (mutation.rs:660-690).  Waits for the stream.
static int stage_rows(hvx_index *ix, const float *vectors, const uint64_t *node_ids, uint32_t count, float *vdst, float *hdr_dst) {
    const DevIndex &d = ix->dev;
    hipStream_t s = ix->stream;
    if (d.ld == d.dim) {
        HIP_TRY(hipMemcpyAsync(vdst, vectors, (size_t)count * d.dim * 4, hipMemcpyDefault, s));
    } else {
        HIP_TRY(hipMemsetAsync(vdst, 0, (size_t)count * d.ld * 4, s));
        HIP_TRY(hipMemcpy2DAsync(vdst, (size_t)d.ld * 4, vectors, (size_t)d.dim * 4, (size_t)d.dim * 4, count, hipMemcpyDefault, s));
    }
    if (d.dtype == HVX_BF16) HIP_TRY(launch_round_bf16_inplace(vdst, (size_t)count * d.ld, s));
    DevTemp status;
    HIP_TRY(status.alloc((size_t)count * 4));
    std::vector<uint32_t> st(count);
    DevIndex view = d;
    view.vec = vdst;
    hipError_t e = launch_validate_rows(view, count, ix->limit, status.as<uint32_t>(), hdr_dst, s);
    if (e == hipSuccess) e = hipMemcpyAsync(st.data(), status.p, (size_t)count * 4, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(HVX_ERR_DEVICE, "row validation: %s", hipGetErrorString(e));
    for (uint32_t i = 0; i < count; ++i)
        if (st[i]) return fail((int)st[i], "vector of node %llu is invalid for this metric (status %u)", (unsigned long long)node_ids[i], st[i]);
    return HVX_OK;
}

extern "C" int hvx_index_build(const hvx_index_desc *desc, const uint64_t *node_ids, const float *vectors, const uint16_t *levels,
                               const hvx_build_params *params, hvx_index **out, hvx_build_stats *stats) {
    if (!desc || !out || !params) return fail(HVX_ERR_INVARIANT, "null argument");
    *out = nullptr;
    const uint64_t n = desc->n;
    if (n && (!node_ids || !vectors)) return fail(HVX_ERR_INVARIANT, "null array");
    const WriteDegrees g = write_degrees(*desc, params);
    if (desc->dtype != HVX_F32 && desc->dtype != HVX_BF16)
        return fail(HVX_ERR_UNSUPPORTED, "the device build reads f32 and bf16 rows (import the built graph with dtype fp8 afterwards)");
    const WriteRefusal refused = write_refusal(g, 0u, 0u, kRefuseDegrees | kRefuseEf);
    if (refused == kRefuseDegrees) return refuse_write(refused, "device build", "s");
    if (desc->dtype == HVX_BF16) { // what the bf16 import and the unrolled build search over bf16 rows serve
        const uint32_t nk = desc->dim >> 5;
        const bool dim_ok = desc->dim % 32u == 0u && (nk == 4 || nk == 8 || nk == 12 || nk == 16 || nk == 24 || nk == 32 || nk == 48);
        if (!dim_ok || desc->float_kernel != HVX_KERNEL_AVX_FMA || (desc->metric != HVX_L2_SQUARED && desc->metric != HVX_COSINE_HALF))
            return fail(HVX_ERR_UNSUPPORTED, "the device build over bf16 rows serves L2 / cosine, the AVX+FMA summation tree and dim in {128, 256, 384, 512, 768, 1024, 1536}");
        if (wave_build_need(g.ef0, g.efu) > kBeamNarrowMax)
            return fail(HVX_ERR_UNSUPPORTED, "the device build over bf16 rows serves max(ef_construction, m0, 2 m) <= %u", kBeamNarrowMax - kBeamSlack);
    }
    if (refused) return refuse_write(refused, "device build", "s");

    // ---- the image: rows + EMPTY graph with rows sized for m0 / m (+ room for rows appended later: hvx_index_insert_batch) ----
    hvx_index_desc d0 = *desc;
    d0.m = g.m;
    d0.m0 = g.m0;
    d0.has_entry = 0;
    d0.max_layer = 0;
    if (d0.max_batch == 0) d0.max_batch = 1024;
    uint64_t up_rows = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const uint16_t lv = levels ? levels[i] : 0;
        if (lv > 63) return fail(HVX_ERR_INVARIANT, "node level > 63");
        up_rows += lv;
    }
    std::vector<uint64_t> zeros0(n + 1, 0), zerosu(up_rows + 1, 0);
    uint64_t dummy = 0;
    hvx_index *ix = nullptr;
    int rc = import_index(&d0, node_ids, vectors, zeros0.data(), &dummy, levels, zerosu.data(), &dummy, g.m0, g.m, &ix, params->reserve_rows,
                          params->reserve_upper_rows);
    if (rc) return rc;
    auto bail = [&](int code) { hvx_index_free(ix); return code; };
    if (!hnsw_wave_build_supported(ix->dev, g.ef0, g.efu))
        return bail(fail(HVX_ERR_UNSUPPORTED, "device build serves neighbour rows of <= 64 ids"));
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n == 0) { *out = ix; return HVX_OK; }
    // scatter: rows whose ORDER follows the data (a dump sorted by topic, an index hydrated in key order) would put each other's nearest
    // neighbours into one batch, where they cannot see each other: insert in the order (i * stride) mod n instead, stride ~ 0.618 n and
    // coprime with n (position 0 stays row 0).  Sequential mode keeps id order: it IS the reference's order.
    uint32_t stride = 1;
    if (params->scatter && !one_node_batches(params) && n > 2) {
        auto gcd = [](uint64_t a, uint64_t b) { while (b) { const uint64_t t = a % b; a = b; b = t; } return a; };
        uint64_t st = (uint64_t)((double)n * 0.6180339887498949);
        while (st > 1 && gcd(st, n) != 1) --st;
        stride = (uint32_t)std::max<uint64_t>(st, 1);
    }
    if ((rc = insert_range(ix, WriteRows{0, n, stride, n, levels, 0, nullptr}, params, stats))) return bail(rc);
    publish_write(ix, /*bump=*/false); // generation 1 = the built image (import_index published the empty graph under the same number)
    *out = ix;
    return HVX_OK;
}

// insert_hnsw for rows APPENDED to a live image (mutation.rs:642-780 insert -> :787-895 insert_hnsw): the reference inserts one node at
// a time into the store its readers snapshot; here a batch of new rows lands in the spare capacity of a growable image
// (hvx_build_params.reserve_rows), is validated and given its headers / SimHash rows like imported rows, and is then linked into the
// graph by the SAME loop the device build runs -- sequential mode = the reference's insertion, row for row.  The new generation
// becomes visible (visible_seq + 1: rows, entry point, top layer) when the batch is complete; forks adopt it with hvx_index_refresh.
// Searches that run on forks meanwhile keep their generation's entry point and read neighbour rows as stale-or-current, never torn:
// a new node's vector, header and own rows are complete before the first link to it is stored (hvx_build.hip, row locks +
// agent-scope stores), exactly what the overlapped batches of the device build rely on.
extern "C" int hvx_index_insert_batch(hvx_index *ix, const uint64_t *node_ids, const float *vectors, const uint16_t *levels, uint32_t count,
                                      const hvx_build_params *params, hvx_build_stats *stats) {
    if (!ix || (count && (!node_ids || !vectors))) return fail(HVX_ERR_INVARIANT, "null argument");
    hvx_build_params dflt;
    hvx_build_params_default(&dflt);
    if (!params) params = &dflt;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (count == 0) { ix->last_write_path = 0u; ix->last_write_tie_overflows = 0u; return HVX_OK; }
    if (ix->is_fork) return fail(HVX_ERR_UNSUPPORTED, "rows are inserted through the handle that owns the image, not a fork");
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->last_write_path = 0u; // hvx_index_last_write_path: the batches of THIS call
    ix->last_write_tie_overflows = 0u;
    HIP_TRY(hipSetDevice(ix->device));
    DevIndex &d = ix->dev;
    if (d.dtype != HVX_F32 && d.dtype != HVX_BF16) return fail(HVX_ERR_UNSUPPORTED, "rows are inserted into f32 and bf16 images (fp8 images are read-only)");
    const bool bf16 = d.dtype == HVX_BF16; // (rounded, validated, packed, linked over the bf16 rows)
    hvx_build_params one = *params;
    if (bf16 && params->sequential == HVX_BUILD_AUTO) { // the library's choice for appends to a bf16 image: one node per step
        one.sequential = HVX_BUILD_ONE_NODE;
        params = &one;
    }
    const WriteDegrees g = write_degrees(ix->desc, params);
    if (const WriteRefusal refused = write_refusal(g, d.s0, d.su, kRefuseDegrees | kRefuseRowsNarrow | kRefuseRowsOver64 | kRefuseEf))
        return refuse_write(refused, "device inserts", "");
    const uint64_t n0 = d.n;
    if (n0 + count > ix->cap_rows)
        return fail(HVX_ERR_CANDIDATE_LIMIT, "the image holds %llu of %llu rows: %u more do not fit (hvx_build_params.reserve_rows)", (unsigned long long)n0,
                    (unsigned long long)ix->cap_rows, count);
    uint64_t up_need = 0;
    for (uint32_t i = 0; i < count; ++i) {
        const uint16_t lv = levels ? levels[i] : 0;
        if (lv > 63) return fail(HVX_ERR_INVARIANT, "node level > 63");
        up_need += lv;
        // ids stay strictly ascending over the whole image (the reference allocates dense ascending u64 ids: index_lifecycle_scale.rs:1504-1514)
        const uint64_t prev = i ? node_ids[i - 1] : (n0 ? ix->ids_ref()[n0 - 1] : 0);
        if ((i || n0) && node_ids[i] <= prev) return fail(HVX_ERR_INVARIANT, "inserted node ids must be ascending and above every id of the image (id %llu)", (unsigned long long)node_ids[i]);
    }
    if (ix->up_rows_used + up_need > ix->cap_up_rows)
        return fail(HVX_ERR_CANDIDATE_LIMIT, "the image's upper-layer rows are exhausted (%llu + %llu > %llu: hvx_build_params.reserve_upper_rows)",
                    (unsigned long long)ix->up_rows_used, (unsigned long long)up_need, (unsigned long long)ix->cap_up_rows);
    // (a bf16 image outside the unrolled shapes has no build search either: that one fails at its launch)
    if (!hnsw_wave_build_supported(d, g.ef0, g.efu) && (d.s0 > 64u || d.su > 64u)) return fail(HVX_ERR_UNSUPPORTED, "device build serves neighbour rows of <= 64 ids");
    hipStream_t s = ix->stream;
    // ---- the rows: upload into the spare capacity, validate, headers (nothing is visible yet: d.n still ends before them) ----
    float *vdst;
    if (bf16) { // the rounded vectors as f32: validation, headers, SimHash rows and the build searches read them; the image gets the packed rows
        if ((size_t)count * d.ld * 4 > ix->ins_rows_cap) {
            ix->ins_rows_cap = 0;
            int rc0 = ix->regrow((void **)&ix->ins_rows, (size_t)count * d.ld * 4);
            if (rc0) return rc0;
            ix->ins_rows_cap = (size_t)count * d.ld * 4;
        }
        vdst = ix->ins_rows;
    } else {
        vdst = const_cast<float *>(d.vec) + (size_t)n0 * d.ld;
    }
    int rc = stage_rows(ix, vectors, node_ids, count, vdst, const_cast<float *>(d.hdr) + n0);
    if (rc) return rc;
    // ---- levels, upper-row bases, ids ----
    std::vector<uint16_t> h_lv(count, 0);
    std::vector<uint32_t> h_base(count, kSentinel);
    uint64_t r = ix->up_rows_used;
    for (uint32_t i = 0; i < count; ++i) {
        h_lv[i] = levels ? levels[i] : 0;
        if (h_lv[i]) { h_base[i] = (uint32_t)r; r += h_lv[i]; }
    }
    HIP_TRY(hipMemcpyAsync(const_cast<uint16_t *>(d.level) + n0, h_lv.data(), (size_t)count * 2, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(const_cast<uint32_t *>(d.up_base) + n0, h_base.data(), (size_t)count * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(const_cast<uint64_t *>(d.ids) + n0, node_ids, (size_t)count * 8, hipMemcpyHostToDevice, s));
    if (bf16) HIP_TRY(launch_pack_bf16(vdst, const_cast<uint16_t *>(d.vecb) + (size_t)n0 * d.dim, count, d.dim, s));
    if (ix->has_simhash) { // SimHash rows of the new nodes (SimHasher::hash at insert time: mutation.rs:700-705)
        HIP_TRY(launch_simhash_rows(ix->d_planes_t, vdst, d.dim, d.ld, count, ix->d_node_hash + n0, s));
    }
    HIP_TRY(hipStreamSynchronize(s)); // (the host vectors above leave scope)
    auto grown = std::make_shared<std::vector<uint64_t>>();
    grown->reserve(n0 + count);
    grown->insert(grown->end(), ix->ids_ref().begin(), ix->ids_ref().end());
    grown->insert(grown->end(), node_ids, node_ids + count);
    bool contiguous = ix->contiguous && (n0 == 0 || node_ids[0] == ix->ids_ref()[n0 - 1] + 1);
    for (uint32_t i = 1; i < count && contiguous; ++i) contiguous = node_ids[i] == node_ids[i - 1] + 1;
    ix->ids_p = grown;
    ix->contiguous = contiguous;
    d.n = (uint32_t)(n0 + count);
    ix->desc.n = d.n;
    ix->up_rows_used = r;
    // ---- link them into the graph ----
    rc = insert_range(ix, WriteRows{n0, count, 1u, 0, h_lv.data(), n0, bf16 ? vdst : nullptr}, params, stats);
    if (rc) return rc; // (the image is partially linked: the host discards the handle and re-hydrates)
    ix->desc.shard_id_hi = ix->ids_ref()[d.n - 1];
    publish_write(ix);
    return HVX_OK;
}

namespace hvx {
__global__ void clear_dead_bit_kernel(uint32_t *dead, uint32_t row) { atomicAnd(&dead[row >> 5], ~(1u << (row & 31u))); }
}

// VectorInsertContract::Upsert (mutation.rs:642-780: an insert of an id the index already holds deletes it first, index.rs:2018-2060):
// for every id, in order -- a LIVE id is deleted (hvx_index_delete_batch), then the vector is linked back in under the same id: into the
// node's own row slot when the image holds one (it keeps its position in the ascending id order, so every id tie-break stays the
// reference's), appended when the id is above every id of the image.  The node keeps the level of its slot (the reference draws the
// level of an insert at random: any draw is a valid one); levels[i] is used for appended ids only.
extern "C" int hvx_index_upsert_batch(hvx_index *ix, const uint64_t *node_ids, const float *vectors, const uint16_t *levels, uint32_t count,
                                      const hvx_build_params *params, hvx_build_stats *stats) {
    if (!ix || (count && (!node_ids || !vectors))) return fail(HVX_ERR_INVARIANT, "null argument");
    hvx_build_params seq;
    hvx_build_params_default(&seq);
    if (params) seq = *params;
    seq.sequential = 1; // one node at a time: the reference's order
    if (stats) memset(stats, 0, sizeof(*stats));
    if (count == 0) { ix->last_write_path = 0u; ix->last_write_tie_overflows = 0u; return HVX_OK; }
    if (ix->is_fork) return fail(HVX_ERR_UNSUPPORTED, "rows are written through the handle that owns the image, not a fork");
    const uint32_t ld = ix->dev.ld;
    if (ix->dev.dtype != HVX_F32 && ix->dev.dtype != HVX_BF16) return fail(HVX_ERR_UNSUPPORTED, "rows are written into f32 and bf16 images");
    const bool bf16 = ix->dev.dtype == HVX_BF16; // (round 6: an id the image holds gets its new vector in its slot; bf16 images have no spare rows to append to)
    // the insert half's degree limits, before the delete half changes anything
    if (const WriteRefusal refused = write_refusal(write_degrees(ix->desc, &seq), ix->dev.s0, ix->dev.su, kRefuseDegrees | kRefuseRowsOver64))
        return refuse_write(refused, "device upserts", "");
    // ---- every vector is validated before anything changes (an invalid one fails the call: mutation.rs:660-690) ----
    DevTemp tmp; // the validated (bf16 images: rounded) vectors, row stride ld
    {
        std::lock_guard<std::mutex> lock(ix->mu);
        HIP_TRY(hipSetDevice(ix->device));
        DevTemp tmph;
        if (tmp.alloc((size_t)count * ld * 4) != hipSuccess || tmph.alloc((size_t)count * 4) != hipSuccess)
            return fail(HVX_ERR_DEVICE, "hipMalloc of the upsert staging rows failed");
        if (const int rc = stage_rows(ix, vectors, node_ids, count, tmp.as<float>(), tmph.as<float>())) return rc;
        // ids that are neither in the image nor above it cannot be placed (rows ascend with ids)
        const std::vector<uint64_t> &ids = ix->ids_ref();
        uint64_t last = ids.empty() ? 0 : ids.back();
        bool any = !ids.empty();
        for (uint32_t i = 0; i < count; ++i) {
            if (ix->find_slot(node_ids[i]) != kSentinel) continue;
            if (any && node_ids[i] <= last) return fail(HVX_ERR_UNSUPPORTED, "node %llu lies between the ids of the image: it has no row slot (hydrate the image again)", (unsigned long long)node_ids[i]);
            last = node_ids[i];
            any = true;
        }
    }
    float *const d_tmp = tmp.as<float>();
    uint32_t wpath = 0u, wties = 0u; // hvx_index_last_write_path / _tie_overflows: over every id's insert half (the delete half touches neither)
    auto done = [&](int rc) { (void)hipSetDevice(ix->device); ix->last_write_path |= wpath; ix->last_write_tie_overflows = wties; return rc; };
    ix->last_write_path = 0u;
    ix->last_write_tie_overflows = 0u;
    uint64_t nodes = 0, batches = 0, singles = 0;
    for (uint32_t i = 0; i < count; ++i) {
        int rc;
        if (ix->find(node_ids[i]) != kSentinel && (rc = hvx_index_delete_batch(ix, node_ids + i, 1, nullptr))) return done(rc); // live: the delete half
        hvx_build_stats one{};
        if (ix->find_slot(node_ids[i]) == kSentinel) { // above the image: an ordinary append
            const uint16_t lv = levels ? levels[i] : 0;
            if ((rc = hvx_index_insert_batch(ix, node_ids + i, d_tmp + (size_t)i * ld, &lv, 1, &seq, &one))) return done(rc);
        } else { // the node's own (deleted) slot
            std::lock_guard<std::mutex> lock(ix->mu);
            if (hipSetDevice(ix->device) != hipSuccess) return done(fail(HVX_ERR_DEVICE, "hipSetDevice failed"));
            DevIndex &d = ix->dev;
            hipStream_t s = ix->stream;
            const uint32_t row = ix->find_slot(node_ids[i]);
            float *vsrc = d_tmp + (size_t)i * ld; // the validated (bf16 images: rounded) vector
            float *vdst = bf16 ? vsrc : const_cast<float *>(d.vec) + (size_t)row * d.ld;
            uint16_t lv = 0;
            hipError_t e = bf16 ? launch_pack_bf16(vsrc, const_cast<uint16_t *>(d.vecb) + (size_t)row * d.dim, 1u, d.dim, s)
                                : hipMemcpyAsync(vdst, vsrc, (size_t)ld * 4, hipMemcpyDeviceToDevice, s);
            { // (staged and validated above: only the header of the new vector is taken, the status word is not read back)
                DevTemp one_status;
                if (e == hipSuccess) e = one_status.alloc(4);
                DevIndex view = d;
                view.vec = vdst;
                if (e == hipSuccess) e = launch_validate_rows(view, 1, ix->limit, one_status.as<uint32_t>(), const_cast<float *>(d.hdr) + row, s);
                if (e == hipSuccess && ix->has_simhash) e = launch_simhash_rows(ix->d_planes_t, vdst, d.dim, d.ld, 1, ix->d_node_hash + row, s);
                if (e == hipSuccess) e = hipMemcpyAsync(&lv, d.level + row, 2, hipMemcpyDeviceToHost, s);
                if (e == hipSuccess && ix->d_dead) { hipLaunchKernelGGL(clear_dead_bit_kernel, dim3(1), dim3(1), 0, s, ix->d_dead, row); e = hipGetLastError(); }
                if (e == hipSuccess) e = hipStreamSynchronize(s);
            }
            if (e != hipSuccess) return done(fail(HVX_ERR_DEVICE, "upsert of node %llu: %s", (unsigned long long)node_ids[i], hipGetErrorString(e)));
            { // caches derived from the rows' VECTORS (per-handle |x|^2, the image's bf16 shadow) are rebuilt by their next user
                std::lock_guard<std::mutex> g(ix->shared->mu);
                ix->shared->vec_epoch += 1;
                ix->shared->shadow_rows = 0;
            }
            auto flags = std::make_shared<std::vector<uint8_t>>(*ix->dead_p); // this generation's flags: the slot is live again
            (*flags)[row] = 0;
            ix->dead_p = flags;
            ix->n_dead -= 1;
            ix->last_write_path = 0u;
            ix->last_write_tie_overflows = 0u;
            if ((rc = insert_range(ix, WriteRows{row, 1, 1u, d.n, &lv, row, bf16 ? vsrc : nullptr}, &seq, &one))) return done(rc);
            publish_write(ix);
            ix->seen_rewrite = ix->shared->rewrite_epoch.fetch_add(1, std::memory_order_acq_rel) + 1;
        }
        wpath |= ix->last_write_path;
        wties += ix->last_write_tie_overflows;
        nodes += 1; batches += one.batches; singles += one.single_node_batches;
    }
    if (stats) { stats->nodes = nodes; stats->batches = batches; stats->single_node_batches = singles; }
    return done(HVX_OK);
}

// add_bidirectional_link on layer 0 of an existing image, through build_link_wg_kernel (include/helix_vec.h): the kernel that links
// every batched build, driven link by link so that tests can hold each prune against the oracle's select_diverse + backfill.
extern "C" int hvx_index_link_rows(hvx_index *ix, const uint64_t *from_ids, const uint64_t *to_ids, uint32_t n_links, uint32_t concurrent) {
    if (!ix || (n_links && (!from_ids || !to_ids))) return fail(HVX_ERR_INVARIANT, "null argument");
    if (n_links == 0) return HVX_OK;
    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    DevIndex &d = ix->dev;
    if (ix->is_fork) return fail(HVX_ERR_UNSUPPORTED, "rows are linked through the handle that owns the image, not a fork");
    const WriteDegrees g = write_degrees(ix->desc, nullptr);
    const bool fused = kernel_fused(d.fkernel);
    const bool bf16 = d.dtype == HVX_BF16;
    const BuildKernels kern = pick_build_kernels(d.metric, fused, bf16);
    const LinkGeom geo = g.wide ? wide_link_geom(d, g.m, g.m0) : link_geom(d, g.m, g.m0);
    const uint32_t selw = g.selw;
    // one refusal per cause
    if (d.dtype != HVX_F32 && !bf16) return fail(HVX_ERR_UNSUPPORTED, "the link workgroups serve f32 and bf16 rows (this image holds dtype %u)", d.dtype);
    if (std::max(g.m0, g.m) > 64u) return fail(HVX_ERR_UNSUPPORTED, "the link workgroups serve m0 <= 64 (m <= 32)");
    if (g.wide && bf16) return fail(HVX_ERR_UNSUPPORTED, "the link workgroups serve bf16 rows with m0 <= 32 (the workgroup kernel for m0 <= 64 reads f32 rows)");
    if (bf16 && d.dim % 64u != 0u) return fail(HVX_ERR_UNSUPPORTED, "the link workgroups serve bf16 rows with dim %% 64 == 0");
    if (d.s0 < g.m0) return fail(HVX_ERR_UNSUPPORTED, "the image's layer-0 rows (%u ids) are narrower than m0 = %u", d.s0, g.m0);
    if (!geo.ok)
        return fail(HVX_ERR_UNSUPPORTED, "the link workgroups serve L2 / cosine under the 256-bit summation trees, dim %% 32 == 0, rows of at most 64 ids");
    std::vector<uint32_t> h_nodes(n_links), h_sel((size_t)n_links * selw, kSentinel), h_cnt(n_links, 1u);
    for (uint32_t i = 0; i < n_links; ++i) {
        const uint32_t f = ix->find(from_ids[i]), t = ix->find(to_ids[i]);
        if (f == kSentinel || t == kSentinel || f == t) return fail(HVX_ERR_INVARIANT, "link %u: unknown id or a self link", i);
        h_nodes[i] = f;
        h_sel[(size_t)i * selw] = t;
    }
    hipStream_t s = ix->stream;
    DevTemp t_nodes, t_sel, t_cnt, t_locks, t_err; // (released when the call returns; a failed call waits for the stream first)
    auto bail = [&](int rc) { (void)hipStreamSynchronize(s); return rc; };
    if (t_nodes.alloc((size_t)n_links * 4) != hipSuccess || t_sel.alloc((size_t)n_links * selw * 4) != hipSuccess ||
        t_cnt.alloc((size_t)n_links * 4) != hipSuccess || t_locks.alloc((size_t)d.n * 4) != hipSuccess || t_err.alloc(4) != hipSuccess)
        return bail(fail(HVX_ERR_DEVICE, "hipMalloc of the link scratch failed"));
    uint32_t *const d_nodes = t_nodes.as<uint32_t>(), *const d_sel = t_sel.as<uint32_t>(), *const d_cnt = t_cnt.as<uint32_t>();
    uint32_t *const d_locks = t_locks.as<uint32_t>(), *const d_err = t_err.as<uint32_t>();
    if (hipMemcpyAsync(d_nodes, h_nodes.data(), (size_t)n_links * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_sel, h_sel.data(), h_sel.size() * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemcpyAsync(d_cnt, h_cnt.data(), (size_t)n_links * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(d_locks, 0, (size_t)d.n * 4, s) != hipSuccess || hipMemsetAsync(d_err, 0, 4, s) != hipSuccess)
        return bail(fail(HVX_ERR_DEVICE, "upload of the link list failed"));
    BuildArgs ba{};
    ba.ix = d;
    ba.l0 = const_cast<uint32_t *>(d.l0);
    ba.up = const_cast<uint32_t *>(d.up);
    ba.locks = d_locks;
    ba.layers = 1; // layer 0 only
    ba.sel = d_sel;
    ba.sel_cnt = d_cnt;
    ba.m = g.m;
    ba.m0 = g.m0;
    ba.err = d_err;
    ba.ldp = geo.ldp;
    ba.ncmax = geo.ncmax;
    ba.link_ck = geo.link_ck;
    ba.selw = selw;
    auto launch = [&]() {
        return g.wide ? launch_build_link_wide_wg(ba, fused, 1, geo.lds, s) : launch_step(kern.link_wg, StepGeom{ba.b * 32u, 1u, 256u, geo.lds, 0u, 0u}, ba, s);
    };
    hipError_t e = hipSuccess;
    if (concurrent) {
        ba.nodes = d_nodes;
        ba.b = n_links;
        e = launch();
    } else {
        for (uint32_t i = 0; i < n_links && e == hipSuccess; ++i) { // one launch per link: launches on a stream run in order
            ba.nodes = d_nodes + i;
            ba.sel = d_sel + (size_t)i * selw;
            ba.sel_cnt = d_cnt + i;
            ba.b = 1;
            e = launch();
        }
    }
    if (e != hipSuccess) return bail(fail(HVX_ERR_DEVICE, "link launch failed: %s", hipGetErrorString(e)));
    uint32_t err = 0;
    if (hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return bail(fail(HVX_ERR_DEVICE, "link kernels failed: %s", hipGetErrorString(hipGetLastError())));
    if (err) return fail(HVX_ERR_INVARIANT, "a neighbour row overflowed its stride during the link step");
    return HVX_OK;
}

// ---- graph read-back: what the host persists (values/vectors.rs rows) and what tests compare with the oracle ----
extern "C" int hvx_index_graph_sizes(const hvx_index *cix, uint64_t *l0_edges, uint64_t *up_rows, uint64_t *up_edges,
                                     uint64_t *entry_point, uint32_t *max_layer, uint32_t *has_entry) {
    if (!cix) return fail(HVX_ERR_INVARIANT, "null index");
    hvx_index *ix = const_cast<hvx_index *>(cix);
    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    const DevIndex &d = ix->dev;
    std::vector<uint32_t> h((size_t)d.n * d.s0);
    if (d.n) HIP_TRY(hipMemcpy(h.data(), d.l0, h.size() * 4, hipMemcpyDeviceToHost));
    uint64_t e0 = 0;
    for (uint32_t v : h) e0 += v != kSentinel;
    std::vector<uint16_t> lv(d.n);
    if (d.n) HIP_TRY(hipMemcpy(lv.data(), d.level, (size_t)d.n * 2, hipMemcpyDeviceToHost));
    uint64_t ur = 0;
    for (uint16_t v : lv) ur += v;
    std::vector<uint32_t> hu((size_t)ur * d.su);
    if (ur) HIP_TRY(hipMemcpy(hu.data(), d.up, hu.size() * 4, hipMemcpyDeviceToHost));
    uint64_t eu = 0;
    for (uint32_t v : hu) eu += v != kSentinel;
    if (l0_edges) *l0_edges = e0;
    if (up_rows) *up_rows = ur;
    if (up_edges) *up_edges = eu;
    if (entry_point) *entry_point = d.has_entry ? ix->ids_ref()[d.entry] : 0;
    if (max_layer) *max_layer = d.max_layer;
    if (has_entry) *has_entry = d.has_entry;
    return HVX_OK;
}

extern "C" int hvx_index_export_graph(const hvx_index *cix, uint64_t *l0_offsets, uint64_t *l0_neighbors, uint16_t *level,
                                      uint64_t *up_offsets, uint64_t *up_neighbors) {
    if (!cix || !l0_offsets || !l0_neighbors) return fail(HVX_ERR_INVARIANT, "null argument");
    hvx_index *ix = const_cast<hvx_index *>(cix);
    std::lock_guard<std::mutex> lock(ix->mu);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(hipStreamSynchronize(ix->stream));
    const DevIndex &d = ix->dev;
    const std::vector<uint64_t> &ids = ix->ids_ref();
    std::vector<uint32_t> h((size_t)d.n * d.s0);
    if (d.n) HIP_TRY(hipMemcpy(h.data(), d.l0, h.size() * 4, hipMemcpyDeviceToHost));
    uint64_t w = 0;
    for (uint32_t i = 0; i < d.n; ++i) {
        l0_offsets[i] = w;
        for (uint32_t t = 0; t < d.s0; ++t) {
            const uint32_t v = h[(size_t)i * d.s0 + t];
            if (v != kSentinel) l0_neighbors[w++] = ids[v];
        }
    }
    l0_offsets[d.n] = w;
    std::vector<uint16_t> lv(d.n);
    if (d.n) HIP_TRY(hipMemcpy(lv.data(), d.level, (size_t)d.n * 2, hipMemcpyDeviceToHost));
    if (level) memcpy(level, lv.data(), (size_t)d.n * 2);
    uint64_t ur = 0;
    for (uint16_t v : lv) ur += v;
    if (up_offsets && up_neighbors) {
        std::vector<uint32_t> hu((size_t)ur * d.su);
        if (ur) HIP_TRY(hipMemcpy(hu.data(), d.up, hu.size() * 4, hipMemcpyDeviceToHost));
        uint64_t wu = 0;
        for (uint64_t r = 0; r < ur; ++r) {
            up_offsets[r] = wu;
            for (uint32_t t = 0; t < d.su; ++t) {
                const uint32_t v = hu[(size_t)r * d.su + t];
                if (v != kSentinel) up_neighbors[wu++] = ids[v];
            }
        }
        up_offsets[ur] = wu;
    }
    return HVX_OK;
}
