// hvx_build_wide.hip -- the select / link kernels of the device build (hvx_build.hip) for degree limits above 32: Mmax = max(m0, m) <= 64,
// the reference's scale fixture (M 32 / M0 64: scale_contracts.rs:167-173; insert_hnsw itself has no degree limit, mutation.rs:787-895).
// A select then ranks up to 2 * Mmax = 128 hydrated candidates (mutation.rs:1072-1097), a link prunes a list of up to 65 ids (a full
// layer-0 row + the new node), and a node has up to 64 links per layer: none of it fits "one id per lane, one 64-bit mask".  Here every
// list is held TWO ids per lane (c = lane, lane + 64) and every set is a pair of 64-bit masks.  A neighbour ROW still has at most 64
// ids (stride <= 64): it is read and written one id per lane, only the appended node is the 65th.
//
//   build_select_wide_kernel   select_neighbors_heuristic = select_diverse + backfill (mod.rs:809-856), one wavefront per (node, layer)
//   build_link_wide_kernel     add_bidirectional_link (mutation.rs:1498-1583) for a node's links in selection order, one wavefront per
//                              node: the plain restatement of the reference -- one-node steps under link_mode = 1 (the default runs the
//                              many-workgroup steps of hvx_build_wide_seq.hip), batches over bf16 rows, Manhattan and the shapes the
//                              workgroup kernel does not serve
//   build_link_wide_wg_kernel  the batched link step: one 1 024-thread workgroup per link, the prune's 2 145 pairwise distances
//                              evaluated eagerly from LDS -- the wide twin of build_link_wg_kernel (batches of fewer than 1 024 nodes and
//                              hvx_index_link_rows; larger batches link faster with build_link_wide_kernel: insert_range)
//
// Distances between two resident rows are pair_distance (hvx_graph_dev.h): the reference's summation order over f32 rows of every
// metric and tree, and over bf16 rows (BF), so bf16 images run the same two one-wavefront kernels.
// Every row is read and written with agent-scope atomics (ld_row / st_row) and every lock in this file is the relaxed exchange +
// s_waitcnt of build_link_wg_kernel: no kernel here carries an agent-scope acquire / release (an L2 invalidate / write-back per lock).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hvx_build_plan.h"

using namespace hvx;

namespace hvx {

// select_diverse over cid / csc[0..hyd) (sorted closest first, hyd <= 128), at most m <= 64 kept, then the backfill with the closest
// remaining candidates.  kept[0..return) = the selection in selection order.  One wavefront; the lists live in LDS.
template <uint32_t METRIC, bool FUSED, bool BF>
__device__ __forceinline__ uint32_t select_diverse_wide(const DevIndex &ix, const uint32_t *cid, const float *csc, uint32_t hyd, uint32_t m, uint32_t *kept, int lane) {
    const int grp = lane >> 3, j = lane & 7;
    uint32_t ns = 0;
    for (uint32_t i = 0; i < hyd && ns < m; ++i) {
        const uint32_t ci = cid[i];
        const float si = csc[i];
        bool diverse = true;
        for (uint32_t p0 = 0; p0 < ns; p0 += 8) {
            const uint32_t g = p0 + (uint32_t)grp;
            const uint32_t other = kept[g < ns ? g : ns - 1u];
            const float pd = pair_distance<METRIC, FUSED, BF>(ix, ci, other, j);
            if (__ballot(g < ns && pd < si)) { diverse = false; break; } // strict < rejects (mod.rs:832)
        }
        if (diverse) {
            wave_sync();
            if (lane == 0) kept[ns] = ci;
            ++ns;
            wave_sync();
        }
    }
    if (ns < m) { // backfill, closest first (mod.rs:845-854)
        const unsigned long long lt = (1ull << lane) - 1ull;
        uint32_t mine[2];
        bool free_[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t c = (uint32_t)lane + 64u * (uint32_t)h;
            const bool have = c < hyd;
            mine[h] = have ? cid[c] : kSentinel;
            bool in = false;
            for (uint32_t s = 0; s < ns; ++s) in |= kept[s] == mine[h];
            free_[h] = have && !in;
        }
        const unsigned long long f0 = __ballot(free_[0]), f1 = __ballot(free_[1]);
        const uint32_t n0 = (uint32_t)__builtin_popcountll(f0);
        const uint32_t r0 = (uint32_t)__builtin_popcountll(f0 & lt), r1 = n0 + (uint32_t)__builtin_popcountll(f1 & lt);
        wave_sync();
        if (free_[0] && ns + r0 < m) kept[ns + r0] = mine[0];
        if (free_[1] && ns + r1 < m) kept[ns + r1] = mine[1];
        const uint32_t add = n0 + (uint32_t)__builtin_popcountll(f1);
        ns = ns + add < m ? ns + add : m;
        wave_sync();
    }
    return ns;
}

// ---- step 2: the new node's own neighbour lists ----
template <uint32_t METRIC, bool FUSED, bool BF> __global__ __launch_bounds__(64) void build_select_wide_kernel(BuildArgs a) {
    __shared__ uint32_t s_cid[128], s_kept[64];
    __shared__ float s_csc[128];
    const DevIndex &ix = a.ix;
    const uint32_t q = blockIdx.x, layer = blockIdx.y;
    const int lane = (int)threadIdx.x;
    const uint32_t node = a.nodes[q];
    const uint32_t lv = ix.level[node];
    const uint32_t top = lv < a.layers - 1u ? lv : a.layers - 1u; // min(node level, old max_layer)
    if (layer > top) return; // layers above the old top stay empty rows (mutation.rs:883-894)
    const uint32_t maxn = layer == 0u ? a.m0 : a.m;
    const size_t slot = (size_t)layer * a.b + q;
    const uint32_t cnt = a.cand_cnt[slot];
    const uint32_t lim = 2u * maxn < a.kc ? 2u * maxn : a.kc;
    const uint32_t hyd = cnt < lim ? cnt : lim; // select_neighbors_heuristic hydrates the first 2*Mmax only
    for (uint32_t c = (uint32_t)lane; c < hyd; c += 64u) {
        s_cid[c] = (uint32_t)a.cand_ids[slot * a.kc + c];
        s_csc[c] = a.cand_sc[slot * a.kc + c];
    }
    wave_sync();
    const uint32_t ns = select_diverse_wide<METRIC, FUSED, BF>(ix, s_cid, s_csc, hyd, maxn, s_kept, lane);
    if ((uint32_t)lane < ns) a.sel[slot * a.selw + lane] = s_kept[lane];
    if (lane == 0) a.sel_cnt[slot] = ns;
    uint32_t stride;
    uint32_t *row = row_ptr(a, node, layer, stride);
    if (ns > stride) { if (lane == 0) *a.err = 1u; return; }
    store_canonical_w(row, stride, s_kept, ns, lane); // nobody else can reach this row before the link step
}

// ---- step 3: bidirectional links of the new node, in selection order, top layer first ----
template <uint32_t METRIC, bool FUSED, bool BF> __global__ __launch_bounds__(64) void build_link_wide_kernel(BuildArgs a) {
    __shared__ uint32_t s_ids[128], s_cid[128], s_kept[64];
    __shared__ float s_d[128], s_csc[128];
    const DevIndex &ix = a.ix;
    const uint32_t q = blockIdx.x;
    const int lane = (int)threadIdx.x, grp = lane >> 3, j = lane & 7;
    const uint32_t me = a.nodes[q];
    const uint32_t lv = ix.level[me];
    const uint32_t top = lv < a.layers - 1u ? lv : a.layers - 1u;
    for (int32_t layer = (int32_t)top; layer >= 0; --layer) {
        const uint32_t maxn = layer == 0 ? a.m0 : a.m;
        const size_t slot = (size_t)layer * a.b + q;
        const uint32_t ns = a.sel_cnt[slot];
        for (uint32_t s = 0; s < ns; ++s) {
            const uint32_t to = a.sel[slot * a.selw + s];
            // add_bidirectional_link(from = me, to) (mutation.rs:1498-1583)
            lock_row_w(a.locks, to, lane);
            uint32_t stride;
            uint32_t *row = row_ptr(a, to, (uint32_t)layer, stride);
            uint32_t v = (uint32_t)lane < stride ? ld_row(row + lane) : kSentinel; // (stride <= 64: the host checked)
            uint32_t deg = (uint32_t)__builtin_popcountll(__ballot(v != kSentinel));
            const bool present = __ballot(v == me) != 0ull;
            bool extra = false; // the appended id is the 65th of the list (index 64)
            if (!present) {
                if (deg >= 64u) extra = true;
                else if ((uint32_t)lane == deg) v = me; // rows are canonical: the valid ids occupy lanes 0..deg-1
                ++deg;
            }
            const uint32_t nc = deg;
            uint32_t dropped_id[2] = {kSentinel, kSentinel}; // per lane: candidates this prune removed
            if (nc > maxn) {
                // rank the row's neighbours by distance to its owner, select_diverse with the owner as the reference point
                wave_sync();
                if ((uint32_t)lane < nc) s_ids[lane] = v;
                if (extra && lane == 0) s_ids[64] = me;
                wave_sync();
                for (uint32_t p0 = 0; p0 < nc; p0 += 8) {
                    const uint32_t g = p0 + (uint32_t)grp;
                    const uint32_t other = s_ids[g < nc ? g : nc - 1u];
                    const float d = pair_distance<METRIC, FUSED, BF>(ix, to, other, j);
                    if (g < nc && j == 0) s_d[g] = d;
                }
                wave_sync();
                uint32_t idm[2], rank[2] = {0u, 0u};
                float dm_[2];
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const uint32_t c = (uint32_t)lane + 64u * (uint32_t)h;
                    idm[h] = c < nc ? s_ids[c] : kSentinel;
                    dm_[h] = c < nc ? s_d[c] : 0.f;
                }
                for (uint32_t t = 0; t < nc; ++t) { // Candidate order: score, then id (model.rs:55-61)
                    const float dt = s_d[t];
                    const uint32_t it = s_ids[t];
                    rank[0] += (dt < dm_[0] || (dt == dm_[0] && it < idm[0])) ? 1u : 0u;
                    rank[1] += (dt < dm_[1] || (dt == dm_[1] && it < idm[1])) ? 1u : 0u;
                }
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    if ((uint32_t)lane + 64u * (uint32_t)h < nc) { s_cid[rank[h]] = idm[h]; s_csc[rank[h]] = dm_[h]; }
                wave_sync();
                const uint32_t keepn = select_diverse_wide<METRIC, FUSED, BF>(ix, s_cid, s_csc, nc, maxn, s_kept, lane);
                bool kept_mine[2] = {false, false};
                for (uint32_t t = 0; t < keepn; ++t) { kept_mine[0] |= s_kept[t] == idm[0]; kept_mine[1] |= s_kept[t] == idm[1]; }
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    if ((uint32_t)lane + 64u * (uint32_t)h < nc && !kept_mine[h]) dropped_id[h] = idm[h];
                if (keepn > stride) { if (lane == 0) *a.err = 1u; }
                else store_canonical_w(row, stride, s_kept, keepn, lane);
            } else if (!present) {
                if (nc > stride) { if (lane == 0) *a.err = 1u; }
                else {
                    wave_sync();
                    if ((uint32_t)lane < nc) s_kept[lane] = v; // (nc <= maxn <= 64: the appended id sits in a lane)
                    wave_sync();
                    store_canonical_w(row, stride, s_kept, nc, lane);
                }
            }
            unlock_row_w(a.locks, to, lane);
            // every neighbour dropped by the prune loses its edge to `to` as well: the graph stays symmetric (mutation.rs:1890-1908)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                unsigned long long dm = __ballot(dropped_id[h] != kSentinel);
                while (dm) {
                    const uint32_t src = (uint32_t)__builtin_ctzll(dm);
                    dm &= dm - 1ull;
                    const uint32_t x = __builtin_amdgcn_readlane(dropped_id[h], src);
                    remove_edge_w(a, (uint32_t)layer, x, to, lane);
                }
            }
            wave_sync();
        }
    }
}

// ---- step 3, batched mode: one 1 024-thread workgroup per LINK (new node q, layer, selected neighbour s) ----
// The wide twin of build_link_wg_kernel (hvx_build.hip): up to 65 candidate rows + the owner's = 66 rows, 2 145 pairs.  The narrow
// kernel's shape (4 wavefronts x 18 pair steps) would need 68 float4 accumulators per lane here; instead SIXTEEN wavefronts take 17
// steps of 8 pairs each (16 x 17 x 8 = 2 176 >= 2 145): 68 accumulator registers per lane, under the 128 a 1 024-thread workgroup may
// use.  What makes the narrow kernel work is kept: the rows pass through LDS in column blocks (row stride 128 B mod 256 B), each
// lane's fma chain runs over the depth in the reference's order with its accumulators carried from block to block, the next block is in
// flight in registers under the arithmetic, and the row locks are relaxed atomics + s_waitcnt vmcnt(0).  A 1 024-thread workgroup
// means four wavefronts per SIMD whatever the LDS, so the registers decide the block width: blocks of <= 128 floats (3 float4 per
// thread in flight: 66 rows x 32 float4 / 1 024 threads) compile without scratch, blocks of 256 floats (5 float4) spill 14 dwords.
// 66 rows x 160 floats = 42 KB + a 66 x 66 distance matrix (17 KB) + lists = 68 KB of LDS, one or two workgroups per CU (the second
// only where the first has shrunk to its tail wavefront: 16 + 16 wavefronts of 128 registers do not fit a CU).
// (kWideTasks = 17, kWidePre = 3 float4 in flight, kWideWaves = 16, the LDS size and where the kernel serves: wide_link_geom, hvx_build_plan.h)

struct WideLinkLds {
    float *rows;              // [ncmax + 1][ldp]: this column block of the candidate rows (list order), then the owner's
    float *D;                 // [ncmax + 1][ncmax + 1] pairwise distances (index nc = the owner)
    unsigned long long *P;    // [128][2] predicate masks, sorted order
    uint32_t *cand;           // [128] ids in list order
    uint32_t *cid;            // [128] ids sorted by (distance to the owner, id)
    float *csc;               // [128] their distances
    uint32_t *srow;           // [128] list index of sorted candidate r
    uint32_t *fin;            // [64] ids of the pruned row
    uint32_t *sh;             // [8] nc, prune, present, overflow
    unsigned char *pa, *pb;   // [pairs] the two rows of pair p
};
__device__ __forceinline__ WideLinkLds carve_wide_link(char *smem, uint32_t ldp, uint32_t ncmax) {
    WideLinkLds L;
    L.rows = reinterpret_cast<float *>(smem);
    char *p = smem + (size_t)(ncmax + 1u) * ldp * 4u;
    L.P = reinterpret_cast<unsigned long long *>(p); p += 128 * 16;
    L.D = reinterpret_cast<float *>(p); p += (size_t)(ncmax + 1u) * (ncmax + 1u) * 4u;
    L.cand = reinterpret_cast<uint32_t *>(p); p += 512;
    L.cid = reinterpret_cast<uint32_t *>(p); p += 512;
    L.csc = reinterpret_cast<float *>(p); p += 512;
    L.srow = reinterpret_cast<uint32_t *>(p); p += 512;
    L.fin = reinterpret_cast<uint32_t *>(p); p += 256;
    L.sh = reinterpret_cast<uint32_t *>(p); p += 32;
    L.pa = reinterpret_cast<unsigned char *>(p); p += wide_pairs_max(ncmax);
    L.pb = reinterpret_cast<unsigned char *>(p);
    return L;
}

template <uint32_t METRIC, bool FUSED> __global__ __launch_bounds__(1024) void build_link_wide_wg_kernel(BuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DevIndex &ix = a.ix;
    const uint32_t q = blockIdx.x >> 6, s = blockIdx.x & 63u, layer = blockIdx.y;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 3, j = lane & 7;
    const uint32_t me = a.nodes[q];
    const uint32_t lv = ix.level[me];
    const uint32_t top = lv < a.layers - 1u ? lv : a.layers - 1u;
    if (layer > top) return;
    const size_t slot = (size_t)layer * a.b + q;
    if (s >= a.sel_cnt[slot]) return;
    const uint32_t to = a.sel[slot * a.selw + s];
    const uint32_t maxn = layer == 0u ? a.m0 : a.m;
    WideLinkLds L = carve_wide_link(smem, a.ldp, a.ncmax);
    uint32_t stride;
    uint32_t *row = row_ptr(a, to, layer, stride);

    // ---- add_bidirectional_link(from = me, to) (mutation.rs:1498-1583): append under the row owner's lock ----
    if (wave == 0) {
        lock_row_w(a.locks, to, lane);
        uint32_t v = (uint32_t)lane < stride ? ld_row(row + lane) : kSentinel; // (stride <= 64: the host checked)
        uint32_t deg = (uint32_t)__builtin_popcountll(__ballot(v != kSentinel));
        const bool present = __ballot(v == me) != 0ull;
        bool extra = false; // the appended id is the 65th of the list (index 64)
        if (!present) {
            if (deg >= 64u) extra = true;
            else if ((uint32_t)lane == deg) v = me; // rows are canonical: the valid ids occupy lanes 0..deg-1
            ++deg;
        }
        // more rows than the LDS was sized for, or a list within its limit that the row cannot hold: cannot happen on rows this build wrote
        const bool overflow = (deg > maxn && deg > a.ncmax) || (deg <= maxn && deg > stride) || maxn > stride;
        L.cand[lane] = v;
        if (lane == 0) {
            L.cand[64] = extra ? me : kSentinel;
            L.sh[0] = deg;
            L.sh[1] = (deg > maxn && !overflow) ? 1u : 0u;
            L.sh[2] = present ? 1u : 0u;
            L.sh[3] = overflow ? 1u : 0u;
            if (overflow) *a.err = 1u;
        }
    }
    __syncthreads();
    const uint32_t nc = L.sh[0];
    if (L.sh[1] == 0u) { // no prune: the appended id takes its place in the canonical row
        if (wave == 0) {
            if (L.sh[2] == 0u && L.sh[3] == 0u) store_canonical_w(row, stride, L.cand, nc, lane);
            unlock_row_w(a.locks, to, lane);
            if (lane == 0) HVX_DBG_ADD(a, 3, 1);
        }
        return;
    }

    // ---- all pairwise distances among the nc candidate rows and the owner's row (index nc) ----
    const uint32_t nrows = nc + 1u, npairs = nrows * nc / 2u;
    if ((uint32_t)tid >= 1u && (uint32_t)tid < nrows) { // pair p = b (b - 1) / 2 + a  <->  rows a < b
        const uint32_t b = (uint32_t)tid, base = b * (b - 1u) / 2u;
        for (uint32_t aa = 0; aa < b; ++aa) { L.pa[base + aa] = (unsigned char)aa; L.pb[base + aa] = (unsigned char)b; }
    }
    const uint32_t nk = ix.dim_main >> 5;                 // 32-float chunks of a row (dim == dim_main == ld: the host checked)
    const uint32_t ck = a.link_ck;                        // chunks per column block (even)
    const uint32_t nblocks = (nk + ck - 1u) / ck;
    const uint32_t w4 = ck * 8u;                          // float4 per row and block
    float4 pre[kWidePre];
#pragma unroll
    for (int u = 0; u < kWidePre; ++u) pre[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    auto prefetch = [&](uint32_t blk) __attribute__((always_inline)) {
        const uint32_t c0 = blk * w4, cw = (nk - blk * ck < ck ? nk - blk * ck : ck) * 8u;
#pragma unroll
        for (int u = 0; u < kWidePre; ++u) {
            const uint32_t e = (uint32_t)tid + 1024u * (uint32_t)u;
            const uint32_t r = e / w4, c = e - r * w4;
            if (r < nrows && c < cw) {
                const uint32_t node = r < nc ? L.cand[r] : to;
                pre[u] = reinterpret_cast<const float4 *>(ix.vec + (size_t)node * ix.ld)[c0 + c];
            }
        }
    };
    auto commit = [&](uint32_t blk) __attribute__((always_inline)) {
        const uint32_t cw = (nk - blk * ck < ck ? nk - blk * ck : ck) * 8u;
#pragma unroll
        for (int u = 0; u < kWidePre; ++u) {
            const uint32_t e = (uint32_t)tid + 1024u * (uint32_t)u;
            const uint32_t r = e / w4, c = e - r * w4;
            if (r < nrows && c < cw) reinterpret_cast<float4 *>(L.rows + (size_t)r * a.ldp)[c] = pre[u];
        }
    };
    float4 acc[kWideTasks];
#pragma unroll
    for (int t = 0; t < kWideTasks; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int slot4 = chunk_slot(j);
    prefetch(0);
    for (uint32_t blk = 0; blk < nblocks; ++blk) {
        commit(blk);
        __syncthreads(); // block blk is in LDS (first round: and the pair table)
        if (blk + 1u < nblocks) prefetch(blk + 1u); // in flight underneath the arithmetic
        const uint32_t ckb = nk - blk * ck < ck ? nk - blk * ck : ck;
#pragma unroll
        for (int t = 0; t < kWideTasks; ++t) {
            const uint32_t p0 = ((uint32_t)wave + kWideWaves * (uint32_t)t) * 8u;
            if (p0 >= npairs) continue; // uniform in the wavefront
            const uint32_t p = p0 + (uint32_t)grp;
            const uint32_t pp = p < npairs ? p : npairs - 1u;
            const float4 *qp = reinterpret_cast<const float4 *>(L.rows + (size_t)L.pa[pp] * a.ldp) + slot4;
            const float4 *rp = reinterpret_cast<const float4 *>(L.rows + (size_t)L.pb[pp] * a.ldp) + slot4;
            float4 ac = acc[t];
#pragma unroll 2
            for (uint32_t k = 0; k < ckb; ++k) {
                const float4 x = rp[k * 8u];
                const float4 qq = qp[k * 8u];
                if (METRIC == kL2) {
                    const float d0 = qq.x - x.x, d1 = qq.y - x.y, d2 = qq.z - x.z, d3 = qq.w - x.w;
                    if (FUSED) {
                        ac.x = __builtin_fmaf(d0, d0, ac.x); ac.y = __builtin_fmaf(d1, d1, ac.y);
                        ac.z = __builtin_fmaf(d2, d2, ac.z); ac.w = __builtin_fmaf(d3, d3, ac.w);
                    } else {
                        ac.x = d0 * d0 + ac.x; ac.y = d1 * d1 + ac.y;
                        ac.z = d2 * d2 + ac.z; ac.w = d3 * d3 + ac.w;
                    }
                } else {
                    if (FUSED) {
                        ac.x = __builtin_fmaf(qq.x, x.x, ac.x); ac.y = __builtin_fmaf(qq.y, x.y, ac.y);
                        ac.z = __builtin_fmaf(qq.z, x.z, ac.z); ac.w = __builtin_fmaf(qq.w, x.w, ac.w);
                    } else {
                        ac.x = qq.x * x.x + ac.x; ac.y = qq.y * x.y + ac.y;
                        ac.z = qq.z * x.z + ac.z; ac.w = qq.w * x.w + ac.w;
                    }
                }
            }
            acc[t] = ac;
        }
        __syncthreads(); // everybody is done with block blk before the next one overwrites it
    }
#pragma unroll
    for (int t = 0; t < kWideTasks; ++t) {
        const uint32_t p0 = ((uint32_t)wave + kWideWaves * (uint32_t)t) * 8u;
        if (p0 >= npairs) continue;
        const uint32_t p = p0 + (uint32_t)grp;
        float r = avx_tree_reduce(acc[t]); // every lane of the group takes part
        if (p < npairs) {
            const uint32_t ra = L.pa[p], rb = L.pb[p];
            if (METRIC == kCosine) {
                const uint32_t na = ra < nc ? L.cand[ra] : to, nb = rb < nc ? L.cand[rb] : to;
                r = cosine_finish(r, ix.hdr[na], ix.hdr[nb], ix.vec + (size_t)na * ix.ld, ix.vec + (size_t)nb * ix.ld, ix.dim);
            }
            if (j == 0) { L.D[ra * nrows + rb] = r; L.D[rb * nrows + ra] = r; }
        }
    }
    __syncthreads();

    // ---- rank the row's neighbours by distance to its owner (Candidate order: score, then id; model.rs:55-61) ----
    if ((uint32_t)tid < nc) {
        const float dmine = L.D[nc * nrows + (uint32_t)tid];
        const uint32_t v = L.cand[tid];
        uint32_t rank = 0;
        for (uint32_t t = 0; t < nc; ++t) {
            const float dt = L.D[nc * nrows + t];
            const uint32_t it = L.cand[t];
            rank += (dt < dmine || (dt == dmine && it < v)) ? 1u : 0u;
        }
        L.cid[rank] = v;
        L.csc[rank] = dmine;
        L.srow[rank] = (uint32_t)tid;
    }
    __syncthreads();
    if (wave != 0) return;
    // ---- P[i] bit jj = dist(c_i, c_jj) < dist(c_i, owner), jj < i in sorted order (strict <: mod.rs:832) ----
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t c = (uint32_t)lane + 64u * (uint32_t)h;
        if (c < nc) {
            const uint32_t ri = L.srow[c];
            const float si = L.csc[c];
            unsigned long long lo = 0ull, hi = 0ull;
            for (uint32_t jj = 0; jj < c; ++jj)
                if (L.D[ri * nrows + L.srow[jj]] < si) { if (jj < 64u) lo |= 1ull << jj; else hi |= 1ull << (jj - 64u); }
            L.P[2u * c] = lo;
            L.P[2u * c + 1u] = hi;
        }
    }
    wave_sync();

    // ---- select_diverse + backfill over the masks (mod.rs:809-856); all lanes walk the same chain ----
    unsigned long long klo = 0ull, khi = 0ull;
    uint32_t ns = 0;
    for (uint32_t i = 0; i < nc && ns < maxn; ++i)
        if (((L.P[2u * i] & klo) | (L.P[2u * i + 1u] & khi)) == 0ull) { if (i < 64u) klo |= 1ull << i; else khi |= 1ull << (i - 64u); ++ns; }
    for (uint32_t i = 0; i < nc && ns < maxn; ++i) {
        const bool in = i < 64u ? ((klo >> i) & 1ull) != 0ull : ((khi >> (i - 64u)) & 1ull) != 0ull;
        if (!in) { if (i < 64u) klo |= 1ull << i; else khi |= 1ull << (i - 64u); ++ns; }
    }
    const unsigned long long lt = (1ull << lane) - 1ull;
    const uint32_t nlo = (uint32_t)__builtin_popcountll(klo);
    uint32_t dropped_id[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t c = (uint32_t)lane + 64u * (uint32_t)h;
        const bool have = c < nc;
        const uint32_t mine = have ? L.cid[c] : kSentinel;
        const bool in = have && (((h == 0 ? klo : khi) >> lane) & 1ull) != 0ull;
        if (in) L.fin[h == 0 ? (uint32_t)__builtin_popcountll(klo & lt) : nlo + (uint32_t)__builtin_popcountll(khi & lt)] = mine;
        dropped_id[h] = (have && !in) ? mine : kSentinel;
    }
    wave_sync();
    store_canonical_w(row, stride, L.fin, ns, lane); // (ns <= maxn <= stride)
    unlock_row_w(a.locks, to, lane);
    // every neighbour dropped by the prune loses its edge to `to` as well (mutation.rs:1890-1908): the graph stays symmetric
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        unsigned long long dm = __ballot(dropped_id[h] != kSentinel);
        while (dm) {
            const uint32_t src = (uint32_t)__builtin_ctzll(dm);
            dm &= dm - 1ull;
            const uint32_t x = __builtin_amdgcn_readlane(dropped_id[h], src);
            remove_edge_w(a, layer, x, to, lane);
            if (lane == 0) HVX_DBG_ADD(a, 2, 1);
        }
    }
    if (lane == 0) HVX_DBG_ADD(a, 1, 1);
}

// ---- host side: one instantiation per (metric, summation tree), as in hvx_build.hip ----
using WideKernel = void (*)(BuildArgs);
struct WideKernels { WideKernel select, link, link_wg; };
template <uint32_t METRIC, bool FUSED> static WideKernels wide_kernels_of() {
    WideKernels k{build_select_wide_kernel<METRIC, FUSED, false>, build_link_wide_kernel<METRIC, FUSED, false>, nullptr};
    if constexpr (METRIC != kL1) k.link_wg = build_link_wide_wg_kernel<METRIC, FUSED>;
    return k;
}
template <uint32_t METRIC> static WideKernels wide_kernels_bf16() {
    return WideKernels{build_select_wide_kernel<METRIC, true, true>, build_link_wide_kernel<METRIC, true, true>, nullptr};
}
static WideKernels pick_wide_kernels(uint32_t metric, bool fused, bool bf16) {
    if (bf16) return metric == kL2 ? wide_kernels_bf16<kL2>() : wide_kernels_bf16<kCosine>();
    if (metric == kL2) return fused ? wide_kernels_of<kL2, true>() : wide_kernels_of<kL2, false>();
    if (metric == kCosine) return fused ? wide_kernels_of<kCosine, true>() : wide_kernels_of<kCosine, false>();
    return fused ? wide_kernels_of<kL1, true>() : wide_kernels_of<kL1, false>();
}

hipError_t launch_build_select_wide(const BuildArgs &a, bool fused, bool bf16, dim3 grid, hipStream_t s) {
    const WideKernels k = pick_wide_kernels(a.ix.metric, fused, bf16);
    hipLaunchKernelGGL(k.select, grid, dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_build_link_wide(const BuildArgs &a, bool fused, bool bf16, uint32_t nodes, hipStream_t s) {
    const WideKernels k = pick_wide_kernels(a.ix.metric, fused, bf16);
    hipLaunchKernelGGL(k.link, dim3(nodes), dim3(64), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_build_link_wide_wg(const BuildArgs &a, bool fused, uint32_t layers, size_t lds, hipStream_t s) {
    const WideKernels k = pick_wide_kernels(a.ix.metric, fused, false);
    if (!k.link_wg) return hipErrorInvalidValue;
    if (lds > 48 * 1024) { // (68 KB at 66 rows; the attribute is per function AND device)
        const hipError_t e = hipFuncSetAttribute((const void *)k.link_wg, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k.link_wg, dim3(a.b * kSelWide, layers), dim3(1024), lds, s, a);
    return hipGetLastError();
}

} // namespace hvx
