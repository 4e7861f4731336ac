// hvx_build_wide_seq.hip -- ONE node at a time into an image with degree limits above 32 (M 32 / M0 64, the reference's scale fixture:
// scale_contracts.rs:167-173): sequential builds, every upsert, every promotion, hvx_index_insert_batch with one node per step.  The
// one-wavefront kernels of hvx_build_wide.hip evaluate select_diverse lazily -- a chain of dependent row gathers per candidate.  The two
// kernels here are the wide restatement of build_select_seq_kernel / build_link_seq_kernel (hvx_build.hip): the distance matrices of ALL
// prunes of a step are evaluated up front, spread over the layer's workgroups (one 8-lane group per pair, pair_distance: the reference's
// summation order over f32 and bf16 rows), and the last workgroup to deliver replays the decisions (hvx_graph_dev.h):
//   build_select_wide_seq_kernel   the node's own lists: <= 128 search candidates on layer 0 (8 128 pairs, replay_rows2<128>), <= 64 above
//                                  (2 016 pairs, replay_rows<64>);
//   build_link_wide_seq_kernel     add_bidirectional_link (mutation.rs:1498-1583) for its <= 64 selected neighbours per layer IN SELECTION
//                                  ORDER.  Every link's list (row + the node, <= 65 ids: two per lane, 128-bit position masks) and its matrix
//                                  are taken from the rows as the kernel finds them, sixteen wavefronts replay the links speculatively, and
//                                  one wavefront walks them in order: the only thing an earlier link of the same node can do to a later
//                                  link's row is REMOVE an id, and such a link is replayed over the ids still there (replay_rows2's `alive`).
//                                  The rows go out once each, the removals last.  No row locks: one node is in flight.
// Same distances, same comparisons, same order of decisions as the one-wavefront kernels (hvx_build_params.link_mode = 1 selects those).
// Geometry -- matrices in BuildArgs.gdm, the pair prefix, grids, LDS: wide_seq_geom (hvx_build_dev.h).
// No agent-scope acquire / release: matrix words are st_agent stores, stores_done() + a barrier come before the relaxed ticket, the last
// workgroup resets the ticket word, rows are written with st_row / store_canonical_reg.
#include <hip/hip_runtime.h>

#include "hvx_build_dev.h"

using namespace hvx;

namespace hvx {

static_assert(kWideSeqW2 == kWide2Words, "replay_rows2's scratch");

template <uint32_t METRIC, bool FUSED, bool BF> __global__ __launch_bounds__(256) void build_select_wide_seq_kernel(BuildArgs a) {
    __shared__ uint32_t s_cid[128], s_w2[kWide2Words], s_last;
    const DevIndex &ix = a.ix;
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    uint32_t L, g, G;
    if (blockIdx.x < a.g0) { L = 0u; g = blockIdx.x; G = a.g0; }
    else { L = 1u + (blockIdx.x - a.g0) / a.gu; g = (blockIdx.x - a.g0) % a.gu; G = a.gu; }
    const uint32_t node = a.nodes[0];
    const uint32_t lv = ix.level[node];
    const uint32_t top = lv < a.layers - 1u ? lv : a.layers - 1u; // min(node level, old max_layer)
    if (L > top) return; // layers above the old top stay empty rows (mutation.rs:883-894)
    const WideSeqGeom geo = wide_seq_geom(a.m, a.m0, a.layers);
    const uint32_t maxn = L == 0u ? a.m0 : a.m;
    const uint32_t rw = geo.sel_rw[L ? 1 : 0];
    const size_t slot = (size_t)L * a.b;
    const uint32_t cnt = a.cand_cnt[slot];
    const uint32_t lim = 2u * maxn < a.kc ? 2u * maxn : a.kc;
    const uint32_t hyd = cnt < lim ? cnt : lim; // select_neighbors_heuristic hydrates the first 2*Mmax only
    float *gl = a.gdm + geo.sel_off(L);
    if (tid < hyd) s_cid[tid] = (uint32_t)a.cand_ids[slot * a.kc + tid];
    __syncthreads();
    bool last = g == 0u;
    const uint32_t npairs = hyd * (hyd - (hyd ? 1u : 0u)) / 2u;
    if (npairs != 0u) {
        if (g == 0u && tid < hyd) st_agent(gl + hyd * rw + tid, a.cand_sc[slot * a.kc + tid]); // the owner's row: the search's scores
        const int j = (int)(lane & 7u);
        for (uint32_t q = g * 32u + (tid >> 3); q < npairs; q += G * 32u) {
            uint32_t i, jj;
            pair_of(q, i, jj); // 0 <= jj < i < hyd
            const uint32_t ni = s_cid[i], nj = s_cid[jj];
            const float d = pair_distance<METRIC, FUSED, BF>(ix, ni, nj, j);
            if (j == 0) { st_agent(gl + i * rw + jj, d); st_agent(gl + jj * rw + i, d); }
        }
        last = last_workgroup(a.tick, L, G, &s_last, true); // (hvx_handoff.h; the ticket goes back to zero)
    }
    if (!last || wave != 0u) return;
    uint32_t ns = hyd;
    bool bad = false;
    const uint32_t *kept = s_w2 + kWide2Kept;
    if (hyd >= 2u) {
        if (rw == 128u) ns = replay_rows2<128>(gl, s_cid, hyd, maxn, lane, s_w2, &bad);
        else ns = replay_rows<64>(gl, s_cid, hyd, maxn, lane, WaveScratch{s_w2, s_w2 + kWide2Kept}, &bad);
    } else if (lane < hyd) s_w2[kWide2Kept + lane] = s_cid[lane];
    lds_order();
    const uint32_t kf = lane < ns ? kept[lane] : kSentinel; // (ns <= maxn <= 64)
    if (lane < ns) a.sel[slot * a.selw + lane] = kf;
    if (lane == 0) a.sel_cnt[slot] = ns;
    uint32_t stride;
    uint32_t *row = row_ptr(a, node, L, stride);
    if (ns > stride) { if (lane == 0) *a.err = 1u; return; }
    store_canonical_reg(row, stride, kf, ns, lane); // nobody else can reach this row before the link step
}

struct WideSeqLds {
    uint32_t *rcur, *rkept;   // [64][kWideSeqLS] a link's list (row + the node) / what stays of it
    uint32_t *rdeg, *rkn;     // [64] ids in the list / ids that stay
    uint32_t *rd;             // [64][4] dropped ids by list position (two 64-bit words)
    uint32_t *to;             // [64] the selected neighbours, selection order
    uint32_t *px, *pv;        // [kWideSeqPairs] removals: row px loses pv
    uint32_t *pbase;          // [65]
    uint32_t *wsc;            // [kWideSeqWaves][kWide2Words]
};
__device__ __forceinline__ WideSeqLds carve_wide_seq(char *smem) {
    WideSeqLds S;
    uint32_t *p = reinterpret_cast<uint32_t *>(smem);
    S.wsc = p; p += kWideSeqWaves * kWide2Words; // (first: replay_rows2 reads its keys as 64-bit words)
    S.rcur = p; p += 64 * kWideSeqLS;
    S.rkept = p; p += 64 * kWideSeqLS;
    S.rdeg = p; p += 64; S.rkn = p; p += 64; S.rd = p; p += 64 * 4; S.to = p; p += 64;
    S.px = p; p += kWideSeqPairs; S.pv = p; p += kWideSeqPairs;
    S.pbase = p; // 68
    return S;
}

template <uint32_t METRIC, bool FUSED, bool BF> __global__ __launch_bounds__(1024) void build_link_wide_seq_kernel(BuildArgs a) {
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
    const WideSeqGeom geo = wide_seq_geom(a.m, a.m0, a.layers);
    const WideSeqLds S = carve_wide_seq(smem);
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (tid == 0) s_err = 0u;
    if (tid < ns) S.to[tid] = a.sel[slot * a.selw + tid]; // (ns <= maxn <= 64)
    __syncthreads();
    // ---- the links' lists, from the rows as they are now (every workgroup of the layer arrives at the same lists) ----
    for (uint32_t t = wave; t < ns; t += kWideSeqWaves) {
        const uint32_t to = S.to[t];
        uint32_t stride;
        const uint32_t *row = row_ptr(a, to, L, stride);
        uint32_t v = lane < stride ? ld_row(row + lane) : kSentinel; // (stride <= 64: the host checked)
        uint32_t deg = (uint32_t)__builtin_popcountll(__ballot(v != kSentinel));
        const bool present = __ballot(v == me) != 0ull;
        bool extra = false; // the appended id is the 65th of the list (index 64)
        if (!present) {
            if (deg >= 64u) extra = true;
            else if (lane == deg) v = me; // rows are canonical: the valid ids occupy lanes 0..deg-1
            ++deg;
        }
        if (stride > 64u) { if (lane == 0) s_err = 1u; deg = 0u; }
        if (lane < deg) S.rcur[t * kWideSeqLS + lane] = v;
        if (extra && lane == 0) S.rcur[t * kWideSeqLS + 64u] = me;
        if (lane == 0) S.rdeg[t] = deg;
    }
    __syncthreads();
    if (s_err) { if (g == 0u && tid == 0) *a.err = 1u; return; }
    if (wave == 0) { // first pair of every link's prune (a list within its limit needs no matrix)
        const uint32_t rd = lane < ns ? S.rdeg[lane] : 0u;
        const uint32_t np = wide_seq_list_pairs(rd, maxn);
        uint32_t incl = np;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            const uint32_t o = __shfl_up(incl, sft, 64);
            if ((int)lane >= sft) incl += o;
        }
        S.pbase[lane] = incl - np;
        if (lane == 63u) S.pbase[64] = incl;
    }
    __syncthreads();
    const uint32_t total = S.pbase[64];
    float *gl = a.gdm + geo.link_off(L, 0u);
    pair_sweep<METRIC, FUSED, BF, 1024>(ix, S.pbase, ns, total, g, G, [&](uint32_t t) __attribute__((always_inline)) {
        return PairTask{S.rcur + t * kWideSeqLS, S.rdeg[t], S.to[t], gl + (size_t)t * geo.link_dm, kWideSeqRS};
    });
    // (the ticket is taken even when no list needs a matrix: the last workgroup rewrites rows the others are still reading their lists from)
    if (!last_workgroup(a.tick, a.layers + L, G, &s_last, true)) return;
    // ---- the last workgroup: every link replayed on its list as found (sixteen at a time) ...
    uint32_t *W2 = S.wsc + wave * kWide2Words;
    const uint32_t *kept = W2 + kWide2Kept;
    bool bad = false; // (a distance that is no valid score: add_bidirectional_link does not look, neither does the one-wavefront kernel)
    for (uint32_t t = wave; t < ns; t += kWideSeqWaves) {
        const uint32_t deg = S.rdeg[t];
        const uint32_t *rc = S.rcur + t * kWideSeqLS;
        uint32_t kn = deg;
        unsigned long long dropped[2] = {0ull, 0ull};
        if (deg > maxn) kn = replay_rows2<(int)kWideSeqRS>(gl + (size_t)t * geo.link_dm, rc, deg, maxn, lane, W2, &bad, nullptr, dropped);
        else if (lane < deg) W2[kWide2Kept + lane] = rc[lane]; // (deg <= maxn <= 64)
        lds_order();
        if (lane < kn) S.rkept[t * kWideSeqLS + lane] = kept[lane];
        if (lane == 0) {
            S.rkn[t] = kn;
            S.rd[t * 4u + 0u] = (uint32_t)dropped[0]; S.rd[t * 4u + 1u] = (uint32_t)(dropped[0] >> 32);
            S.rd[t * 4u + 2u] = (uint32_t)dropped[1]; S.rd[t * 4u + 3u] = (uint32_t)(dropped[1] >> 32);
        }
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
            const uint32_t *rc = S.rcur + s * kWideSeqLS;
            const bool have0 = lane < deg, have1 = lane + 64u < deg;
            const uint32_t mine0 = have0 ? rc[lane] : kSentinel, mine1 = have1 ? rc[lane + 64u] : kSentinel;
            bool gone0 = false, gone1 = false; // my id has been removed from this row by an earlier link
            for (uint32_t i = 0; i < np; ++i) {
                const bool here = S.px[i] == to;
                const uint32_t vi = S.pv[i];
                gone0 |= here && vi == mine0;
                gone1 |= here && vi == mine1;
            }
            const unsigned long long alive[2] = {__ballot(have0 && !gone0), __ballot(have1 && !gone1)};
            unsigned long long dropped[2] = {((unsigned long long)S.rd[s * 4u + 1u] << 32) | S.rd[s * 4u + 0u], ((unsigned long long)S.rd[s * 4u + 3u] << 32) | S.rd[s * 4u + 2u]};
            if (alive[0] != __ballot(have0) || alive[1] != __ballot(have1)) {
                const uint32_t nlo = (uint32_t)__builtin_popcountll(alive[0]), nlive = nlo + (uint32_t)__builtin_popcountll(alive[1]);
                uint32_t kn;
                dropped[0] = 0ull; dropped[1] = 0ull;
                if (nlive > maxn) {
                    kn = replay_rows2<(int)kWideSeqRS>(gl + (size_t)s * geo.link_dm, rc, deg, maxn, lane, W2, &bad, alive, dropped);
                } else { // (nlive <= maxn <= 64)
                    if ((alive[0] >> lane) & 1ull) W2[kWide2Kept + (uint32_t)__builtin_popcountll(alive[0] & lt)] = mine0;
                    if ((alive[1] >> lane) & 1ull) W2[kWide2Kept + nlo + (uint32_t)__builtin_popcountll(alive[1] & lt)] = mine1;
                    kn = nlive;
                    lds_order();
                }
                if (lane < kn) S.rkept[s * kWideSeqLS + lane] = kept[lane];
                if (lane == 0) S.rkn[s] = kn;
                lds_order();
            }
            // every neighbour dropped by the prune loses its edge to `to` as well: the graph stays symmetric (mutation.rs:1890-1908)
            const uint32_t dn0 = (uint32_t)__builtin_popcountll(dropped[0]), dn = dn0 + (uint32_t)__builtin_popcountll(dropped[1]);
            const uint32_t at0 = np + (uint32_t)__builtin_popcountll(dropped[0] & lt), at1 = np + dn0 + (uint32_t)__builtin_popcountll(dropped[1] & lt);
            if (((dropped[0] >> lane) & 1ull) != 0ull && at0 < kWideSeqPairs) { S.px[at0] = mine0; S.pv[at0] = to; }
            if (((dropped[1] >> lane) & 1ull) != 0ull && at1 < kWideSeqPairs) { S.px[at1] = mine1; S.pv[at1] = to; }
            np += dn;
            if (np > kWideSeqPairs) { if (lane == 0) *a.err = 1u; np = kWideSeqPairs; } // (rows of more than 64 ids only: never silently)
            lds_order();
        }
        if (lane == 0) s_np = np;
    }
    __syncthreads();
    // ---- the rows.  Every neighbour dropped by a prune loses its edge back (mutation.rs:1890-1908): a neighbour row (a link's own row) gets
    // its removals before it is stored -- one store per row, nothing in this kernel reads a row it has written --, every other row that
    // loses edges (the node's own among them) is read, compacted and stored by the first removal that names it
    const uint32_t np = s_np;
    for (uint32_t t = wave; t < ns; t += kWideSeqWaves) {
        if (S.rdeg[t] == 0u) continue;
        const uint32_t kn = S.rkn[t], to = S.to[t];
        const uint32_t v = lane < kn ? S.rkept[t * kWideSeqLS + lane] : kSentinel; // (kn <= maxn <= 64)
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
    for (uint32_t i = wave; i < np; i += kWideSeqWaves) {
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

// ---- host side: the instantiations of pick_wide_kernels (hvx_build_wide.hip) ----
using WideSeqKernel = void (*)(BuildArgs);
struct WideSeqKernels { WideSeqKernel select, link; };
template <uint32_t METRIC, bool FUSED, bool BF> static WideSeqKernels wide_seq_kernels_of() {
    return WideSeqKernels{build_select_wide_seq_kernel<METRIC, FUSED, BF>, build_link_wide_seq_kernel<METRIC, FUSED, BF>};
}
static WideSeqKernels pick_wide_seq_kernels(uint32_t metric, bool fused, bool bf16) {
    if (bf16) return metric == kL2 ? wide_seq_kernels_of<kL2, true, true>() : wide_seq_kernels_of<kCosine, true, true>();
    if (metric == kL2) return fused ? wide_seq_kernels_of<kL2, true, false>() : wide_seq_kernels_of<kL2, false, false>();
    if (metric == kCosine) return fused ? wide_seq_kernels_of<kCosine, true, false>() : wide_seq_kernels_of<kCosine, false, false>();
    return fused ? wide_seq_kernels_of<kL1, true, false>() : wide_seq_kernels_of<kL1, false, false>();
}

// (a.g0 / a.gu are set per launch from the geometry: the argument block is taken by value)
hipError_t launch_build_select_wide_seq(const BuildArgs &a0, bool fused, bool bf16, hipStream_t s) {
    const WideSeqGeom geo = wide_seq_geom(a0.m, a0.m0, a0.layers);
    if (!geo.ok || a0.b != 1u) return hipErrorInvalidValue;
    BuildArgs a = a0;
    a.g0 = geo.sel_g0; a.gu = geo.sel_gu;
    hipLaunchKernelGGL(pick_wide_seq_kernels(a.ix.metric, fused, bf16).select, dim3(a.g0 + (a.layers - 1u) * a.gu), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_build_link_wide_seq(const BuildArgs &a0, bool fused, bool bf16, hipStream_t s) {
    const WideSeqGeom geo = wide_seq_geom(a0.m, a0.m0, a0.layers);
    if (!geo.ok || a0.b != 1u) return hipErrorInvalidValue;
    BuildArgs a = a0;
    a.g0 = geo.link_g0; a.gu = geo.link_gu;
    const WideSeqKernel k = pick_wide_seq_kernels(a.ix.metric, fused, bf16).link;
    if (geo.link_lds > 48u * 1024u) { // (103 KB; the attribute is per function AND device)
        const hipError_t e = hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)geo.link_lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k, dim3(a.g0 + (a.layers - 1u) * a.gu), dim3(1024), geo.link_lds, s, a);
    return hipGetLastError();
}

} // namespace hvx
