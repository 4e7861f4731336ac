// hvx_restricted_direct.h -- the kernel of the one-launch restricted exact scan (hvx_restricted_exact.hip has the story) and its launch
// tables, shared by the translation units that instantiate it: hvx_restricted_exact.hip builds the k <= 64 kernels (one register pair per
// lane: TopList), hvx_restricted_wide4.hip / hvx_restricted_wide13.hip the builds whose result list spans 4 / 13 registers per lane
// (TopListWide: k <= 256 / k <= 800 = MAX_RESTRICTED_RESULT_COUNT, restricted.rs:55).  Everything here has internal linkage; the wide
// units hand their launch function to the dispatch through restricted_direct_launch_wide4 / _wide13 (hvx_host.h).
#pragma once
#include <hip/hip_runtime.h>

#include "hvx_toplist.h"
#include "hvx_handoff.h"
#include "hvx_host.h"

namespace {

using namespace hvx;

typedef float f2 __attribute__((ext_vector_type(2)));

struct DirectArgs {
    DevIndex ix;
    const float *queries;     // [b][dim] (device copy written by stage_validate_kernel)
    const uint32_t *qstatus;  // [b]
    const float *qhdr;        // [b]
    const uint32_t *rows;     // shared candidate set: internal rows (unique; any order) ...
    uint32_t n_rows;
    const uint32_t *n_rows_dev; // ... whose number a kernel earlier on the stream left on the device (then n_rows = the host's bound, the grid's size)
    const uint64_t *ext_ids;  // ... or per-query sets: external ids, query q owns [offsets[q], offsets[q + 1]) ...
    const uint64_t *offsets;
    const uint32_t *lens;     // ... or, with offsets == NULL, [q * ext_stride, + lens[q]) (the batching operator's fixed slots)
    uint32_t ext_stride;
    uint32_t contiguous;
    uint32_t b, k, k_stride;
    uint32_t chunk, slices;   // candidate positions per slice (a multiple of 64), slices per query
    float *part_sc;           // [b][slices][k] every slice's k smallest, padded with (+inf, kSentinel)
    uint32_t *part_row;
    uint32_t *bad;            // [b] a score failed Candidate::try_new (zero between launches)
    uint32_t *done;           // [query tiles] workgroups of the tile that have delivered (zero between launches)
    uint64_t *out_ids;        // [b][k_stride]
    float *out_scores;
    uint32_t *out_counts, *out_status;
};

// external node id -> internal row (ids ascending), kSentinel when the id holds no (live) vector
__device__ __forceinline__ uint32_t row_of_id(const DevIndex &ix, uint64_t id, bool contiguous) {
    uint32_t row;
    if (contiguous) {
        const uint64_t first = ix.ids[0];
        if (!(id >= first && id - first < ix.n)) return kSentinel;
        row = (uint32_t)(id - first);
    } else {
        uint32_t lo = 0, hi = ix.n;
        while (lo < hi) {
            const uint32_t mid = lo + ((hi - lo) >> 1);
            if (ix.ids[mid] < id) lo = mid + 1;
            else hi = mid;
        }
        if (!(lo < ix.n && ix.ids[lo] == id)) return kSentinel;
        row = lo;
    }
    if (row_dead(ix, row)) return kSentinel;
    return row;
}

struct Acc { f2 lo, hi; }; // a float4 accumulator as two packed halves
constexpr int load_group(int nl) {
    for (int g = 8; g > 1; --g)
        if (nl % g == 0) return g;
    return 1;
}
// (the slices' lists, the flags and the counters cross workgroups that may sit on different XCDs, one L2 each: st_agent / ld_agent)

template <uint32_t METRIC> __device__ __forceinline__ void fma_chunk_pk(Acc &acc, const float4 qq, const float4 xv) {
    const f2 ql = {qq.x, qq.y}, qh = {qq.z, qq.w}, xl = {xv.x, xv.y}, xh = {xv.z, xv.w};
    if (METRIC == kL2) {
        const f2 d0 = ql - xl, d1 = qh - xh;
        acc.lo = __builtin_elementwise_fma(d0, d0, acc.lo);
        acc.hi = __builtin_elementwise_fma(d1, d1, acc.hi);
    } else {
        acc.lo = __builtin_elementwise_fma(ql, xl, acc.lo);
        acc.hi = __builtin_elementwise_fma(qh, xh, acc.hi);
    }
}

// distance/cosine.rs:39-59: the f64 fallback of the cosine kernel (extreme norms only) -- out of line: it is rare, and inlined once per
// (row, query) pair it made the cosine builds several times the size of the Euclidean ones
__device__ __noinline__ float slow_half_cosine(const DevIndex &ix, const float *qv, uint32_t node) {
    if (ix.dtype == HVX_BF16) {
        const uint16_t *rb = ix.vecb + (size_t)node * ix.dim;
        return stable_half_cosine_fn(ix.dim, [&](uint32_t i) { return qv[i]; }, [&](uint32_t i) { return bf16_to_f32(rb[bf16_slot_of(i)]); });
    }
    const float *rf = ix.vec + (size_t)node * ix.ld;
    return stable_half_cosine_fn(ix.dim, [&](uint32_t i) { return qv[i]; }, [&](uint32_t i) { return rf[i]; });
}
// (the wide builds take it inline: the call's frame is scratch, which a build with up to 26 list registers per lane must not carry)
__device__ __forceinline__ float slow_half_cosine_inline(const DevIndex &ix, const float *qv, uint32_t node) {
    if (ix.dtype == HVX_BF16) {
        const uint16_t *rb = ix.vecb + (size_t)node * ix.dim;
        return stable_half_cosine_fn(ix.dim, [&](uint32_t i) { return qv[i]; }, [&](uint32_t i) { return bf16_to_f32(rb[bf16_slot_of(i)]); });
    }
    const float *rf = ix.vec + (size_t)node * ix.ld;
    return stable_half_cosine_fn(ix.dim, [&](uint32_t i) { return qv[i]; }, [&](uint32_t i) { return rf[i]; });
}


// the result list of one wavefront and query: R == 1 is TopList (k <= 64), wider lists are TopListWide<R> (k <= 64 R)
template <int R> struct DirectList { typedef TopListWide<R> type; };
template <> struct DirectList<1> { typedef TopList type; };

// NK = dim / 32 (unrolled shapes: AVX+FMA tree, dim == ld == dim_main); NK == 0: any dimension / metric / summation tree through
// group_distance (one row per group at a time).  BF: bf16 rows (interleaved layout).  EXT: per-query external id lists (TQ == 1).
// R: registers per lane of the result list (R > 1: TQ == 1).
template <uint32_t METRIC, int NK, bool BF, int TQ, bool EXT, bool FUSED, int R>
__global__ __launch_bounds__(256) void restricted_direct_kernel(DirectArgs a) {
    static_assert(R == 1 || TQ == 1, "the wide lists serve one query per tile");
    typedef typename DirectList<R>::type List;
    constexpr int P = 2;
    constexpr bool GEN = NK == 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float m_sc[TQ][4][64 * R];
    __shared__ uint32_t m_id[TQ][4][64 * R];
    __shared__ uint32_t s_last;
    const DevIndex &ix = a.ix;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 3, j = lane & 7, slot = chunk_slot(j);
    const uint32_t G = (uint32_t)(wave * 8 + grp);
    const uint32_t tile = blockIdx.y, q0 = tile * TQ, slice = blockIdx.x;
    const uint32_t ld = ix.ld;
    float *qs = reinterpret_cast<float *>(smem); // [TQ][ld]
    const float inf = __uint_as_float(0x7F800000u);

    bool qok[TQ];
    float qh[TQ];
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
        const uint32_t q = q0 + (uint32_t)t;
        qok[t] = q < a.b && a.qstatus[q] == 0u;
        qh[t] = (METRIC == kCosine && qok[t]) ? a.qhdr[q] : 0.f;
        for (uint32_t i = (uint32_t)tid; i < ld; i += 256)
            qs[(size_t)t * ld + i] = (qok[t] && i < ix.dim) ? a.queries[(size_t)q * ix.dim + i] : 0.f;
    }
    uint64_t off = 0;
    uint32_t n = a.n_rows;
    if (EXT) {
        if (a.offsets) {
            off = a.offsets[q0];
            n = (uint32_t)(a.offsets[q0 + 1] - off);
        } else {
            off = (uint64_t)q0 * a.ext_stride;
            n = a.lens[q0];
        }
    }
    __syncthreads();

    uint32_t chunk = a.chunk;
    if (!EXT && a.n_rows_dev) { // the list's real length: the slices divide IT (whole 64-row passes), not the bound the grid was sized for
        n = *a.n_rows_dev < a.n_rows ? *a.n_rows_dev : a.n_rows;
        chunk = ((n + a.slices * 64u - 1u) / (a.slices * 64u)) * 64u;
    }
    List top[TQ];
#pragma unroll
    for (int t = 0; t < TQ; ++t) top[t].init();
    uint32_t badmask = 0;
    const uint32_t lo = slice * chunk, hi = lo + chunk < n ? lo + chunk : n;
    for (uint32_t pass0 = lo; pass0 < hi; pass0 += 32u * P) {
        uint32_t nd[P];
        bool ok[P];
#pragma unroll
        for (int p = 0; p < P; ++p) {
            const uint32_t pos = pass0 + (uint32_t)p * 32u + G;
            uint32_t row = kSentinel;
            if (pos < hi) row = EXT ? row_of_id(ix, a.ext_ids[off + pos], a.contiguous != 0u) : a.rows[pos];
            ok[p] = row != kSentinel;
            nd[p] = ok[p] ? row : 0u; // (a group without a row of its own re-reads row 0: no divergence in the gather)
        }
        if (!__ballot(ok[0] || ok[1])) continue;
        float sc[P][TQ];
        if constexpr (GEN) {
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int t = 0; t < TQ; ++t) {
                    float d = 0.f;
                    if (ok[p]) { // group-uniform
                        if (BF) d = group_distance_bf16<METRIC == kL1 ? kL2 : METRIC>(ix, qs + (size_t)t * ld, qh[t], nd[p], j);
                        else d = group_distance<METRIC, FUSED>(ix, qs + (size_t)t * ld, qh[t], nd[p], j);
                    }
                    sc[p][t] = d;
                }
        } else {
            constexpr int NL = BF ? NK / 2 : NK;     // 16-byte pieces per lane and row
            constexpr int NG = load_group(NL);       // pieces requested together: the largest divisor of NL that is <= 8
            constexpr int STAGES = NL / NG;
            static_assert(NL % NG == 0, "a row is a whole number of load groups");
            float hdr[P];
            const float4 *rp[P];
#pragma unroll
            for (int p = 0; p < P; ++p) {
                hdr[p] = METRIC == kCosine ? ix.hdr[nd[p]] : 0.f;
                rp[p] = BF ? reinterpret_cast<const float4 *>(ix.vecb + (size_t)nd[p] * ix.dim) + slot
                           : reinterpret_cast<const float4 *>(ix.vec + (size_t)nd[p] * ld) + slot;
            }
            Acc acc[P][TQ];
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int t = 0; t < TQ; ++t) { acc[p][t].lo = f2{0.f, 0.f}; acc[p][t].hi = f2{0.f, 0.f}; }
            float4 xa[P][NG], xb[P][NG];
            auto request = [&](float4 (&x)[P][NG]) __attribute__((always_inline)) { // the next NG pieces of both rows; the row pointers move on
#pragma unroll
                for (int p = 0; p < P; ++p) {
#pragma unroll
                    for (int u = 0; u < NG; ++u) x[p][u] = rp[p][u * 8];
                    rp[p] += NG * 8;
                }
            };
            const uint32_t ld4 = ld >> 2;
            const float4 *qp = reinterpret_cast<const float4 *>(qs) + slot; // piece 0 of query 0; moves on with every stage consumed
            auto consume = [&](const float4 (&x)[P][NG]) __attribute__((always_inline)) {
#pragma unroll
                for (int u = 0; u < NG; ++u) {
#pragma unroll
                    for (int t = 0; t < TQ; ++t) {
                        if (!BF) {
                            const float4 qq = qp[(size_t)t * ld4 + u * 8];
#pragma unroll
                            for (int p = 0; p < P; ++p) fma_chunk_pk<METRIC>(acc[p][t], qq, x[p][u]);
                        } else { // piece u = the lane's virtual lanes of chunks 2u, 2u + 1
                            const float4 qa = qp[(size_t)t * ld4 + (2 * u) * 8], qb = qp[(size_t)t * ld4 + (2 * u + 1) * 8];
#pragma unroll
                            for (int p = 0; p < P; ++p) { // bf16 -> f32 is exact: the halfword becomes the high half of the word
                                const uint32_t w0 = __float_as_uint(x[p][u].x), w1 = __float_as_uint(x[p][u].y);
                                const uint32_t w2 = __float_as_uint(x[p][u].z), w3 = __float_as_uint(x[p][u].w);
                                fma_chunk_pk<METRIC>(acc[p][t], qa, make_float4(__uint_as_float(w0 << 16), __uint_as_float(w0 & 0xFFFF0000u),
                                                                                __uint_as_float(w1 << 16), __uint_as_float(w1 & 0xFFFF0000u)));
                                fma_chunk_pk<METRIC>(acc[p][t], qb, make_float4(__uint_as_float(w2 << 16), __uint_as_float(w2 & 0xFFFF0000u),
                                                                                __uint_as_float(w3 << 16), __uint_as_float(w3 & 0xFFFF0000u)));
                            }
                        }
                    }
                }
                qp += (BF ? 2 : 1) * NG * 8;
            };
            request(xa);
#pragma unroll 1
            for (int s = 0; s < STAGES; s += 2) { // stage s + 1 is requested before stage s is multiplied
                if (s + 1 < STAGES) request(xb);
                __builtin_amdgcn_sched_barrier(0);
                consume(xa);
                if (s + 1 < STAGES) {
                    if (s + 2 < STAGES) request(xa);
                    __builtin_amdgcn_sched_barrier(0);
                    consume(xb);
                }
            }
#pragma unroll
            for (int p = 0; p < P; ++p)
#pragma unroll
                for (int t = 0; t < TQ; ++t) {
                    float r = avx_tree_reduce(make_float4(acc[p][t].lo.x, acc[p][t].lo.y, acc[p][t].hi.x, acc[p][t].hi.y));
                    if (METRIC == kCosine) {
                        const uint32_t node = nd[p];
                        const float *qv = qs + (size_t)t * ld;
                        if constexpr (R == 1) r = cosine_finish_fn(r, qh[t], hdr[p], [&]() { return slow_half_cosine(ix, qv, node); });
                        else r = cosine_finish_fn(r, qh[t], hdr[p], [&]() { return slow_half_cosine_inline(ix, qv, node); });
                    }
                    sc[p][t] = r;
                }
        }
        // admission: Candidate::try_new per score (model.rs:21-29), then the wavefront's list
#pragma unroll
        for (int t = 0; t < TQ; ++t)
#pragma unroll
            for (int p = 0; p < P; ++p) {
                float d = sc[p][t];
                const bool live = ok[p] && qok[t];
                const bool valid = score_valid(d);
                if (live && !valid) badmask |= 1u << t;
                top[t].offer(live && valid && j == 0 && top[t].admits(d, nd[p]), d, nd[p], a.k, lane);
            }
    }

    // the workgroup's four lists of a query -> one (wavefront t mod 4), padded with (+inf, kSentinel) -> HBM
    if constexpr (R == 1) {
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
        m_sc[t][wave][lane] = top[t].sc;
        m_id[t][wave][lane] = top[t].id;
        const unsigned long long anybad = __ballot((badmask >> t) & 1u);
        if (anybad && lane == 0 && q0 + (uint32_t)t < a.b) atomicOr(&a.bad[q0 + (uint32_t)t], 1u);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < TQ; ++t) {
        if ((t & 3) != wave) continue;
        const uint32_t q = q0 + (uint32_t)t;
        if (q >= a.b) continue;
        TopList l;
        l.init();
        for (int w = 0; w < 4; ++w) {
            const float es = m_sc[t][w][lane];
            const uint32_t ei = m_id[t][w][lane];
            l.offer(ei != kSentinel, es, ei, a.k, lane);
        }
        if ((uint32_t)lane < a.k) {
            const size_t at = ((size_t)q * a.slices + slice) * a.k + (uint32_t)lane;
            st_agent(a.part_sc + at, l.sc);
            st_agent(a.part_row + at, l.id);
        }
    }
    } else {
        // R registers per lane: wavefronts 1 - 3 hand their lists over; wavefront 0 keeps its own and takes theirs in.  A list is sorted:
        // once a register of it offers nothing that is admitted, nothing behind it can be.
        if (wave != 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                m_sc[0][wave][r * 64 + lane] = top[0].sc[r];
                m_id[0][wave][r * 64 + lane] = top[0].id[r];
            }
        }
        const unsigned long long anybad = __ballot(badmask & 1u);
        if (anybad && lane == 0 && q0 < a.b) atomicOr(&a.bad[q0], 1u);
        __syncthreads();
        if (wave == 0 && q0 < a.b) {
            List &l = top[0];
            for (int w = 1; w < 4; ++w) {
#pragma unroll 1
                for (int r = 0; r < R; ++r) {
                    const float es = m_sc[0][w][r * 64 + lane];
                    const uint32_t ei = m_id[0][w][r * 64 + lane];
                    const bool take = ei != kSentinel && l.admits(es, ei);
                    if (!__ballot(take)) break;
                    l.offer(take, es, ei, a.k, lane);
                }
            }
            const size_t at0 = ((size_t)q0 * a.slices + slice) * a.k;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t e = (uint32_t)(r * 64 + lane);
                if (e < a.k) {
                    st_agent(a.part_sc + at0 + e, l.sc[r]);
                    st_agent(a.part_row + at0 + e, l.id[r]);
                }
            }
        }
    }
    // the last workgroup of the tile to get here merges the slices' lists (no device-scope fence: hvx_handoff.h)
    if (!last_workgroup(a.done, tile, a.slices, &s_last, false)) return;
    const uint32_t per_query = a.slices * a.k;
    if constexpr (R > 1) {
        // every wavefront merges the lists of slices wave, wave + 4, ...: the first fills its registers as it is, the others are read a
        // register row at a time and left at the first row that offers nothing; the four results meet in LDS and wavefront 0 finishes
        const uint32_t q = q0;
        List l;
        l.init();
        if (q < a.b) {
            const float *ps = a.part_sc + (size_t)q * per_query;
            const uint32_t *pr = a.part_row + (size_t)q * per_query;
            if ((uint32_t)wave < a.slices) {
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const uint32_t e = (uint32_t)(r * 64 + lane);
                    const bool in = e < a.k;
                    l.sc[r] = in ? ld_agent(ps + (size_t)wave * a.k + e) : inf;
                    l.id[r] = in ? ld_agent(pr + (size_t)wave * a.k + e) : kSentinel;
                }
                l.adopt(a.k);
            }
            for (uint32_t s = (uint32_t)wave + 4u; s < a.slices; s += 4u) {
                for (uint32_t e0 = 0; e0 < a.k; e0 += 64u) {
                    const uint32_t e = e0 + (uint32_t)lane;
                    const bool in = e < a.k;
                    const float es = in ? ld_agent(ps + (size_t)s * a.k + e) : inf;
                    const uint32_t ei = in ? ld_agent(pr + (size_t)s * a.k + e) : kSentinel;
                    const bool take = ei != kSentinel && l.admits(es, ei);
                    if (!__ballot(take)) break;
                    l.offer(take, es, ei, a.k, lane);
                }
            }
        }
        __syncthreads(); // (the hand-over above has been read)
        if (wave != 0) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                m_sc[0][wave][r * 64 + lane] = l.sc[r];
                m_id[0][wave][r * 64 + lane] = l.id[r];
            }
        }
        __syncthreads();
        if (wave == 0 && q < a.b) {
            for (int w = 1; w < 4; ++w) {
#pragma unroll 1
                for (int r = 0; r < R; ++r) {
                    const float es = m_sc[0][w][r * 64 + lane];
                    const uint32_t ei = m_id[0][w][r * 64 + lane];
                    const bool take = ei != kSentinel && l.admits(es, ei);
                    if (!__ballot(take)) break;
                    l.offer(take, es, ei, a.k, lane);
                }
            }
            uint32_t st = a.qstatus[q];
            if (EXT && n == 0u) st = 0u; // an empty candidate set answers with nothing BEFORE the query is validated (restricted.rs:539-541)
            uint32_t isbad = 0;
            if (lane == 0) { isbad = ld_agent(a.bad + q); if (isbad) st_agent(a.bad + q, 0u); }
            isbad = __builtin_amdgcn_readfirstlane(isbad);
            uint32_t outn = l.count < a.k ? l.count : a.k;
            if (st != 0u || isbad) outn = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t e = (uint32_t)(r * 64 + lane);
                if (e < outn) {
                    a.out_ids[(size_t)q * a.k_stride + e] = ix.ids[l.id[r]];
                    a.out_scores[(size_t)q * a.k_stride + e] = l.sc[r];
                }
            }
            if (lane == 0) {
                a.out_counts[q] = outn;
                if (a.out_status) a.out_status[q] = st != 0u ? st : (isbad ? 8u /*HVX_ERR_INVARIANT*/ : 0u);
            }
        }
    } else
    for (int t0 = 0; t0 < TQ; t0 += (TQ >= 4 ? 4 : 1)) {
        // TQ >= 4: wavefront w merges query t0 + w on its own; fewer queries: the four wavefronts split one query's lists
        const int t = TQ >= 4 ? t0 + wave : t0;
        const uint32_t q = q0 + (uint32_t)t;
        List l;
        l.init();
        if (q < a.b) {
            const float *ps = a.part_sc + (size_t)q * per_query;
            const uint32_t *pr = a.part_row + (size_t)q * per_query;
            const uint32_t share = TQ >= 4 ? per_query : (per_query + 3u) / 4u;
            const uint32_t e0 = TQ >= 4 ? 0u : (uint32_t)wave * share, e1 = e0 + share < per_query ? e0 + share : per_query;
            for (uint32_t e = e0; e < e1; e += 256u) { // four coalesced requests in flight
                float es[4];
                uint32_t ei[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t i = e + (uint32_t)u * 64u + (uint32_t)lane;
                    const bool in = i < e1;
                    es[u] = in ? ld_agent(ps + i) : inf;
                    ei[u] = in ? ld_agent(pr + i) : kSentinel;
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) l.offer(ei[u] != kSentinel && l.admits(es[u], ei[u]), es[u], ei[u], a.k, lane);
            }
        }
        if (TQ < 4) { // the four partial merges of the one query meet in LDS (wavefront 0 finishes)
            __syncthreads();
            m_sc[0][wave][lane] = l.sc;
            m_id[0][wave][lane] = l.id;
            __syncthreads();
            if (wave != 0) continue;
            l.init();
            for (int w = 0; w < 4; ++w) {
                const float es = m_sc[0][w][lane];
                const uint32_t ei = m_id[0][w][lane];
                l.offer(ei != kSentinel, es, ei, a.k, lane);
            }
        }
        if (q >= a.b) continue;
        // results (restricted.rs:820-835): the k smallest, sorted; a rejected query keeps its status, an invalid score is an invariant error
        uint32_t st = a.qstatus[q];
        if (EXT && n == 0u) st = 0u; // an empty candidate set answers with nothing BEFORE the query is validated (restricted.rs:539-541)
        uint32_t isbad = 0;
        if (lane == 0) { isbad = ld_agent(a.bad + q); if (isbad) st_agent(a.bad + q, 0u); }
        isbad = __builtin_amdgcn_readfirstlane(isbad);
        uint32_t outn = l.count < a.k ? l.count : a.k;
        if (st != 0u || isbad) outn = 0;
        if ((uint32_t)lane < outn) {
            a.out_ids[(size_t)q * a.k_stride + (uint32_t)lane] = ix.ids[l.id];
            a.out_scores[(size_t)q * a.k_stride + (uint32_t)lane] = l.sc;
        }
        if (lane == 0) {
            a.out_counts[q] = outn;
            if (a.out_status) a.out_status[q] = st != 0u ? st : (isbad ? 8u /*HVX_ERR_INVARIANT*/ : 0u);
        }
    }
    if (tid == 0) st_agent(a.done + tile, 0u); // (the next launch starts from zero)
}

// static_lds: what the kernel declares itself beside the `lds` bytes of query rows (the wide builds' hand-over: 8 - 26 KiB)
template <typename K> hipError_t launch_direct_kernel(K kern, const DirectArgs &a, uint32_t tiles, size_t lds, hipStream_t s, size_t static_lds = 0) {
    if (lds + static_lds > 48 * 1024) { // (a workgroup above 48 KiB in all asks for it)
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(a.slices, tiles), dim3(256), lds, s, a);
    return hipGetLastError();
}

// Launch table of one wide translation unit.  Every shape has the any-shape build (NK = 0: all metrics, all five summation trees, f32
// and bf16 rows); the unrolled builds are those of the two dimensions the prefiltered branch is measured at (768 and 1536: NK 24 and 48).
template <uint32_t METRIC, int NK, bool BF, bool FUSED, int R> hipError_t launch_wide_q(const DirectArgs &a, bool ext, hipStream_t s) {
    const size_t row = (size_t)a.ix.ld * 4;
    constexpr size_t hand_over = (size_t)R * 2048u + 64u;
    if (ext) return launch_direct_kernel(restricted_direct_kernel<METRIC, NK, BF, 1, true, FUSED, R>, a, a.b, row, s, hand_over);
    return launch_direct_kernel(restricted_direct_kernel<METRIC, NK, BF, 1, false, FUSED, R>, a, a.b, row, s, hand_over);
}
template <uint32_t METRIC, bool BF, int R> hipError_t launch_wide_nk(const DirectArgs &a, bool ext, bool unrolled, hipStream_t s) {
    if constexpr (METRIC != kL1) {
        if (unrolled && (a.ix.dim >> 5) == 24u) return launch_wide_q<METRIC, 24, BF, true, R>(a, ext, s);
        if (unrolled && (a.ix.dim >> 5) == 48u) return launch_wide_q<METRIC, 48, BF, true, R>(a, ext, s);
    }
    if (BF) return launch_wide_q<METRIC, 0, BF, true, R>(a, ext, s);
    return kernel_fused(a.ix.fkernel) ? launch_wide_q<METRIC, 0, false, true, R>(a, ext, s) : launch_wide_q<METRIC, 0, false, false, R>(a, ext, s);
}
// `args`: the DirectArgs of the launch (the type has internal linkage: it crosses translation units as a pointer)
template <int R> hipError_t launch_wide(const void *args, bool ext, bool unrolled, hipStream_t s) {
    const DirectArgs &a = *static_cast<const DirectArgs *>(args);
    const bool bf = a.ix.dtype == HVX_BF16;
    switch (a.ix.metric) {
    case kCosine: return bf ? launch_wide_nk<kCosine, true, R>(a, ext, unrolled, s) : launch_wide_nk<kCosine, false, R>(a, ext, unrolled, s);
    case kL2: return bf ? launch_wide_nk<kL2, true, R>(a, ext, unrolled, s) : launch_wide_nk<kL2, false, R>(a, ext, unrolled, s);
    default: return launch_wide_nk<kL1, false, R>(a, ext, false, s);
    }
}

} // namespace
