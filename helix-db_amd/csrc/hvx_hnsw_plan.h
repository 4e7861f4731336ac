// hvx_hnsw_plan.h -- host only: WHICH build of the one-wavefront-per-query HNSW kernel (hvx_hnsw_wave.h) or of its owner / gatherer
// sibling (hvx_hnsw_pair.h) a launch runs, and with what geometry.  plan_wave() is the one place that decides; hvx_hnsw.hip maps a plan
// to the translation unit that instantiates it, and launch_wave_kernel / launch_pair_kernel refuse a kernel whose template arguments
// are not the plan's.  The beam thresholds, the LDS sizes and the support predicates live here and nowhere else.
#pragma once
#include <algorithm>
#include <stddef.h>
#include <stdint.h>

#include "hvx_kernels.h"

namespace hvx {

// LDS window of the query RNG (QueryRngT, hvx_hnsw_wave.h), in words: the one-per-SIMD and the two-per-SIMD builds of the non-strict arms
constexpr uint32_t kRngWords = 1024, kRngWordsOcc2 = 256;

// Everything a launch is: the kernel, its template arguments (in the kernels' own order), and the launch geometry.
struct WavePlan {
    bool ok;   // false: no build of the kernel serves these arguments
    bool pair; // hnsw_pair_kernel<METRIC, R, NK, BF, G>, else hnsw_wave_kernel<METRIC, R, NK, BF, PROF, AD, ST, OCC, BUILD>
    uint32_t metric;
    int r;  // register beam of 64 * R entries
    int nk; // dim / 32, 0 = the GENERIC build (any dimension, metric and summation tree)
    bool bf, prof, ad, st;
    int occ; // wavefronts per SIMD the build is budgeted for (1 or 2)
    bool build;
    int g;            // pair kernel: gatherer wavefronts per query
    uint32_t threads; // per workgroup = per query
    uint32_t cap;     // slots of the LDS visited table
    size_t lds;       // dynamic LDS bytes
};

// The beam ladders.  A beam of 64 * R entries must hold need = ef + 32 entries: ef plus slack for equal-score evictions (build
// searches: max(ef_construction, 2 M) on every layer).  The RE-RUN of the queries whose slack overflowed (launch_hnsw_wave) takes a
// rung only where need <= rerun_max, i.e. never the rung its search launch ran on: slack 32 -> 224+.
struct BeamRung {
    uint32_t need_max;
    int r;
    uint32_t rerun_max;
};
// unrolled builds, narrow: strict and non-strict arms at either occupancy, the pair kernel, the unrolled build searches
constexpr BeamRung kBeamNarrow[] = {{192, 3, 0}, {384, 6, 384}};
// wide beams (round 4): the strict arm on the unrolled shapes runs register beams of 448 / 832 entries too (hvx_hnsw_wave_wide*.hip:
// ef up to 800 = the reference's restricted-path limit; search.rs:267-1067 itself has no limit, ef beyond that takes the general
// kernel); the 832-entry build is also the re-run of a 384- or 448-entry launch
constexpr BeamRung kBeamWide[] = {{448, 7, 0}, {832, 13, 832}};
// GENERIC builds (NK = 0): the non-strict arms and the build searches outside the unrolled shapes
constexpr BeamRung kBeamGeneric[] = {{192, 3, 0}, {448, 7, 192}, {832, 13, 832}};
constexpr uint32_t kBeamNarrowMax = 384, kBeamMax = 832;
constexpr uint32_t kBeamSlack = 32;

template <size_t N> inline int beam_rung(const BeamRung (&ladder)[N], uint32_t need, bool rerun) {
    for (const BeamRung &g : ladder)
        if (need <= g.need_max && (!rerun || need <= g.rerun_max)) return g.r;
    return 0;
}

// the unrolled builds (NK = dim / 32) with a beam of `need` entries; only the strict arm has the wide beams
inline bool wave_unrolled_serves(const DevIndex &ix, uint32_t need, bool strict) {
    if (ix.metric != kL2 && ix.metric != kCosine) return false;
    if (ix.fkernel != kKernelAvxFma) return false;
    if (ix.dim % 32u != 0u || ix.dim_main != ix.dim || ix.ld != ix.dim) return false;
    if (ix.dtype != HVX_F32 && ix.dtype != HVX_BF16) return false;
    const uint32_t nk = ix.dim >> 5;
    if (nk != 4 && nk != 8 && nk != 12 && nk != 16 && nk != 24 && nk != 32 && nk != 48) return false; // (12 = dim 384: round 6)
    return ix.s0 <= 64 && ix.su <= 64 && need <= (strict ? kBeamMax : kBeamNarrowMax);
}
inline bool hnsw_wave_supported(const HnswArgs &a) {
    return wave_unrolled_serves(a.ix, a.ef + kBeamSlack, !(a.adaptive || a.build_nodes || a.prof));
}
// the GENERIC builds: any dimension, metric and summation tree over f32 rows; one id per lane still bounds the neighbour rows at
// 64 ids, the register beam bounds ef at 800 (the restricted path's k limit)
inline bool wave_generic_serves(const DevIndex &ix, uint32_t need) {
    return ix.dtype == HVX_F32 && ix.s0 <= 64 && ix.su <= 64 && need <= kBeamMax;
}
inline bool hnsw_wave_adaptive_supported(const HnswArgs &a) { return hnsw_wave_supported(a) || wave_generic_serves(a.ix, a.ef + kBeamSlack); }
// the searches of a device build / insert: the beam holds max(ef_construction, 2 M) entries on every layer.  The unrolled builds
// serve L2 / cosine, the AVX+FMA tree, dim in {128,...,1536}, beams up to 352 + 32 (f32 rows; bf16 rows, one search per SIMD: builds, inserts, upserts);
// everything else over f32 rows (any dimension, Manhattan, the scalar / AVX summation trees, beams up to 800 + 32) takes the GENERIC
// build of the same kernel
inline uint32_t wave_build_need(uint32_t ef_layer0, uint32_t ef_upper) { return std::max(ef_layer0, ef_upper) + kBeamSlack; }
inline bool hnsw_wave_build_supported(const DevIndex &ix, uint32_t ef_layer0, uint32_t ef_upper) {
    const uint32_t need = wave_build_need(ef_layer0, ef_upper);
    return wave_unrolled_serves(ix, need, false) || wave_generic_serves(ix, need);
}

inline WavePlan plan_wave(const HnswArgs &a) {
    WavePlan p{};
    const DevIndex &ix = a.ix;
    const bool build = a.build_nodes != nullptr, ad = a.adaptive != 0, bf = ix.dtype == HVX_BF16;
    const bool rerun = a.only_flagged && !build; // (a build search has no re-run)
    const uint32_t need = build ? wave_build_need(a.ef, a.build_ef_upper) : a.ef + kBeamSlack;
    // GENERIC: the non-strict arms and the build searches outside the unrolled shapes (one query per SIMD)
    const bool generic = !wave_unrolled_serves(ix, need, !(ad || build || a.prof));
    if (generic && !((ad || build) && wave_generic_serves(ix, need))) return p;
    if (build && (ad || (bf && !a.queries))) return p; // (a bf16 image's build search reads the node's rounded vector as an f32 query)
    // the 448 / 832-entry register beams (hvx_hnsw_wave_wide*.hip): strict searches with ef 353..800, and the re-run of a 384-entry beam
    const bool wide = !ad && !build && !a.prof && (need > kBeamNarrowMax || (rerun && need > kBeamNarrow[0].need_max));

    // visited hash: 64 slots per beam entry (load factor ~0.15-0.3 at the measured ~10 distance evaluations
    // per expansion); the kernel spills to the exact HBM bitmap beyond 3/4 full
    uint32_t log2cap = 11;
    while ((1u << log2cap) < 64u * a.ef && log2cap < 15) ++log2cap;
    const bool big_table = generic && !build; // the GENERIC builds of the non-strict arms
    if (big_table && log2cap > 14) log2cap = 14; // 64 KiB table (two workgroups per CU); larger visited sets spill to the bitmap
    // Unrolled builds: 8 192 slots (32 KiB) whatever the beam width -- FOUR wavefronts per CU, one per SIMD.  (Rounds 1-3 sized the
    // table at 64 slots per beam entry: 64 KiB from ef = 129, 128 KiB from ef = 257, i.e. two / one wavefronts per CU, which is
    // where the ef sweep lost its throughput; a search visits ~10 rows per expansion, ~14 slots per beam entry at 3/4 load.)  A
    // query that visits more than 6 144 rows continues on the exact HBM bitmap.  Build searches (ef_construction ~200), the GENERIC
    // ones included: the same, to keep four workgroups per CU
    if (!big_table && log2cap > 13) log2cap = 13;
    const bool forced = a.log2cap >= 7 && a.log2cap <= 15; // HVX_OPT_WAVE_LOG2CAP: a tiny table exercises the spill path
    if (forced) log2cap = a.log2cap;
    // 160 KiB / 4: exactly four resident wavefronts per CU, one per SIMD, each with the SIMD's whole register file.
    // occ = 2 (a.occupancy): eight per CU, two per SIMD -- the table shrinks until query + frontier + table fit 20 KiB
    // (the wide beams have two-per-SIMD builds too; the one for bf16 rows at dim 1536 spills ~200 registers: it stays one per SIMD)
    // Round 5: the non-strict arms (the production default, SearchParams::new(k): access/search/storage.rs:140-141) have two-per-SIMD builds
    // as well -- f32 and bf16 rows, the unrolled shapes; their RNG window shrinks to 256 words so that the visited table keeps its size.
    p.occ = (a.occupancy == 2 && !generic && !a.prof && !(wide && bf && (ix.dim >> 5) == 48u)) ? 2 : 1;
    size_t fixed = 512 + (size_t)ix.ld * 4 + (ad ? (p.occ == 2 ? kRngWordsOcc2 : kRngWords) * 4 : 0);
    p.cap = 1u << log2cap;
    if (p.occ == 2) {
        // the table takes what the 20 KiB of a half-SIMD wavefront leave (any multiple of 64 slots: the hash maps onto [0, cap) by a
        // multiply-high, hvx_hnsw_wave.h) -- 4 224 slots at dim 768, 3 456 at dim 1536 where a power of two allowed 4 096 / 2 048
        const size_t room = 20 * 1024 > fixed ? (20 * 1024 - fixed) / 4 / 64 * 64 : 0;
        if (!(forced && p.cap <= room)) {
            p.cap = (uint32_t)std::min<size_t>(room, 8192);
            if (p.cap < 512) { // no room for a useful table next to the query: one query per SIMD
                p.occ = 1;
                p.cap = 1u << log2cap;
                fixed = 512 + (size_t)ix.ld * 4 + (ad ? kRngWords * 4 : 0);
            }
        }
    }
    p.lds = std::max((size_t)4 * p.cap + fixed, (size_t)(p.occ == 2 ? 20 : 40) * 1024);
    p.metric = ix.metric;
    p.nk = generic ? 0 : (int)(ix.dim >> 5);
    p.bf = bf;
    p.ad = ad;
    p.st = ad ? a.ad.stats != nullptr : true; // non-strict arms: with the per-query SearchStats of the filter / sampling stages when
                                              // the caller asked for them, else the diagnostics-free build
    p.build = build;
    p.threads = 64;
    if (build) {
        if (bf && p.occ != 1) return p; // one-node inserts into bf16 images: one per SIMD only
        p.r = generic ? beam_rung(kBeamGeneric, need, false) : beam_rung(kBeamNarrow, need, false);
    } else if (a.pair && !ad && !a.prof && !rerun && !wide && p.occ == 1) {
        // one batch in flight: two wavefronts per query (owner + gatherer); the strict arm, beams of 192 / 384 entries
        p.pair = true;
        p.r = beam_rung(kBeamNarrow, need, false);
        // three gatherers where a row is <= 24 pieces per lane, else one
        p.g = (bf ? p.nk / 2 : p.nk) <= 24 && a.pair_gatherers != 1u ? 3 : 1;
        p.threads = 64u * (1u + (uint32_t)p.g);
        p.lds = std::max((size_t)4 * p.cap + 528 + (size_t)ix.ld * 4, (size_t)40 * 1024);
    } else if (wide) {
        p.r = beam_rung(kBeamWide, need, rerun);
    } else if (generic || p.occ == 2 || !a.prof) {
        p.r = generic ? beam_rung(kBeamGeneric, need, rerun) : beam_rung(kBeamNarrow, need, rerun);
    } else {
        // the phase-timing build (kernel tuning): R 3, dim 768, f32 rows; the non-strict arms only in tuning builds of the library
        p.prof = true;
        p.r = 3;
        bool prof_ad = false;
#ifdef HVX_TUNING // the non-strict arms, phase-timed (slot 6 = decision epoch + candidate selection)
        prof_ad = ad;
#endif
        p.ad = prof_ad;
        p.st = !prof_ad;
        if ((!prof_ad && ix.metric != kL2) || bf || p.nk != 24 || need > kBeamNarrow[0].need_max) return p;
    }
    p.ok = p.r != 0;
    return p;
}

// The re-run launch of the queries whose beam overflowed on equal scores (launch_hnsw_wave): the same search with only_flagged set,
// which takes the next beam size of its ladder.  Returns false when no re-run follows: nobody would read the flags or empty the
// list, or no wider instantiation exists.
// The re-run's workgroups leave at once (unless duplicates overflowed a beam): give them the build that fits NEXT TO whatever is
// resident -- two per SIMD, 20 KiB of LDS -- wherever it exists (the unrolled builds).  A one-per-SIMD re-run needs a SIMD
// with nothing else on it: behind the batches of other lanes that is a wait of 0.2 ms (round 3), behind the batcher's lanes
// running the four-wavefront pair kernel it starved for tens of milliseconds (gpurun r04c: p99 47 ms).
// The re-run keeps the launch's register budget where the wider build exists for it (two queries per SIMD: its few wavefronts
// fit next to the resident batches of the other lanes); the 832-entry beams are one-per-SIMD builds
inline bool plan_wave_rerun(const HnswArgs &a, const WavePlan &p, bool ad_one_per_simd /* HVX_AD_RERUN_OCC1, tuning builds */, HnswArgs *r, WavePlan *rp) {
    *r = a;
    r->only_flagged = 1;
    if (!a.adaptive || (hnsw_wave_supported(a) && !ad_one_per_simd)) r->occupancy = 2;
    *rp = plan_wave(*r);
    return !a.prof && !a.build_nodes && a.tie_flags && a.rerun_ctl && p.ok && rp->ok && rp->r > p.r;
}

} // namespace hvx
