// wave_plan_probe.cpp -- prints what plan_wave() / plan_wave_rerun() (helix-db_amd/csrc/hvx_hnsw_plan.h) decide for a grid of launch
// arguments: one line per input, the kernel instantiation(s) a search or build-search launch would run and their geometry.
// tests/test_wave_plan.py compares the output with tests/wave_plan_table.txt.  Host only: no device is touched.
#include <cstdio>
#include <set>
#include <string>

#include "../../helix-db_amd/csrc/hvx_hnsw_plan.h"

using namespace hvx;

static std::string launch_text(const WavePlan &p, const HnswArgs &a) {
    auto tf = [](bool v) { return v ? "true" : "false"; };
    char buf[320];
    if (p.pair)
        snprintf(buf, sizeof buf, " | void hvx::hnsw_pair_kernel<%uu, %d, %d, %s, %d>(hvx::HnswArgs, unsigned int)", p.metric, p.r, p.nk, tf(p.bf), p.g);
    else
        snprintf(buf, sizeof buf, " | void hvx::hnsw_wave_kernel<%uu, %d, %d, %s, %s, %s, %s, %d, %s>(hvx::HnswArgs, unsigned int)", p.metric, p.r, p.nk, tf(p.bf),
                 tf(p.prof), tf(p.ad), tf(p.st), p.occ, tf(p.build));
    std::string s = buf;
    snprintf(buf, sizeof buf, " threads=%u cap=%u lds=%zu ef=%u flagged=%u rerun_ctl=%d;", p.threads, p.cap, p.lds, a.ef, a.only_flagged, a.rerun_ctl ? 1 : 0);
    return s + buf;
}

// what launch_hnsw_wave does with these arguments
static std::string launches(HnswArgs a) {
    HnswArgs r;
    WavePlan rp;
    const WavePlan p = plan_wave(a);
    const bool rerun = plan_wave_rerun(a, p, false, &r, &rp);
    if (!rerun) a.rerun_ctl = nullptr;
    if (!p.ok) return "";
    return launch_text(p, a) + (rerun ? launch_text(rp, r) : "");
}

static std::set<std::string> g_seen;
static uint32_t *const P = (uint32_t *)0x1000; // "set" pointers: never dereferenced
static hvx_adaptive_stats g_stats;

static DevIndex index_of(uint32_t dt, uint32_t me, uint32_t fk, uint32_t dim, uint32_t s0) {
    DevIndex ix{};
    ix.dtype = dt; ix.metric = me; ix.fkernel = fk; ix.dim = dim; ix.ld = dim; ix.dim_main = dim & ~7u; ix.s0 = s0; ix.su = 32;
    return ix;
}

// ad: 0 strict, 1 non-strict, 2 non-strict with per-query stats
static void search(uint32_t dt, uint32_t me, uint32_t fk, uint32_t dim, uint32_t s0, int ad, uint32_t occ, uint32_t pair, uint32_t pg, uint32_t ef, uint32_t l2c,
                   int prof, int tie) {
    HnswArgs a{};
    a.ix = index_of(dt, me, fk, dim, s0);
    a.ef = ef; a.k = 10; a.adaptive = ad ? 1 : 0; a.ad.stats = ad == 2 ? &g_stats : nullptr;
    a.occupancy = occ; a.pair = pair; a.pair_gatherers = pg; a.log2cap = l2c; a.prof = prof ? (unsigned long long *)P : nullptr;
    if (tie) { a.tie_flags = P; a.rerun_list = P; a.rerun_ctl = P; }
    const bool sup = a.adaptive ? hnsw_wave_adaptive_supported(a) : hnsw_wave_supported(a);
    std::string out = sup ? launches(a) : " none";
    if (out.empty()) out = " | ERROR";
    char key[256];
    snprintf(key, sizeof key, "S dt=%u me=%u fk=%u dim=%u s0=%u ad=%d occ=%u pair=%u pg=%u ef=%u l2c=%u prof=%d tie=%d sup=%d/%d ->", dt, me, fk, dim, s0, ad, occ, pair, pg,
             ef, l2c, prof, tie, (int)hnsw_wave_supported(a), (int)hnsw_wave_adaptive_supported(a));
    if (g_seen.insert(key).second) printf("%s%s\n", key, out.c_str());
}

static void build(uint32_t dt, uint32_t me, uint32_t fk, uint32_t dim, uint32_t s0, uint32_t occ, uint32_t ef, uint32_t efu, uint32_t l2c, int q) {
    HnswArgs a{};
    a.ix = index_of(dt, me, fk, dim, s0);
    a.ef = ef; a.build_ef_upper = efu; a.k = 64; a.build_nodes = P; a.occupancy = occ; a.log2cap = l2c; a.tie_flags = P;
    a.queries = q ? (const float *)P : nullptr;
    std::string out = hnsw_wave_build_supported(a.ix, ef, efu) ? launches(a) : "";
    if (out.empty()) out = " none";
    char key[256];
    snprintf(key, sizeof key, "B dt=%u me=%u fk=%u dim=%u s0=%u occ=%u ef=%u efu=%u l2c=%u q=%d ->", dt, me, fk, dim, s0, occ, ef, efu, l2c, q);
    if (g_seen.insert(key).second) printf("%s%s\n", key, out.c_str());
}

int main() {
    const uint32_t F32 = HVX_F32, BF16 = HVX_BF16, FP8 = HVX_FP8_E4M3, FMA = kKernelAvxFma, AVX = kKernelAvx;
    const uint32_t efs[] = {1, 160, 161, 352, 353, 416, 417, 800, 801}; // both sides of every beam threshold (ef + 32 vs 192 / 384 / 448 / 832)
    // every rung of the narrow, wide and generic ladders, with and without the re-run: strict (one / two per SIMD, pair), non-strict
    // (one / two per SIMD, with stats), generic non-strict (dim 100)
    for (uint32_t ef : efs)
        for (int tie = 0; tie < 2; ++tie) {
            search(F32, kL2, FMA, 768, 32, 0, 1, 0, 0, ef, 0, 0, tie);
            search(F32, kL2, FMA, 768, 32, 0, 1, 1, 0, ef, 0, 0, tie);
            search(F32, kL2, FMA, 768, 32, 0, 2, 0, 0, ef, 0, 0, tie);
            search(F32, kL2, FMA, 768, 32, 1, 1, 0, 0, ef, 0, 0, tie);
            search(F32, kL2, FMA, 768, 32, 1, 2, 0, 0, ef, 0, 0, tie);
            search(F32, kL2, FMA, 768, 32, 2, 1, 0, 0, ef, 0, 0, tie);
            search(F32, kL2, FMA, 100, 32, 1, 1, 0, 0, ef, 0, 0, tie);
        }
    // the other translation units of each family: metric x dtype, and the remaining unrolled dimensions
    const uint32_t some_efs[] = {160, 353, 800};
    for (uint32_t dt : {F32, BF16})
        for (uint32_t me : {(uint32_t)kL2, (uint32_t)kCosine})
            for (uint32_t ef : some_efs)
                for (int ad = 0; ad < 3; ad += 1)
                    for (uint32_t occ = 1; occ <= 2; ++occ) {
                        search(dt, me, FMA, 128, 32, ad, occ, 0, 0, ef, 0, 0, 1);
                        search(dt, me, FMA, 1536, 32, ad, occ, 0, 0, ef, 0, 0, 1); // bf16, wide, two per SIMD asked: stays one per SIMD
                    }
    for (uint32_t dim : {128u, 384u, 768u, 1536u}) // pair kernel: three gatherers up to 24 pieces per lane, else one; one on request
        for (uint32_t dt : {F32, BF16})
            for (uint32_t me : {(uint32_t)kL2, (uint32_t)kCosine})
                for (uint32_t pg = 0; pg < 2; ++pg) search(dt, me, FMA, dim, 64, 0, 1, 1, pg, dim == 384 ? 352 : 160, 0, 0, 0);
    search(F32, kL2, FMA, 768, 32, 0, 2, 1, 0, 160, 0, 0, 1); // pair asked on a two-per-SIMD handle
    for (uint32_t me : {(uint32_t)kL2, (uint32_t)kCosine, (uint32_t)kL1}) // generic: every metric, the AVX tree on an unrolled dimension, with stats
        for (int ad = 1; ad < 3; ++ad) {
            search(F32, me, FMA, 776, 64, ad, 2, 0, 0, 160, 0, 0, 1);
            search(F32, me, AVX, 768, 32, ad, 1, 0, 0, 417, 0, 0, 1);
        }
    // the forced table size (tiny: spill path; 15: does not fit two per SIMD) and the automatic sizes
    for (uint32_t l2c : {0u, 7u, 15u})
        for (uint32_t occ = 1; occ <= 2; ++occ)
            for (int ad = 0; ad < 2; ++ad) {
                search(F32, kL2, FMA, 768, 32, ad, occ, 0, 0, 352, l2c, 0, 0);
                search(BF16, kCosine, FMA, 1536, 32, ad, occ, 0, 0, 1, l2c, 0, 0);
                search(F32, kCosine, FMA, 100, 32, 1, occ, 0, 0, 800, l2c, 0, 0);
            }
    // phase-timing build
    for (int ad = 0; ad < 2; ++ad)
        for (uint32_t me : {(uint32_t)kL2, (uint32_t)kCosine}) {
            search(F32, me, FMA, 768, 32, ad, 1, 0, 0, 160, 0, 1, 1);
            search(F32, me, FMA, 768, 32, ad, 2, 1, 0, 161, 0, 1, 1);
            search(F32, me, FMA, 128, 32, ad, 1, 0, 0, 160, 0, 1, 0);
            search(BF16, me, FMA, 768, 32, ad, 1, 0, 0, 160, 0, 1, 0);
        }
    // unsupported inputs
    search(FP8, kL2, FMA, 768, 32, 0, 1, 0, 0, 160, 0, 0, 0);
    search(FP8, kL2, FMA, 768, 32, 1, 1, 0, 0, 160, 0, 0, 0);
    search(F32, kL2, FMA, 768, 65, 0, 1, 0, 0, 160, 0, 0, 0);
    search(F32, kL2, FMA, 768, 65, 1, 1, 0, 0, 160, 0, 0, 0);
    search(F32, kL1, FMA, 768, 32, 0, 1, 0, 0, 160, 0, 0, 0);
    search(F32, kL2, AVX, 768, 32, 0, 1, 0, 0, 160, 0, 0, 0);
    search(F32, kL2, FMA, 100, 32, 0, 1, 0, 0, 160, 0, 0, 0);
    search(BF16, kL2, FMA, 100, 32, 1, 1, 0, 0, 160, 0, 0, 0);
    search(BF16, kL2, FMA, 768, 32, 1, 1, 0, 0, 353, 0, 0, 0);
    // build searches: unrolled 3 / 6, generic 3 / 7 / 13, two per SIMD, bf16 images (with and without the node's f32 vector)
    for (uint32_t efu : {64u, 200u, 400u})
        for (uint32_t ef : {100u, 200u, 353u, 800u})
            for (uint32_t occ = 1; occ <= 2; ++occ) {
                build(F32, kL2, FMA, 768, 32, occ, ef, efu, 0, 0);
                build(F32, kCosine, FMA, 100, 32, occ, ef, efu, 0, 0);
                build(BF16, kCosine, FMA, 768, 32, occ, ef, efu, 0, 1);
            }
    build(F32, kCosine, FMA, 1536, 64, 2, 200, 64, 0, 0);
    build(F32, kL1, FMA, 768, 32, 1, 200, 64, 0, 0);
    build(F32, kL2, AVX, 768, 32, 2, 100, 64, 7, 0);
    build(F32, kL2, FMA, 768, 32, 2, 100, 64, 7, 0);
    build(F32, kL2, FMA, 768, 32, 1, 100, 64, 15, 0);
    build(BF16, kL2, FMA, 128, 32, 1, 100, 64, 0, 0);
    build(BF16, kL2, FMA, 128, 32, 1, 100, 64, 0, 1);
    build(BF16, kL2, FMA, 100, 32, 1, 100, 64, 0, 1);
    build(FP8, kL2, FMA, 768, 32, 1, 100, 64, 0, 1);
    build(F32, kL2, FMA, 768, 65, 1, 100, 64, 0, 0);
    build(F32, kL2, FMA, 100, 65, 1, 100, 64, 0, 0);
    return 0;
}
