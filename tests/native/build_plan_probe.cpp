// build_plan_probe.cpp -- prints what helix-db_amd/csrc/hvx_build_plan.h decides for a grid of write calls, one line per input:
//   W  plan_write_batch: the select and link steps of a batch with their grids, workgroup sizes, LDS bytes and g0 / gu, serial, the build
//      search's occupancy and the HVX_WRITE_* bits -- or the refusal of the image (as insert_range asks for it)
//   D  write_degrees + write_refusal with every check asked (as hvx_index_insert_batch does)
//   G  link_geom / wide_link_geom (hvx_index_link_rows)
//   B  write_batch_size
//   S  write_scratch
// tests/test_build_plan.py compares the output with tests/build_plan_table.txt.  Host only: no device is touched.  `full` as the first
// argument walks the whole grid the table was recorded over instead of the committed subset.
#include <cstdio>
#include <cstring>
#include <set>
#include <string>

#include "../../helix-db_amd/csrc/hvx_build_plan.h"

using namespace hvx;

struct Image { uint32_t dt, me, fk, dim, ld, m, m0, s0, su; };
struct Call { uint32_t link_mode, mode, max_batch, divisor, efc; };

static DevIndex index_of(const Image &im) {
    DevIndex d{};
    d.dtype = im.dt; d.metric = im.me; d.fkernel = im.fk; d.dim = im.dim; d.ld = im.ld; d.dim_main = kernel_dim_main(im.fk, im.dim); d.s0 = im.s0; d.su = im.su;
    return d;
}
static hvx_index_desc desc_of(const Image &im) {
    hvx_index_desc desc{};
    desc.m = im.m; desc.m0 = im.m0;
    return desc;
}
static hvx_build_params params_of(const Call &c) {
    hvx_build_params p{};
    p.link_mode = c.link_mode; p.sequential = c.mode; p.max_batch = c.max_batch; p.batch_divisor = c.divisor; p.ef_construction = c.efc;
    return p;
}

// ---- the decisions ----
static const char *select_name(SelectStep s) {
    switch (s) {
    case SelectStep::narrow_wave: return "narrow_wave";
    case SelectStep::narrow_eager: return "narrow_eager";
    case SelectStep::wide_wave: return "wide_wave";
    default: return "wide_eager";
    }
}
static const char *link_name(LinkStep s) {
    switch (s) {
    case LinkStep::none: return "none";
    case LinkStep::narrow_wave: return "narrow_wave";
    case LinkStep::narrow_wg: return "narrow_wg";
    case LinkStep::wide_wave: return "wide_wave";
    default: return "wide_wg";
    }
}
static std::string geom_text(const StepGeom &g) {
    char buf[128];
    snprintf(buf, sizeof buf, "grid=%ux%u threads=%u lds=%zu g0=%u gu=%u", g.gx, g.gy, g.threads, g.lds, g.g0, g.gu);
    return buf;
}
static std::string decide_batch(const Image &im, const Call &c, uint32_t bsz, bool promotes, uint32_t layers) {
    const WriteCtx ctx = write_ctx(index_of(im), desc_of(im), params_of(c), 2048u, layers);
    const WriteRefusal r = write_refusal(ctx.g, im.s0, im.su, kRefuseDegrees | (ctx.g.wide ? kRefuseRowsNarrow | kRefuseRowsOver64 : 0u));
    if (r) return r == kRefuseDegrees ? "refused: degrees" : "refused: rows";
    const WriteBatchPlan p = plan_write_batch(ctx, bsz, promotes, layers);
    char tail[96];
    snprintf(tail, sizeof tail, " | serial=%d occupancy=%d path=0x%x", (int)p.serial, p.occupancy, p.path);
    return std::string("select=") + select_name(p.select) + " " + geom_text(p.sel) + " | link=" + link_name(p.link) + " " + geom_text(p.lnk) + tail;
}
static std::string decide_degrees(const Image &im, uint32_t efc) {
    hvx_build_params p{};
    p.ef_construction = efc;
    const WriteDegrees g = write_degrees(desc_of(im), &p);
    char buf[160];
    snprintf(buf, sizeof buf, "m=%u m0=%u efc=%u ef0=%u efu=%u wide=%d kc=%u selw=%u refusal=%u", g.m, g.m0, g.efc, g.ef0, g.efu, (int)g.wide, g.kc, g.selw,
             (uint32_t)write_refusal(g, im.s0, im.su, kRefuseDegrees | kRefuseRowsNarrow | kRefuseRowsOver64 | kRefuseEf));
    return buf;
}
static std::string decide_geom(const Image &im) {
    const WriteDegrees g = write_degrees(desc_of(im), nullptr);
    const DevIndex d = index_of(im);
    const LinkGeom n = link_geom(d, g.m, g.m0), w = g.wide ? wide_link_geom(d, g.m, g.m0) : LinkGeom{};
    char buf[200];
    snprintf(buf, sizeof buf, "narrow ncmax=%u ck=%u ldp=%u lds=%zu ok=%d | wide ncmax=%u ck=%u ldp=%u lds=%zu ok=%d", n.ncmax, n.link_ck, n.ldp, n.lds, (int)n.ok, w.ncmax,
             w.link_ck, w.ldp, w.lds, (int)w.ok);
    return buf;
}
// the node at position `promoter` (if below `end`) rises above the top layer
static std::string decide_size(const Image &im, const Call &c, uint64_t done, uint64_t end, bool promotes, uint64_t promoter) {
    const WriteCtx ctx = write_ctx(index_of(im), desc_of(im), params_of(c), 1024u, 1u);
    char buf[64];
    snprintf(buf, sizeof buf, "bsz=%u", write_batch_size(ctx, done, end, promotes, [&](uint64_t pos) { return pos == promoter; }));
    return buf;
}
static std::string decide_scratch(const Image &im, const Call &c, uint64_t count, uint32_t layers_max, bool own_bq) {
    const WriteCtx ctx = write_ctx(index_of(im), desc_of(im), params_of(c), 1024u, layers_max);
    const WriteScratch w = write_scratch(ctx, count, layers_max, im.dim, own_bq);
    char buf[320];
    snprintf(buf, sizeof buf, "tick=%zu iota=%zu cids=%zu csc=%zu cnt=%zu selcnt=%zu sel=%zu status=%zu err=%zu gdm=%zu bq=%zu has_bq=%d need=%zu sz=%zu/%zu/%zu", w.tick, w.iota,
             w.cids, w.csc, w.cnt, w.selcnt, w.sel, w.status, w.err, w.gdm, w.bq, (int)w.has_bq, w.need, w.sz_cids, w.sz_cnt, w.sz_sel);
    return buf;
}

// ---- the grid ----
static std::string image_text(const Image &im) {
    char buf[160];
    snprintf(buf, sizeof buf, "dt=%u me=%u fk=%u dim=%u ld=%u m=%u m0=%u s0=%u su=%u", im.dt, im.me, im.fk, im.dim, im.ld, im.m, im.m0, im.s0, im.su);
    return buf;
}
static std::set<std::string> g_seen;
static void emit(const std::string &key, const std::string &out) {
    if (g_seen.insert(key).second) printf("%s -> %s\n", key.c_str(), out.c_str());
}
static void batch(const Image &im, uint32_t link_mode, uint32_t mode, uint32_t bsz, int promotes, uint32_t layers) {
    const Call c{link_mode, mode, 0u, 0u, 0u};
    char k[96];
    snprintf(k, sizeof k, " lm=%u mode=%u bsz=%u promotes=%d layers=%u", link_mode, mode, bsz, promotes, layers);
    emit("W " + image_text(im) + k, decide_batch(im, c, bsz, promotes != 0, layers));
}
static void degrees(const Image &im, uint32_t efc) {
    char k[32];
    snprintf(k, sizeof k, " efc=%u", efc);
    emit("D " + image_text(im) + k, decide_degrees(im, efc));
}
static void geom(const Image &im) { emit("G " + image_text(im), decide_geom(im)); }
static void size(const Image &im, const Call &c, uint64_t done, uint64_t end, int promotes, uint64_t promoter) {
    char k[160];
    snprintf(k, sizeof k, " mode=%u max_batch=%u divisor=%u done=%llu end=%llu promotes=%d promoter=%llu", c.mode, c.max_batch, c.divisor, (unsigned long long)done,
             (unsigned long long)end, promotes, (unsigned long long)promoter);
    emit("B " + image_text(im) + k, decide_size(im, c, done, end, promotes != 0, promoter));
}
static void scratch(const Image &im, const Call &c, uint64_t count, uint32_t layers_max, int own_bq) {
    char k[128];
    snprintf(k, sizeof k, " lm=%u max_batch=%u count=%llu layers_max=%u own_bq=%d", c.link_mode, c.max_batch, (unsigned long long)count, layers_max, own_bq);
    emit("S " + image_text(im) + k, decide_scratch(im, c, count, layers_max, own_bq != 0));
}

static const uint32_t F32 = HVX_F32, BF16 = HVX_BF16, FMA = kKernelAvxFma, AVX = kKernelAvx, SSE = kKernelSse;
static const uint32_t AUTO = HVX_BUILD_AUTO, BATCHED = HVX_BUILD_BATCHED, ONE = HVX_BUILD_ONE_NODE;
static const uint32_t kDegrees[5][2] = {{8, 16}, {16, 32}, {17, 33}, {24, 48}, {32, 64}};
static const uint32_t kSizes[] = {1, 2, 1023, 1024, 1025, 2048};

// rows: 0 = as wide as the limits, 1 = 64 ids, 2 = 65 ids
static Image image(uint32_t dt, uint32_t me, uint32_t fk, uint32_t dim, uint32_t pad, uint32_t m, uint32_t m0, int rows) {
    return Image{dt, me, fk, dim, dim + pad, m, m0, rows == 0 ? m0 : rows == 1 ? 64u : 65u, rows == 0 ? m : rows == 1 ? 64u : 65u};
}

static void walk_full() {
    for (uint32_t dt : {F32, BF16})
        for (uint32_t me : {(uint32_t)kL2, (uint32_t)kCosine, (uint32_t)kL1})
            for (uint32_t fk : {FMA, AVX, SSE})
                for (uint32_t dim : {32u, 100u, 128u, 192u, 768u})
                    for (uint32_t pad : {0u, 4u})
                        for (const auto &mm : kDegrees)
                            for (int rows = 0; rows < 3; ++rows) {
                                const Image im = image(dt, me, fk, dim, pad, mm[0], mm[1], rows);
                                geom(im);
                                for (uint32_t efc : {0u, 64u, 800u, 801u}) degrees(im, efc);
                                for (uint32_t lm = 0; lm < 2; ++lm)
                                    for (uint32_t mode : {AUTO, BATCHED, ONE}) {
                                        for (uint32_t bsz : kSizes)
                                            for (int pr = 0; pr < 2; ++pr)
                                                for (uint32_t layers : {1u, 3u, 6u}) batch(im, lm, mode, bsz, pr, layers);
                                        if (dim != 128u || me != kL2 || fk != FMA || pad) continue;
                                        for (uint32_t mb : {0u, 64u, 4096u})
                                            for (uint32_t dv : {0u, 16u})
                                                for (uint64_t done : {1ull, 31ull, 640ull, 100000ull})
                                                    for (uint64_t left : {1ull, 7ull, 5000ull})
                                                        for (int pr = 0; pr < 2; ++pr)
                                                            for (uint64_t ahead : {1ull, 5ull, 1ull << 40}) size(im, Call{lm, mode, mb, dv, 0u}, done, done + left, pr, done + ahead);
                                        for (uint32_t mb : {0u, 100u})
                                            for (uint64_t count : {1ull, 1000ull, 65536ull})
                                                for (uint32_t lmax : {1u, 4u})
                                                    for (int bq = 0; bq < 2; ++bq) scratch(im, Call{lm, mode, mb, 0u, 0u}, count, lmax, bq);
                                    }
                            }
}

// the committed subset: every step kind, both sides of the 1 024 threshold and of ncmax 33 / 65, the bf16 dim % 64 rule, every refusal
static void walk_subset() {
    const Image n8 = image(F32, kL2, FMA, 128, 0, 8, 16, 0), n16 = image(F32, kCosine, FMA, 768, 0, 16, 32, 0), w32 = image(F32, kL2, FMA, 128, 0, 32, 64, 1);
    const Image b8 = image(BF16, kL2, FMA, 128, 0, 8, 16, 0), b8odd = image(BF16, kCosine, FMA, 192, 0, 8, 16, 0), bw = image(BF16, kL2, FMA, 128, 0, 32, 64, 1);
    const Image *const imgs[] = {&n8, &n16, &w32, &b8, &b8odd, &bw};
    // every step kind: narrow / wide / bf16 x batched, one node, link_mode 1, on both sides of 1 024
    for (const Image *im : imgs)
        for (uint32_t lm = 0; lm < 2; ++lm)
            for (uint32_t mode : {AUTO, ONE})
                for (uint32_t bsz : kSizes)
                    for (int pr = 0; pr < 2; ++pr) {
                        if (pr && bsz != 1u) continue; // (a promoting node is inserted alone)
                        batch(*im, lm, mode, bsz, pr, pr ? 1u : 3u);
                    }
    { // the inputs tests/test_gpu_build.py holds hvx_index_last_write_path to (rows as import_index sizes them: multiples of 32 / 16 ids)
        const Image t8{F32, kL2, FMA, 64, 64, 8, 16, 32, 16}, t32{F32, kL2, FMA, 64, 64, 32, 64, 64, 32}, tb{BF16, kL2, FMA, 128, 128, 8, 16, 32, 16};
        batch(t8, 0, BATCHED, 100, 0, 3);
        batch(t32, 0, BATCHED, 50, 0, 3);
        for (const Image *im : {&t8, &t32, &tb})
            for (uint32_t lm = 0; lm < 2; ++lm) batch(*im, lm, ONE, 1, 0, 3);
    }
    batch(n8, 0, BATCHED, 400, 0, 6);
    batch(w32, 0, BATCHED, 400, 0, 6);
    batch(w32, 0, AUTO, 1, 0, 6);
    // ncmax 33 / 65 and what else decides the link workgroups: (m, m0), metric, summation tree, dimension, padding, rows
    for (const auto &mm : kDegrees)
        for (int rows = 0; rows < 3; ++rows) {
            const Image im = image(F32, kL2, FMA, 128, 0, mm[0], mm[1], rows);
            geom(im);
            batch(im, 0, AUTO, 2, 0, 3);
            batch(im, 0, AUTO, 1, 0, 3);
        }
    for (uint32_t me : {(uint32_t)kL2, (uint32_t)kCosine, (uint32_t)kL1})
        for (uint32_t fk : {FMA, AVX, SSE})
            for (uint32_t dim : {32u, 100u, 192u, 768u})
                for (uint32_t pad : {0u, 4u}) {
                    if (pad && (me != kL2 || fk != FMA)) continue;
                    for (const auto &mm : {kDegrees[1], kDegrees[4]}) {
                        const Image im = image(F32, me, fk, dim, pad, mm[0], mm[1], 0);
                        geom(im);
                        batch(im, 0, AUTO, 64, 0, 3);
                    }
                }
    for (uint32_t dim : {128u, 192u, 768u}) // bf16 rows: dim % 64
        for (const auto &mm : {kDegrees[1], kDegrees[2], kDegrees[4]}) {
            const Image im = image(BF16, kCosine, FMA, dim, 0, mm[0], mm[1], 0);
            geom(im);
            batch(im, 0, BATCHED, 64, 0, 3);
        }
    // degree limits, their defaults and every refusal
    for (uint32_t efc : {0u, 64u, 800u, 801u}) {
        degrees(Image{F32, kL2, FMA, 128, 128, 0, 0, 32, 16}, efc);
        degrees(n8, efc);
        degrees(w32, efc);
    }
    degrees(Image{F32, kL2, FMA, 128, 128, 16, 0, 32, 16}, 0);
    degrees(Image{F32, kL2, FMA, 128, 128, 16, 20, 32, 16}, 0);
    degrees(Image{F32, kL2, FMA, 128, 128, 12, 40, 64, 16}, 0);
    degrees(Image{F32, kL2, FMA, 128, 128, 32, 96, 96, 32}, 0);
    degrees(Image{F32, kL2, FMA, 128, 128, 40, 64, 64, 64}, 0);
    degrees(Image{F32, kL2, FMA, 128, 128, 16, 32, 16, 16}, 0);
    degrees(Image{F32, kL2, FMA, 128, 128, 16, 32, 32, 8}, 0);
    degrees(Image{F32, kL2, FMA, 128, 128, 16, 32, 96, 96}, 0);
    degrees(image(F32, kL2, FMA, 128, 0, 32, 64, 2), 0);
    degrees(image(F32, kL2, FMA, 128, 0, 17, 33, 0), 0);
    batch(Image{F32, kL2, FMA, 128, 128, 40, 80, 96, 64}, 0, AUTO, 2, 0, 1);
    batch(image(F32, kL2, FMA, 128, 0, 32, 64, 2), 0, AUTO, 2, 0, 1);
    batch(Image{F32, kL2, FMA, 128, 128, 32, 64, 32, 32}, 0, AUTO, 2, 0, 1);
    // batch sizes
    for (const Image *im : {&n8, &w32})
        for (uint32_t mode : {AUTO, ONE})
            for (uint64_t done : {1ull, 31ull, 640ull, 100000ull}) {
                size(*im, Call{0, mode, 0, 0, 0}, done, done + 5000, 0, 1ull << 40);
                size(*im, Call{0, mode, 64, 16, 0}, done, done + 7, 0, done + 5);
                size(*im, Call{0, mode, 4096, 0, 0}, done, done + 5000, 1, 1ull << 40);
            }
    // scratch
    for (const Image *im : {&n8, &w32, &b8, &bw})
        for (uint32_t lm = 0; lm < 2; ++lm)
            for (uint64_t count : {1ull, 1000ull, 65536ull})
                for (int bq = 0; bq < 2; ++bq) scratch(*im, Call{lm, AUTO, count == 1000 ? 100u : 0u, 0u, 0u}, count, count == 1 ? 1u : 4u, bq);
}

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "full")) walk_full();
    walk_subset();
    return 0;
}
