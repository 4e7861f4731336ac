// hvx_build_plan.h -- host only: WHAT a device write (hvx_index_build, hvx_index_insert_batch, hvx_index_upsert_batch,
// hvx_index_link_rows; hvx_build.hip) runs, and with what geometry.  The degree limits and their defaults, the refusals that go with
// them, the geometry of the two link-workgroup kernels, the batch sizes, the scratch layout and -- plan_write_batch() -- which select
// and link kernels a batch takes are decided here and nowhere else; hvx_build.hip maps a plan to launches.  No kernel is included:
// tests/native/build_plan_probe.cpp prints the decisions on the host, tests/test_build_plan.py pins them.
#pragma once
#include <algorithm>
#include <stddef.h>
#include <stdint.h>

#include "hvx_build_dev.h"
#include "hvx_hnsw_plan.h"

namespace hvx {

// ---- degree limits: MutationDegreeLimits (mutation.rs:178-196), DEFAULT_EF_CONSTRUCTION (mod.rs:702-708) ----
struct WriteDegrees {
    uint32_t m, m0;    // upper layers / layer 0: m0 = max(m0, 2 m)
    uint32_t efc;      // ef_construction
    uint32_t ef0, efu; // beam of the build search on layer 0 / above
    bool wide;         // limits above 32: the kernels of hvx_build_wide.hip (two ids per lane, 128-bit masks) ...
    uint32_t kc, selw; // ... with twice the search candidates / selected neighbours per layer and node
};
inline WriteDegrees write_degrees(const hvx_index_desc &desc, const hvx_build_params *params) {
    WriteDegrees g{};
    g.m = desc.m ? desc.m : 16u;
    g.m0 = std::max(desc.m0 ? desc.m0 : 2u * g.m, 2u * g.m);
    g.efc = params && params->ef_construction ? params->ef_construction : 200u;
    g.ef0 = std::max(g.efc, g.m0);
    g.efu = std::max(g.efc, 2u * g.m);
    g.wide = std::max(g.m0, g.m) > 32u;
    g.kc = g.wide ? kCandWide : kCand;
    g.selw = g.wide ? kSelWide : 32u;
    return g;
}

// What the write path refuses about degree limits and row widths.  write_refusal() returns the first of the asked checks that fails,
// in this order; the caller words it (its own noun: "device build", "device inserts", "device upserts").
enum WriteRefusal : uint32_t {
    kWriteServed = 0,
    kRefuseDegrees = 1,    // m0 > 64 (m > 32)
    kRefuseRowsNarrow = 2, // the image's rows hold fewer ids than the limits
    kRefuseRowsOver64 = 4, // limits above 32 on rows of more than 64 ids
    kRefuseEf = 8,         // the build search's beam: ef_construction > 800
};
inline WriteRefusal write_refusal(const WriteDegrees &g, uint32_t s0, uint32_t su, uint32_t checks) {
    if ((checks & kRefuseDegrees) && (g.m0 > 64u || g.m > 32u)) return kRefuseDegrees;
    if ((checks & kRefuseRowsNarrow) && (s0 < g.m0 || su < g.m)) return kRefuseRowsNarrow;
    if ((checks & kRefuseRowsOver64) && g.m0 > 32u && (s0 > 64u || su > 64u)) return kRefuseRowsOver64;
    if ((checks & kRefuseEf) && wave_build_need(g.ef0, g.efu) > kBeamMax) return kRefuseEf;
    return kWriteServed;
}

// ---- the link workgroups: one workgroup per link, the prune evaluated from LDS ----
struct LinkGeom {
    uint32_t ldp, ncmax, link_ck; // row stride of a column block in LDS (floats), candidate rows the LDS holds, 32-float chunks per block
    size_t lds;                   // dynamic LDS bytes
    bool ok;                      // false: the kernel has no build for this image (the one-wavefront kernel links instead)
};
// build_link_wg_kernel (hvx_build_link_wg.h): column blocks of <= 8 chunks (256 floats) of Mmax + 1 candidate rows and the owner's in LDS,
// row stride = 128 B mod 256 B (the eight row groups of a wavefront read different rows: conflict-free ds_read_b128 for neighbouring rows)
constexpr int kLinkPre = 9, kLinkPreBf16 = 5; // 16-byte pieces of the next column block a thread holds in registers: f32 / bf16 rows
__device__ __host__ __forceinline__ size_t link_pairs_max(uint32_t ncmax) { return (size_t)(ncmax + 1u) * ncmax / 2u; }
inline size_t link_lds_bytes(uint32_t ldp, uint32_t ncmax) {
    return (size_t)(ncmax + 1u) * ldp * 4u + 512u + (size_t)(ncmax + 1u) * (ncmax + 1u) * 4u + 5u * 256u + 32u +
           2u * ((link_pairs_max(ncmax) + 15u) & ~(size_t)15u);
}
inline LinkGeom link_geom(const DevIndex &d, uint32_t m, uint32_t m0) {
    LinkGeom g{};
    g.ncmax = std::max(m0, m) + 1u;
    const uint32_t nk_rows = d.dim_main >> 5;
    g.link_ck = std::min<uint32_t>(8u, (nk_rows + 1u) & ~1u);
    g.ldp = g.link_ck * 32u + 32u;
    g.lds = link_lds_bytes(g.ldp, g.ncmax);
    const bool bf16 = d.dtype == HVX_BF16;
    // L2 / cosine (Manhattan has no instantiation), the 32-lane summation trees, rows without a scalar tail (dim % 32 == 0, no padding)
    // and <= 33 candidates (561 pairs = 4 wavefronts x 18 steps x 8); bf16 rows: a column block never splits a 16-byte piece
    g.ok = (bf16 || d.metric != kL1) && !kernel_w4(d.fkernel) && g.ncmax <= 33u && nk_rows > 0 && d.dim_main == d.dim && d.ld == d.dim &&
           (bf16 ? d.dim % 64u == 0u && (size_t)(g.ncmax + 1u) * g.link_ck * 4u <= (size_t)kLinkPreBf16 * 256u
                 : (size_t)(g.ncmax + 1u) * g.link_ck * 8u <= (size_t)kLinkPre * 256u);
    return g;
}
// build_link_wide_wg_kernel (hvx_build_wide.hip): 66 rows, 2 145 pairs
constexpr int kWideTasks = 17; // wave-steps of 8 pairs per wavefront
constexpr int kWidePre = 3;    // float4 a thread carries for the next block
constexpr uint32_t kWideWaves = 16;
__device__ __host__ __forceinline__ size_t wide_pairs_max(uint32_t ncmax) { return (((size_t)(ncmax + 1u) * ncmax / 2u) + 15u) & ~(size_t)15u; }
inline size_t wide_link_lds_bytes(uint32_t ldp, uint32_t ncmax) {
    return (size_t)(ncmax + 1u) * ldp * 4u + 128u * 16u + (size_t)(ncmax + 1u) * (ncmax + 1u) * 4u + 4u * 512u + 256u + 32u + 2u * wide_pairs_max(ncmax);
}
inline LinkGeom wide_link_geom(const DevIndex &d, uint32_t m, uint32_t m0) {
    LinkGeom g{};
    g.ncmax = std::max(m0, m) + 1u;
    const uint32_t nk_rows = d.dim_main >> 5;
    g.link_ck = std::min<uint32_t>(4u, (nk_rows + 1u) & ~1u);
    g.ldp = g.link_ck * 32u + 32u;
    g.lds = wide_link_lds_bytes(g.ldp, g.ncmax);
    // f32 rows without a scalar tail (dim % 32 == 0, no padding), L2 / cosine, the 32-lane summation trees, <= 65 candidates
    // (2 145 pairs = 16 wavefronts x 17 steps x 8; a column block of 66 rows = 3 float4 per thread)
    g.ok = d.dtype == HVX_F32 && (d.metric == kL2 || d.metric == kCosine) && !kernel_w4(d.fkernel) && g.ncmax <= 65u && nk_rows > 0 && d.dim_main == d.dim &&
           d.ld == d.dim && d.s0 <= 64u && d.su <= 64u && (size_t)(g.ncmax + 1u) * g.link_ck * 8u <= (size_t)kWidePre * 1024u &&
           (size_t)(g.ncmax + 1u) * g.ncmax / 2u <= (size_t)kWideWaves * kWideTasks * 8u;
    return g;
}

// hvx_build_params.sequential: HVX_BUILD_ONE_NODE (and any value the header does not name) = one node per batch
inline bool one_node_batches(const hvx_build_params *p) { return p->sequential != HVX_BUILD_AUTO && p->sequential != HVX_BUILD_BATCHED; }

// ---- one write call: everything its batches share ----
struct WriteCtx {
    WriteDegrees g;
    LinkGeom link, wide_link; // the two link-workgroup kernels (wide_link: ok = false below limits of 33)
    bool bf16;
    uint32_t link_mode;       // hvx_build_params.link_mode: 1 = the one-wavefront kernels everywhere
    bool one_node;            // one node per batch (the reference's order exactly)
    bool wide_seq;            // limits above 32: one-node batches take the many-workgroup steps of hvx_build_wide_seq.hip
    uint32_t ld, s0, su;      // of the image
    uint32_t bmax, divisor;   // batch sizes: at most bmax nodes, at most inserted / divisor
};
inline WriteCtx write_ctx(const DevIndex &d, const hvx_index_desc &desc, const hvx_build_params &params, uint32_t handle_max_batch, uint32_t layers_max) {
    WriteCtx c{};
    c.g = write_degrees(desc, &params);
    c.link = link_geom(d, c.g.m, c.g.m0);
    c.wide_link = c.g.wide ? wide_link_geom(d, c.g.m, c.g.m0) : LinkGeom{};
    c.bf16 = d.dtype == HVX_BF16;
    c.link_mode = params.link_mode;
    c.one_node = one_node_batches(&params);
    // (wherever their geometry fits: rows <= 64 ids are the caller's refusal)
    c.wide_seq = c.g.wide && params.link_mode != 1u && wide_seq_geom(c.g.m, c.g.m0, layers_max).ok;
    c.ld = d.ld; c.s0 = d.s0; c.su = d.su;
    c.bmax = std::min(params.max_batch ? params.max_batch : 2048u, handle_max_batch); // per-batch scratch of the search kernel is sized by max_batch
    // (degree limits above 32: half the batch fraction -- a batch holds UP TO inserted / divisor nodes.  Nodes of a batch do not see each
    // other, and at M 32 / M0 64 that costs more than the 0.01 of recall batching is granted: 8 000 x 128 Gaussian rows, divisor 16, ef 32:
    // 0.8213 - 0.8240 against the sequential graph's 0.8326; with half the fraction 0.829)
    c.divisor = (params.batch_divisor ? params.batch_divisor : 32u) * (c.g.wide ? 2u : 1u);
    return c;
}

// batch = consecutive positions [done, done + size) of the insertion order; a node above the current top layer (promotes, and
// promotes_at(position) for the ones behind it) is inserted alone and becomes the entry point
template <typename PromotesAt> inline uint32_t write_batch_size(const WriteCtx &c, uint64_t done, uint64_t end, bool promotes, PromotesAt promotes_at) {
    uint32_t bsz = 1;
    if (!promotes && !c.one_node) {
        uint64_t want = std::min<uint64_t>(std::max<uint64_t>(done / c.divisor, 1), c.bmax);
        want = std::min<uint64_t>(want, end - done);
        while (bsz < want && !promotes_at(done + bsz)) ++bsz;
    }
    return bsz;
}

// ---- one batch ----
enum class SelectStep : uint32_t { narrow_wave, narrow_eager, wide_wave, wide_eager }; // eager: select AND links, as two many-workgroup kernels
enum class LinkStep : uint32_t { none, narrow_wave, narrow_wg, wide_wave, wide_wg };   // none: the eager pair has linked
struct StepGeom {
    uint32_t gx, gy, threads; // grid, workgroup
    size_t lds;               // dynamic LDS bytes
    uint32_t g0, gu;          // eager steps: workgroups of layer 0 / of every upper layer (BuildArgs.g0 / gu)
};
struct WriteBatchPlan {
    SelectStep select;
    LinkStep link;
    StepGeom sel, lnk; // (lnk of an eager pair: its second kernel)
    bool serial;       // the batch starts when everything before it is in the graph, and nothing overlaps it
    int occupancy;     // of the build search (HnswArgs.occupancy)
    uint32_t path;     // HVX_WRITE_* (hvx_index_last_write_path)
};
// The wide workgroup kernel reads 2 145 pairs x dim out of LDS per link: LDS-bandwidth bound, ~48 us per link at dim 768 with one
// workgroup per CU.  Once a batch has enough nodes for the one-wavefront kernel's dependent gathers to overlap across nodes
// (>= 1 024: four wavefronts per CU) that kernel is the faster link step -- 1M x 768, batches of 2 048: 13.9 s against 15.9 s --,
// below that the workgroup kernel is (8 000 x 128, batches <= 250: 0.22 s against 0.99 s).
constexpr uint32_t kWideWgMaxBatch = 1024;

// layers = old max_layer + 1
inline WriteBatchPlan plan_write_batch(const WriteCtx &c, uint32_t bsz, bool promotes, uint32_t layers) {
    WriteBatchPlan p{};
    const bool workgroups = c.link_mode != 1u;
    // (degree limits above 32 do not overlap either: at M 32 / M0 64 a batch that sees neither its own nodes nor the batch before it
    // costs 0.002 of recall@10 at ef 32 on 8 000 Gaussian rows -- 0.8216 against 0.8235 --, a fifth of the margin batching is granted)
    p.serial = promotes || bsz == 1u || c.one_node || !workgroups || c.g.wide;
    // more nodes than SIMDs: two searches per SIMD instead of two rounds (bf16 rows: the build search exists one per SIMD only)
    p.occupancy = (bsz > 1024u && workgroups && !c.bf16) ? 2 : 1;
    p.path = c.g.wide ? HVX_WRITE_WIDE : 0u;
    const size_t wave_lds = build_lds_bytes(c.ld);
    if (c.g.wide && bsz == 1u && c.wide_seq) { // two ids per lane, one node: select and links as two many-workgroup steps (f32 and bf16 rows)
        const WideSeqGeom q = wide_seq_geom(c.g.m, c.g.m0, layers);
        p.select = SelectStep::wide_eager;
        p.sel = StepGeom{q.sel_g0 + (layers - 1u) * q.sel_gu, 1u, 256u, 0, q.sel_g0, q.sel_gu};
        p.link = LinkStep::none;
        p.lnk = StepGeom{q.link_g0 + (layers - 1u) * q.link_gu, 1u, 1024u, q.link_lds, q.link_g0, q.link_gu};
        p.path |= HVX_WRITE_EAGER_STEPS;
    } else if (c.g.wide) { // the one-wavefront kernels for one node (link_mode = 1), one workgroup per link for a batch
        p.select = SelectStep::wide_wave;
        p.sel = StepGeom{bsz, layers, 64u, 0, 0u, 0u};
        if (bsz > 1u && bsz < kWideWgMaxBatch && workgroups && c.wide_link.ok) { // (f32 rows: wide_link_geom; a bf16 batch of any size takes the one-wavefront kernel)
            p.link = LinkStep::wide_wg;
            p.lnk = StepGeom{bsz * kSelWide, layers, 1024u, c.wide_link.lds, 0u, 0u};
            p.path |= HVX_WRITE_LINK_WG;
        } else {
            p.link = LinkStep::wide_wave;
            p.lnk = StepGeom{bsz, 1u, 64u, 0, 0u, 0u};
            p.path |= HVX_WRITE_ONE_WAVE;
        }
    } else if (bsz == 1u && workgroups && c.s0 + 1u <= kSeqRow && c.su + 1u <= kSeqRow) {
        // one node: its select and its links as two many-workgroup steps with every prune's distance matrix evaluated up front
        p.select = SelectStep::narrow_eager;
        p.sel = StepGeom{63u + (layers - 1u) * 16u, 1u, 256u, 0, 63u, 16u}; // 32 row groups per workgroup: 2 016 pairs among 64 candidates on layer 0, 496 among 32 above
        p.link = LinkStep::none;
        p.lnk = StepGeom{96u + (layers - 1u) * 12u, 1u, 1024u, seq_lds_bytes(), 96u, 12u}; // 128 row groups per workgroup: <= 32 links x 561 pairs on layer 0, <= 16 x 153 above
        p.path |= HVX_WRITE_EAGER_STEPS;
    } else {
        p.select = SelectStep::narrow_wave;
        p.sel = StepGeom{bsz, layers, 64u, wave_lds, 0u, 0u};
        if (bsz > 1u && workgroups && c.link.ok) { // batched mode: one workgroup per link, prunes evaluated from LDS
            p.link = LinkStep::narrow_wg;
            p.lnk = StepGeom{bsz * 32u, layers, 256u, c.link.lds, 0u, 0u};
            p.path |= HVX_WRITE_LINK_WG;
        } else { // one node (the reference's order exactly), or rows the workgroup kernel does not serve: one wavefront per node
            p.link = LinkStep::narrow_wave;
            p.lnk = StepGeom{bsz, 1u, 64u, wave_lds, 0u, 0u};
            p.path |= HVX_WRITE_ONE_WAVE;
        }
    }
    return p;
}

// ---- the call's scratch (hvx_index.ins_scratch): byte offsets, in this order, every piece a multiple of 256 bytes ----
struct WriteScratch {
    size_t tick;   // [2][64] tickets of the eager steps (first: zero between calls, set once by the memset when the scratch grows)
    size_t iota;   // [count] the nodes in insertion order
    size_t cids, csc, cnt, selcnt, sel; // candidate / selection buffers, two sets each (sz_* elements per set)
    size_t status; // [bmax]
    size_t err;    // the error word, the flagged nodes
    size_t gdm;    // the one-node steps' matrices
    size_t bq;     // bf16 images without the caller's f32 rows: the batch's rows widened to f32 (0 bytes otherwise)
    bool has_bq;
    size_t need;   // bytes in all; the buffer grows to need + need / 4
    size_t sz_cids, sz_cnt, sz_sel;
};
inline WriteScratch write_scratch(const WriteCtx &c, uint64_t count, uint32_t layers_max, uint32_t dim, bool own_bq) {
    auto up = [](size_t b) { return (b + 255u) & ~(size_t)255u; };
    WriteScratch w{};
    w.sz_cids = (size_t)layers_max * c.bmax * c.g.kc;
    w.sz_cnt = (size_t)layers_max * c.bmax;
    w.sz_sel = (size_t)layers_max * c.bmax * c.g.selw;
    const size_t b_cnt = up(2 * w.sz_cnt * 4);
    // the one-node steps' matrices: wide images by their geometry (a 129 x 128 select matrix and 64 link matrices on layer 0)
    const size_t b_gdm = up((c.wide_seq ? wide_seq_geom(c.g.m, c.g.m0, layers_max).total_floats() : (size_t)layers_max * kSeqLayerDm) * 4);
    w.has_bq = c.bf16 && own_bq;
    size_t p = 0;
    w.tick = p; p += up(2 * 64 * 4);
    w.iota = p; p += up(count * 4);
    w.cids = p; p += up(2 * w.sz_cids * 8);
    w.csc = p; p += up(2 * w.sz_cids * 4);
    w.cnt = p; p += b_cnt;
    w.selcnt = p; p += b_cnt;
    w.sel = p; p += up(2 * w.sz_sel * 4);
    w.status = p; p += up((size_t)c.bmax * 4);
    w.err = p; p += 256;
    w.gdm = p; p += b_gdm;
    w.bq = p; p += w.has_bq ? up((size_t)c.bmax * dim * 4) : 0;
    w.need = p;
    return w;
}

} // namespace hvx
