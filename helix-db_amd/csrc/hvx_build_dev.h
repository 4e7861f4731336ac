// hvx_build_dev.h -- what the translation units of the device build share: the argument block of the select / link kernels, row
// addressing, the row locks and the one-wavefront row helpers.  hvx_build.hip holds the kernels for degree limits up to 32 (one id per
// lane, 64-bit masks) and the host side; hvx_build_wide.hip the kernels for limits up to 64 (two ids per lane, 128-bit masks);
// hvx_build_wide_seq.hip the many-workgroup one-node steps for those limits.
#pragma once
#include <hip/hip_runtime.h>

#include "hvx_host.h"
#include "hvx_graph_dev.h"

namespace hvx {

#ifdef HVX_TUNING
#define HVX_DBG_ADD(a, i, v) do { if ((a).dbg) atomicAdd(&(a).dbg[i], (uint32_t)(v)); } while (0)
#else
#define HVX_DBG_ADD(a, i, v) do { } while (0)
#endif

constexpr uint32_t kCand = 64; // candidates kept per layer and node (2 * Mmax <= 64)

struct BuildArgs {
    DevIndex ix;
    uint32_t *l0, *up;          // the same rows as ix.l0 / ix.up, writable
    uint32_t *locks;            // [n] one lock per row owner (all its layers)
    const uint32_t *nodes;      // [b] internal ids of the batch
    uint32_t b, layers;         // layers = old max_layer + 1
    const uint64_t *cand_ids;   // [layers][b][kCand] internal ids (search output)
    const float *cand_sc;       // [layers][b][kCand]
    const uint32_t *cand_cnt;   // [layers][b]
    uint32_t *sel;              // [layers][b][32] selected neighbours in selection order
    uint32_t *sel_cnt;          // [layers][b]
    uint32_t m, m0;             // degree limits: upper layers / layer 0 (m0 = max(m0, 2m), mutation.rs:178-196)
    uint32_t *err;              // [1] set when a row would overflow its stride (invariant violation)
    uint32_t ldp, ncmax;        // build_link_wg_kernel: row stride of a column block in LDS (floats), candidate rows the LDS holds
    uint32_t link_ck;           // 32-float chunks per column block
    uint32_t *dbg;              // tuning builds (HVX_BUILD_DEBUG): [0] lock spins [1] prunes [2] reverse-edge removals [3] plain appends
    float *gdm;                 // one-node steps: [layers][kSeqLayerDm] distance matrices (device-scope stores / loads; wide images: WideSeqGeom)
    uint32_t *tick;             // ... [2][layers] workgroups that have delivered (zero between launches)
    uint32_t g0, gu;            // ... workgroups of layer 0 / of every upper layer
    uint32_t kc, selw;          // wide kernels (hvx_build_wide.hip): ids per slot of cand_ids / cand_sc, of sel (the others: kCand, 32)
};

__device__ __forceinline__ void lock_row(uint32_t *locks, uint32_t node, int lane) {
    if (lane == 0) {
        while (__hip_atomic_exchange(&locks[node], 1u, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) != 0u) __builtin_amdgcn_s_sleep(2);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    __syncthreads();
}
__device__ __forceinline__ void unlock_row(uint32_t *locks, uint32_t node, int lane) {
    __syncthreads();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0) __hip_atomic_store(&locks[node], 0u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
}

// row of `node` on `layer`, and its stride
__device__ __forceinline__ uint32_t *row_ptr(const BuildArgs &a, uint32_t node, uint32_t layer, uint32_t &stride) {
    if (layer == 0u) { stride = a.ix.s0; return a.l0 + (size_t)node * a.ix.s0; }
    stride = a.ix.su;
    return a.up + (size_t)(a.ix.up_base[node] + layer - 1u) * a.ix.su;
}

// the tail of a link runs on ONE wavefront of the workgroup (the others have left): wavefront-level ordering instead of s_barrier
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
// Row locks of build_link_wg_kernel.  Everything a lock protects (the neighbour rows) is read and written with agent-scope
// atomics (ld_row / st_row: coherent across the XCDs' L2s by themselves), so taking and dropping a lock needs ORDER only, not
// cache maintenance: no acquire / release at agent scope (on gfx950 that is an L2 invalidate / write-back of the whole XCD per
// link, with hundreds of links in flight), but relaxed atomics and an explicit wait for this wavefront's outstanding stores.
__device__ __forceinline__ void lock_row_w(uint32_t *locks, uint32_t node, int lane) {
    if (lane == 0) {
        while (__hip_atomic_exchange(&locks[node], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) __builtin_amdgcn_s_sleep(2);
    }
    __builtin_amdgcn_wave_barrier(); // the row is read after lane 0 has left the loop (one wavefront: program order)
    asm volatile("" ::: "memory");
}
__device__ __forceinline__ void unlock_row_w(uint32_t *locks, uint32_t node, int lane) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // every row store of this wavefront has been performed
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) __hip_atomic_store(&locks[node], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// canonical row (ascending id, sentinel padded) of ids_lds[0..ns), written with agent-scope stores by one wavefront
__device__ __forceinline__ void store_canonical_w(uint32_t *row, uint32_t stride, const uint32_t *ids_lds, uint32_t ns, int lane) {
    const uint32_t mine = (uint32_t)lane < ns ? ids_lds[lane] : kSentinel;
    uint32_t rank = 0;
    for (uint32_t s = 0; s < ns; ++s) rank += ids_lds[s] < mine ? 1u : 0u;
    if ((uint32_t)lane >= ns && (uint32_t)lane < stride) st_row(row + lane, kSentinel);
    if ((uint32_t)lane < ns) st_row(row + rank, mine);
}
__device__ __forceinline__ void remove_edge_w(const BuildArgs &a, uint32_t layer, uint32_t owner, uint32_t victim, int lane) {
    lock_row_w(a.locks, owner, lane);
    uint32_t stride;
    uint32_t *row = row_ptr(a, owner, layer, stride);
    const uint32_t v = (uint32_t)lane < stride ? ld_row(row + lane) : kSentinel;
    const bool keep = v != kSentinel && v != victim;
    const unsigned long long km = __ballot(keep);
    const uint32_t pos = (uint32_t)__builtin_popcountll(km & ((1ull << lane) - 1ull));
    const uint32_t nk = (uint32_t)__builtin_popcountll(km);
    if (keep) st_row(row + pos, v);   // every lane holds its id in a register: the order of the stores does not matter
    if ((uint32_t)lane >= nk && (uint32_t)lane < stride) st_row(row + lane, kSentinel);
    unlock_row_w(a.locks, owner, lane);
}

// ---- ONE node at a time, degree limits up to 32 (hvx_build.hip: build_select_seq_kernel / build_link_seq_kernel) ----
constexpr uint32_t kSeqRow = 35;                 // ids of a link's list (row + the node); wider rows take the one-wavefront kernel
constexpr uint32_t kSeqRS = 36;                  // stride of a link's matrix: rows 0 .. nc (row nc: the owner's), columns 0 .. nc - 1
constexpr uint32_t kSeqSelDm = 65 * 64;          // the select's matrix
constexpr uint32_t kSeqLinkDm = kSeqRS * kSeqRS;
constexpr uint32_t kSeqLayerDm = kSeqSelDm + 32u * kSeqLinkDm;
constexpr uint32_t kSeqPairs = 128;              // (row, victim) removals one layer's links can log
static size_t seq_lds_bytes() { return (size_t)(2 * 32 * kSeqRS + 5 * 32 + 2 * kSeqPairs + 36 + 16 * 128) * 4; } // SeqLds (hvx_build.hip)

using BuildKernel = void (*)(BuildArgs);
// build_link_wg_kernel over bf16 rows (hvx_build_bf16.hip; hvx_build_link_wg.h), L2 / cosine
BuildKernel build_link_wg_bf16_kernel(uint32_t metric);

// ---- degree limits above 32 (hvx_build_wide.hip): Mmax = max(m0, m) <= 64 ----
constexpr uint32_t kCandWide = 128; // candidates kept per layer and node (2 * Mmax <= 128)
constexpr uint32_t kSelWide = 64;   // selected neighbours per layer and node
// (geometry of build_link_wide_wg_kernel for an image: wide_link_geom, hvx_build_plan.h)
hipError_t launch_build_select_wide(const BuildArgs &a, bool fused, bool bf16, dim3 grid, hipStream_t s);
hipError_t launch_build_link_wide(const BuildArgs &a, bool fused, bool bf16, uint32_t nodes, hipStream_t s);
hipError_t launch_build_link_wide_wg(const BuildArgs &a, bool fused, uint32_t layers, size_t lds, hipStream_t s);

// ---- ONE node into a wide image as two many-workgroup steps (hvx_build_wide_seq.hip): the wide restatement of build_select_seq_kernel /
// build_link_seq_kernel.  Everything the two kernels and insert_range agree on is decided here, for (m, m0, layers = old max_layer + 1):
//   the matrices in BuildArgs.gdm, layer by layer (floats; layer L starts at layer_off(L)):
//     [0, sel_dm)                     the select's matrix: rows 0 .. hyd (row hyd: the owner's, = the search's scores), sel_rw floats wide,
//                                     hyd <= 2 * Mmax.  128 wide where 2 * Mmax > 64 (replay_rows2<128>), 64 wide otherwise (replay_rows<64>)
//     [sel_dm + t * link_dm, ...)     link t < Mmax: rows 0 .. nc (row nc: the owner's), kWideSeqRS floats wide, nc <= kWideSeqRow ids
//   the pair prefix: a link whose list holds deg ids takes wide_seq_list_pairs(deg, Mmax) consecutive pair numbers, links in selection
//     order -- (deg + 1) deg / 2 where the list exceeds its limit (all pairs among the ids and the owner), none otherwise;
//   the grids: layer 0 takes g0 workgroups, every upper layer gu (the select step 256 threads, the link step 1 024);
//   the link step's dynamic LDS.
// ok = false: the shape does not fit (the one-wavefront kernels serve it).  It fits whenever the host serves the image at all: Mmax <= 64
// on rows of at most 64 ids, m <= 32.
constexpr uint32_t kWideSeqRow = 65;   // ids of a link's list: a row of <= 64 ids + the node
constexpr uint32_t kWideSeqLS = 66;    // ... its stride in LDS
constexpr uint32_t kWideSeqRS = 96;    // row stride of a link's matrix (floats): a multiple of 32 that holds 65 columns
// removals (row, victim) one layer's links can log: <= Mmax links, each list of <= 65 ids pruned to Mmax drops <= 65 - Mmax ids, and
// x (65 - x) <= 32 * 33 -- rows of at most 64 ids cannot overflow it
constexpr uint32_t kWideSeqPairs = 32 * 33;
constexpr uint32_t kWideSeqWaves = 16; // wavefronts of the link step
constexpr uint32_t kWideSeqW2 = 128 * 2 + 128 * 4 + 128 + 64; // = kWide2Words (hvx_graph_dev.h): replay_rows2's scratch per wavefront
__host__ __device__ __forceinline__ uint32_t wide_seq_list_pairs(uint32_t deg, uint32_t maxn) { return deg > maxn ? (deg + 1u) * deg / 2u : 0u; }
struct WideSeqGeom {
    uint32_t maxn[2];     // degree limit: layer 0 / upper layers
    uint32_t sel_rw[2];   // row stride of the select's matrix
    uint32_t sel_dm[2];   // floats of the select's matrix
    uint32_t link_dm;     // floats of one link's matrix
    uint32_t layer_dm[2]; // floats of one layer's matrices
    uint32_t layers;
    uint32_t sel_g0, sel_gu, link_g0, link_gu;
    uint32_t link_lds;    // bytes
    bool ok;
    __host__ __device__ size_t layer_off(uint32_t L) const { return L == 0u ? 0u : (size_t)layer_dm[0] + (size_t)(L - 1u) * layer_dm[1]; }
    __host__ __device__ size_t sel_off(uint32_t L) const { return layer_off(L); }
    __host__ __device__ size_t link_off(uint32_t L, uint32_t t) const { return layer_off(L) + sel_dm[L ? 1 : 0] + (size_t)t * link_dm; }
    __host__ __device__ size_t total_floats() const { return layer_off(layers); }
};
__host__ __device__ __forceinline__ WideSeqGeom wide_seq_geom(uint32_t m, uint32_t m0, uint32_t layers) {
    WideSeqGeom g{};
    g.maxn[0] = m0; g.maxn[1] = m;
    g.layers = layers;
    g.link_dm = (kWideSeqRow + 1u) * kWideSeqRS;
    for (int u = 0; u < 2; ++u) {
        const uint32_t hyd = 2u * g.maxn[u] < kCandWide ? 2u * g.maxn[u] : kCandWide;
        g.sel_rw[u] = hyd > 64u ? 128u : 64u;
        g.sel_dm[u] = (hyd + 1u) * g.sel_rw[u];
        g.layer_dm[u] = g.sel_dm[u] + g.maxn[u] * g.link_dm;
    }
    // select: 32 pairs per workgroup and pass -- 8 128 pairs among 128 candidates on layer 0 (one pass of 254 workgroups), 2 016 above;
    // link: 128 pairs per workgroup and pass -- <= 64 lists x 2 145 pairs on layer 0, <= 32 x 561 above on rows within their limit
    g.sel_g0 = 254u; g.sel_gu = 63u;
    g.link_g0 = 256u; g.link_gu = 32u;
    // lists and kept lists [64][kWideSeqLS], per link: ids / ids that stay / dropped positions [4] / the neighbour, the removal log,
    // the pair prefix, replay_rows2's scratch per wavefront
    g.link_lds = (2u * 64u * kWideSeqLS + 64u * (2u + 4u + 1u) + 2u * kWideSeqPairs + 68u + kWideSeqWaves * kWideSeqW2) * 4u;
    g.ok = m0 <= 64u && m <= 32u && (m0 > 32u || m > 32u) && layers >= 1u && layers <= 64u && g.link_lds <= 160u * 1024u;
    return g;
}
hipError_t launch_build_select_wide_seq(const BuildArgs &a, bool fused, bool bf16, hipStream_t s);
hipError_t launch_build_link_wide_seq(const BuildArgs &a, bool fused, bool bf16, hipStream_t s);

} // namespace hvx
