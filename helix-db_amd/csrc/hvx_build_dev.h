// hvx_build_dev.h -- what the translation units of the device build share: the argument block of the select / link kernels, row
// addressing, the row locks and the one-wavefront row helpers.  hvx_build.hip holds the kernels for degree limits up to 32 (one id per
// lane, 64-bit masks) and the host side; hvx_build_wide.hip the kernels for limits up to 64 (two ids per lane, 128-bit masks).
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
    float *gdm;                 // one-node steps: [layers][kSeqLayerDm] distance matrices (device-scope stores / loads)
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

using BuildKernel = void (*)(BuildArgs);
// build_link_wg_kernel over bf16 rows (hvx_build_bf16.hip; hvx_build_link_wg.h), L2 / cosine
BuildKernel build_link_wg_bf16_kernel(uint32_t metric);

// ---- degree limits above 32 (hvx_build_wide.hip): Mmax = max(m0, m) <= 64 ----
constexpr uint32_t kCandWide = 128; // candidates kept per layer and node (2 * Mmax <= 128)
constexpr uint32_t kSelWide = 64;   // selected neighbours per layer and node
struct WideLinkGeom { uint32_t ldp, ncmax, link_ck; size_t lds; bool ok; };
// geometry of build_link_wide_wg_kernel for this image; ok = false where it has no build (the one-wavefront kernel links instead)
WideLinkGeom wide_link_geom(const DevIndex &d, uint32_t m, uint32_t m0);
hipError_t launch_build_select_wide(const BuildArgs &a, bool fused, bool bf16, dim3 grid, hipStream_t s);
hipError_t launch_build_link_wide(const BuildArgs &a, bool fused, bool bf16, uint32_t nodes, hipStream_t s);
hipError_t launch_build_link_wide_wg(const BuildArgs &a, bool fused, uint32_t layers, size_t lds, hipStream_t s);

} // namespace hvx
