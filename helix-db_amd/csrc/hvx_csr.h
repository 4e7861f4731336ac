// hvx_csr.h -- the device-resident CSR graph behind the opaque hvx_csr handle, and the staging helpers its users share: hvx_traverse.hip
// (import, free, the traversals) and hvx_prefilter.hip (the fused prefilter searches).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "hvx_csr_dev.h"
#include "hvx_host.h"

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(HVX_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

struct hvx_csr {
    int device = 0;
    uint32_t n = 0;
    uint64_t e = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::vector<void *> allocs;
    // outgoing and incoming adjacency (crates/graph-algorithms/src/model.rs:376-417 builds both)
    uint64_t *out_off = nullptr, *in_off = nullptr;
    uint32_t *out_tgt = nullptr, *in_tgt = nullptr;
    uint32_t *out_lab = nullptr, *in_lab = nullptr; // null when the graph is unlabeled
    uint32_t *visited = nullptr;                    // [words] bitmap
    uint32_t *depth = nullptr;                      // [n]
    uint32_t *front[2] = {nullptr, nullptr};        // frontier queues [n]
    uint32_t *counter = nullptr;                    // [2] next-frontier size
    uint32_t *labels = nullptr;                     // allowed-label scratch
    uint32_t labels_cap = 0;
    // ordered traversal (hvx_traverse_ordered)
    bool rows_sorted = true;                        // every outgoing row ascends by target (the reference's rows do: model.rs:656-666)
    uint32_t *in_arc = nullptr;                     // [e] incoming slot -> index of the stored edge in the outgoing arrays (e < 2^32)
    uint32_t *owner = nullptr;                      // [n] frontier position that claimed the node at its level
    uint32_t *pc_out = nullptr, *pc_in = nullptr;   // [e] per arc: bit 31 = discovery arc, low bits = discovery arcs before it in its row
    uint32_t *cnt = nullptr;                        // [n + 1] per frontier position: discovery arcs (then their exclusive scan)
    uint32_t *ord_node = nullptr, *ord_parent = nullptr, *ord_arc = nullptr; // [n] visits in discovery order
    uint32_t *lvl = nullptr;                        // [4] level start, level size, next level size
    void *host = nullptr;                           // HostCsr mirror (hvx_traverse_dfs), fetched on first use
    uint32_t *h_seeds = nullptr;                    // pinned: the seeds of the traversal in flight (a pageable upload is a synchronous staged copy)
    size_t cap_h_seeds = 0;
    hipEvent_t done = nullptr;                      // recorded behind a traversal whose consumer runs on another stream (fused prefilter search)
    uint64_t max_out_deg = 0, max_in_deg = 0;       // largest row of either adjacency: bounds what one hop from s seeds can reach (round 6)
    // chains of expand hops (hvx_expand_path_filter / hvx_prefilter_path_search_batch_params), allocated on first use
    uint32_t *visited2 = nullptr;                   // [words] the second frontier bitmap: the hops ping-pong between it and `visited`
    uint32_t *hop_cnt = nullptr;                    // [16] per hop: bits set in its target bitmap
    uint32_t *mask_dev = nullptr;                   // [words] the Filter step's node mask
    uint32_t *h_mask = nullptr;                     // pinned staging of the mask
    uint32_t *h_hops = nullptr;                     // pinned [16]: the hop sizes read back
    // chains with per-query seeds (hvx_expand_path_lists / hvx_prefilter_path_search_lists_params), allocated on first use, grown on demand:
    // [b][max_frontier] u64 scan slots | [b][2][max_frontier] u32 frontier lists | [b] lengths | [b] statuses | [b][16] hop sizes
    void *lists_buf = nullptr;
    size_t lists_cap = 0;
    // repeat(expand) with per-query seeds (hvx_expand_repeat_lists / hvx_prefilter_repeat_search_lists_params) shares lists_buf -- its
    // control words are [b] lengths | [b] statuses | [b][16] emitted sizes | [b] stop depths -- and adds the `until` predicate's bitmap:
    uint32_t *until_dev = nullptr;                  // [words]
    uint32_t *h_until = nullptr;                    // pinned staging of it
    // shortest paths for a batch of requests (hvx_shortest_path_batch, hvx_shortest_path.hip), allocated on first use, grown on demand:
    // [b][max_depth + 1] u64 paths | [b] lengths | [b] statuses | [b][max_depth] reach sizes | [b][max_reach] u32 discovery order |
    // [b][slots] u8 levels.  The endpoints travel in h_seeds.
    void *sp_buf = nullptr;
    size_t sp_cap = 0;
    // shortest paths of any reach (hvx_shortest_path_batch_dense, hvx_shortest_path_dense.hip), allocated on first use, grown on demand:
    // the sibling's outputs ([b][max_depth + 1] u64 paths | [b] lengths | [b] statuses | [b][max_depth] reach sizes) | [b] x 5 u32 request
    // words | [groups] u64 active | [2][groups] u64 grew || one round of hvx_shortest_path_dense_plan.h's node state (88 B per node and group)
    void *spd_buf = nullptr;
    size_t spd_cap = 0;
    // live edits (hvx_csr_apply_edges, hvx_csr_edit.hip), allocated on the first edit: the spare set of the offset and edge-sized
    // arrays a batch is written into (the two sets swap when the batch is accepted), the plan's staging, the counters
    uint64_t cap_arcs = 0, cap_arcs2 = 0;           // arcs the live / the spare edge-sized arrays hold
    uint64_t cap_pc = 0;                            // arcs pc_out / pc_in hold
    uint64_t *out_off2 = nullptr, *in_off2 = nullptr;
    uint32_t *out_tgt2 = nullptr, *in_tgt2 = nullptr, *out_lab2 = nullptr, *in_lab2 = nullptr, *in_arc2 = nullptr;
    void *edit_plan = nullptr;                      // the plan on the device
    void *h_edit = nullptr;                         // pinned: [64 B read-back of the counters][the plan]
    size_t cap_edit_plan = 0, cap_h_edit = 0;
    uint32_t *edit_ctr = nullptr;                   // [4] removals without a stored arc, largest new outgoing row, largest new incoming row
};

namespace hvx {

static inline CsrView csr_view(const hvx_csr *g) { return CsrView{g->out_off, g->in_off, g->out_tgt, g->in_tgt, g->out_lab, g->in_lab, g->n}; }

static inline int csr_alloc(hvx_csr *g, void **p, size_t bytes) {
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(HVX_ERR_DEVICE, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    g->allocs.push_back(*p);
    return HVX_OK;
}

// caller holds g->mu.  A grow-on-demand device buffer of the handle (*buf, *cap) of at least `bytes`; every call that used the old one has
// waited for its stream.
static inline int csr_reserve(hvx_csr *g, void **buf, size_t *cap, size_t bytes) {
    if (bytes <= *cap) return HVX_OK;
    if (*buf) {
        g->allocs.erase(std::remove(g->allocs.begin(), g->allocs.end(), *buf), g->allocs.end());
        (void)hipFree(*buf);
        *buf = nullptr;
        *cap = 0;
    }
    int rc = csr_alloc(g, buf, bytes);
    if (rc) return rc;
    *cap = bytes;
    return HVX_OK;
}

static inline int upload_labels(hvx_csr *g, const uint32_t *labels, uint32_t n, hipStream_t s = nullptr) {
    if (n > g->labels_cap) {
        int rc = csr_alloc(g, (void **)&g->labels, (size_t)n * 4);
        if (rc) return rc;
        g->labels_cap = n;
    }
    if (n) HIP_TRY(hipMemcpyAsync(g->labels, labels, (size_t)n * 4, hipMemcpyHostToDevice, s ? s : g->stream));
    return HVX_OK;
}

// caller holds g->mu.  The pinned seed buffer of at least n_words u32; when it has to grow, nothing may still read the old one: the
// graph's stream is waited for, and `consumer` (a stream whose kernels read the seeds in place) when one is given.
static inline int seeds_reserve(hvx_csr *g, size_t n_words, hipStream_t consumer) {
    if (n_words <= g->cap_h_seeds) return HVX_OK;
    if (consumer) HIP_TRY(hipStreamSynchronize(consumer));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (g->h_seeds) (void)hipHostFree(g->h_seeds);
    g->h_seeds = nullptr;
    g->cap_h_seeds = 0;
    const size_t want = std::max<size_t>(n_words + n_words / 2, 4096);
    if (hipHostMalloc((void **)&g->h_seeds, want * 4, hipHostMallocDefault) != hipSuccess) return fail(HVX_ERR_DEVICE, "hipHostMalloc(%zu) seeds", want * 4);
    g->cap_h_seeds = want;
    return HVX_OK;
}

// a node bitmap (the Filter step's mask, repeat's `until` predicate) through its pinned staging buffer into its device buffer, on `s`
static inline int stage_bitmap(hvx_csr *g, hipStream_t s, const uint64_t *words, uint32_t **dev, uint32_t **pinned) {
    const size_t words32 = std::max<size_t>(((g->n + 63) / 64) * 2, 2), bytes = (size_t)((g->n + 63) / 64) * 8;
    int rc;
    if (!*dev && (rc = csr_alloc(g, (void **)dev, words32 * 4))) return rc;
    if (!*pinned && hipHostMalloc((void **)pinned, words32 * 4, hipHostMallocDefault) != hipSuccess)
        return fail(HVX_ERR_DEVICE, "hipHostMalloc(%zu) mask", words32 * 4);
    memcpy(*pinned, words, bytes);
    HIP_TRY(hipMemcpyAsync(*dev, *pinned, bytes, hipMemcpyHostToDevice, s));
    return HVX_OK;
}

// caller holds g->mu; the visited bitmap stays in g->visited (device) whether or not it is copied out (hvx_traverse.hip; the library
// does not export it)
__attribute__((visibility("hidden"))) int run_bfs_locked(hvx_csr *g, const uint64_t *seeds, uint32_t n_seeds, uint32_t max_depth, uint32_t direction, const uint32_t *labels,
                   uint32_t n_labels, uint32_t hub_degree, uint32_t include_seeds, bool expand_only, uint64_t *out_bitmap, uint32_t *out_depth,
                   hipStream_t consumer = nullptr);

// what both shortest-path batch calls and the host loop refuse about the plan the requests share (hvx_shortest_path.hip)
__attribute__((visibility("hidden"))) int shortest_path_plan_check(uint32_t max_depth, uint32_t direction, const uint32_t *allowed_label_ids, uint32_t n_labels);

// caller holds g->mu: the host mirror behind hvx_traverse_dfs is dropped (an edit changed the arrays); the next call fetches it again
__attribute__((visibility("hidden"))) void csr_drop_host_mirror(hvx_csr *g);

} // namespace hvx
