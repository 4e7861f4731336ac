// hvx_shortest_path_host.h -- shortest_path (crates/db/src/execution/interpreter/shortest_path.rs:16-96, neighbours :143-214) on the host,
// over caller-held CSR arrays: the LITERAL loop of the reference -- queue, visited set, predecessor map, a node's neighbours as the sorted
// set of its distinct allowed neighbours, stop at the arc that discovers the target, predecessor chain reversed.  The device kernel
// (hvx_shortest_path.hip) computes the same path another way (levels from the target, then the smallest neighbour one level closer), so
// that the two agreeing means something.  No HIP in here: tests/native/shortest_path_host_probe.cpp compiles this header alone.
#pragma once
#include <algorithm>
#include <cstdint>
#include <deque>
#include <map>
#include <set>
#include <vector>

namespace hvx_sp {

enum : uint32_t { kDirOut = 0, kDirIn = 1, kDirBoth = 2 }; // = HVX_DIR_*

// The outgoing arrays are the caller's; the incoming adjacency is built from them once (build_incoming), as hvx_traverse_host does.
struct HostGraph {
    uint64_t n = 0;
    const uint64_t *out_off = nullptr, *out_tgt = nullptr;
    const uint32_t *out_lab = nullptr; // null: unlabeled, every arc passes
    std::vector<uint64_t> in_off, in_src;
    std::vector<uint32_t> in_lab;
};

// 0, or 1 + the index of the first arc whose target is not a node / whose offsets descend (the caller refuses the graph)
inline uint64_t build_incoming(uint64_t n_nodes, uint64_t n_edges, const uint64_t *out_offsets, const uint64_t *out_targets, const uint32_t *edge_labels,
                               HostGraph *g) {
    g->n = n_nodes;
    g->out_off = out_offsets;
    g->out_tgt = out_targets;
    g->out_lab = edge_labels;
    if (out_offsets[0] != 0 || out_offsets[n_nodes] != n_edges) return 1;
    for (uint64_t u = 0; u < n_nodes; ++u)
        if (out_offsets[u + 1] < out_offsets[u] || out_offsets[u + 1] > n_edges) return 1 + out_offsets[u];
    g->in_off.assign(n_nodes + 1, 0);
    for (uint64_t a = 0; a < n_edges; ++a) {
        if (out_targets[a] >= n_nodes) return 1 + a;
        ++g->in_off[out_targets[a] + 1];
    }
    for (uint64_t v = 0; v < n_nodes; ++v) g->in_off[v + 1] += g->in_off[v];
    g->in_src.resize(n_edges);
    if (edge_labels) g->in_lab.resize(n_edges);
    std::vector<uint64_t> cur(g->in_off.begin(), g->in_off.end() - 1);
    for (uint64_t u = 0; u < n_nodes; ++u)
        for (uint64_t a = out_offsets[u]; a < out_offsets[u + 1]; ++a) {
            const uint64_t slot = cur[out_targets[a]]++;
            g->in_src[slot] = u;
            if (edge_labels) g->in_lab[slot] = edge_labels[a];
        }
    return 0;
}

// shortest_path_neighbors: the BTreeSet of the allowed neighbours in `direction` (n_labels == 0: every label)
inline void neighbors(const HostGraph &g, uint64_t node, uint32_t direction, const uint32_t *allowed, uint32_t n_labels, std::set<uint64_t> *out) {
    out->clear();
    auto ok = [&](const uint32_t *lab, uint64_t a) {
        if (!lab || n_labels == 0) return true;
        return std::find(allowed, allowed + n_labels, lab[a]) != allowed + n_labels;
    };
    if (direction == kDirOut || direction == kDirBoth)
        for (uint64_t a = g.out_off[node]; a < g.out_off[node + 1]; ++a)
            if (ok(g.out_lab, a)) out->insert(g.out_tgt[a]);
    if (direction == kDirIn || direction == kDirBoth)
        for (uint64_t a = g.in_off[node]; a < g.in_off[node + 1]; ++a)
            if (ok(g.out_lab ? g.in_lab.data() : nullptr, a)) out->insert(g.in_src[a]);
}

// execute_shortest_path for resolved endpoints (both < g.n): the path source first, empty when none has at most max_depth arcs
inline std::vector<uint64_t> shortest_path(const HostGraph &g, uint64_t source, uint64_t target, uint32_t max_depth, uint32_t direction,
                                           const uint32_t *allowed, uint32_t n_labels) {
    if (source == target) return {source};
    std::deque<uint64_t> queue{source};
    std::set<uint64_t> visited{source}, nbrs;
    std::map<uint64_t, uint64_t> predecessor;
    bool found = false;
    for (uint32_t depth = 0; depth < max_depth && !found; ++depth) {
        const size_t level_len = queue.size();
        if (level_len == 0) break;
        for (size_t i = 0; i < level_len && !found; ++i) {
            const uint64_t current = queue.front();
            queue.pop_front();
            neighbors(g, current, direction, allowed, n_labels, &nbrs);
            for (uint64_t nb : nbrs) {
                if (!visited.insert(nb).second) continue;
                predecessor[nb] = current;
                if (nb == target) {
                    found = true;
                    break;
                }
                queue.push_back(nb);
            }
        }
    }
    if (!found) return {};
    std::vector<uint64_t> path{target};
    for (uint64_t current = target; current != source;) {
        current = predecessor.at(current);
        path.push_back(current);
    }
    std::reverse(path.begin(), path.end());
    return path;
}

} // namespace hvx_sp
