// hvx_csr_edit_plan.h -- the host plan of hvx_csr_apply_edges (hvx_csr_edit.hip): plain C++, no HIP, so the CPU tests compile it alone
// (tests/native/csr_edit_plan_probe.cpp).
//
// A batch of removals and additions is turned, for each adjacency (outgoing: row = src, neighbour = dst; incoming: row = dst,
// neighbour = src), into the list of rows it touches.  Every touched row gets its segment of the sorted removals, its segment of
// the sorted additions and the running sum of (additions - removals) of the touched rows below it.  The host therefore knows every
// row's change of degree without reading the graph: new_off[u] = old_off[u] + cum[number of touched rows below u].
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace hvx_edit {

struct SidePlan {
    std::vector<uint32_t> rows;              // [nt] touched rows, ascending
    std::vector<int64_t> cum;                // [nt + 1] cum[k] = sum of (adds - dels) over rows[0 .. k)
    std::vector<uint32_t> del_beg, add_beg;  // [nt + 1] row k owns del_*[del_beg[k] .. del_beg[k + 1]) and add_*[add_beg[k] .. add_beg[k + 1])
    std::vector<uint32_t> del_nbr, del_lab;  // removals sorted by (row, neighbour, label); del_lab empty for an unlabelled graph
    std::vector<uint32_t> add_nbr, add_lab;  // additions STABLY sorted by (row, neighbour): equal arcs keep batch order
};

struct EditPlan {
    SidePlan out, in;
};

// one adjacency's plan; `row` / `nbr` are the batch's endpoint arrays seen from that side
inline void plan_side(const uint64_t *del_row, const uint64_t *del_nbr, const uint32_t *del_lab, uint64_t n_del, const uint64_t *add_row,
                      const uint64_t *add_nbr, const uint32_t *add_lab, uint64_t n_add, SidePlan *p) {
    std::vector<uint32_t> dord(n_del), aord(n_add);
    std::iota(dord.begin(), dord.end(), 0u);
    std::iota(aord.begin(), aord.end(), 0u);
    std::stable_sort(dord.begin(), dord.end(), [&](uint32_t x, uint32_t y) {
        if (del_row[x] != del_row[y]) return del_row[x] < del_row[y];
        if (del_nbr[x] != del_nbr[y]) return del_nbr[x] < del_nbr[y];
        return del_lab && del_lab[x] < del_lab[y];
    });
    std::stable_sort(aord.begin(), aord.end(), [&](uint32_t x, uint32_t y) {
        if (add_row[x] != add_row[y]) return add_row[x] < add_row[y];
        return add_nbr[x] < add_nbr[y];
    });
    p->del_nbr.resize(n_del);
    p->add_nbr.resize(n_add);
    p->del_lab.resize(del_lab ? n_del : 0);
    p->add_lab.resize(add_lab ? n_add : 0);
    for (uint64_t i = 0; i < n_del; ++i) {
        p->del_nbr[i] = (uint32_t)del_nbr[dord[i]];
        if (del_lab) p->del_lab[i] = del_lab[dord[i]];
    }
    for (uint64_t i = 0; i < n_add; ++i) {
        p->add_nbr[i] = (uint32_t)add_nbr[aord[i]];
        if (add_lab) p->add_lab[i] = add_lab[aord[i]];
    }
    p->rows.clear();
    p->cum.assign(1, 0);
    p->del_beg.assign(1, 0);
    p->add_beg.assign(1, 0);
    uint64_t d = 0, a = 0;
    while (d < n_del || a < n_add) { // the next touched row: the smaller head of the two sorted lists
        const uint64_t rd = d < n_del ? del_row[dord[d]] : UINT64_MAX, ra = a < n_add ? add_row[aord[a]] : UINT64_MAX;
        const uint64_t row = std::min(rd, ra);
        const uint64_t d0 = d, a0 = a;
        while (d < n_del && del_row[dord[d]] == row) ++d;
        while (a < n_add && add_row[aord[a]] == row) ++a;
        p->rows.push_back((uint32_t)row);
        p->del_beg.push_back((uint32_t)d);
        p->add_beg.push_back((uint32_t)a);
        p->cum.push_back(p->cum.back() + (int64_t)(a - a0) - (int64_t)(d - d0));
    }
}

// 0, or 1 + the position of the first endpoint at or above n_nodes (removals first, then additions).  Labels: both arrays or neither.
inline uint64_t plan_edits(uint64_t n_nodes, const uint64_t *del_src, const uint64_t *del_dst, const uint32_t *del_lab, uint64_t n_del,
                           const uint64_t *add_src, const uint64_t *add_dst, const uint32_t *add_lab, uint64_t n_add, EditPlan *plan) {
    for (uint64_t i = 0; i < n_del; ++i)
        if (del_src[i] >= n_nodes || del_dst[i] >= n_nodes) return 1 + i;
    for (uint64_t i = 0; i < n_add; ++i)
        if (add_src[i] >= n_nodes || add_dst[i] >= n_nodes) return 1 + n_del + i;
    plan_side(del_src, del_dst, del_lab, n_del, add_src, add_dst, add_lab, n_add, &plan->out);
    plan_side(del_dst, del_src, del_lab, n_del, add_dst, add_src, add_lab, n_add, &plan->in);
    return 0;
}

} // namespace hvx_edit
