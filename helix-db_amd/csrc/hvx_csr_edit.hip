// hvx_csr_edit.hip -- batches of edge removals and additions applied to a live device graph (hvx_csr_apply_edges), and the two
// calls that show what a handle holds (hvx_csr_sizes, hvx_csr_export).
//
// Reference: crates/db/src/mutation/adjacency.rs:12-62 (add_adjacency / remove_adjacency: the host's adjacency rows change with
// every edge mutation); the arrays a batch leaves are those hvx_csr_import would build from the edited edge list.
//
// The host plan (hvx_csr_edit_plan.h) knows every row's change of degree without reading the graph, so per adjacency the device runs
//   offsets -- new_off[u] = old_off[u] + cum[touched rows below u], one thread per node (binary search over the touched rows), and
//              the largest new row by the way;
//   copy    -- the arcs of untouched rows move by the constant shift of their segment between two touched rows: a grid-stride,
//              coalesced copy with the segment found once per wavefront step;
//   rows    -- one wavefront per touched row: marks the arcs its removals hit (the LAST stored matches), places the survivors and
//              the additions;
// and the incoming-slot -> stored-edge map moves with the incoming copy (by the shift of the source's outgoing row) and is recomputed
// from the two new adjacencies for the arcs of touched rows only.  Kernel boundaries order the phases; the only
// atomics are the counter of removals without a stored arc and the two maxima.  Everything is written into the handle's spare set of
// arrays: the sets swap after the one host wait, when the counter is zero.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <vector>

#include "hvx_csr.h"
#include "hvx_csr_edit_plan.h"

using namespace hvx;

namespace {

// one adjacency's plan on the device (SidePlan)
struct EditSide {
    const long long *cum;
    const uint32_t *rows, *del_beg, *add_beg, *del_nbr, *del_lab, *add_nbr, *add_lab;
    uint32_t nt;
};

// one adjacency's arrays: the live ones (read) and the spare ones (written); `cap` = arcs the spare ones hold.  `arc` / `arc2`: the
// incoming side's slot -> stored-edge map (null on the outgoing side)
struct EditArrays {
    const uint64_t *off;
    const uint32_t *tgt, *lab, *arc;
    uint64_t *off2;
    uint32_t *tgt2, *lab2, *arc2;
    uint32_t n;
    uint64_t e, cap;
};

constexpr uint32_t kCopyBlocks = 2048; // x 4 wavefronts x kCopyUnroll x 64 arcs = 1 048 576 arcs per pass of the grid
constexpr uint32_t kCopyUnroll = 2;
constexpr uint32_t kRowBlocks = 1024;
constexpr uint32_t kFixupSplit = 32;  // wavefronts that share one touched row in edit_arc_fixup_kernel
constexpr uint32_t kFixupBlocks = 4096;

__device__ __forceinline__ uint64_t lower_bound_u32(const uint32_t *a, uint64_t lo, uint64_t hi, uint32_t v) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ uint64_t upper_bound_u32(const uint32_t *a, uint64_t lo, uint64_t hi, uint32_t v) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (a[mid] <= v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void edit_offsets_kernel(EditSide s, EditArrays a, uint32_t *max_deg) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    uint32_t deg = 0;
    if (i <= a.n) {
        const uint32_t k = (uint32_t)lower_bound_u32(s.rows, 0, s.nt, (uint32_t)i); // touched rows below i
        const uint64_t o = a.off[i] + (uint64_t)s.cum[k];
        a.off2[i] = o;
        if (i < a.n) {
            const uint32_t k1 = k + ((k < s.nt && s.rows[k] == (uint32_t)i) ? 1u : 0u);
            deg = (uint32_t)(a.off[i + 1] + (uint64_t)s.cum[k1] - o);
        }
    }
    for (int d = 32; d; d >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)deg, d);
        deg = o > deg ? o : deg;
    }
    if ((threadIdx.x & 63u) == 0 && deg) atomicMax(max_deg, deg);
}

// Arcs of untouched rows.  k = touched rows whose stored row starts at or below the arc; the arc lies inside row k - 1 (the rows
// kernel's) or behind all k of them, where every arc moves by cum[k].  On the incoming side the slot's stored-edge index moves too, by
// the shift of its SOURCE's outgoing row (`o` = the outgoing plan): right for every source whose own row is untouched, overwritten by
// edit_arc_fixup_kernel for the others.
__global__ __launch_bounds__(256) void edit_copy_kernel(EditSide s, EditArrays a, EditSide o) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t span = 64ull * kCopyUnroll, n_waves = (uint64_t)gridDim.x * 4u;
    for (uint64_t base = (((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6) * span; base < a.e; base += n_waves * span) {
        uint32_t t[kCopyUnroll], l[kCopyUnroll], x[kCopyUnroll];
#pragma unroll
        for (uint32_t j = 0; j < kCopyUnroll; ++j) {
            const uint64_t p = base + j * 64u + lane;
            t[j] = p < a.e ? a.tgt[p] : 0u;
            l[j] = (a.lab && p < a.e) ? a.lab[p] : 0u;
            x[j] = (a.arc && p < a.e) ? a.arc[p] : 0u;
        }
        uint32_t lo = 0, hi = s.nt; // the segment of the step's first arc: the same for the whole wavefront
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (a.off[s.rows[mid]] <= base) lo = mid + 1; else hi = mid;
        }
        uint32_t k = lo;
        // the usual step lies inside one untouched stretch -- no touched row starts in it, the one before ended at or below its first
        // arc -- and every lane takes the same shift without looking at the rows again
        const uint64_t last = (base + span < a.e ? base + span : a.e) - 1;
        const bool plain = (k == s.nt || a.off[s.rows[k]] > last) && (k == 0 || a.off[s.rows[k - 1] + 1] <= base);
#pragma unroll
        for (uint32_t j = 0; j < kCopyUnroll; ++j) {
            const uint64_t p = base + j * 64u + lane;
            if (p >= a.e) continue;
            if (!plain) {
                while (k < s.nt && a.off[s.rows[k]] <= p) ++k;
                if (k && p < a.off[s.rows[k - 1] + 1]) continue; // inside a touched row
            }
            const uint64_t d = p + (uint64_t)s.cum[k];
            if (d >= a.cap) continue; // (only a batch that is about to be refused: more removals than arcs in some row)
            a.tgt2[d] = t[j];
            if (a.lab) a.lab2[d] = l[j];
            if (a.arc) a.arc2[d] = x[j] + (uint32_t)o.cum[lower_bound_u32(o.rows, 0, o.nt, t[j])];
        }
    }
}

__device__ __forceinline__ bool same_key(const EditSide &s, uint32_t x, uint32_t y) {
    return s.del_nbr[x] == s.del_nbr[y] && (!s.del_lab || s.del_lab[x] == s.del_lab[y]);
}

// removals of the key (v, l) in [d0, d1): the list ascends by (neighbour, label)
__device__ __forceinline__ uint32_t removals_of(const EditSide &s, uint32_t d0, uint32_t d1, uint32_t v, uint32_t l) {
    uint32_t lo = d0, hi = d1;
    while (lo < hi) { // first entry >= (v, l)
        const uint32_t mid = (lo + hi) >> 1;
        const bool less = s.del_nbr[mid] < v || (s.del_nbr[mid] == v && s.del_lab && s.del_lab[mid] < l);
        if (less) lo = mid + 1; else hi = mid;
    }
    const uint32_t first = lo;
    hi = d1;
    while (lo < hi) { // first entry > (v, l)
        const uint32_t mid = (lo + hi) >> 1;
        const bool le = s.del_nbr[mid] < v || (s.del_nbr[mid] == v && (!s.del_lab || s.del_lab[mid] <= l));
        if (le) lo = mid + 1; else hi = mid;
    }
    return lo - first;
}

// One wavefront per touched row, lanes stride over the row (walk_heavy_rows' stride: a hub row with one new arc does not serialise).
__global__ __launch_bounds__(256) void edit_rows_kernel(EditSide s, EditArrays a, uint32_t *unmatched) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_waves = gridDim.x * 4u;
    for (uint32_t k = (blockIdx.x * 256u + threadIdx.x) >> 6; k < s.nt; k += n_waves) {
        const uint32_t row = s.rows[k];
        const uint64_t r0 = a.off[row], r1 = a.off[row + 1], n0 = a.off2[row];
        const uint32_t d0 = s.del_beg[k], d1 = s.del_beg[k + 1], a0 = s.add_beg[k], a1 = s.add_beg[k + 1];
        // every removed key needs as many stored arcs as it has removals
        for (uint32_t j = d0 + lane; j < d1; j += 64) {
            if (j > d0 && same_key(s, j - 1, j)) continue; // (the first removal of a key counts for all of them)
            uint32_t c = 1;
            while (j + c < d1 && same_key(s, j, j + c)) ++c;
            const uint32_t v = s.del_nbr[j], l = s.del_lab ? s.del_lab[j] : 0u;
            uint32_t m = 0;
            for (uint64_t p = lower_bound_u32(a.tgt, r0, r1, v); p < r1 && a.tgt[p] == v && m < c; ++p) m += (!a.lab || a.lab[p] == l) ? 1u : 0u;
            if (m < c) atomicAdd(unmatched, 1u);
        }
        // survivors: a key removed c times loses its LAST c stored arcs; a survivor lands behind the survivors before it and the
        // additions with a smaller neighbour
        uint64_t kept = 0;
        for (uint64_t base = r0; base < r1; base += 64) {
            const uint64_t p = base + lane;
            bool keep = false;
            uint32_t v = 0, l = 0;
            if (p < r1) {
                v = a.tgt[p];
                l = a.lab ? a.lab[p] : 0u;
                keep = true;
                const uint32_t c = d1 > d0 ? removals_of(s, d0, d1, v, l) : 0u;
                if (c) {
                    uint32_t later = 0; // equal arcs stored behind this one
                    for (uint64_t q = p + 1; q < r1 && a.tgt[q] == v && later < c; ++q) later += (!a.lab || a.lab[q] == l) ? 1u : 0u;
                    keep = later >= c;
                }
            }
            const unsigned long long m = __ballot(keep);
            if (keep) {
                const uint64_t pos = n0 + kept + (uint64_t)__popcll(m & ((1ull << lane) - 1ull)) + (lower_bound_u32(s.add_nbr, a0, a1, v) - a0);
                if (pos < a.cap) {
                    a.tgt2[pos] = v;
                    if (a.lab) a.lab2[pos] = l;
                }
            }
            kept += (uint64_t)__popcll(m);
        }
        // additions, in the plan's (stable) order: behind the survivors whose neighbour is not larger
        for (uint32_t j = a0 + lane; j < a1; j += 64) {
            const uint32_t v = s.add_nbr[j];
            const uint64_t stored_le = upper_bound_u32(a.tgt, r0, r1, v) - r0, removed_le = upper_bound_u32(s.del_nbr, d0, d1, v) - d0;
            const uint64_t pos = n0 + (j - a0) + stored_le - removed_le;
            if (pos < a.cap) {
                a.tgt2[pos] = v;
                if (a.lab) a.lab2[pos] = s.add_lab[j];
            }
        }
    }
}

// The stored-edge map where the copy's shift does not hold: the touched rows, over the NEW arrays of both adjacencies.  Every arc is
// independent here (two binary searches), so a row is shared by kFixupSplit wavefronts: a hub row of 200 000 arcs took 14 ms in one.  The
// arc u -> v in incoming slot s is the (s - first slot of u in v's row)-th of the arcs to v in u's outgoing row (outgoing rows ascend by
// target, incoming rows by (source, stored position)).  incoming == 1: the slots of a touched incoming row; 0: the arcs of a touched
// outgoing row, each written into its slot.  An arc both walks reach gets the same value twice.
__global__ __launch_bounds__(256) void edit_arc_fixup_kernel(EditSide s, uint32_t incoming, const uint64_t *out_off, const uint32_t *out_tgt,
                                                             const uint64_t *in_off, const uint32_t *in_tgt, uint32_t *in_arc, const uint32_t *unmatched) {
    if (*unmatched) return; // a refused batch: its offsets mean nothing
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_waves = (uint64_t)gridDim.x * 4u, n_items = (uint64_t)s.nt * kFixupSplit;
    const uint64_t *my_off = incoming ? in_off : out_off, *other_off = incoming ? out_off : in_off;
    const uint32_t *my_tgt = incoming ? in_tgt : out_tgt, *other_tgt = incoming ? out_tgt : in_tgt;
    for (uint64_t item = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; item < n_items; item += n_waves) {
        const uint32_t row = s.rows[item / kFixupSplit];
        const uint64_t r0 = my_off[row], r1 = my_off[row + 1];
        for (uint64_t p = r0 + (item % kFixupSplit) * 64u + lane; p < r1; p += 64ull * kFixupSplit) {
            const uint32_t nb = my_tgt[p];
            const uint64_t q = lower_bound_u32(other_tgt, other_off[nb], other_off[nb + 1], row) + (p - lower_bound_u32(my_tgt, r0, p, nb));
            if (incoming) in_arc[p] = (uint32_t)q; else in_arc[q] = (uint32_t)p;
        }
    }
}

// a device buffer of the handle replaced by a larger one (contents are not kept): `allocs` stays what hvx_csr_free releases
int edit_regrow(hvx_csr *g, void **p, size_t bytes) {
    void *nu = nullptr;
    if (bytes == 0) bytes = 16;
    hipError_t e = hipMalloc(&nu, bytes);
    if (e != hipSuccess) return fail(HVX_ERR_DEVICE, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    if (*p) {
        auto it = std::find(g->allocs.begin(), g->allocs.end(), *p);
        if (it != g->allocs.end()) g->allocs.erase(it);
        (void)hipFree(*p);
    }
    g->allocs.push_back(nu);
    *p = nu;
    return HVX_OK;
}

size_t align8(size_t x) { return (x + 7) & ~(size_t)7; }

size_t side_bytes(const hvx_edit::SidePlan &p) {
    return (p.cum.size()) * 8 + align8(p.rows.size() * 4) + 2 * align8(p.del_beg.size() * 4) + align8(p.del_nbr.size() * 4) + align8(p.del_lab.size() * 4) +
           align8(p.add_nbr.size() * 4) + align8(p.add_lab.size() * 4);
}

// the side's arrays into the pinned buffer at h + *at; the device view points into d at the same offsets
void side_pack(const hvx_edit::SidePlan &p, char *h, const char *d, size_t *at, EditSide *v) {
    auto put = [&](const void *src, size_t bytes) -> const void * {
        const char *dev = d + *at;
        if (bytes) memcpy(h + *at, src, bytes);
        *at += align8(bytes);
        return dev;
    };
    v->nt = (uint32_t)p.rows.size();
    v->cum = (const long long *)put(p.cum.data(), p.cum.size() * 8);
    v->rows = (const uint32_t *)put(p.rows.data(), p.rows.size() * 4);
    v->del_beg = (const uint32_t *)put(p.del_beg.data(), p.del_beg.size() * 4);
    v->add_beg = (const uint32_t *)put(p.add_beg.data(), p.add_beg.size() * 4);
    v->del_nbr = (const uint32_t *)put(p.del_nbr.data(), p.del_nbr.size() * 4);
    const void *dl = put(p.del_lab.data(), p.del_lab.size() * 4);
    v->del_lab = p.del_lab.empty() ? nullptr : (const uint32_t *)dl;
    v->add_nbr = (const uint32_t *)put(p.add_nbr.data(), p.add_nbr.size() * 4);
    const void *al = put(p.add_lab.data(), p.add_lab.size() * 4);
    v->add_lab = p.add_lab.empty() ? nullptr : (const uint32_t *)al;
}

constexpr size_t kReadback = 64; // the counters' read-back at the head of the pinned buffer

} // namespace

extern "C" int hvx_csr_apply_edges(hvx_csr *g, const uint64_t *del_src, const uint64_t *del_dst, const uint32_t *del_labels, uint64_t n_del,
                                   const uint64_t *add_src, const uint64_t *add_dst, const uint32_t *add_labels, uint64_t n_add) {
    if (!g) return fail(HVX_ERR_INVARIANT, "null graph");
    if (n_del == 0 && n_add == 0) return HVX_OK;
    if ((n_del && (!del_src || !del_dst)) || (n_add && (!add_src || !add_dst))) return fail(HVX_ERR_INVARIANT, "null argument");
    if (n_del >= (1ull << 31) || n_add >= (1ull << 31)) return fail(HVX_ERR_UNSUPPORTED, "a batch holds fewer than 2^31 removals and 2^31 additions");
    std::lock_guard<std::mutex> lock(g->mu);
    const bool labeled = g->out_lab != nullptr;
    if ((n_del && (del_labels != nullptr) != labeled) || (n_add && (add_labels != nullptr) != labeled))
        return fail(HVX_ERR_INVARIANT, labeled ? "the graph is labelled: every edit carries a label" : "the graph is unlabelled: edits carry no labels");
    if (!g->rows_sorted) return fail(HVX_ERR_UNSUPPORTED, "edits need outgoing rows sorted by target (model.rs:656-666)");
    if (n_del > g->e) return fail(HVX_ERR_INVARIANT, "%llu removals, the graph stores %llu arcs", (unsigned long long)n_del, (unsigned long long)g->e);
    const uint64_t e_new = g->e - n_del + n_add;
    if (g->e >= (1ull << 32) || e_new >= (1ull << 32) || !g->in_arc) return fail(HVX_ERR_UNSUPPORTED, "edited graphs hold fewer than 2^32 arcs");
    hvx_edit::EditPlan plan;
    const uint64_t bad = hvx_edit::plan_edits(g->n, del_src, del_dst, n_del ? del_labels : nullptr, n_del, add_src, add_dst, n_add ? add_labels : nullptr,
                                              n_add, &plan);
    if (bad) return fail(HVX_ERR_INVARIANT, "%s %llu names a node outside the graph's %u", bad <= n_del ? "removal" : "addition",
                         (unsigned long long)(bad <= n_del ? bad - 1 : bad - 1 - n_del), g->n);
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipStreamSynchronize(g->stream)); // nothing of an earlier call reads the spare set or the scratch this call may replace
    int rc;
    // the spare set: a refused batch (fewer stored arcs than removals) still writes at most old arcs + additions
    const uint64_t need = g->e + n_add;
    if (!g->out_off2) {
        if ((rc = csr_alloc(g, (void **)&g->out_off2, ((size_t)g->n + 1) * 8))) return rc;
        if ((rc = csr_alloc(g, (void **)&g->in_off2, ((size_t)g->n + 1) * 8))) return rc;
        if ((rc = csr_alloc(g, (void **)&g->edit_ctr, 16))) return rc;
    }
    if (!g->out_tgt2 || g->cap_arcs2 < need) {
        const uint64_t cap = std::max<uint64_t>(need + need / 2, 1024); // geometric: a steady stream of batches allocates nothing
        g->cap_arcs2 = 0;
        if ((rc = edit_regrow(g, (void **)&g->out_tgt2, cap * 4))) return rc;
        if ((rc = edit_regrow(g, (void **)&g->in_tgt2, cap * 4))) return rc;
        if ((rc = edit_regrow(g, (void **)&g->in_arc2, cap * 4))) return rc;
        if (labeled) {
            if ((rc = edit_regrow(g, (void **)&g->out_lab2, cap * 4))) return rc;
            if ((rc = edit_regrow(g, (void **)&g->in_lab2, cap * 4))) return rc;
        }
        g->cap_arcs2 = cap;
    }
    const size_t plan_bytes = side_bytes(plan.out) + side_bytes(plan.in);
    if (plan_bytes > g->cap_edit_plan) {
        const size_t cap = std::max<size_t>(plan_bytes * 2, 1 << 16);
        g->cap_edit_plan = 0;
        if ((rc = edit_regrow(g, &g->edit_plan, cap))) return rc;
        g->cap_edit_plan = cap;
    }
    if (kReadback + plan_bytes > g->cap_h_edit) {
        const size_t cap = kReadback + std::max<size_t>(plan_bytes * 2, 1 << 16);
        if (g->h_edit) (void)hipHostFree(g->h_edit);
        g->h_edit = nullptr;
        g->cap_h_edit = 0;
        if (hipHostMalloc(&g->h_edit, cap, hipHostMallocDefault) != hipSuccess) return fail(HVX_ERR_DEVICE, "hipHostMalloc(%zu) edit plan", cap);
        g->cap_h_edit = cap;
    }
    char *h_plan = (char *)g->h_edit + kReadback;
    EditSide so, si;
    size_t at = 0;
    side_pack(plan.out, h_plan, (const char *)g->edit_plan, &at, &so);
    side_pack(plan.in, h_plan, (const char *)g->edit_plan, &at, &si);
    hipStream_t s = g->stream;
    HIP_TRY(hipMemcpyAsync(g->edit_plan, h_plan, at, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(g->edit_ctr, 0, 16, s));
    const EditArrays ao{g->out_off, g->out_tgt, g->out_lab, nullptr, g->out_off2, g->out_tgt2, g->out_lab2, nullptr, g->n, g->e, g->cap_arcs2};
    const EditArrays ai{g->in_off, g->in_tgt, g->in_lab, g->in_arc, g->in_off2, g->in_tgt2, g->in_lab2, g->in_arc2, g->n, g->e, g->cap_arcs2};
    const uint32_t off_blocks = (uint32_t)(((uint64_t)g->n + 1 + 255) / 256);
    const uint64_t copy_waves = (g->e + 64ull * kCopyUnroll - 1) / (64ull * kCopyUnroll);
    const uint32_t copy_blocks = (uint32_t)std::min<uint64_t>((copy_waves + 3) / 4, kCopyBlocks);
    for (int side = 0; side < 2; ++side) {
        const EditSide &sd = side ? si : so;
        const EditArrays &ar = side ? ai : ao;
        hipLaunchKernelGGL(edit_offsets_kernel, dim3(off_blocks), dim3(256), 0, s, sd, ar, g->edit_ctr + 1 + side);
        if (copy_blocks) hipLaunchKernelGGL(edit_copy_kernel, dim3(copy_blocks), dim3(256), 0, s, sd, ar, so);
        hipLaunchKernelGGL(edit_rows_kernel, dim3(std::min<uint32_t>((sd.nt + 3) / 4, kRowBlocks)), dim3(256), 0, s, sd, ar, g->edit_ctr);
        HIP_TRY(hipGetLastError());
    }
    for (uint32_t incoming = 0; incoming < 2; ++incoming) {
        const EditSide &sd = incoming ? si : so;
        hipLaunchKernelGGL(edit_arc_fixup_kernel, dim3((uint32_t)std::min<uint64_t>(((uint64_t)sd.nt * kFixupSplit + 3) / 4, kFixupBlocks)), dim3(256), 0, s, sd, incoming, g->out_off2,
                           g->out_tgt2, g->in_off2, g->in_tgt2, g->in_arc2, g->edit_ctr);
        HIP_TRY(hipGetLastError());
    }
    uint32_t *ctr = (uint32_t *)g->h_edit;
    HIP_TRY(hipMemcpyAsync(ctr, g->edit_ctr, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (ctr[0]) return fail(HVX_ERR_INVARIANT, "%u removed edges have no stored arc left to match (absent, or removed more often than stored)", ctr[0]);
    // accepted: the spare set becomes the graph
    std::swap(g->out_off, g->out_off2);
    std::swap(g->in_off, g->in_off2);
    std::swap(g->out_tgt, g->out_tgt2);
    std::swap(g->in_tgt, g->in_tgt2);
    std::swap(g->out_lab, g->out_lab2);
    std::swap(g->in_lab, g->in_lab2);
    std::swap(g->in_arc, g->in_arc2);
    std::swap(g->cap_arcs, g->cap_arcs2);
    g->e = e_new;
    g->max_out_deg = ctr[1];
    g->max_in_deg = ctr[2];
    csr_drop_host_mirror(g); // hvx_traverse_dfs fetches it again on its next use
    if (g->pc_out && e_new > g->cap_pc) { // the ordered traversal's per-arc scratch
        const uint64_t cap = e_new + e_new / 2;
        if ((rc = edit_regrow(g, (void **)&g->pc_out, cap * 4))) return rc;
        if ((rc = edit_regrow(g, (void **)&g->pc_in, cap * 4))) return rc;
        g->cap_pc = cap;
    }
    return HVX_OK;
}

extern "C" int hvx_csr_sizes(const hvx_csr *g, uint64_t *n_nodes, uint64_t *n_edges, uint64_t *max_out_degree, uint64_t *max_in_degree,
                             uint32_t *rows_sorted) {
    if (!g) return fail(HVX_ERR_INVARIANT, "null graph");
    std::lock_guard<std::mutex> lock(const_cast<hvx_csr *>(g)->mu);
    if (n_nodes) *n_nodes = g->n;
    if (n_edges) *n_edges = g->e;
    if (max_out_degree) *max_out_degree = g->max_out_deg;
    if (max_in_degree) *max_in_degree = g->max_in_deg;
    if (rows_sorted) *rows_sorted = g->rows_sorted ? 1u : 0u;
    return HVX_OK;
}

extern "C" int hvx_csr_export(const hvx_csr *cg, uint64_t *out_offsets, uint64_t *out_targets, uint32_t *out_labels, uint64_t *in_offsets,
                              uint64_t *in_sources, uint32_t *in_labels, uint64_t *in_edge_index) {
    if (!cg) return fail(HVX_ERR_INVARIANT, "null graph");
    hvx_csr *g = const_cast<hvx_csr *>(cg);
    std::lock_guard<std::mutex> lock(g->mu);
    if ((out_labels || in_labels) && !g->out_lab) return fail(HVX_ERR_INVARIANT, "the graph is unlabelled");
    if (in_edge_index && !g->in_arc) return fail(HVX_ERR_UNSUPPORTED, "the stored-edge map exists below 2^32 edges");
    HIP_TRY(hipSetDevice(g->device));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (out_offsets) HIP_TRY(hipMemcpy(out_offsets, g->out_off, ((size_t)g->n + 1) * 8, hipMemcpyDeviceToHost));
    if (in_offsets) HIP_TRY(hipMemcpy(in_offsets, g->in_off, ((size_t)g->n + 1) * 8, hipMemcpyDeviceToHost));
    if (!g->e) return HVX_OK;
    if (out_labels) HIP_TRY(hipMemcpy(out_labels, g->out_lab, g->e * 4, hipMemcpyDeviceToHost));
    if (in_labels) HIP_TRY(hipMemcpy(in_labels, g->in_lab, g->e * 4, hipMemcpyDeviceToHost));
    std::vector<uint32_t> tmp(g->e);
    const struct { const uint32_t *dev; uint64_t *out; } wide[3] = {{g->out_tgt, out_targets}, {g->in_tgt, in_sources}, {g->in_arc, in_edge_index}};
    for (const auto &w : wide) { // stored as u32 on the device, u64 in the ABI (as hvx_csr_import takes them)
        if (!w.out) continue;
        HIP_TRY(hipMemcpy(tmp.data(), w.dev, g->e * 4, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < g->e; ++i) w.out[i] = tmp[i];
    }
    return HVX_OK;
}
