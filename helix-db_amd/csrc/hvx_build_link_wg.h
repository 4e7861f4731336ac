// hvx_build_link_wg.h -- build_link_wg_kernel, the link step of every batched build over degree limits up to 32, and its LDS layout.
// A header because the kernel is instantiated in two translation units: over f32 rows in hvx_build.hip (per metric and summation
// tree), over bf16 rows in hvx_build_bf16.hip.  Why two: tests/test_abi_and_host.py compiles hvx_build.hip to assembly and holds every
// build_link_wg_kernel it finds there -- exactly the four f32 instantiations -- to "no cache maintenance, <= 64 B of scratch"; the bf16
// instantiations are new kernels with their own record (profiles/bf16_build_kernel_meta.json) and stay out of that unit.
#pragma once
#include <hip/hip_runtime.h>

#include "hvx_build_plan.h"

namespace hvx {

// ---- step 3, batched mode: one 256-thread workgroup per LINK (new node q, layer, selected neighbour s) ----
// build_link_kernel walks a node's <= 32 links one after the other, and every prune inside it is a chain of ~100 dependent row
// gathers (select_diverse stages candidate i, then scores it against the kept rows eight at a time, stops at the first hit):
// 9.4 ms per 2 048-node batch, 70 % of the build (profiles/history/r02f).  In a batch the order in which links reach the graph is not
// defined anyway, so every link gets its own workgroup, and the prune is evaluated EAGERLY from LDS: the nc <= Mmax + 1 rows of
// the overflowing row and its owner's cross HBM once, and ALL pairwise distances among them (every pair independent of every
// other: 561 pairs for 33 + 1 rows, eight per wavefront step) are computed with the reference's summation order -- the
// distance is symmetric bit for bit (squares / products commute), so the pair set does not depend on the (score, id) order that
// select_diverse walks.  The rows pass through LDS in COLUMN blocks of <= 256 floats: a pair's four AVX-lane accumulators are
// carried in registers from block to block (each lane's fma chain runs over the depth in the same order as in one pass), the
// next block is in flight in registers while this one is being used, and a workgroup holds ~46 KB of LDS: three per CU, so
// the lock / row / store latencies of one link sit under the arithmetic of the others.  Then: owner distances -> Candidate order
// (model.rs:55-61), P[i] bit j = D[c_i][c_j] < D[c_i][owner] (the test of mod.rs:832), and select_diverse + backfill
// (mod.rs:809-856) is a walk over 64-bit masks: candidate i is diverse iff P[i] & kept == 0.  Same decisions as the lazy
// evaluation, bit for bit.
constexpr int kLinkTasks = 18; // wave-steps of 8 pairs per wavefront: 4 x 18 x 8 >= 561 pairs of 33 candidates + owner
// (kLinkPre / kLinkPreBf16, link_pairs_max and link_lds_bytes: hvx_build_plan.h, next to the predicate that decides where the kernel serves)

struct LinkLds {
    float *rows;              // [ncmax + 1][ldp]: this column block of the candidate rows (row order of the neighbour row), then the owner's
    float *D;                 // [ncmax + 1][ncmax + 1] pairwise distances (index nc = the owner)
    uint32_t *cand;           // [64] ids in row order
    uint32_t *cid;            // [64] ids sorted by (distance to the owner, id)
    float *csc;               // [64] their distances
    uint32_t *srow;           // [64] row index of sorted candidate r
    unsigned long long *P;    // [64] predicate masks, sorted order
    uint32_t *fin;            // [64] ids of the pruned row
    uint32_t *sh;             // [8] nc, prune, present, overflow
    unsigned char *pa, *pb;   // [pairs] the two rows of pair p
};
__device__ __forceinline__ LinkLds carve_link(char *smem, uint32_t ldp, uint32_t ncmax) {
    LinkLds L;
    L.rows = reinterpret_cast<float *>(smem);
    char *p = smem + (size_t)(ncmax + 1u) * ldp * 4u;
    L.P = reinterpret_cast<unsigned long long *>(p); p += 512;
    L.D = reinterpret_cast<float *>(p); p += (size_t)(ncmax + 1u) * (ncmax + 1u) * 4u;
    L.cand = reinterpret_cast<uint32_t *>(p); p += 256;
    L.cid = reinterpret_cast<uint32_t *>(p); p += 256;
    L.csc = reinterpret_cast<float *>(p); p += 256;
    L.srow = reinterpret_cast<uint32_t *>(p); p += 256;
    L.fin = reinterpret_cast<uint32_t *>(p); p += 256;
    L.sh = reinterpret_cast<uint32_t *>(p); p += 32;
    L.pa = reinterpret_cast<unsigned char *>(p); p += (link_pairs_max(ncmax) + 15u) & ~(size_t)15u;
    L.pb = reinterpret_cast<unsigned char *>(p);
    return L;
}

template <uint32_t METRIC, bool FUSED, bool BF> __global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void build_link_wg_kernel(BuildArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const DevIndex &ix = a.ix;
    const uint32_t q = blockIdx.x >> 5, s = blockIdx.x & 31u, layer = blockIdx.y;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6, grp = lane >> 3, j = lane & 7;
    const uint32_t me = a.nodes[q];
    const uint32_t lv = ix.level[me];
    const uint32_t top = lv < a.layers - 1u ? lv : a.layers - 1u;
    if (layer > top) return;
    const size_t slot = (size_t)layer * a.b + q;
    if (s >= a.sel_cnt[slot]) return;
    const uint32_t to = a.sel[slot * 32u + s];
    const uint32_t maxn = layer == 0u ? a.m0 : a.m;
    LinkLds L = carve_link(smem, a.ldp, a.ncmax);
    uint32_t stride;
    uint32_t *row = row_ptr(a, to, layer, stride);

    // ---- add_bidirectional_link(from = me, to) (mutation.rs:1498-1583): append under the row owner's lock ----
    if (wave == 0) {
#ifdef HVX_TUNING
        if (a.dbg && lane == 0) { // contention probe: how often the target's lock is found taken
            uint32_t spins = 0;
            while (__hip_atomic_load(&a.locks[to], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u && spins < 1000000u) { ++spins; __builtin_amdgcn_s_sleep(2); }
            atomicAdd(&a.dbg[0], spins);
        }
#endif
        lock_row_w(a.locks, to, lane);
        uint32_t v = (uint32_t)lane < stride ? ld_row(row + lane) : kSentinel;
        uint32_t deg = (uint32_t)__builtin_popcountll(__ballot(v != kSentinel));
        const bool present = __ballot(v == me) != 0ull;
        bool overflow = false;
        if (!present) {
            if (deg >= 64u) overflow = true;
            else {
                if ((uint32_t)lane == deg) v = me; // rows are canonical: the valid ids occupy lanes 0..deg-1
                ++deg;
            }
        }
        if (deg > maxn && deg > a.ncmax) overflow = true; // more rows than the LDS was sized for: cannot happen on rows this build wrote
        L.cand[lane] = v;
        if (lane == 0) {
            L.sh[0] = deg;
            L.sh[1] = (deg > maxn && !overflow) ? 1u : 0u;
            L.sh[2] = present ? 1u : 0u;
            L.sh[3] = overflow ? 1u : 0u;
            if (overflow) *a.err = 1u;
        }
    }
    __syncthreads();
    const uint32_t nc = L.sh[0];
    if (L.sh[1] == 0u) { // no prune: the appended id takes its place in the canonical row
        if (wave == 0) {
            if (L.sh[2] == 0u && L.sh[3] == 0u) store_canonical_w(row, stride, L.cand, nc, lane);
            unlock_row_w(a.locks, to, lane);
            if (lane == 0) HVX_DBG_ADD(a, 3, 1);
        }
        return;
    }

    // ---- all pairwise distances among the nc candidate rows and the owner's row (index nc) ----
    const uint32_t nrows = nc + 1u, npairs = nrows * nc / 2u;
    if ((uint32_t)tid >= 1u && (uint32_t)tid < nrows) { // pair p = b (b - 1) / 2 + a  <->  rows a < b
        const uint32_t b = (uint32_t)tid, base = b * (b - 1u) / 2u;
        for (uint32_t aa = 0; aa < b; ++aa) { L.pa[base + aa] = (unsigned char)aa; L.pb[base + aa] = (unsigned char)b; }
    }
    const uint32_t nk = ix.dim_main >> 5;                 // 32-float chunks of a row (dim == dim_main == ld: the host checked)
    const uint32_t ck = a.link_ck;                        // chunks per column block (even)
    const uint32_t nblocks = (nk + ck - 1u) / ck;
    // bf16 rows (BF) cross HBM as 16-byte pieces of EIGHT values -- a lane's four virtual lanes of two consecutive chunks (hvx_device.h) --
    // and are widened (exact) on their way into LDS, where the block lies in plain order as an f32 block does: half the bytes, half
    // the registers in flight, and the pair loop below reads the same floats in the same order as group_distance_bf16
    const uint32_t w4 = BF ? ck * 4u : ck * 8u;           // 16-byte pieces per row and block
    constexpr int kPre = BF ? kLinkPreBf16 : kLinkPre;    // pieces a thread carries for the next block: 34 rows x 64 (32) pieces / 256 threads
    float4 pre[kPre];
#pragma unroll
    for (int u = 0; u < kPre; ++u) pre[u] = make_float4(0.f, 0.f, 0.f, 0.f);
    auto prefetch = [&](uint32_t blk) __attribute__((always_inline)) {
        const uint32_t c0 = blk * w4, cw = (nk - blk * ck < ck ? nk - blk * ck : ck) * (BF ? 4u : 8u);
#pragma unroll
        for (int u = 0; u < kPre; ++u) {
            const uint32_t e = (uint32_t)tid + 256u * (uint32_t)u;
            if constexpr (BF) {
                const Bf16BlockPiece pc = bf16_block_piece(e, blk, ck);
                if (pc.row < nrows && pc.col < cw) {
                    const uint32_t node = pc.row < nc ? L.cand[pc.row] : to;
                    pre[u] = reinterpret_cast<const float4 *>(ix.vecb + (size_t)node * ix.dim)[pc.src];
                }
            } else {
                const uint32_t r = e / w4, c = e - r * w4;
                if (r < nrows && c < cw) {
                    const uint32_t node = r < nc ? L.cand[r] : to;
                    pre[u] = reinterpret_cast<const float4 *>(ix.vec + (size_t)node * ix.ld)[c0 + c];
                }
            }
        }
    };
    auto commit = [&](uint32_t blk) __attribute__((always_inline)) {
        const uint32_t cw = (nk - blk * ck < ck ? nk - blk * ck : ck) * (BF ? 4u : 8u);
#pragma unroll
        for (int u = 0; u < kPre; ++u) {
            const uint32_t e = (uint32_t)tid + 256u * (uint32_t)u;
            if constexpr (BF) {
                const Bf16BlockPiece pc = bf16_block_piece(e, blk, ck);
                if (pc.row < nrows && pc.col < cw) {
                    const uint32_t w[4] = {__float_as_uint(pre[u].x), __float_as_uint(pre[u].y), __float_as_uint(pre[u].z), __float_as_uint(pre[u].w)};
                    float lo[4], hi[4];
                    bf16_piece_widen(w, lo, hi);
                    float *dst = L.rows + (size_t)pc.row * a.ldp + pc.dst;
                    *reinterpret_cast<float4 *>(dst) = make_float4(lo[0], lo[1], lo[2], lo[3]);
                    *reinterpret_cast<float4 *>(dst + 32) = make_float4(hi[0], hi[1], hi[2], hi[3]);
                }
            } else {
                const uint32_t r = e / w4, c = e - r * w4;
                if (r < nrows && c < cw) reinterpret_cast<float4 *>(L.rows + (size_t)r * a.ldp)[c] = pre[u];
            }
        }
    };
    float4 acc[kLinkTasks];
#pragma unroll
    for (int t = 0; t < kLinkTasks; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int slot4 = chunk_slot(j);
    prefetch(0);
    if (tid < 64) L.P[tid] = 0ull;
    for (uint32_t blk = 0; blk < nblocks; ++blk) {
        commit(blk);
        __syncthreads(); // block blk is in LDS (first round: and the pair table)
        if (blk + 1u < nblocks) prefetch(blk + 1u); // in flight underneath the arithmetic
        const uint32_t ckb = nk - blk * ck < ck ? nk - blk * ck : ck;
#pragma unroll
        for (int t = 0; t < kLinkTasks; ++t) {
            const uint32_t p = ((uint32_t)wave + 4u * (uint32_t)t) * 8u + (uint32_t)grp;
            if (((uint32_t)wave + 4u * (uint32_t)t) * 8u >= npairs) continue; // uniform in the wavefront
            const uint32_t pp = p < npairs ? p : npairs - 1u;
            const float4 *qp = reinterpret_cast<const float4 *>(L.rows + (size_t)L.pa[pp] * a.ldp) + slot4;
            const float4 *rp = reinterpret_cast<const float4 *>(L.rows + (size_t)L.pb[pp] * a.ldp) + slot4;
            float4 ac = acc[t];
#pragma unroll 4
            for (uint32_t k = 0; k < ckb; ++k) {
                const float4 x = rp[k * 8u];
                const float4 qq = qp[k * 8u];
                if (METRIC == kL2) {
                    const float d0 = qq.x - x.x, d1 = qq.y - x.y, d2 = qq.z - x.z, d3 = qq.w - x.w;
                    if (FUSED) {
                        ac.x = __builtin_fmaf(d0, d0, ac.x); ac.y = __builtin_fmaf(d1, d1, ac.y);
                        ac.z = __builtin_fmaf(d2, d2, ac.z); ac.w = __builtin_fmaf(d3, d3, ac.w);
                    } else {
                        ac.x = d0 * d0 + ac.x; ac.y = d1 * d1 + ac.y;
                        ac.z = d2 * d2 + ac.z; ac.w = d3 * d3 + ac.w;
                    }
                } else {
                    if (FUSED) {
                        ac.x = __builtin_fmaf(qq.x, x.x, ac.x); ac.y = __builtin_fmaf(qq.y, x.y, ac.y);
                        ac.z = __builtin_fmaf(qq.z, x.z, ac.z); ac.w = __builtin_fmaf(qq.w, x.w, ac.w);
                    } else {
                        ac.x = qq.x * x.x + ac.x; ac.y = qq.y * x.y + ac.y;
                        ac.z = qq.z * x.z + ac.z; ac.w = qq.w * x.w + ac.w;
                    }
                }
            }
            acc[t] = ac;
        }
        __syncthreads(); // everybody is done with block blk before the next one overwrites it
    }
#pragma unroll
    for (int t = 0; t < kLinkTasks; ++t) {
        const uint32_t p = ((uint32_t)wave + 4u * (uint32_t)t) * 8u + (uint32_t)grp;
        if (((uint32_t)wave + 4u * (uint32_t)t) * 8u >= npairs) continue;
        float r = avx_tree_reduce(acc[t]); // every lane of the group takes part
        if (p < npairs) {
            const uint32_t ra = L.pa[p], rb = L.pb[p];
            if (METRIC == kCosine) {
                const uint32_t na = ra < nc ? L.cand[ra] : to, nb = rb < nc ? L.cand[rb] : to;
                if constexpr (BF) {
                    const uint16_t *va = ix.vecb + (size_t)na * ix.dim, *vb = ix.vecb + (size_t)nb * ix.dim;
                    r = cosine_finish_fn(r, ix.hdr[na], ix.hdr[nb], [&]() {
                        return stable_half_cosine_fn(ix.dim, [&](uint32_t i) { return bf16_to_f32(va[bf16_slot_of(i)]); }, [&](uint32_t i) { return bf16_to_f32(vb[bf16_slot_of(i)]); });
                    });
                } else {
                    r = cosine_finish(r, ix.hdr[na], ix.hdr[nb], ix.vec + (size_t)na * ix.ld, ix.vec + (size_t)nb * ix.ld, ix.dim);
                }
            }
            if (j == 0) { L.D[ra * nrows + rb] = r; L.D[rb * nrows + ra] = r; }
        }
    }
    __syncthreads();

    // ---- rank the row's neighbours by distance to its owner (Candidate order: score, then id; model.rs:55-61) ----
    if ((uint32_t)tid < nc) {
        const float dmine = L.D[nc * nrows + (uint32_t)tid];
        const uint32_t v = L.cand[tid];
        uint32_t rank = 0;
        for (uint32_t t = 0; t < nc; ++t) {
            const float dt = L.D[nc * nrows + t];
            const uint32_t it = L.cand[t];
            rank += (dt < dmine || (dt == dmine && it < v)) ? 1u : 0u;
        }
        L.cid[rank] = v;
        L.csc[rank] = dmine;
        L.srow[rank] = (uint32_t)tid;
    }
    __syncthreads();
    if (wave != 0) return;
    // ---- P[i] bit jj = dist(c_i, c_jj) < dist(c_i, owner), jj < i in sorted order (strict <: mod.rs:832) ----
    if ((uint32_t)lane < nc) {
        const uint32_t ri = L.srow[lane];
        const float si = L.csc[lane];
        unsigned long long bits = 0ull;
        for (uint32_t jj = 0; jj < (uint32_t)lane; ++jj)
            if (L.D[ri * nrows + L.srow[jj]] < si) bits |= 1ull << jj;
        L.P[lane] = bits;
    }
    wave_sync();

    // ---- select_diverse + backfill over the masks (mod.rs:809-856); all lanes walk the same chain ----
    unsigned long long kept = 0ull;
    uint32_t ns = 0;
    for (uint32_t i = 0; i < nc && ns < maxn; ++i)
        if ((L.P[i] & kept) == 0ull) { kept |= 1ull << i; ++ns; }
    for (uint32_t i = 0; i < nc && ns < maxn; ++i)
        if (((kept >> i) & 1ull) == 0ull) { kept |= 1ull << i; ++ns; }
    const bool have = (uint32_t)lane < nc;
    const uint32_t mine = have ? L.cid[lane] : kSentinel;
    const bool in = have && ((kept >> lane) & 1ull) != 0ull;
    const unsigned long long im = __ballot(in);
    if (in) L.fin[__builtin_popcountll(im & ((1ull << lane) - 1ull))] = mine;
    const uint32_t dropped_id = (have && !in) ? mine : kSentinel;
    wave_sync();
    store_canonical_w(row, stride, L.fin, ns, lane);
    unlock_row_w(a.locks, to, lane);
    // every neighbour dropped by the prune loses its edge to `to` as well (mutation.rs:1890-1908): the graph stays symmetric
    unsigned long long dm = __ballot(dropped_id != kSentinel);
    while (dm) {
        const uint32_t src = (uint32_t)__builtin_ctzll(dm);
        dm &= dm - 1ull;
        const uint32_t x = __builtin_amdgcn_readlane(dropped_id, src);
        remove_edge_w(a, layer, x, to, lane);
        if (lane == 0) HVX_DBG_ADD(a, 2, 1);
    }
    if (lane == 0) HVX_DBG_ADD(a, 1, 1);
}

} // namespace hvx
