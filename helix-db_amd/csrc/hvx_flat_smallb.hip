// hvx_flat_smallb.hip -- candidate generation of the exact scan for SMALL query batches (b <= 128) in ONE pass over the rows.
//
// Where it sits: restricted_exact_scan (crates/db/src/search/vector/restricted.rs:753-835) over a prefiltered candidate set
// is the common shape of BASELINE config #3: a handful of queries (the benchmark issues them one at a time; 32 share a
// batch here) against 10^3..10^6 candidate rows.  With so few queries the scan is a pure stream: every candidate row has
// to cross HBM once and nothing else is big.  The 128 x 128 / 256 x 256 contraction kernels are built for large batches:
// they pad the batch to their query tile, stage both operands through LDS behind barriers, and the filtered pipeline
// around them needs 8-10 launches -- 0.10 of the HBM roofline on the 100 000-candidate group.
//
// Two builds of the candidate kernel (launch_flat_smallb picks): the LDS-RING build further down (round 4, batches of <= 32 queries:
// rows through per-wavefront rings of whole 128-byte lines, queries in registers) and the REGISTER-FRAGMENT build (round 3, up to
// 128 queries and every shape the ring build does not serve), followed by the sort-free selection both share.
//
// The register-fragment build: one wavefront owns 32 candidate rows at a time and keeps them in REGISTERS -- lane l reads 8 consecutive
// stored elements of row (l & 31), depth half (l >> 5), which is exactly the B-operand layout of v_mfma_f32_32x32x16_bf16
// (f32 rows are rounded to bf16 in registers: the one-pass contraction's rounding, covered by the certificate's bound);
// the queries (bf16 hi parts, <= 4 tiles of 32) sit in LDS once per workgroup, padded so that the A-operand
// ds_read_b128 is conflict-free.  No barrier after the query tile is staged, no LDS traffic for the rows, the next group
// of row loads is issued before the current group's MFMAs.  16 wavefronts per CU x 8-16 KB in flight each.  The epilogue
// writes the [b][candidates] score matrix (b x 4 bytes per row against dim x 4 bytes read: 2 % at b = 32, dim = 1536).
// Selection (flat_select_radix_kernel below: four 8-bit radix rounds per 4 096-score slice), exact re-rank and certificate follow.
// Algorithmic bytes per launch = candidates x dim x sizeof(row element).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hvx_device.h"
#include "hvx_flat_mfma.h"

namespace hvx {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;

// two f32 -> two bf16 (RNE) in one v_cvt_pk_bf16_f32
__device__ __forceinline__ uint32_t pack_bf16(float lo, float hi) {
    const f32x2 f = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2));
}

// KIND 0: bf16 rows (a bf16 index, or the bf16 shadow of an f32 index), 2: f32 rows.  NQT: 32-query tiles held in LDS.
// FULL: the hi + lo split (acc += q_hi.x_hi + q_lo.x_hi [+ q_hi.x_lo for f32 rows]; the dropped lo.lo term is covered by the
// certificate's bound) -- false = the one-pass build (q_hi.x_hi only, scan_error_bound (hvx_flat_mfma.h) widens the bound).
// WAVES: wavefronts per workgroup = per CU (the query tiles fill most of the LDS).  U: MFMA steps (16 deep) per register group.
// Output = the raw dot products [b][rows] in a.dist (the selection kernel below turns them into scores).  The query tiles of
// one workgroup must fit the LDS: when they do not (dim 1536 with the lo tile) the depth is split over gridDim.y workgroup
// rows, each streaming its depth range [k0, k0 + klen) of every row -- still one pass over the bytes -- and the partial
// dot products meet in a.dist by float atomic add (two or three addends onto a zeroed word: order-independent).
template <int KIND, int NQT, int WAVES, int U, bool FULL>
__global__ __launch_bounds__(WAVES * 64) void flat_smallb_kernel(MfmaArgs a, uint32_t n_blocks, uint32_t lds_stride, uint32_t klen) {
    const uint32_t k0 = blockIdx.y * klen;
    const bool accumulate = gridDim.y > 1;
    extern __shared__ __attribute__((aligned(16))) unsigned char qlds[];
    constexpr bool F32 = KIND == 2;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t fr = lane & 31u, half = lane >> 5;
    // the query tile(s) of this depth range: [NQT * 32][klen] bf16 hi (then lo), rows padded by 16 bytes
    unsigned char *qlo_lds = qlds + (size_t)NQT * 32u * lds_stride;
    const uint32_t vec_per_row = klen / 8u;
    for (uint32_t i = tid; i < (uint32_t)NQT * 32u * vec_per_row; i += WAVES * 64) {
        const uint32_t r = i / vec_per_row, c = i - r * vec_per_row;
        *reinterpret_cast<uint4 *>(qlds + (size_t)r * lds_stride + c * 16u) = *reinterpret_cast<const uint4 *>(a.qhi + (size_t)r * a.dim + k0 + c * 8u);
        if (FULL)
            *reinterpret_cast<uint4 *>(qlo_lds + (size_t)r * lds_stride + c * 16u) = *reinterpret_cast<const uint4 *>(a.qlo + (size_t)r * a.dim + k0 + c * 8u);
    }
    __syncthreads();
    const unsigned char *qa = qlds + (size_t)fr * lds_stride + half * 16u; // this lane's A fragment of tile 0, step 0
    const unsigned char *qal = qlo_lds + (size_t)fr * lds_stride + half * 16u;
    const uint32_t ngroups = klen / (16u * U);
    struct Group {
        uint4 v[U][F32 ? 2 : 1];
    };
    for (uint32_t blk = blockIdx.x * WAVES + wave; blk < n_blocks; blk += gridDim.x * WAVES) {
        const uint32_t rloc = blk * 32u + fr;
        const uint32_t rcl = rloc < a.nrows ? rloc : a.nrows - 1u; // the ragged tail re-reads the last row; masked below
        const size_t node = a.subset ? a.subset[a.row0 + rcl] : a.row0 + rcl;
        const unsigned char *rp = reinterpret_cast<const unsigned char *>(a.rows) + (node * a.dim + k0) * (F32 ? 4u : 2u) + half * (F32 ? 32u : 16u);
        auto load_group = [&](Group &g, uint32_t grp) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const unsigned char *p = rp + (size_t)(grp * U + u) * (F32 ? 64u : 32u);
                g.v[u][0] = *reinterpret_cast<const uint4 *>(p);
                if (F32) g.v[u][F32 ? 1 : 0] = *reinterpret_cast<const uint4 *>(p + 16);
            }
        };
        f32x16 acc[NQT];
#pragma unroll
        for (int t = 0; t < NQT; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[t][e] = 0.f;
        auto compute_group = [&](const Group &g, uint32_t grp) __attribute__((always_inline)) {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                uint4 bw, bl = make_uint4(0, 0, 0, 0);
                if (F32) {
                    float x[8];
                    const uint4 x0 = g.v[u][0], x1 = g.v[u][F32 ? 1 : 0];
                    x[0] = __uint_as_float(x0.x); x[1] = __uint_as_float(x0.y); x[2] = __uint_as_float(x0.z); x[3] = __uint_as_float(x0.w);
                    x[4] = __uint_as_float(x1.x); x[5] = __uint_as_float(x1.y); x[6] = __uint_as_float(x1.z); x[7] = __uint_as_float(x1.w);
                    uint32_t h[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) h[i] = pack_bf16(x[2 * i], x[2 * i + 1]);
                    bw = make_uint4(h[0], h[1], h[2], h[3]);
                    if (FULL) { // residuals x - bf16(x), rounded to bf16 again
                        uint32_t l[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            l[i] = pack_bf16(x[2 * i] - __uint_as_float(h[i] << 16), x[2 * i + 1] - __uint_as_float(h[i] & 0xFFFF0000u));
                        bl = make_uint4(l[0], l[1], l[2], l[3]);
                    }
                } else {
                    bw = g.v[u][0];
                }
                const bf16x8 fb = __builtin_bit_cast(bf16x8, bw);
                const bf16x8 fbl = __builtin_bit_cast(bf16x8, bl);
                const uint32_t koff = (grp * U + (uint32_t)u) * 32u; // bytes of bf16 depth before this step
#pragma unroll
                for (int t = 0; t < NQT; ++t) {
                    const bf16x8 fa = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(qa + (size_t)t * 32u * lds_stride + koff));
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[t], 0, 0, 0);
                    if (FULL) {
                        const bf16x8 fal = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(qal + (size_t)t * 32u * lds_stride + koff));
                        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fal, fb, acc[t], 0, 0, 0);
                        if (F32) acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fbl, acc[t], 0, 0, 0);
                    }
                }
            }
        };
        // two register groups: group g + 1 is requested before group g is consumed
        Group g0, g1;
        load_group(g0, 0);
        for (uint32_t grp = 0; grp < ngroups; grp += 2) {
            if (grp + 1 < ngroups) load_group(g1, grp + 1);
            compute_group(g0, grp);
            if (grp + 1 < ngroups) {
                if (grp + 2 < ngroups) load_group(g0, grp + 2);
                compute_group(g1, grp + 1);
            }
        }
        // epilogue: C[m = query][n = row]; lane holds n = lane & 31, m = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
        if (rloc < a.nrows) {
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint32_t qq = (uint32_t)t * 32u + (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * half;
                    if (qq >= a.b) continue;
                    float *dp = a.dist + (size_t)qq * a.chunk_ld + rloc;
                    if (accumulate) atomicAdd(dp, acc[t][e]);
                    else *dp = acc[t][e];
                }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The ring build for batches of <= 32 queries (round 4; VERDICT r3 weak #3: the kernel above asks for 32 rows x two 16-byte
// pieces per load instruction -- 4.3-4.6 TB/s, and 3 125 row blocks over 2 048 wavefronts leave the second half of the launch
// half empty).  Here the ROWS go through LDS in whole 128-byte lines and the QUERIES sit in registers:
//   * a workgroup is 8 wavefronts = `ds` depth slices x 8 / ds row blocks of 32 rows; wavefront (rb, j) holds the A fragments
//     of depth slice j (CH chunks of CD = 32 f32 / 64 bf16 elements, chunk c = elements [(c ds + j) CD, + CD): <= 64
//     registers, twice that with the lo parts) of all 32 queries in registers and streams that slice of its 32 rows;
//   * a chunk = 32 rows x 128 bytes = four global_load_lds_dwordx4 copies of 8 rows x 128 bytes (8 lanes per row: the HNSW
//     gather's pattern, every line requested once and whole) into the wavefront's PRIVATE ring of three 4-KB stages; two
//     chunks are always in flight per wavefront (64 KB per CU), the request cursor runs across row blocks, no barrier and no
//     other wavefront is involved: counted s_waitcnt vmcnt only;
//   * the copy's LDS image is lane-linear, so the bank swizzle is on the SOURCE: lane 8 r + p fetches piece p ^ ((row >> 1) & 7)
//     of its row, and the B-fragment ds_read_b128 (lane = row, 16 lanes per LDS cycle) applies the same XOR: conflict-free;
//   * the 32 x 32 partial dot products of the `ds` wavefronts of a row block meet in LDS (fixed order: deterministic), every
//     wavefront adds and stores 16 / ds of the 16 accumulator registers;
//   * subset ids (restricted scans) arrive by LDS-DMA as well, two row blocks ahead: nothing the compiler would wait for.
// Work unit = 32 rows x 8 / ds per workgroup: 100 000 candidates x 1536 f32 = 3 125 units over 256 CUs (12.2 each: 94 %
// balanced, against 76 % above).  Algorithmic bytes per launch as above.
#define HVX_SQ_GLDS16(gptr, lptr)                                                                                     \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gptr),                           \
                                     (__attribute__((address_space(3))) void *)(lptr), 16, 0, 0)
#define HVX_SQ_GLDS4(gptr, lptr)                                                                                      \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gptr),                           \
                                     (__attribute__((address_space(3))) void *)(lptr), 4, 0, 0)

template <int N> __device__ __forceinline__ void sq_wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
// LDS accesses as inline asm: the compiler answers an LDS load that "may alias" an LDS-DMA copy in flight with s_waitcnt
// vmcnt(0) (it would drain the ring); the kernel states its waits itself
__device__ __forceinline__ uint4 sq_lds_read16(uint32_t addr) {
    uint4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
__device__ __forceinline__ uint32_t sq_lds_read4(uint32_t addr) {
    uint32_t v;
    asm volatile("ds_read_b32 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
__device__ __forceinline__ void sq_lds_write4(uint32_t addr, float v) { asm volatile("ds_write_b32 %0, %1" ::"v"(addr), "v"(v) : "memory"); }
__device__ __forceinline__ void sq_wait_lgkm0() {
    __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0), nothing else
    __builtin_amdgcn_sched_barrier(0);
}

#ifndef HVX_SQ_STAGES
#define HVX_SQ_STAGES 3
#endif
constexpr int kSqStages = HVX_SQ_STAGES;                      // ring stages per wavefront (4 KB each)
constexpr int kSqRedHalves = kSqStages >= 4 ? 2 : 1;          // a four-stage ring leaves LDS for half the accumulators at a time
constexpr uint32_t kSqRing = 8u * kSqStages * 4096u;          // 96 KB (three stages)
constexpr uint32_t kSqIds = 8u * 2u * 256u;                   // two id slots of 64 words per wavefront
constexpr uint32_t kSqRed = 8u * (16u / kSqRedHalves) * 64u * 4u; // partial dot products: 32 KB
constexpr uint32_t kSqLds = kSqRing + kSqIds + kSqRed;
static_assert(kSqLds <= 160u * 1024u, "the ring, the id slots and the partial sums share one CU's LDS");

template <int KIND, int CH, bool FULL>
__global__ __launch_bounds__(512) void flat_smallq_kernel(MfmaArgs a, uint32_t n_blocks, uint32_t n_groups, uint32_t ds_log2) {
    constexpr bool F32 = KIND == 2;
    constexpr int S = kSqStages, P = S - 1;       // P chunks requested ahead of the one being multiplied
    constexpr int SPC = F32 ? 2 : 4, CD = SPC * 16; // MFMA steps and depth per 128-byte chunk
    constexpr int NST = CH * SPC;
    static_assert(CH >= P, "the request cursor may run one row block ahead, not two");
    extern __shared__ __attribute__((aligned(1024))) unsigned char sq_lds[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const uint32_t fr = lane & 31u, h = lane >> 5;
    const uint32_t ds = 1u << ds_log2, j = w & (ds - 1u), rb = w >> ds_log2, RB = 8u >> ds_log2;
    // depth slices interleaved by 128-byte lines: chunk c of slice j is line c ds + j of the row, so the `ds` wavefronts of a row
    // block, which move through their chunks together, ask for ds CONSECUTIVE lines of every row at about the same time (DRAM
    // pages see runs of up to 1 KB instead of isolated lines 768 bytes apart)
    const uint32_t k0 = j * (uint32_t)CD;
    const uint32_t esz = F32 ? 4u : 2u;
    const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>(sq_lds);
    unsigned char *ring = sq_lds + w * (uint32_t)(S * 4096);
    const uint32_t ring0 = lds0 + w * (uint32_t)(S * 4096);
    unsigned char *ids_lds = sq_lds + kSqRing + w * 512u;
    const uint32_t ids0 = lds0 + kSqRing + w * 512u;
    const uint32_t red0 = lds0 + kSqRing + kSqIds;

    // the queries' A fragments of this depth range: lane = query (l & 31), depth half (l >> 5)
    bf16x8 qa[NST], ql[FULL ? NST : 1];
#pragma unroll
    for (int s = 0; s < NST; ++s) {
        const size_t at = (size_t)fr * a.dim + k0 + (uint32_t)(s / SPC) * (ds * (uint32_t)CD) + (uint32_t)(s % SPC) * 16u + h * 8u;
        qa[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(a.qhi + at));
        if (FULL) ql[s] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4 *>(a.qlo + at));
    }
    // copy roles: copy i (0..3) of a chunk moves rows 8 i .. 8 i + 7, lane 8 r + p piece p ^ ((row >> 1) & 7) of row 8 i + r
    uint32_t cpiece[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) cpiece[i] = ((lane & 7u) ^ (((uint32_t)(4 * i) + (lane >> 4)) & 7u)) * 16u;
    // fragment reads: lane = row fr; f32: step s reads pieces 4 s + 2 h, + 1; bf16: step s reads piece 2 s + h
    uint32_t roff[4];
    {
        const uint32_t base = (fr >> 3) * 1024u + (fr & 7u) * 128u, swz = (fr >> 1) & 7u;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t c = F32 ? (uint32_t)(4 * (r >> 1) + (r & 1)) + 2u * h : (uint32_t)(2 * r) + h;
            roff[r] = base + ((c ^ swz) << 4);
        }
    }
    const unsigned char *rows = reinterpret_cast<const unsigned char *>(a.rows) + (size_t)k0 * esz;
    const size_t rowbytes = (size_t)a.dim * esz;
    const uint32_t last_row = a.nrows - 1u;
    auto block_of = [&](uint32_t g) -> uint32_t { // (past the end: the last block again -- requested, never multiplied into an output)
        const uint32_t blk = g * RB + rb;
        return blk < n_blocks ? blk : n_blocks - 1u;
    };
    auto request_ids = [&](uint32_t g, uint32_t slot) { // the 32 subset entries of group g's block -> this wavefront's id slot
        if (!a.subset) return;
        uint32_t rloc = block_of(g) * 32u + fr;
        rloc = rloc < last_row ? rloc : last_row;
        HVX_SQ_GLDS4(a.subset + a.row0 + rloc, ids_lds + slot * 256u);
    };
    const unsigned char *gp[4];
    auto pointers_from = [&](const uint32_t (&node)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) gp[i] = rows + (size_t)node[i] * rowbytes + cpiece[i];
    };
    auto request_chunk = [&](uint32_t pc, uint32_t stage) {
        unsigned char *dst = ring + stage * 4096u;
#pragma unroll
        for (int i = 0; i < 4; ++i) HVX_SQ_GLDS16(gp[i] + pc * (ds * 128u), dst + i * 1024);
    };

    uint32_t g = blockIdx.x;
    {   // prologue: the first block's ids by plain loads (nothing is in flight yet)
        uint32_t node[4];
        const uint32_t blk = block_of(g);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            uint32_t rloc = blk * 32u + (uint32_t)(8 * i) + (lane >> 3);
            rloc = rloc < last_row ? rloc : last_row;
            node[i] = a.subset ? a.subset[a.row0 + rloc] : a.row0 + rloc;
        }
        pointers_from(node);
    }
    // everything loaded so far is in its registers before the first copy is requested: the compiler's own waits for these plain
    // loads would otherwise land inside the loop, where a counted wait of its choosing drains the ring
#pragma unroll
    for (int s = 0; s < NST; ++s) {
        asm volatile("" : "+v"(qa[s]));
        if (FULL) asm volatile("" : "+v"(ql[s]));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) asm volatile("" : "+v"(gp[i]));
    uint32_t id_slot = 0; // the slot holding the ids of the NEXT block the request cursor enters
    request_ids(g + gridDim.x, 0);
#pragma unroll
    for (int c = 0; c < P; ++c) request_chunk((uint32_t)c, (uint32_t)c);
    uint32_t stage_c = 0, stage_p = P;

    for (; g < n_groups; g += gridDim.x) {
        f32x16 acc;
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[e] = 0.f;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            if (c + P == CH) { // the request cursor enters the next group's row block
                uint32_t node[4];
                const uint32_t gn = g + gridDim.x;
                if (a.subset) {
                    if (CH == P) sq_wait_vmcnt<4 * P>(); // (first iteration: the id copy is the oldest request)
                    uint32_t raw[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) raw[i] = sq_lds_read4(ids0 + id_slot * 256u + ((uint32_t)(8 * i) + (lane >> 3)) * 4u);
                    sq_wait_lgkm0();
#pragma unroll
                    for (int i = 0; i < 4; ++i) node[i] = raw[i];
                    id_slot ^= 1u;
                    request_ids(gn + gridDim.x, id_slot); // (that slot's ids were turned into pointers one iteration ago)
                } else {
                    const uint32_t blk = block_of(gn);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const uint32_t rloc = blk * 32u + (uint32_t)(8 * i) + (lane >> 3);
                        node[i] = a.row0 + (rloc < last_row ? rloc : last_row);
                    }
                }
                pointers_from(node);
            }
            request_chunk((uint32_t)((c + P) % CH), stage_p); // into the stage multiplied one step ago (its reads have returned)
            stage_p = stage_p + 1u == (uint32_t)S ? 0u : stage_p + 1u;
            // chunk c has landed when at most the P younger chunks are outstanding (loads return in order; an id copy or the
            // previous block's stores among the younger requests only make the wait stricter)
            sq_wait_vmcnt<4 * P>();
            const uint32_t sb = ring0 + stage_c * 4096u;
            stage_c = stage_c + 1u == (uint32_t)S ? 0u : stage_c + 1u;
            uint4 raw[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) raw[r] = sq_lds_read16(sb + roff[r]);
            sq_wait_lgkm0();
#pragma unroll
            for (int s = 0; s < SPC; ++s) {
                uint4 bw, bl = make_uint4(0, 0, 0, 0);
                if (F32) {
                    const uint4 x0 = raw[2 * s], x1 = raw[F32 ? 2 * s + 1 : 0];
                    float x[8];
                    x[0] = __uint_as_float(x0.x); x[1] = __uint_as_float(x0.y); x[2] = __uint_as_float(x0.z); x[3] = __uint_as_float(x0.w);
                    x[4] = __uint_as_float(x1.x); x[5] = __uint_as_float(x1.y); x[6] = __uint_as_float(x1.z); x[7] = __uint_as_float(x1.w);
                    uint32_t hh[4];
#pragma unroll
                    for (int i = 0; i < 4; ++i) hh[i] = pack_bf16(x[2 * i], x[2 * i + 1]);
                    bw = make_uint4(hh[0], hh[1], hh[2], hh[3]);
                    if (FULL) { // residuals x - bf16(x), rounded to bf16 again
                        uint32_t l[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            l[i] = pack_bf16(x[2 * i] - __uint_as_float(hh[i] << 16), x[2 * i + 1] - __uint_as_float(hh[i] & 0xFFFF0000u));
                        bl = make_uint4(l[0], l[1], l[2], l[3]);
                    }
                } else {
                    bw = raw[F32 ? 0 : s];
                }
                const bf16x8 fb = __builtin_bit_cast(bf16x8, bw);
                acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[c * SPC + s], fb, acc, 0, 0, 0);
                if (FULL) {
                    acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ql[FULL ? c * SPC + s : 0], fb, acc, 0, 0, 0);
                    if (F32) acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qa[c * SPC + s], __builtin_bit_cast(bf16x8, bl), acc, 0, 0, 0);
                }
            }
        }
        // C[m = query][n = row]: lane holds n = lane & 31, m = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
        const uint32_t blk = g * RB + rb, rloc = blk * 32u + fr;
        const bool live = blk < n_blocks && rloc < a.nrows;
        if (ds_log2 == 0u) {
            if (live) {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const uint32_t qq = (uint32_t)(e & 3) + 8u * (uint32_t)(e >> 2) + 4u * h;
                    if (qq < a.b) a.dist[(size_t)qq * a.chunk_ld + rloc] = acc[e];
                }
            }
        } else {
            // the stores are inline asm: the compiler's hazard recogniser does not see them read the accumulator, so the wait
            // states between the last MFMA's write-back (8 passes) and an LDS instruction reading it are stated here -- without
            // them acc[0] left for the LDS one MFMA step short (found by tests/native/smallq_probe.hip on bf16 rows)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            constexpr int EH = 16 / kSqRedHalves; // accumulator registers per reduction pass
#pragma unroll
            for (int hh = 0; hh < kSqRedHalves; ++hh) {
#pragma unroll
                for (int e = 0; e < EH; ++e) sq_lds_write4(red0 + ((w * (uint32_t)EH + (uint32_t)e) * 64u + lane) * 4u, acc[hh * EH + e]);
                sq_wait_lgkm0();
                __builtin_amdgcn_s_barrier();
                const uint32_t epw = (uint32_t)EH >> ds_log2;
                for (uint32_t ee = 0; ee < epw; ++ee) {
                    const uint32_t el = j * epw + ee, e = (uint32_t)(hh * EH) + el;
                    uint32_t part[8];
#pragma unroll
                    for (uint32_t jj = 0; jj < 8u; ++jj)
                        if (jj < ds) part[jj] = sq_lds_read4(red0 + (((rb * ds + jj) * (uint32_t)EH + el) * 64u + lane) * 4u);
                    sq_wait_lgkm0();
                    float v = 0.f;
#pragma unroll
                    for (uint32_t jj = 0; jj < 8u; ++jj)
                        if (jj < ds) v += __uint_as_float(part[jj]); // slice 0 first: the same sum on every run
                    const uint32_t qq = (e & 3u) + 8u * (e >> 2) + 4u * h;
                    if (live && qq < a.b) a.dist[(size_t)qq * a.chunk_ld + rloc] = v;
                }
                __builtin_amdgcn_s_barrier(); // the partial sums are read: the next pass / block may overwrite them
            }
        }
    }
    sq_wait_vmcnt<0>(); // (requests past the last block are still landing in this wavefront's ring)
}

// ---------------------------------------------------------------------------------------------------------------------
// Selection without sorting.  The certificate (hvx_flat_mfma.hip) needs, per query, a candidate set C of m + 1 rows and a
// threshold t such that every row outside C has approximate score >= t: the m + 1 smallest scores and the largest of them.
// A workgroup holds 4 096 scores of its slice in registers (16 per thread) and finds the kc-th smallest by a bitwise
// descent over the f32 bit patterns (non-negative scores order like their bits): 32 rounds of "how many keys carry this
// prefix with a 0 here" -- 16 compares per thread, one wave reduction, one LDS add, one barrier.  Keys below the result are
// emitted, ties fill the remaining quota.  Slices longer than one register chunk carry their survivors into the next chunk.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int kSelR = 16;              // scores per thread and chunk
constexpr int kSelChunk = kSelR * 256; // 4 096

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

struct SelectArgs {
    const float *dots;        // [b][chunk_ld] raw dot products
    uint32_t chunk_ld, rows, row0;
    const uint32_t *subset;   // scan position -> row (restricted scans), or NULL
    const float *rowterm;     // [n] |x|^2 (L2) / |x| (cosine)
    const float *qn2;         // [b]
    const float *rowscale;    // unused (fp8 rows do not take this path)
    uint32_t metric, b, kc, slice_rows;
    uint32_t *status;         // [b] query status: rejected queries are skipped, an invalid score sets 8
    float *sl_sc;             // [b][slices * kc] out: every slice's kc smallest (score, row) pairs, padded with +inf
    uint32_t *sl_id;
    uint32_t sl_stride;
};

__global__ __launch_bounds__(256) void flat_select_radix_kernel(SelectArgs a) {
    __shared__ uint32_t sv_key[256], sv_id[256], n_lt, n_tie, bad;
    __shared__ __attribute__((aligned(16))) uint32_t hist[4][256]; // one histogram per 8-bit round
    const uint32_t q = blockIdx.x, sl = blockIdx.y, tid = threadIdx.x;
    const uint32_t kc = a.kc;
    float *out_sc = a.sl_sc + (size_t)q * a.sl_stride + (size_t)sl * kc;
    uint32_t *out_id = a.sl_id + (size_t)q * a.sl_stride + (size_t)sl * kc;
    const float inf = __uint_as_float(0x7F800000u);
    if (a.status && a.status[q] != 0u) {
        for (uint32_t i = tid; i < kc; i += 256) { out_sc[i] = inf; out_id[i] = 0xFFFFFFFFu; }
        return;
    }
    const uint32_t lo = sl * a.slice_rows, hi = lo + a.slice_rows < a.rows ? lo + a.slice_rows : a.rows;
    const float *dq = a.dots + (size_t)q * a.chunk_ld;
    const float qn2 = a.qn2[q], qn = sqrtf(qn2);
    uint32_t n_surv = 0; // survivors carried from the previous chunk (in sv_key / sv_id)
    if (tid == 0) bad = 0;
    __syncthreads();
    for (uint32_t base = lo; base < hi; base += kSelChunk) {
        if (tid == 0) { n_lt = 0; n_tie = 0; }
#pragma unroll
        for (int d = 0; d < 4; ++d) hist[d][tid] = 0;
        uint32_t key[kSelR + 1];
#pragma unroll
        for (int r = 0; r < kSelR; ++r) {
            const uint32_t i = base + (uint32_t)r * 256u + tid;
            uint32_t kbits = 0xFFFFFFFFu;
            if (i < hi) {
                const uint32_t scan = a.row0 + i;
                const uint32_t node = a.subset ? a.subset[scan] : scan;
                const float dot = dq[i], term = a.rowterm[node];
                float s;
                if (a.metric == kL2) {
                    s = (qn2 + term) - 2.0f * dot;
                    s = s < 0.f ? 0.f : s;
                } else {
                    s = approx_half_cosine(dot, qn, term);
                }
                if (!score_valid(s)) bad = 1; // Candidate::try_new rejects the score (model.rs:21-29)
                else kbits = __float_as_uint(s);
            }
            key[r] = kbits;
        }
        key[kSelR] = tid < n_surv ? sv_key[tid] : 0xFFFFFFFFu;
        const uint32_t carried_id = tid < n_surv ? sv_id[tid] : 0xFFFFFFFFu;
        const uint32_t in_chunk = (hi - base) < (uint32_t)kSelChunk ? (hi - base) : (uint32_t)kSelChunk;
        const uint32_t total = in_chunk + n_surv;
        const uint32_t kth = kc < total ? kc : total;
        __syncthreads(); // counters zeroed; every thread holds its carried survivor in a register
        // the kth smallest key by four rounds of 8 bits, most significant first (an invalid score holds the all-ones key and sorts
        // last): keys that carry the prefix chosen so far are counted by digit in LDS, then every wavefront reads the histogram
        // and finds the digit of rank kk itself -- one barrier per round (round 3's 32-round bitwise descent: 32)
        uint32_t prefix = 0, kk = kth, less = 0;
#ifdef HVX_SELECT_ABLATE // (probe builds: how long the kernel takes without its selection rounds)
        kk = 0;
#endif
#pragma unroll
        for (int d = 3; d >= 0; --d) {
            const int sh = 8 * d;
            const uint32_t hi_mask = d == 3 ? 0u : (0xFFFFFFFFu << (sh + 8));
#ifdef HVX_SELECT_ABLATE
            if (HVX_SELECT_ABLATE >= 1) continue;
#endif
#pragma unroll
            for (int r = 0; r <= kSelR; ++r)
                radix_count(hist[d], (key[r] & hi_mask) == prefix, (key[r] >> sh) & 255u); // (padding keys are all ones: last bin, beyond any rank asked for)
            __syncthreads();
            uint32_t g = 0, below = 0;
            if (kk) radix_digit_of_rank(hist[d], kk, g, below);
            prefix |= g << sh; kk -= below; less += below;
        }
        // emit into the survivor arrays: keys below the kth value, then ties up to the quota
        const uint32_t quota = kth - less;
#pragma unroll
        for (int r = 0; r <= kSelR; ++r) {
            const uint32_t kb = key[r];
            bool take = kb < prefix;
            if (!take && kb == prefix && kb != 0xFFFFFFFFu) take = atomicAdd(&n_tie, 1u) < quota;
            if (take) {
                uint32_t id = carried_id;
                if (r < kSelR) {
                    const uint32_t scan = a.row0 + base + (uint32_t)r * 256u + tid;
                    id = a.subset ? a.subset[scan] : scan;
                }
                const uint32_t pos = atomicAdd(&n_lt, 1u);
                if (pos < 256u) { sv_key[pos] = kb; sv_id[pos] = id; }
            }
        }
        __syncthreads();
        n_surv = n_lt < kth ? n_lt : kth;
        __syncthreads(); // n_lt is re-zeroed at the top of the next chunk
    }
    __syncthreads();
    for (uint32_t i = tid; i < kc; i += 256) {
        out_sc[i] = i < n_surv ? __uint_as_float(sv_key[i]) : inf;
        out_id[i] = i < n_surv ? sv_id[i] : 0xFFFFFFFFu;
    }
    if (tid == 0 && lo < hi && bad && a.status && a.status[q] == 0u) a.status[q] = 8u; // HVX_ERR_INVARIANT
}

constexpr size_t kSmallbLds = 150u * 1024u;

static uint32_t smallb_tiles(uint32_t b) {
    const uint32_t nqt = (b + 31u) / 32u;
    return nqt == 3 ? 4u : nqt;
}
// depth passes needed so that the query tiles of one pass fit the LDS (0 = not servable)
static uint32_t smallb_passes(uint32_t dim, uint32_t b, bool full) {
    const uint32_t tiles = smallb_tiles(b) * (full ? 2u : 1u);
    for (uint32_t p = 1; p <= 4; ++p) {
        if (dim % (p * 128u) != 0u) continue; // a pass is a whole number of 8-step register groups
        if ((size_t)tiles * 32u * ((size_t)(dim / p) * 2u + 16u) <= kSmallbLds) return p;
    }
    return 0;
}

bool flat_smallb_supported(uint32_t dim, uint32_t b, int kind) {
    if (kind != 0 && kind != 2) return false;
    if (b == 0 || b > 128u || dim % 128u != 0u) return false;
    return smallb_passes(dim, b, true) != 0 && smallb_passes(dim, b, false) != 0;
}

template <int KIND, int NQT, bool FULL>
static hipError_t launch_smallb_t(const MfmaArgs &a, uint32_t n_blocks, uint32_t cus, hipStream_t s) {
    // 8 wavefronts per CU with 256 registers each: two groups of 8 steps in flight (16 KB of f32 rows per wavefront)
    constexpr int WAVES = 8, U = NQT == 4 ? (KIND == 2 ? 2 : 4) : ((NQT == 2 && KIND == 2 && FULL) ? 4 : 8);
    const uint32_t passes = smallb_passes(a.dim, a.b, FULL);
    if (passes == 0) return hipErrorInvalidValue;
    const uint32_t klen = a.dim / passes, stride = klen * 2u + 16u;
    const size_t lds = (size_t)NQT * (FULL ? 2u : 1u) * 32u * stride;
    auto kern = flat_smallb_kernel<KIND, NQT, WAVES, U, FULL>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (passes > 1) { // partial dot products are added into zeroed words
        hipError_t e = hipMemsetAsync(a.dist, 0, (size_t)a.b * a.chunk_ld * 4, s);
        if (e != hipSuccess) return e;
    }
    const uint32_t per = std::max<uint32_t>(1u, cus / passes);
    const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>(per, (n_blocks + WAVES - 1) / WAVES));
    hipLaunchKernelGGL(kern, dim3(grid, passes), dim3(WAVES * 64), lds, s, a, n_blocks, stride, klen);
    return hipGetLastError();
}

template <int KIND, bool FULL> static hipError_t launch_smallb_q(const MfmaArgs &a, uint32_t n_blocks, uint32_t cus, hipStream_t s) {
    switch (smallb_tiles(a.b)) {
    case 1: return launch_smallb_t<KIND, 1, FULL>(a, n_blocks, cus, s);
    case 2: return launch_smallb_t<KIND, 2, FULL>(a, n_blocks, cus, s);
    default: return launch_smallb_t<KIND, 4, FULL>(a, n_blocks, cus, s);
    }
}

// the ring build's shape for (dim, kind): ds depth slices x ch chunks of 32 f32 / 64 bf16 elements (false: not servable)
static bool smallq_plan(uint32_t dim, uint32_t b, int kind, uint32_t &ds_log2, uint32_t &ch) {
    if (b == 0 || b > 32u || (kind != 0 && kind != 2)) return false;
    const uint32_t cd = kind == 2 ? 32u : 64u;
    if (dim % cd != 0u) return false;
    const uint32_t t = dim / cd;
    for (int pass = 0; pass < 2; ++pass) // the finest depth split with >= 3 chunks per wavefront; two chunks as a last resort
        for (int l = 3; l >= 0; --l) {
            if (t % (1u << l) != 0u) continue;
            const uint32_t c = t >> l;
            if (kind == 0 && c > 4u) continue; // (bf16 rows: 16 registers of query fragments per chunk and operand)
            if (pass == 0 ? (c == 3 || c == 4 || c == 6 || c == 8) : (c == 2 && kSqStages - 1 <= 2)) { ds_log2 = (uint32_t)l; ch = c; return true; }
        }
    return false;
}

template <int KIND, bool FULL>
static hipError_t launch_smallq_k(const MfmaArgs &a, uint32_t n_blocks, uint32_t ds_log2, uint32_t ch, uint32_t cus, hipStream_t s) {
    const uint32_t rb = 8u >> ds_log2, n_groups = (n_blocks + rb - 1) / rb;
    const uint32_t grid = std::max<uint32_t>(1u, std::min<uint32_t>(cus, n_groups));
#define HVX_SQ_LAUNCH(CH)                                                                                                       \
    do {                                                                                                                          \
        auto kern = flat_smallq_kernel<KIND, CH, FULL>;                                                                           \
        hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSqLds);          \
        if (e != hipSuccess) return e;                                                                                            \
        hipLaunchKernelGGL(kern, dim3(grid), dim3(512), kSqLds, s, a, n_blocks, n_groups, ds_log2);                               \
    } while (0)
    switch (ch) {
    case 2: if constexpr (kSqStages - 1 <= 2) { HVX_SQ_LAUNCH(2); break; } else return hipErrorInvalidValue;
    case 3: HVX_SQ_LAUNCH(3); break;
    case 4: HVX_SQ_LAUNCH(4); break;
    case 6: if constexpr (KIND == 2) { HVX_SQ_LAUNCH(6); break; } else return hipErrorInvalidValue;
    case 8: if constexpr (KIND == 2) { HVX_SQ_LAUNCH(8); break; } else return hipErrorInvalidValue;
    default: return hipErrorInvalidValue;
    }
#undef HVX_SQ_LAUNCH
    return hipGetLastError();
}

// raw dot products of rows [a.row0, a.row0 + a.nrows) of the scan order against a.b <= 128 queries into a.dist (row length a.chunk_ld)
// build: 0 = the ring build for b <= 32 where its shapes allow, the register-fragment build otherwise; 1 = always the latter
hipError_t launch_flat_smallb(const MfmaArgs &a, int kind, bool full, uint32_t cus, uint32_t build, hipStream_t s) {
    if (a.nrows == 0) return hipSuccess;
    if (!flat_smallb_supported(a.dim, a.b, kind)) return hipErrorInvalidValue;
    const uint32_t n_blocks = (a.nrows + 31u) / 32u;
    uint32_t ds_log2 = 0, ch = 0;
    if (build == 0 && smallq_plan(a.dim, a.b, kind, ds_log2, ch)) {
        if (kind == 2) return full ? launch_smallq_k<2, true>(a, n_blocks, ds_log2, ch, cus, s) : launch_smallq_k<2, false>(a, n_blocks, ds_log2, ch, cus, s);
        return full ? launch_smallq_k<0, true>(a, n_blocks, ds_log2, ch, cus, s) : launch_smallq_k<0, false>(a, n_blocks, ds_log2, ch, cus, s);
    }
    if (kind == 2) return full ? launch_smallb_q<2, true>(a, n_blocks, cus, s) : launch_smallb_q<2, false>(a, n_blocks, cus, s);
    return full ? launch_smallb_q<0, true>(a, n_blocks, cus, s) : launch_smallb_q<0, false>(a, n_blocks, cus, s);
}

// slices per query for a scan of `rows` rows with kc <= 256: <= 32, each a whole number of 4 096-score register chunks
uint32_t flat_smallb_slices(uint32_t rows) {
    const uint32_t chunks = (rows + (uint32_t)kSelChunk - 1) / (uint32_t)kSelChunk;
    return std::max<uint32_t>(1u, std::min<uint32_t>(32u, chunks));
}

// the kc smallest approximate scores of every slice: a.dist (raw dots) -> sl_sc / sl_id [b][slices * kc] (row length sl_stride)
hipError_t launch_flat_select_radix(const MfmaArgs &a, uint32_t kc, uint32_t *status, float *sl_sc, uint32_t *sl_id, uint32_t sl_stride,
                                    uint32_t *out_slices, hipStream_t s) {
    if (a.b == 0 || kc == 0 || kc > 256u) return hipErrorInvalidValue;
    const uint32_t slices = flat_smallb_slices(a.nrows);
    const uint32_t chunks = (a.nrows + (uint32_t)kSelChunk - 1) / (uint32_t)kSelChunk;
    SelectArgs g{};
    g.dots = a.dist; g.chunk_ld = a.chunk_ld; g.rows = a.nrows; g.row0 = a.row0; g.subset = a.subset; g.rowterm = a.rowterm; g.qn2 = a.qn2;
    g.metric = a.metric; g.b = a.b; g.kc = kc; g.slice_rows = ((chunks + slices - 1) / slices) * (uint32_t)kSelChunk;
    g.status = status; g.sl_sc = sl_sc; g.sl_id = sl_id; g.sl_stride = sl_stride;
    const uint32_t used = (a.nrows + g.slice_rows - 1) / g.slice_rows;
    if ((size_t)used * kc > sl_stride) return hipErrorInvalidValue;
    *out_slices = used;
    hipLaunchKernelGGL(flat_select_radix_kernel, dim3(a.b, used), dim3(256), 0, s, g);
    return hipGetLastError();
}

} // namespace hvx
