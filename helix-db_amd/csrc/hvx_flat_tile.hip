// hvx_flat_tile.hip -- the large-tile contraction kernels of the matrix-core exact scan (BASELINE configs #4 / #5 and the
// f32 exact scan): candidate generation for restricted_exact_scan (crates/db/src/search/vector/restricted.rs:753-835), see
// the pipeline description at the top of hvx_flat_mfma.hip.  These kernels only FILTER: a score leaves the tile when it is
// below the query's running threshold, as a (score, row) pair; the first chunk of a scan (which has no threshold yet) and
// the repeat passes stay on the 128 x 128 kernel.
//
// Common structure (gfx950): every wavefront owns 128 queries x 64 rows = 4 x 2 accumulators of v_mfma_f32_32x32x16_bf16
// (128 registers).  Operand stages are copied HBM/L2 -> LDS by global_load_lds_dwordx4 (no registers, no ds_write pass).
// The LDS image is lane-linear per wave instruction (1 KB = 8 tile rows x 128 B, or 16 x 64 B), so the XOR swizzle that
// makes the fragment reads (ds_read_b128, lane = tile row) conflict-free (SQ_LDS_BANK_CONFLICT = 0 measured) is applied to
// the SOURCE address and again to the read address: 128-B rows: 16-B slot ^ ((row >> 1) & 7); 64-B rows: slot ^ ((row >> 2) & 3).
// fp8 codes are widened to bf16 (exactly) in registers between the ds_read and the MFMA: v_cvt_pk_f32_fp8 + v_perm; one
// ds_read_b128 of the code tile feeds two MFMA steps (the query operand is stored in the matching order: tile_slot_fp8).
// Workgroups are mapped to tiles XCD-aware (tile_coords): the workgroups an XCD runs at a time form a super-tile that shares
// its operand tiles in that XCD's L2 (measured: L2 hit rate 0.91, HBM traffic = the rows once).
//
// Two builds, both 256 threads = 2 x 2 wavefronts on a 256 x 128 tile, TWO independent workgroups per CU, counted vmcnt + raw
// s_barrier, fragment reads as inline asm with stated lgkmcnt waits (launch_flat_tile picks one):
//   flat_tile2_kernel    bf16 rows (a bf16 index or the bf16 shadow of an f32 one): a ring of three 32-deep stages (72 KB);
//                        fp8 codes widened to bf16 (HVX_OPT_FLAT_TILE_BUILD = 4): two 64-deep stages (80 KB)
//   flat_tile2mx_kernel  fp8 codes x the query as two e4m3 pieces on the MX-scaled fp8 instruction (the fp8 default)
// History: the 512-thread builds on 256 x 256 tiles (one workgroup per CU, lock-step and role-split) and a 128 x 128-per-wavefront
// build were measured against these and retired.  What bounds a tile (profiles/history/r02g_*): the matrix cores are NOT the limit.
// Ablation of the 512-thread build, 1024 x 1M x 768 bf16 (ms per launch): MFMAs alone 0.35 (= the dense peak at the 2.1 GHz the chip
// holds), fragment reads + barriers alone 0.24, + operand copies 0.17-0.29, + epilogue 0.17; the full kernel takes 0.93 = their SUM.
// A four-buffer ring with counted waits, fragment registers double-buffered across the stage barrier, and two workgroups per CU all
// land within 4 % of that (fp8, K = 1536: two workgroups per CU + 10 %), i.e. the tile is bound by what goes through the LDS -- 48 KB
// of fragment reads + 16 KB of LDS-DMA writes per 16-deep step and CU against 512 matrix-core cycles -- not by exposed latency.
// The role split (the two wavefronts of a SIMD in opposite read / MFMA phases) gained 1-2 % over the two-workgroup build
// (profiles/history/r04j_tile_builds_ab.txt) and was not adopted.
//
// Epilogue: score < threshold is tested in the accumulator's own units -- fma(acc, alpha_row, -beta_row) > h_query with a
// conservative margin -- 2 VALU operations per score; the rare survivors are pushed to a workgroup list in LDS and
// finished (exact score formula, exact `s < thr` test of the 128 x 128 kernel, global append) by the first threads.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "hvx_device.h"
#include "hvx_flat_mfma.h"

namespace hvx {
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(2))) float f32x2;

constexpr int kTM = 256, kTN = 128;      // queries x rows per workgroup
constexpr int kWgList = 2048;            // survivors a workgroup can hold

#define HVX_GLDS16(gptr, lptr)                                                                                       \
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(gptr),                          \
                                     (__attribute__((address_space(3))) void *)(lptr), 16, 0, 0)

// workgroup -> tile, XCD-aware (workgroup b runs on XCD b % 8, every XCD has its own 4 MB L2): the 32 workgroups an XCD
// runs at a time form a super-tile of sup_r row tiles x sup_q query tiles, so each operand tile is fetched into that L2
// once per super-tile and shared; the query blocks of one row block follow each other (the rows come from HBM once).
__device__ __forceinline__ bool tile_coords(const MfmaArgs &a, uint32_t &qt, uint32_t &rt) {
    const uint32_t x = blockIdx.x & 7u, l = blockIdx.x >> 3;
    const uint32_t rq = a.sup_r * a.sup_q, per_rblock = a.sup_qblocks * rq;
    const uint32_t rblock = l / per_rblock, rem = l % per_rblock;
    const uint32_t qblock = rem / rq, rem2 = rem % rq;
    rt = (rblock * a.sup_r + rem2 / a.sup_q) * 8u + x;
    qt = qblock * a.sup_q + rem2 % a.sup_q;
    return rt < a.nr_tiles && qt < a.nq_tiles;
}

// ---- epilogue shared by both builds.  acc = C[m = query][n = row] of this wavefront's 128 x 64 block.
template <bool FP8>
__device__ __forceinline__ void tile_epilogue(const MfmaArgs &a, f32x16 (&acc)[4][2], unsigned char *lds, uint32_t q0, uint32_t r0, int wm,
                                              int wn, int tid, float xmax2, uint32_t *wg_overflow) { // 256 threads
    const int lane = tid & 63, fr = lane & 31, h = lane >> 5;
    // ---- epilogue.  C[m = query][n = row]: lane holds n = lane & 31, m = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).
    __syncthreads(); // the stage buffers are free
    float *sH = reinterpret_cast<float *>(lds);                      // [256] per-query pass level
    uint32_t *sCnt = reinterpret_cast<uint32_t *>(lds + 1024);       // [1] survivors of this workgroup
    float *sLv = reinterpret_cast<float *>(lds + 2048);              // [kWgList] accumulator value
    uint32_t *sLc = reinterpret_cast<uint32_t *>(lds + 2048 + kWgList * 4); // [kWgList] (query << 8) | row, tile-local
    const float inf = __uint_as_float(0x7F800000u);
    if (tid < kTM) {
        const uint32_t qq = q0 + (uint32_t)tid;
        float hq = inf; // padded query rows let nothing through
        if (qq < a.b) {
            const float t = a.thr[qq], n2 = a.qn2[qq];
            // s < t  <=>  dot - |x|^2/2 > (|q|^2 - t)/2 (L2)   resp.   dot / |x| > (1 - 2t) |q| (cosine), up to the rounding of
            // the two evaluation orders: the margin lets a few more in, the exact test below decides
            if (a.metric == kL2) hq = 0.5f * (n2 - t) - 4e-6f * (n2 + xmax2);
            else { const float qn = sqrtf(n2); hq = (1.0f - 2.0f * t) * qn - 8e-6f * qn; }
        }
        sH[tid] = hq;
    }
    if (tid == 0) *sCnt = 0u;
    float alpha[2], nbeta[2];
    bool untrusted[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t rloc = r0 + (uint32_t)(wn * 64 + j * 32 + fr);
        alpha[j] = 0.f;
        nbeta[j] = -inf; // rows past the end of the scan never pass (not even with a NaN accumulator: see the test below)
        untrusted[j] = false;
        if (rloc < a.nrows) {
            const size_t node = a.subset ? a.subset[a.row0 + rloc] : (size_t)a.row0 + rloc;
            const float term = a.rowterm[node];
            const float rsc = FP8 && a.rowscale ? a.rowscale[node] : 1.0f; // (cosine over fp8 rows: the term is the codes' norm, no scale)
            if (a.metric == kL2) { alpha[j] = rsc; nbeta[j] = -0.5f * term; }
            else if (cosine_term_trusted(term)) { alpha[j] = rsc / term; nbeta[j] = 0.f; }
            else { alpha[j] = 0.f; nbeta[j] = inf; untrusted[j] = true; } // no approximation for this row (hvx_flat_mfma.h): it passes for every query, the exact test below scores it 0
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int m = wm * 128 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * h; // tile-local query
            const float hq = sH[m];
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // an untrusted row passes for every real query, also where its dot product overflowed (0 x inf = NaN compares false);
                // every other NaN -- the accumulator of a padding row -- stays out
                if (__builtin_fmaf(acc[i][j][e], alpha[j], nbeta[j]) > hq || (untrusted[j] && hq < inf)) {
                    const uint32_t pos = atomicAdd(sCnt, 1u);
                    if (pos < (uint32_t)kWgList) {
                        sLv[pos] = acc[i][j][e];
                        sLc[pos] = ((uint32_t)m << 8) | (uint32_t)(wn * 64 + j * 32 + fr);
                    }
                }
            }
        }
    __syncthreads();
    uint32_t cnt = *sCnt;
    if (cnt > (uint32_t)kWgList) { // more survivors than the list holds: the scan is repeated unfiltered, never guessed
        if (tid == 0) atomicOr(wg_overflow, 1u);
        cnt = kWgList;
    }
    for (uint32_t t = (uint32_t)tid; t < cnt; t += blockDim.x) {
        const uint32_t code = sLc[t];
        const uint32_t qq = q0 + (code >> 8), rloc = r0 + (code & 255u);
        if (qq >= a.b || rloc >= a.nrows) continue;
        const size_t node = a.subset ? a.subset[a.row0 + rloc] : (size_t)a.row0 + rloc;
        const float term = a.rowterm[node];
        const float dot = FP8 && a.rowscale ? sLv[t] * a.rowscale[node] : sLv[t];
        float sc;
        if (a.metric == kL2) {
            sc = (a.qn2[qq] + term) - 2.0f * dot;
            sc = sc < 0.f ? 0.f : sc;
        } else {
            sc = approx_half_cosine(dot, sqrtf(a.qn2[qq]), term);
        }
        if (sc < a.thr[qq]) {
            const uint32_t pos = atomicAdd(&a.cand_cnt[qq], 1u);
            if (pos < a.cand_cap) {
                a.cand_sc[(size_t)qq * a.cand_cap + pos] = sc;
                a.cand_id[(size_t)qq * a.cand_cap + pos] = (uint32_t)node;
            }
        }
    }
}

template <int N>
__device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// ds_read_b128 as inline asm: the compiler then neither sees an LDS load that "may alias" the LDS-DMA copies in flight (it
// answers that with s_waitcnt vmcnt(0), draining the copy ring -- it did so for the fp8 code reads of an earlier build) nor
// places its own lgkmcnt waits; the kernel states both waits itself, each followed by a sched_barrier (an MFMA may not be
// hoisted over them).
template <int OFF>
__device__ __forceinline__ uint4 lds_read16(uint32_t addr) {
    uint4 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF) : "memory");
    return v;
}
__device__ __forceinline__ void wait_lgkm0() {
    __builtin_amdgcn_s_waitcnt(0xC07F); // lgkmcnt(0), nothing else
    __builtin_amdgcn_sched_barrier(0);
}

template <int LGKM> // everything but the LGKM youngest LDS requests has arrived (they return in order)
__device__ __forceinline__ void wait_lgkm() {
    __builtin_amdgcn_s_waitcnt(0xC07F | (LGKM << 8));
    __builtin_amdgcn_sched_barrier(0);
}

// ---- the two-workgroups-per-CU build (see the file header): a workgroup is four wavefronts (one per SIMD, 2 x 2, each 128
// queries x 64 rows) on a 256 x 128 tile, so a CU holds two independent workgroups: while one waits at its barrier, starts a
// tile or runs its epilogue, the other one's MFMAs have the matrix cores.

template <int KIND>
__global__ __launch_bounds__(256, 2) void flat_tile2_kernel(MfmaArgs a, float xmax2, uint32_t *wg_overflow) {
    constexpr bool FP8 = KIND == 1;
    constexpr int KS = FP8 ? 64 : 32, SPS = KS / 16;
    constexpr int AROWB = KS * 2, BROWB = 64;       // bytes per tile row and stage
    constexpr int ASTAGE = kTM * AROWB, STAGE = ASTAGE + kTN * BROWB; // 24 KB (bf16) / 40 KB (fp8)
    constexpr int NBUF = FP8 ? 2 : 3;               // 72 KB / 80 KB per workgroup
    constexpr int GA = AROWB / 16, GB = 2, G = GA + GB; // 1-KB copies per wave and stage: queries 64 rows, rows 32 rows per wave
    __shared__ __attribute__((aligned(1024))) unsigned char lds[NBUF * STAGE];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    uint32_t qt, rt;
    if (!tile_coords(a, qt, rt)) return;
    const uint32_t q0 = qt * kTM, r0 = rt * kTN;

    // staging: wave w copies query rows 64 w .. 64 w + 63 and tile rows 32 w .. 32 w + 31 (64-byte rows: 16 rows per 1-KB copy, slot (l & 3) ^ ((row >> 2) & 3); 128-byte rows: 8 rows, slot (l & 7) ^ ((row >> 1) & 7))
    const unsigned char *gA[GA], *gB[GB];
#pragma unroll
    for (int t = 0; t < GA; ++t) {
        uint32_t row, slot;
        if (AROWB == 64) { row = (uint32_t)(64 * wave + 16 * t + (lane >> 2)); slot = (uint32_t)(lane & 3) ^ ((row >> 2) & 3u); }
        else { row = (uint32_t)(64 * wave + 8 * t + (lane >> 3)); slot = (uint32_t)(lane & 7) ^ ((row >> 1) & 7u); }
        gA[t] = reinterpret_cast<const unsigned char *>(a.qhi) + (size_t)(q0 + row) * a.dim * 2 + slot * 16;
    }
#pragma unroll
    for (int t = 0; t < GB; ++t) {
        const uint32_t row = (uint32_t)(32 * wave + 16 * t + (lane >> 2));
        const uint32_t slot = (uint32_t)(lane & 3) ^ ((row >> 2) & 3u);
        uint32_t rloc = r0 + row;
        if (rloc >= a.nrows) rloc = a.nrows - 1;
        const size_t node = a.subset ? a.subset[a.row0 + rloc] : (size_t)a.row0 + rloc;
        gB[t] = reinterpret_cast<const unsigned char *>(a.rows) + node * a.dim * (FP8 ? 1 : 2) + slot * 16;
    }
    auto issue_stage = [&](uint32_t s) {
        unsigned char *sA = lds + (s % NBUF) * STAGE + wave * (64 * AROWB);
        unsigned char *sB = lds + (s % NBUF) * STAGE + ASTAGE + wave * (32 * BROWB);
#pragma unroll
        for (int t = 0; t < GA; ++t) HVX_GLDS16(gA[t] + s * (uint32_t)AROWB, sA + t * 1024);
#pragma unroll
        for (int t = 0; t < GB; ++t) HVX_GLDS16(gB[t] + s * (uint32_t)BROWB, sB + t * 1024);
    };
    const int fr = lane & 31, h = lane >> 5;
    int off128[4], off64[2];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) off128[kk] = fr * 128 + (((2 * kk + h) ^ ((fr >> 1) & 7)) << 4);
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) off64[jj] = fr * 64 + (((2 * jj + h) ^ ((fr >> 2) & 3)) << 4);
    const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>(lds);
    const uint32_t baseA = lds0 + (uint32_t)(wm * (128 * AROWB)), baseB = lds0 + (uint32_t)(ASTAGE + wn * (64 * BROWB));

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    uint4 c8[2];
    auto read_raw = [&](uint32_t buf, int kk, bf16x8 (&fa)[4], bf16x8 (&fb)[2]) { // 6 reads (bf16; fp8 even steps) or 4 (fp8 odd steps)
        const uint32_t pa = baseA + buf * (uint32_t)STAGE + (uint32_t)(FP8 ? off128[kk] : off64[kk]);
        fa[0] = __builtin_bit_cast(bf16x8, lds_read16<0>(pa));
        fa[1] = __builtin_bit_cast(bf16x8, lds_read16<32 * AROWB>(pa));
        fa[2] = __builtin_bit_cast(bf16x8, lds_read16<64 * AROWB>(pa));
        fa[3] = __builtin_bit_cast(bf16x8, lds_read16<96 * AROWB>(pa));
        if (FP8) {
            if ((kk & 1) == 0) {
                const uint32_t pb = baseB + buf * (uint32_t)STAGE + (uint32_t)off64[kk >> 1];
                c8[0] = lds_read16<0>(pb);
                c8[1] = lds_read16<32 * 64>(pb);
            }
        } else {
            const uint32_t pb = baseB + buf * (uint32_t)STAGE + (uint32_t)off64[kk];
            fb[0] = __builtin_bit_cast(bf16x8, lds_read16<0>(pb));
            fb[1] = __builtin_bit_cast(bf16x8, lds_read16<32 * 64>(pb));
        }
    };
    auto widen = [&](int kk, bf16x8 (&fb)[2]) {
        if (!FP8) return;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t w0 = (kk & 1) ? c8[j].z : c8[j].x, w1 = (kk & 1) ? c8[j].w : c8[j].y;
            const f32x2 a01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, false), a23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w0, true);
            const f32x2 b01 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, false), b23 = __builtin_amdgcn_cvt_pk_f32_fp8((int)w1, true);
            uint4 wv;
            wv.x = __builtin_amdgcn_perm(__float_as_uint(a01[1]), __float_as_uint(a01[0]), 0x07060302u);
            wv.y = __builtin_amdgcn_perm(__float_as_uint(a23[1]), __float_as_uint(a23[0]), 0x07060302u);
            wv.z = __builtin_amdgcn_perm(__float_as_uint(b01[1]), __float_as_uint(b01[0]), 0x07060302u);
            wv.w = __builtin_amdgcn_perm(__float_as_uint(b23[1]), __float_as_uint(b23[0]), 0x07060302u);
            fb[j] = __builtin_bit_cast(bf16x8, wv);
        }
    };
    auto mfma8 = [&](const bf16x8 (&fa)[4], const bf16x8 (&fb)[2]) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    };

    const uint32_t nstage = a.dim / (uint32_t)KS;
#pragma unroll
    for (int s = 0; s < NBUF - 1; ++s)
        if ((uint32_t)s < nstage) issue_stage((uint32_t)s);
    bf16x8 fa0[4], fb0[2], fa1[4], fb1[2];
    for (uint32_t s = 0; s < nstage; ++s) {
        // stage s has landed when at most the copies of the younger stages in flight (NBUF - 2 of them) are outstanding
        const uint32_t younger = nstage - 1u - s < (uint32_t)(NBUF - 2) ? nstage - 1u - s : (uint32_t)(NBUF - 2);
        if (younger >= 1u) wait_vmcnt<G>(); else wait_vmcnt<0>();
        __builtin_amdgcn_s_barrier(); // everyone's copies of stage s are in LDS; nobody still reads the buffer of stage s - 1
        if (s + (uint32_t)(NBUF - 1) < nstage) issue_stage(s + (uint32_t)(NBUF - 1));
        const uint32_t buf = s % NBUF;
        read_raw(buf, 0, fa0, fb0);
#pragma unroll
        for (int kk = 0; kk < SPS; kk += 2) {
            read_raw(buf, kk + 1, fa1, fb1);                  // step kk + 1 requested ...
            if (FP8) wait_lgkm<4>(); else wait_lgkm<6>();      // ... step kk has arrived (fp8: with the codes of both steps)
            widen(kk, fb0);
            widen(kk + 1, fb1);                                // before the next pair's codes replace c8
            mfma8(fa0, fb0);
            __builtin_amdgcn_sched_barrier(0);
            if (kk + 2 < SPS) {
                read_raw(buf, kk + 2, fa0, fb0);
                wait_lgkm<6>();
            } else {
                wait_lgkm<0>();
            }
            mfma8(fa1, fb1);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    tile_epilogue<FP8>(a, acc, lds, q0, r0, wm, wn, tid, xmax2, wg_overflow);
}

// ---- the MX-scaled fp8 build (round 4; VERDICT r3 missing #6): fp8 rows x fp8 query pieces on v_mfma_scale_f32_32x32x64_f8f6f4, the
// only large-K low-precision matrix instruction of gfx950 (measured 4 447 TFLOP/s against 1 820 for bf16 32x32x16 in
// scripts/mfma_rate_probe.hip).  Same tile, same stage geometry and the same copies as flat_tile2_kernel<1>: a stage is 64 deep,
// a query's stage row is 128 bytes -- but they hold the query as TWO e4m3 pieces (64 hi codes | 64 lo codes, split_queries_mx_kernel)
// instead of 64 bf16 values, and the row codes go into the matrix cores as they are: no v_cvt_pk_f32_fp8 / v_perm widening (8 VALU
// operations per fragment), and K = 64 per instruction.  Per stage and wavefront: 4 + 16 fragment reads (ds_read_b128: 32 consecutive
// codes of a tile row per lane = the operand layout, tests/native/mx_probe.hip), 16 matrix instructions (8 hi, 8 lo; 64 cycles each by
// the bf16-relative rate, i.e. the same 1 024 cycles per stage as 32 bf16 steps -- the gain, if any, is the measured rate and the
// missing VALU work).  The query's power-of-two scale rides in the instruction's block scale (E8M0, the lo piece 4 less); the rows'
// f32 scales stay in the epilogue as before.
typedef __attribute__((ext_vector_type(8))) int i32x8;

__global__ __launch_bounds__(256, 2) void flat_tile2mx_kernel(MfmaArgs a, float xmax2, uint32_t *wg_overflow) {
    constexpr int AROWB = 128, BROWB = 64;
    constexpr int ASTAGE = kTM * AROWB, STAGE = ASTAGE + kTN * BROWB; // 40 KB
    constexpr int NBUF = 2;
    constexpr int GA = AROWB / 16, GB = 2;
    __shared__ __attribute__((aligned(1024))) unsigned char lds[NBUF * STAGE];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    uint32_t qt, rt;
    if (!tile_coords(a, qt, rt)) return;
    const uint32_t q0 = qt * kTM, r0 = rt * kTN;

    const unsigned char *gA[GA], *gB[GB];
#pragma unroll
    for (int t = 0; t < GA; ++t) {
        const uint32_t row = (uint32_t)(64 * wave + 8 * t + (lane >> 3)), slot = (uint32_t)(lane & 7) ^ ((row >> 1) & 7u);
        gA[t] = reinterpret_cast<const unsigned char *>(a.qhi) + (size_t)(q0 + row) * a.dim * 2 + slot * 16;
    }
#pragma unroll
    for (int t = 0; t < GB; ++t) {
        const uint32_t row = (uint32_t)(32 * wave + 16 * t + (lane >> 2));
        const uint32_t slot = (uint32_t)(lane & 3) ^ ((row >> 2) & 3u);
        uint32_t rloc = r0 + row;
        if (rloc >= a.nrows) rloc = a.nrows - 1;
        const size_t node = a.subset ? a.subset[a.row0 + rloc] : (size_t)a.row0 + rloc;
        gB[t] = reinterpret_cast<const unsigned char *>(a.rows) + node * a.dim + slot * 16;
    }
    auto issue_stage = [&](uint32_t s) {
        unsigned char *sA = lds + (s % NBUF) * STAGE + wave * (64 * AROWB);
        unsigned char *sB = lds + (s % NBUF) * STAGE + ASTAGE + wave * (32 * BROWB);
#pragma unroll
        for (int t = 0; t < GA; ++t) HVX_GLDS16(gA[t] + s * (uint32_t)AROWB, sA + t * 1024);
#pragma unroll
        for (int t = 0; t < GB; ++t) HVX_GLDS16(gB[t] + s * (uint32_t)BROWB, sB + t * 1024);
    };
    const int fr = lane & 31, h = lane >> 5;
    // fragment reads: 32 consecutive codes = two 16-byte slots; queries: hi codes in slots 0-3, lo codes in slots 4-7 of the 128-byte row
    int offA[2][2], offB[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        offA[0][t] = fr * 128 + (((2 * h + t) ^ ((fr >> 1) & 7)) << 4);
        offA[1][t] = fr * 128 + (((4 + 2 * h + t) ^ ((fr >> 1) & 7)) << 4);
        offB[t] = fr * 64 + (((2 * h + t) ^ ((fr >> 2) & 3)) << 4);
    }
    const uint32_t lds0 = (uint32_t)reinterpret_cast<uintptr_t>(lds);
    const uint32_t baseA = lds0 + (uint32_t)(wm * (128 * AROWB)), baseB = lds0 + (uint32_t)(ASTAGE + wn * (64 * BROWB));
    // block scales of this lane's four query rows (one per 32-query tile): E8M0 of the hi piece, the lo piece is 2^-4 of it
    int sc_hi[4], sc_lo[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int e = (int)a.qexp[q0 + (uint32_t)(wm * 128 + i * 32 + fr)]; // (queries are padded to 256: the padding rows hold zero codes)
        sc_hi[i] = e;
        sc_lo[i] = e >= 4 ? e - 4 : 0;
    }

    f32x16 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    auto frag = [&](uint32_t addr0, uint32_t addr1) -> i32x8 {
        const uint4 x = lds_read16<0>(addr0), y = lds_read16<0>(addr1);
        i32x8 v;
        v[0] = (int)x.x; v[1] = (int)x.y; v[2] = (int)x.z; v[3] = (int)x.w;
        v[4] = (int)y.x; v[5] = (int)y.y; v[6] = (int)y.z; v[7] = (int)y.w;
        return v;
    };
    const uint32_t nstage = a.dim / 64u;
    issue_stage(0);
    for (uint32_t s = 0; s < nstage; ++s) {
        wait_vmcnt<0>();              // this wave's copies of stage s have landed ...
        __builtin_amdgcn_s_barrier(); // ... everyone's have; nobody still reads the other buffer
        if (s + 1 < nstage) issue_stage(s + 1);
        const uint32_t buf = s % NBUF, pa = baseA + buf * (uint32_t)STAGE, pb = baseB + buf * (uint32_t)STAGE;
        // all 20 fragment reads of the stage first, into registers of their own (a read that lands in a register an earlier matrix
        // instruction may still be fetching its operand from would be a hazard nobody checks for an inline-asm read)
        i32x8 fb[2], fh[4], fl[4];
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j] = frag(pb + (uint32_t)(j * 32 * BROWB + offB[0]), pb + (uint32_t)(j * 32 * BROWB + offB[1]));
#pragma unroll
        for (int i = 0; i < 4; ++i) fh[i] = frag(pa + (uint32_t)(i * 32 * AROWB + offA[0][0]), pa + (uint32_t)(i * 32 * AROWB + offA[0][1]));
#pragma unroll
        for (int i = 0; i < 4; ++i) fl[i] = frag(pa + (uint32_t)(i * 32 * AROWB + offA[1][0]), pa + (uint32_t)(i * 32 * AROWB + offA[1][1]));
        wait_lgkm<8>(); // the row codes and the hi pieces have arrived (LDS answers in order), the lo pieces are on their way
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fh[i], fb[j], acc[i][j], 0, 0, 0, sc_hi[i], 0, 127);
        __builtin_amdgcn_sched_barrier(0);
        wait_lgkm0();
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fl[i], fb[j], acc[i][j], 0, 0, 0, sc_lo[i], 0, 127);
        __builtin_amdgcn_sched_barrier(0);
    }
    tile_epilogue<true>(a, acc, lds, q0, r0, wm, wn, tid, xmax2, wg_overflow);
}

// the launch: 256 x 128 tiles, 256 threads, two workgroups per CU; super-tiles of 64 workgroups per XCD (tile_coords)
hipError_t launch_flat_tile(const MfmaArgs &a, int kind, uint32_t bpad, float xmax2, uint32_t *wg_overflow, bool mx, hipStream_t s) {
    if (a.nrows == 0) return hipSuccess;
    if (a.dim % 64u != 0u || bpad % (uint32_t)kTM != 0u) return hipErrorInvalidValue;
    if (mx && kind != 1) return hipErrorInvalidValue; // (the MX build multiplies fp8 codes)
    MfmaArgs t = a;
    t.nq_tiles = bpad / kTM;
    t.nr_tiles = (a.nrows + kTN - 1) / kTN;
    t.sup_q = std::min<uint32_t>(t.nq_tiles, 8u);
    t.sup_r = 64u / t.sup_q;
    t.sup_qblocks = (t.nq_tiles + t.sup_q - 1) / t.sup_q;
    const uint32_t rblocks = (t.nr_tiles + 8u * t.sup_r - 1) / (8u * t.sup_r);
    const dim3 grid(8u * rblocks * t.sup_qblocks * t.sup_r * t.sup_q);
    if (mx) hipLaunchKernelGGL(flat_tile2mx_kernel, grid, dim3(256), 0, s, t, xmax2, wg_overflow);
    else if (kind == 1) hipLaunchKernelGGL((flat_tile2_kernel<1>), grid, dim3(256), 0, s, t, xmax2, wg_overflow);
    else hipLaunchKernelGGL((flat_tile2_kernel<0>), grid, dim3(256), 0, s, t, xmax2, wg_overflow);
    return hipGetLastError();
}

} // namespace hvx
