// hvx_flat_mfma.h -- launch interface shared by the two contraction kernels of the matrix-core exact scan
// (hvx_flat_mfma.hip: 128 x 128 tiles, writes the score matrix or filters; hvx_flat_tile.hip: 256 x 128 tiles, filters only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hvx {

struct MfmaArgs {
    const uint16_t *qhi, *qlo; // [bpad][dim]
    const uint32_t *subset;    // optional: scan position -> row (restricted scans); NULL = the rows themselves
    const void *rows;          // [n][dim] bf16, or fp8 codes
    const float *rowscale;     // [n] fp8 only; NULL for cosine over fp8 rows (rowterm = the codes' norms)
    const float *rowterm;      // [n]: |x|^2 (L2) or |x| (cosine)
    const float *qn2;          // [b]
    uint32_t dim, b, row0, nrows, metric;
    float *dist;               // [b][chunk_ld]
    uint32_t chunk_ld;
    // FILT launches: only scores below the query's running threshold leave the tile, as (score, row) pairs
    const float *thr;          // [b] approximate score of the (m+1)-th candidate so far (+inf while fewer are known)
    float *cand_sc;            // [b][cand_cap]
    uint32_t *cand_id;         // [b][cand_cap] internal ids
    uint32_t *cand_cnt;        // [b] pairs appended (may exceed cand_cap: overflow, detected by the merge)
    uint32_t cand_cap;
    // 1-D launch: workgroup id -> (row tile, query tile).  Rows are walked in groups of `group_tiles` row tiles (~64 MB of
    // rows: they stay in the Infinity Cache), inside a group the QUERY tile is the outer loop: a query tile's 128 x dim
    // operand stays in L2 while the group's row tiles stream past it, and the group's rows come from HBM once.
    uint32_t nq_tiles, nr_tiles, group_tiles;
    // large-tile kernels: XCD-aware super-tiles (hvx_flat_tile.hip)
    uint32_t sup_q, sup_r, sup_qblocks;
    const uint32_t *qexp; // MX build of the fp8 tile kernel: [bpad] E8M0 scale of a query's hi codes (a.qhi = the e4m3 operand there)
};

// large-tile filtered contraction (hvx_flat_tile.hip: 256 x 128 tiles, two 256-thread workgroups per CU).  kind: 0 = bf16 rows (a bf16
// index, or the bf16 shadow of an f32 index; a.rows in the order a.qhi uses), 1 = fp8 codes (a.qhi in tile order, see tile_slot_fp8).
// a.dim % 64 == 0.  `wg_overflow` is set when a workgroup's pair list overflowed (the caller repeats the scan unfiltered).
// mx (fp8 codes only): the MX-scaled fp8 build, a.qhi = two e4m3 pieces per query value, a.qexp their scales
hipError_t launch_flat_tile(const MfmaArgs &a, int kind, uint32_t bpad, float xmax2, uint32_t *wg_overflow, bool mx, hipStream_t s);

// one-pass score matrix for small batches (hvx_flat_smallb.hip): b <= 128 queries, kind 0 = bf16 rows / shadow, 2 = f32 rows
bool flat_smallb_supported(uint32_t dim, uint32_t b, int kind);
hipError_t launch_flat_smallb(const MfmaArgs &a, int kind, bool full, uint32_t cus, uint32_t build, hipStream_t s); // raw dot products into a.dist; build 1 = never the ring build
// sort-free selection over those dot products: every slice's kc (<= 256) smallest approximate scores as (score, row) pairs
hipError_t launch_flat_select_radix(const MfmaArgs &a, uint32_t kc, uint32_t *status, float *sl_sc, uint32_t *sl_id, uint32_t sl_stride,
                                    uint32_t *out_slices, hipStream_t s);

// ---- the exact scan's error bound E: |approximate score - reference-order score| for every row, the ONE number the re-rank certificate
// (hvx_flat_mfma.hip, rerank_bf16_kernel: kth < t - E) and the exact tail (hvx_flat_tail.hip: re-score iff s~ - E <= T) rest on ----
// Contraction kinds: what the matrix cores multiplied.
enum ScanErrKind : uint32_t {
    kErrBf16OnePass,      // bf16 rows x the query's bf16 hi part
    kErrBf16Full,         // bf16 rows x (hi + lo)
    kErrF32ShadowOnePass, // f32 rows through their bf16 shadow (RNE) x hi
    kErrF32RegOnePass,    // f32 rows rounded to bf16 (RNE) in registers x hi
    kErrF32Full,          // f32 rows split hi + lo too: q_hi.x_hi + q_lo.x_hi + q_hi.x_lo
    kErrFp8OnePass,       // fp8 codes widened to bf16 (exact; the row scale is applied in f32) x hi
    kErrFp8Full,          // fp8 codes x (hi + lo)
    kErrMxFp8,            // fp8 codes x the query as two e4m3 pieces (the MX-scaled 256 x 256 build)
};

// E relative to (|q|^2 + max |x|^2) / 2 for L2, absolute for cosine, at `dim` terms.  u = 2^-8 is bf16's unit roundoff: 8 significant
// bits, so RNE moves a value by <= 2^-8 of it (half of 2^-7, the step of [1, 2)).  Per dot product the contraction is off by <= eps |q||x|:
//   * one rounded operand (bf16 / fp8 rows x q_hi): |q - q_hi| <= u |q| per element, eps = u;
//   * both rounded (f32 rows x q_hi, shadow or registers: both RNE): q_hi x_hi - q x = (q_hi - q) x_hi + q (x_hi - x), eps = 2u + u^2;
//   * the hi + lo split of one value leaves r = v - hi - lo with |r| <= 2^-17 |v| (v - hi, |v - hi| <= 2^-8 2^e, rounded again: half a
//     step of its binade, <= 2^-17 2^e <= 2^-17 |v|), so bf16 / fp8 rows x (hi + lo): eps = 2^-17; f32 rows with q_lo.x_lo dropped:
//     r_q.x + q_hi.r_x + q_lo.x_lo + q_lo.r_x <= (2^-17 + 2^-17 (1 + u) + 2^-16 + 2^-25) |q||x| <= (2^-15 + 2^-23) |q||x|;
//   * MX: hi = RNE(q / s) and lo = RNE(16 (q - s hi) / s) in e4m3 (3 mantissa bits): for q / s in [2^e, 2^e+1) the hi residual is <= 2^(e-4),
//     lo lies below 2^e and rounds by <= 2^(e-5), i.e. 2^(e-9) of q / s -- |q - s hi - s lo / 16| <= 2^-9 |q| for normal pieces; a
//     subnormal lo piece is off by <= 2^-10 s / 16 with s <= max |q| / 128 (split_queries_mx_kernel), i.e. <= 2^-21 max |q| per element,
//     <= 2^-21 sqrt(dim) |q||x| summed against x.  eps = u + 2^-21 sqrt(dim): the normal pieces' term keeps u = 2^-8, twice their worst
//     case (the value the MX build has used for L2 since it was added; tests/test_exact_bound_fixtures.py drives the error to 0.4-0.5 of the bound).
// L2: s = |q|^2 + |x|^2 - 2 q.x moves by 2 eps |q||x| <= 2 eps (|q|^2 + |x|^2) / 2.  Cosine: s = (1 - c) / 2 with c = q.x / (|q||x|) moves by
// eps / 2; the bound keeps eps, a factor two over that worst case (the value the cosine scan has always used).  Both add f32 accumulation
// over dim terms in BOTH summation orders (6 dim 2^-24), doubled for whatever order the matrix core accumulates in, and 2^-18 for the f32
// roundings of |q|^2, |x|^2 (f64 sums rounded once) and the few f32 operations of the epilogue.
__host__ __device__ inline float scan_error_bound(uint32_t kind, bool l2, uint32_t dim) {
    const float u = 0x1p-8f;
    float eps;
    switch (kind) {
    case kErrBf16OnePass: case kErrFp8OnePass: eps = u; break;
    case kErrBf16Full: case kErrFp8Full: eps = 0x1p-17f; break;
    case kErrF32ShadowOnePass: case kErrF32RegOnePass: eps = 2.0f * u + u * u; break;
    case kErrF32Full: eps = 0x1p-15f + 0x1p-23f; break;
    case kErrMxFp8: eps = u + 0x1p-21f * sqrtf((float)dim); break;
    default: eps = 1.0f; break; // (unknown kind: a bound that certifies nothing)
    }
    return (l2 ? 2.0f * eps : eps) + 12.0f * (float)dim * 0x1p-24f + 0x1p-18f;
}

// ---- cosine: the magnitude precondition of the bound ----
// scan_error_bound's cosine figure is relative to |q||x| and holds only while |q|^2, |q||x|, the dot product and every partial sum of the
// contraction are normal f32 numbers.  Cosine has no component limit (the reference answers any finite magnitude through its f64
// fallback), so the scans make the precondition true instead of assuming it:
//   * the query: cosine is scale-invariant, so the contraction's copy of a cosine query (split_queries_kernel, split_queries_mx_kernel)
//     is q^ = q 2^-e with max |q^_i| in [2^12, 2^13) -- an exact scaling -- and qn2 is |q^|^2: 2^12 <= |q^| < 2^13 sqrt(dim) <= 2^18.3
//     (dim <= 1536) whatever |q| was.  The exact kernels (re-rank, tail, VALU) read the caller's query, never q^.
//   * a row is TRUSTED when its norm header lies in [kCosTermMin, kCosTermMax] = [2^-100, 2^107].  Then every partial sum is at most
//     |q^||x| < 2^126 (no overflow), and whatever a matrix core may flush -- products below 2^-126, at most dim 2^-126 in all, and row
//     elements below 2^-126, at most sqrt(dim) 2^-126 of |x| -- is below 2^-27 |q^||x| and 2^-20 |q^||x|: inside the bound's 2^-18 term.
//   * an UNTRUSTED row (an outlier whose norm overflows the product, a norm header clamped at FLT_MAX, a norm near the subnormals) and
//     a non-finite dot product have no approximation: approx_half_cosine gives them 0, the smallest score there is.  Such a row
//     passes every filter and is always among the candidates, where it is re-scored in the reference's order; it never moves the
//     threshold the wrong way (a certificate whose (m+1)-th approximate score is 0 fails: more than m rows are untrusted -- the exact
//     tail, the VALU scan or the next attempt answers, never a guess).
//   * non-zero fp8 rows never leave the trusted range: x = scale codes, so cos(q, x) = cos(q, codes) and their scan divides the raw
//     accumulator by |q^||codes| (fp8_code_norm_kernel; MfmaArgs.rowscale is NULL then): |codes| lies in [448, 448 sqrt(dim)].  An
//     all-zero row (codes 0, scale 1) has |codes| = 0 and is untrusted.
constexpr float kCosTermMin = 0x1p-100f, kCosTermMax = 0x1p107f;
constexpr int kCosQueryExp = 12; // max |q^_i| in [2^12, 2^13)
__host__ __device__ inline bool cosine_term_trusted(float term) { return term >= kCosTermMin && term <= kCosTermMax; }
// exponent e of the exact scaling q^ = q 2^-e of a cosine query whose largest finite magnitude is mx (0: no scaling)
__host__ __device__ inline int cosine_query_exponent(float mx) {
    if (!(mx > 0.f)) return 0;
    int ex;
    (void)frexpf(mx, &ex); // mx = f 2^ex, f in [0.5, 1)
    return ex - 1 - kCosQueryExp;
}
#if defined(__HIPCC__)
// (1 - c) / 2 from the contraction's dot product, qn = |q^| and the row's norm header; 0 where there is no approximation (see above)
__device__ __forceinline__ float approx_half_cosine(float dot, float qn, float term) {
    if (!cosine_term_trusted(term) || !(__builtin_fabsf(dot) <= 3.4028234664e38f)) return 0.f;
    const float den = qn * term;
    float c = den > 0.f ? dot / den : 0.f; // (den = 0: a rejected query, masked to zeros; its scores are never reported)
    c = c < -1.f ? -1.f : (c > 1.f ? 1.f : c);
    return (1.0f - c) * 0.5f;
}
#endif

// position of stored code `slot` (its index in the fp8 row) in the query operand of the 256 x 256 fp8 kernel: inside a
// 64-code stage, MFMA step kk (0..3), lane half h, element e read code (2 (kk >> 1) + h) * 16 + (kk & 1) * 8 + e, so one
// ds_read_b128 of the code tile feeds two steps.
__host__ __device__ inline uint32_t tile_slot_fp8(uint32_t slot) {
    const uint32_t c = slot & 63u, u = c >> 4, sb = (c >> 3) & 1u, e = c & 7u;
    const uint32_t kk = (u >> 1) * 2u + sb, h = u & 1u;
    return (slot & ~63u) + kk * 16u + h * 8u + e;
}

#if defined(__HIPCC__)
// histogram increment with the wavefront's most common digits combined first: approximate scores of one query share their
// leading bytes, and 64 lanes adding to ONE LDS word serialise (measured: the four selection rounds of a 4 096-score slice cost
// 26 us with per-lane atomics alone, the rest of the kernel 12; two fixed rounds of combining still left 40-70 us kernels on the
// topic-ordered C3 corpus, whose scores share three bytes).
__device__ __forceinline__ void radix_count(uint32_t *hist, bool active, uint32_t digit) {
    // groups of equal digits are taken out one at a time (the first active lane's digit: one add for all lanes holding it) for as long
    // as they are BIG: a group of a dozen lanes costs a dozen serialised adds against one round here, a group of four costs the same
    // either way, and a wavefront of many small groups is served best by its per-lane adds (the clustered corpus: a 12-round loop that
    // went on at >= 4 lanes per group was 15-40 % slower than this; the topic-ordered C3 corpus has the big groups)
    for (int round = 0; round < 6; ++round) {
        const unsigned long long todo = __ballot(active);
        if (!todo) return;
        if (__builtin_popcountll(todo) < 12) break;
        const int leader = __builtin_ctzll(todo);
        const uint32_t pivot = (uint32_t)__shfl((int)digit, leader, 64);
        const bool same = active && digit == pivot;
        const unsigned long long votes = __ballot(same);
        if ((int)(threadIdx.x & 63u) == leader) atomicAdd(&hist[pivot], (uint32_t)__builtin_popcountll(votes));
        active = active && !same;
        if (__builtin_popcountll(votes) < 12) break;
    }
    if (active) atomicAdd(&hist[digit], 1u);
}

// One step of an 8-bit radix selection, run by EVERY wavefront of the workgroup on the same 256-bin histogram (no broadcast, no
// extra barrier): the digit g whose bin holds the kk-th smallest key (1-based) among the keys counted in `hist`, and the number
// of counted keys with a smaller digit.  kk <= the histogram's total by construction of the callers.
__device__ __forceinline__ void radix_digit_of_rank(const uint32_t *hist, uint32_t kk, uint32_t &g, uint32_t &below) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint4 c = reinterpret_cast<const uint4 *>(hist)[lane]; // bins 4 lane .. 4 lane + 3
    const uint32_t s = c.x + c.y + c.z + c.w;
    uint32_t incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if ((int)lane >= d) incl += up;
    }
    const uint32_t excl = incl - s;
    const bool mine = excl < kk && kk <= incl;
    uint32_t gg = 0, bb = 0;
    if (mine) {
        uint32_t run = excl;
        gg = 4u * lane; bb = run;
        if (run + c.x < kk) { run += c.x; gg = 4u * lane + 1u; bb = run;
            if (run + c.y < kk) { run += c.y; gg = 4u * lane + 2u; bb = run;
                if (run + c.z < kk) { run += c.z; gg = 4u * lane + 3u; bb = run; } } }
    }
    const unsigned long long m = __ballot(mine);
    const int src = m ? __builtin_ctzll(m) : 0;
    g = __shfl(gg, src, 64);
    below = __shfl(bb, src, 64);
}
#endif

} // namespace hvx
