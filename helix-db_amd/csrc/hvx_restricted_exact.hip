// hvx_restricted_exact.hip -- the restricted (prefiltered) exact scan as ONE launch (round 6; SURVEY.md rows a10 / a12, BASELINE config #3).
//
// Reference: restricted_exact_scan + restricted_score_keys (crates/db/src/search/vector/restricted.rs:753-835, :661-704): score every
// candidate with D::distance, keep the k smallest by Candidate order (score, then id: model.rs:55-61), return them sorted; candidate
// ids that hold no vector are skipped (:615-659); RestrictedVectorCandidates is a SET (:303-371: duplicates count once).  The
// operator above it serves one query with ITS OWN candidate set per call (execution/interpreter/access/search/storage.rs:140-163).
//
// Why a second exact scan beside hvx_flat*.hip: the matrix-core pipeline (approximate contraction -> selection -> exact re-rank ->
// certificate read back by the host) is built for candidate sets that are streams -- 10^5 rows and more per launch.  The sets a
// where_() filter produces are mostly small (10^2 .. 10^4 ids), there are MANY of them in flight (one per request), and each request
// brings its own: four dependent launches and a host round trip per set left the device idle (0.001 - 0.12 of HBM, one
// set at a time).  This kernel answers a whole batch of (query, candidate set) pairs in one launch, exactly:
//   * grid = (slices, query tiles); a workgroup = 4 wavefronts = 32 row groups of 8 lanes (hvx_device.h); a tile's TQ queries sit in
//     LDS, every row group gathers 2 candidate rows at a time (8 lanes x 16 B = whole 128-byte lines, 8 chunks ahead) and scores them
//     against the TQ queries in the reference's summation order -- the scores ARE the reference's f32 bits, nothing to certify;
//     the FMAs are packed (v_pk_add_f32 / v_pk_fma_f32: two virtual lanes per instruction, same IEEE operations);
//   * per-query candidate sets arrive as EXTERNAL ids (CSR): id -> row (arithmetic for contiguous ids, binary search otherwise), deleted
//     rows and unknown ids drop out, duplicates are rejected where the result list is kept;
//   * every wavefront keeps its k smallest (score, row) pairs per query in a register list (hvx_beam.h: ballot rank + one wave shift);
//     the four lists of a workgroup meet in LDS, the slices' lists in HBM, and the LAST workgroup of a tile to finish (one fetch-add)
//     merges them and writes ids / scores / counts / status -- straight into pinned host rows when the caller passes such.
//   * k <= 64 is one register pair per lane; k <= 256 / k <= 800 (MAX_RESTRICTED_RESULT_COUNT, restricted.rs:55) are lists of 4 / 13
//     registers per lane, one query per tile, built in hvx_restricted_wide4.hip / hvx_restricted_wide13.hip (kernel: hvx_restricted_direct.h).
// Algorithmic bytes per (query tile, candidate) = dim x sizeof(row element); the roofline is HBM for one query per set, the packed
// FMA rate for tiles of several queries over a shared set (8 lane-operations per row chunk and query).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "hvx_restricted_direct.h" // the kernel, its argument block, launch_direct_kernel

using namespace hvx;

#define HIP_TRY(expr)                                                                              \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) return fail(HVX_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

namespace {

// Queries from (pinned) host memory: validation (ValidatedMetricVector::try_new, domain.rs:113-157), the cosine header, and the device
// copy the scan reads -- one kernel instead of a DMA copy + a kernel (a copy engine hop costs more than these few KB are worth)
__global__ __launch_bounds__(256) void stage_queries_kernel(const float *src, float *dst, uint32_t dim, uint32_t b) {
    const uint32_t q = blockIdx.x;
    if (q >= b) return;
    for (uint32_t i = threadIdx.x; i < dim; i += 256) dst[(size_t)q * dim + i] = src[(size_t)q * dim + i];
}

// Queries per tile of a SHARED set: registers bound it (8 accumulator + 4 list registers per query next to the gather's 128) -- the builds
// below are the ones that keep everything in registers (profiles/r06_kernel_meta.json); the any-shape build scores one row at a time: two.
// Every candidate row is then read b / TQ times, from L2 after the first.
constexpr bool tq_built(uint32_t metric, int nk, bool bf, int tq) {
    if (tq <= 1) return true;
    if (nk == 0) return tq <= 2;
    if (metric == kCosine) {
        if (bf) return nk == 32 ? false : tq <= 2;
        return tq <= 4;
    }
    if (bf) return nk <= 24 ? tq <= 8 : (nk <= 48 ? tq <= 4 : tq <= 2);
    return nk <= 24 ? tq <= 8 : tq <= 4;
}
uint32_t direct_tq(const DevIndex &d, uint32_t b, bool unrolled) {
    const int nk = unrolled ? (int)(d.dim >> 5) : 0;
    uint32_t tq = 8;
    while (tq > 1 && (tq > b || !tq_built(d.metric, nk, d.dtype == HVX_BF16, (int)tq))) tq >>= 1;
    return tq;
}

template <uint32_t METRIC, int NK, bool BF, bool FUSED> hipError_t launch_direct_q(const DirectArgs &a, uint32_t tq, bool ext, hipStream_t s) {
    const size_t row = (size_t)a.ix.ld * 4;
    const uint32_t tiles = (a.b + tq - 1) / tq;
    if (ext) return launch_direct_kernel(restricted_direct_kernel<METRIC, NK, BF, 1, true, FUSED, 1>, a, a.b, row, s);
    switch (tq) {
    case 1: return launch_direct_kernel(restricted_direct_kernel<METRIC, NK, BF, 1, false, FUSED, 1>, a, tiles, row, s);
    case 2: if constexpr (tq_built(METRIC, NK, BF, 2)) return launch_direct_kernel(restricted_direct_kernel<METRIC, NK, BF, 2, false, FUSED, 1>, a, tiles, 2 * row, s); else break;
    case 4: if constexpr (tq_built(METRIC, NK, BF, 4)) return launch_direct_kernel(restricted_direct_kernel<METRIC, NK, BF, 4, false, FUSED, 1>, a, tiles, 4 * row, s); else break;
    case 8: if constexpr (tq_built(METRIC, NK, BF, 8)) return launch_direct_kernel(restricted_direct_kernel<METRIC, NK, BF, 8, false, FUSED, 1>, a, tiles, 8 * row, s); else break;
    default: break;
    }
    return hipErrorInvalidValue;
}

template <uint32_t METRIC, bool BF> hipError_t launch_direct_nk(const DirectArgs &a, uint32_t tq, bool ext, bool unrolled, hipStream_t s) {
    if constexpr (METRIC != kL1) {
        if (unrolled) {
            switch (a.ix.dim >> 5) {
            case 4: return launch_direct_q<METRIC, 4, BF, true>(a, tq, ext, s);
            case 8: return launch_direct_q<METRIC, 8, BF, true>(a, tq, ext, s);
            case 12: return launch_direct_q<METRIC, 12, BF, true>(a, tq, ext, s);
            case 16: return launch_direct_q<METRIC, 16, BF, true>(a, tq, ext, s);
            case 24: return launch_direct_q<METRIC, 24, BF, true>(a, tq, ext, s);
            case 32: return launch_direct_q<METRIC, 32, BF, true>(a, tq, ext, s);
            case 48: return launch_direct_q<METRIC, 48, BF, true>(a, tq, ext, s);
            case 64: return launch_direct_q<METRIC, 64, BF, true>(a, tq, ext, s);
            case 96: return launch_direct_q<METRIC, 96, BF, true>(a, tq, ext, s);
            default: break;
            }
        }
    }
    if (BF) return launch_direct_q<METRIC, 0, BF, true>(a, tq, ext, s);
    return kernel_fused(a.ix.fkernel) ? launch_direct_q<METRIC, 0, false, true>(a, tq, ext, s) : launch_direct_q<METRIC, 0, false, false>(a, tq, ext, s);
}

// registers per lane of the result list: one pair serves k <= 64, the wide builds k <= 256 and k <= 800
uint32_t direct_width(uint32_t k) { return k <= 64u ? 1u : (k <= 256u ? 4u : 13u); }
// the unrolled wide builds: 768 and 1536 (the other unrolled shapes take the any-shape wide build)
bool wide_unrolled_shape(const DevIndex &d) { return (d.dim >> 5) == 24u || (d.dim >> 5) == 48u; }

bool direct_unrolled_shape(const DevIndex &d) {
    const uint32_t nk = d.dim >> 5;
    const bool dims = nk == 4 || nk == 8 || nk == 12 || nk == 16 || nk == 24 || nk == 32 || nk == 48 || nk == 64 || nk == 96;
    return d.dim % 32u == 0u && dims && d.fkernel == kKernelAvxFma && d.metric != kL1 && (d.dtype == HVX_BF16 || (d.ld == d.dim && d.dim_main == d.dim));
}

} // namespace

namespace hvx {

bool restricted_direct_supported(const hvx_index *ix, uint32_t k) {
    const DevIndex &d = ix->dev;
    if (d.n == 0 || k == 0 || k > 800u) return false; // MAX_RESTRICTED_RESULT_COUNT (restricted.rs:55)
    // a wide build's workgroup holds the query row and the four lists it hands over (8 x 64 R x 4 B) in LDS: 64 KiB at most
    if (k > 64u && (size_t)d.ld * 4 + (size_t)direct_width(k) * 2048u + 64u > 64u * 1024u) return false;
    if (d.dtype == HVX_F32) return true;                       // any dimension / metric / summation tree (group_distance)
    if (d.dtype == HVX_BF16) return d.metric != kL1 && d.dim % 64u == 0u; // what the import accepts for bf16 rows
    return false;                                              // fp8 rows: the matrix-core pipeline
}

// Where the wide builds are the better choice when nothing is forced (HVX_OPT_RESTRICTED_DIRECT = 2 takes them always).  An insertion into
// a list of R registers is a chain of ~14 R dependent instructions, and a wavefront inserts every candidate it sees until its list holds k:
// one query's scan is a serial chain that grows with k, while the older pipeline answers a list in 0.11 - 0.75 ms whatever k is -- but
// list after list.  Measured on 50 000 x 1536 f32 rows (profiles/restricted_wide_ab.log; one launch against the older pipeline, ms):
//   lists of 1 000 / 10 000 ids at k 800: 1 list 1.06 / 3.03 against 0.12 / 0.75; 4 lists 1.07 / 3.06 against 0.57 / 3.05; 8 lists
//   1.08 / 3.13 against 1.24 / 6.13; 64 lists 1.21 / 3.31 against 9.7 / 49.4; 256 lists of 1 000 ids at k 100: 1.13 against 43;
//   one list of 10 000 ids: k 100 0.38 against 0.47, k 128 0.44 against 0.58, k 256 0.72 against 0.71, k 300 1.76 against 0.71;
//   one list of 1 000 ids: k 128 0.22 against 0.12, k 256 0.29 against 0.11.
// The lines: 8 lists at k > 256 and 4 lists at k <= 256 (between 1 and 256 lists at k <= 256 nothing was measured: four lists of the
// older pipeline cost what one launch costs at k 256); ONE list at k <= 128 from 8 192 ids on (measured at 1 000 and at 10 000 only).
bool restricted_older_serves(const hvx_index *ix, uint32_t k) {
    const DevIndex &d = ix->dev;
    if (d.dtype != HVX_BF16) return true;
    const uint32_t nk = d.dim >> 5; // (flat_mfma_impl: the bf16 contraction's shapes and its selection's width)
    return k <= 511u && d.dim % 32u == 0u && (nk == 4 || nk == 8 || nk == 16 || nk == 24 || nk == 32 || nk == 48);
}
bool restricted_direct_pays(const hvx_index *ix, uint32_t k, uint32_t lists, uint64_t longest) {
    if (k <= 64u || ix->opt[HVX_OPT_RESTRICTED_DIRECT] == 2u || !restricted_older_serves(ix, k)) return true;
    if (lists == 1u) return k <= 128u && longest >= 8192u;
    return lists >= (k <= 256u ? 4u : 8u);
}

// scratch of the one-launch scan: the slices' lists and the two self-cleaning counter arrays
static int direct_scratch(hvx_index *ix, uint32_t b, uint32_t slices, uint32_t k, uint32_t tiles) {
    int rc;
    const size_t need = (size_t)b * slices * k;
    if (need > ix->cap_x_part) {
        if ((rc = ix->regrow((void **)&ix->x_part_sc, need * 4))) return rc;
        if ((rc = ix->regrow((void **)&ix->x_part_row, need * 4))) return rc;
        ix->cap_x_part = need;
    }
    const uint32_t words = std::max(b, tiles);
    if (words > ix->cap_x_ctl) {
        const uint32_t cap = std::max<uint32_t>(words, 1024u);
        if ((rc = ix->regrow((void **)&ix->x_bad, (size_t)cap * 4))) return rc;
        if ((rc = ix->regrow((void **)&ix->x_done, (size_t)cap * 4))) return rc;
        HIP_TRY(hipMemsetAsync(ix->x_bad, 0, (size_t)cap * 4, ix->stream));
        HIP_TRY(hipMemsetAsync(ix->x_done, 0, (size_t)cap * 4, ix->stream));
        ix->cap_x_ctl = cap;
    }
    return HVX_OK;
}

// Enqueue the one-launch exact scan for b device-resident, VALIDATED queries (ix->d_qstatus / d_qhdr hold their status and headers).
// Shared set: d_rows / n_rows (internal rows, ascending, unique).  Per-query sets: d_ext_ids + d_offsets[b + 1] (external ids, any
// order, duplicates allowed), max_set = the largest set's length.  Outputs: device-visible arrays (HBM or mapped host rows) of row
// length k_stride.  Nothing is synchronised here.
int restricted_direct_enqueue(hvx_index *ix, const float *d_queries, uint32_t b, uint32_t k, uint32_t k_stride, const uint32_t *d_rows,
                              uint32_t n_rows, const uint64_t *d_ext_ids, const uint64_t *d_offsets, uint32_t max_set, uint64_t *d_ids,
                              float *d_scores, uint32_t *d_counts, uint32_t *d_status, const uint32_t *d_lens, uint32_t ext_stride,
                              const uint32_t *d_n_rows) {
    const DevIndex &d = ix->dev;
    const bool ext = d_ext_ids != nullptr;
    const uint32_t width = direct_width(k);
    const bool unrolled = direct_unrolled_shape(d) && (width == 1u || wide_unrolled_shape(d));
    const uint32_t n = ext ? max_set : n_rows;
    const uint32_t tq = (ext || width > 1u) ? 1u : direct_tq(d, b, unrolled);
    const uint32_t tiles = ext ? b : (b + tq - 1) / tq;
    // slices: a whole number of 64-row passes each, enough workgroups to fill the chip four times over, at most 1 024 per query
    const uint32_t passes = std::max<uint32_t>(1u, (n + 63u) / 64u);
    uint32_t want = std::max<uint32_t>(1u, std::min<uint32_t>(1024u, (1024u + tiles - 1u) / tiles));
    if (width > 1u) {
        // every slice leaves k entries for the last workgroup to merge: a slice of a wide build holds 8 k candidates (a quarter of them per
        // wavefront: twice its list), and a set too small for that is still cut in four
        const uint32_t by_k = (n + 8u * k - 1u) / (8u * k);
        want = std::min(want, std::max(by_k, std::min<uint32_t>(4u, passes)));
    }
    const uint32_t per = (passes + want - 1u) / want;
    const uint32_t chunk = per * 64u, slices = std::max<uint32_t>(1u, (n + chunk - 1u) / chunk);
    int rc = direct_scratch(ix, b, slices, k, tiles);
    if (rc) return rc;
    DirectArgs a{};
    a.ix = d;
    a.queries = d_queries;
    a.qstatus = ix->d_qstatus;
    a.qhdr = ix->d_qhdr;
    a.rows = d_rows;
    a.n_rows = n_rows;
    a.n_rows_dev = d_n_rows;
    a.ext_ids = d_ext_ids;
    a.offsets = d_offsets;
    a.lens = d_lens;
    a.ext_stride = ext_stride;
    a.contiguous = ix->contiguous ? 1u : 0u;
    a.b = b; a.k = k; a.k_stride = k_stride;
    a.chunk = chunk; a.slices = slices;
    a.part_sc = ix->x_part_sc; a.part_row = ix->x_part_row; a.bad = ix->x_bad; a.done = ix->x_done;
    a.out_ids = d_ids; a.out_scores = d_scores; a.out_counts = d_counts; a.out_status = d_status;
    hipError_t e;
    const bool bf = d.dtype == HVX_BF16;
    if (width == 4u) e = restricted_direct_launch_wide4(&a, ext, unrolled, ix->stream);
    else if (width == 13u) e = restricted_direct_launch_wide13(&a, ext, unrolled, ix->stream);
    else switch (d.metric) {
    case kCosine: e = bf ? launch_direct_nk<kCosine, true>(a, tq, ext, unrolled, ix->stream) : launch_direct_nk<kCosine, false>(a, tq, ext, unrolled, ix->stream); break;
    case kL2: e = bf ? launch_direct_nk<kL2, true>(a, tq, ext, unrolled, ix->stream) : launch_direct_nk<kL2, false>(a, tq, ext, unrolled, ix->stream); break;
    default: e = launch_direct_nk<kL1, false>(a, tq, ext, false, ix->stream); break;
    }
    if (e != hipSuccess) return fail(HVX_ERR_DEVICE, "restricted exact scan launch: %s", hipGetErrorString(e));
    ix->last_scan_path = HVX_PATH_DIRECT;
    return HVX_OK;
}

// candidate ids of a batch from the batching operator's pinned slots (fixed stride) into device memory: only the ids that are there
__global__ __launch_bounds__(256) void stage_ids_kernel(const uint64_t *src, const uint32_t *lens, uint32_t stride, uint64_t *dst, uint32_t b) {
    const uint32_t q = blockIdx.x;
    if (q >= b) return;
    const uint32_t n = lens[q] < stride ? lens[q] : stride;
    for (uint32_t i = threadIdx.x; i < n; i += 256) dst[(size_t)q * stride + i] = src[(size_t)q * stride + i];
}
hipError_t launch_stage_ids(const uint64_t *src, const uint32_t *lens, uint32_t stride, uint64_t *dst, uint32_t b, hipStream_t s) {
    if (b == 0) return hipSuccess;
    hipLaunchKernelGGL(stage_ids_kernel, dim3(b), dim3(256), 0, s, src, lens, stride, dst, b);
    return hipGetLastError();
}

hipError_t launch_stage_queries(const float *src, float *dst, uint32_t dim, uint32_t b, hipStream_t s) {
    if (b == 0) return hipSuccess;
    hipLaunchKernelGGL(stage_queries_kernel, dim3(b), dim3(256), 0, s, src, dst, dim, b);
    return hipGetLastError();
}

} // namespace hvx

// Device-resident surface of the prefiltered branch: b queries in HBM, query q with its own candidate ids d_allowed_ids[q * stride ..
// + d_lens[q]) (external ids, any order, duplicates allowed, unknown ids skipped); exact strategy, one launch, nothing synchronised.
extern "C" int hvx_search_restricted_lists_device(const hvx_index *cix, const float *d_queries, uint32_t b, uint32_t k, const uint64_t *d_allowed_ids,
                                                  uint32_t stride, const uint32_t *d_lens, uint32_t max_len, uint64_t *d_out_ids, float *d_out_scores,
                                                  uint32_t *d_out_counts, uint32_t *d_out_status) {
    if (!cix || !d_queries || !d_allowed_ids || !d_lens || !d_out_ids || !d_out_scores || !d_out_counts) return fail(HVX_ERR_INVARIANT, "null argument");
    hvx_index *ix = const_cast<hvx_index *>(cix);
    if (k == 0) return fail(HVX_ERR_K_RANGE, "result count must be non-zero");
    if (b == 0) return HVX_OK;
    if (b > ix->max_batch) return fail(HVX_ERR_UNSUPPORTED, "batch %u exceeds max_batch %u given at import", b, ix->max_batch);
    if (max_len > stride) return fail(HVX_ERR_INVARIANT, "a candidate list longer than its slot");
    std::lock_guard<std::mutex> lock(ix->mu);
    ix->sync_rewrites();
    if (!restricted_direct_supported(ix, k))
        return fail(HVX_ERR_UNSUPPORTED, "the one-launch restricted scan serves k <= 800 over f32 / bf16 rows of a non-empty image (k > 64: rows of "
                    "at most %u floats, the query row and the lists' hand-over share 64 KiB of LDS)", k > 256u ? 9712u : 14320u);
    HIP_TRY(hipSetDevice(ix->device));
    HIP_TRY(launch_validate_queries(ix->dev, d_queries, b, ix->limit, ix->d_qstatus, ix->d_qhdr, ix->stream));
    return restricted_direct_enqueue(ix, d_queries, b, k, k, nullptr, 0, d_allowed_ids, nullptr, max_len, d_out_ids, d_out_scores, d_out_counts,
                                     d_out_status, d_lens, stride);
}
