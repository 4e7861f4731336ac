"""The matrix-core exact scan along its result count k and down every rung of its attempt ladder (hvx_api.hip: flat_scan_device;
hvx_flat_mfma.hip: flat_mfma_impl, rerank_bf16_kernel, flat_merge_pairs_kernel; hvx_flat_smallb.hip; hvx_flat_tail.hip; hvx_flat_tile.hip).
k chooses the kernels: the re-rank's one-wavefront sort up to k = 31, the exact tail up to k = 64, the radix selection, the filtered
epilogue and the 256 x 256 tile kernel up to k = 127 (kc = max(63, 2 k) + 1 <= 256), the sorted-pool selection and the pair merge above,
k = 511 the last value served.  The ladder (one pass, full split, m = 1023, last resort) is climbed by corpora built for each rung
(fixtures.py: scan_image, rung1_fixture, ladder_block, overflow_fixture; their arithmetic is checked on the CPU by
test_scan_ladder_fixtures.py).  Every case compares ids and score bits of every query with the oracle's exact scan over the stored
values, and the route with last_scan_path() as the code states it."""
import numpy as np
import pytest

import fixtures as fx

pytestmark = pytest.mark.gpu

DTYPE_METRIC = [(d, m) for d in ("bf16", "fp8", "f32") for m in (1, 0)]


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def index(hv, data, metric, dtype, max_batch=256):
    n = data.shape[0]
    dt = {"bf16": hv.BF16, "f32": hv.F32, "fp8": hv.FP8_E4M3}[dtype]
    return hv.ValidatedVectorReadIndex.managed(dim=data.shape[1], metric=metric, node_ids=np.arange(n, dtype=np.uint64) + 5, vectors=data,
                                               dtype=dt, l0_offsets=np.zeros(n + 1, np.uint64), l0_neighbors=np.zeros(0, np.uint64),
                                               max_batch=max_batch)


_REFERENCE = {}


def reference(orc, key, metric, stored, queries, k, dtype):
    """the oracle's top-k (row positions, score bits) of every query, computed once per key; a smaller k is a prefix of it"""
    if key not in _REFERENCE:
        kern = {"kernel": orc.K_AVX_FMA_HW} if dtype == "f32" else {}
        out = []
        for q in queries:
            rc, oid, osc = orc.flat_matrix(metric, stored, q, k, **kern)
            assert rc == orc.OK
            out.append((oid.astype(np.int64), bits(osc)))
        _REFERENCE[key] = out
    return _REFERENCE[key]


def flat(gix, qs, k):
    gid, gsc, gcnt, _, gst = gix.flat_search_batch(qs, k, per_query_status=True)
    return gid, gsc, gcnt, gst


def route(gix, what):
    """last_scan_path(), printed before anything is asserted about it"""
    path = gix.last_scan_path()
    print(f"route {what}: {path:#06x}")
    return path


def with_nan(qs):
    """the batch plus one rejected query behind it"""
    bad = qs[-1].copy()
    bad[5] = np.nan
    return np.concatenate([qs, bad[None, :]])


def check(hv, ref, which, k, out, what, nan=()):
    """out = flat()'s answer to a batch whose query p is entry which[p] of the reference; the positions in `nan` hold a rejected query"""
    gid, gsc, gcnt, gst = out
    assert gid.shape[0] == len(which)
    for p, r in enumerate(which):
        if p in nan:
            assert gst[p] == hv.ERR_NONFINITE and gcnt[p] == 0, f"{what}: rejected query {p}: status {gst[p]}, count {gcnt[p]}"
            continue
        oid, osc = ref[r]
        c = min(k, oid.size)
        assert gst[p] == 0 and gcnt[p] == c, f"{what} query {p}: status {gst[p]}, count {gcnt[p]} (expected {c})"
        got = gid[p, :c].astype(np.int64) - 5
        assert np.array_equal(got, oid[:c]), f"{what} query {p}: ids differ from rank {int(np.argmax(got != oid[:c]))}: {got[:3]} != {oid[:3]}"
        assert np.array_equal(bits(gsc[p, :c]), osc[:c]), f"{what} query {p}: score bits differ"


def check_route(hv, dtype, b, k, path, what):
    """the route table of flat_scan_device / flat_mfma_impl for whole-index scans of <= 65 536 rows under default options"""
    if dtype == "f32" and b > 128:          # below 2^33 query x row elements: the reference-order VALU scan
        assert path == hv.PATH_VALU, f"{what}: {path}"
    elif dtype == "fp8" or b > 128:         # fp8 rows have no small-batch kernel; one chunk holds every row: no filtered epilogue
        assert path & hv.PATH_MFMA_128 and not path & (hv.PATH_FILTERED | hv.PATH_TILE_256 | hv.PATH_SMALL_BATCH | hv.PATH_VALU), f"{what}: {path}"
    elif k <= 64:                           # the one-launch exact tail
        assert path == hv.PATH_SMALL_BATCH | hv.PATH_EXACT_TAIL, f"{what}: {path}"
    else:                                   # selection, re-rank and certificate
        assert path & hv.PATH_SMALL_BATCH and not path & (hv.PATH_EXACT_TAIL | hv.PATH_MFMA_128 | hv.PATH_TILE_256), f"{what}: {path}"


def image_reference(orc, dtype, metric):
    im = fx.scan_image(dtype)
    return im, reference(orc, ("image", dtype, metric), metric, im["stored"], im["pool"], 512, dtype)


# ---- 1. result counts ----

@pytest.mark.parametrize("dtype,metric", DTYPE_METRIC)
def test_one_handle_through_every_result_count(orc, hv, dtype, metric):
    """ONE handle (max_batch 256) runs k = 10, 511, 1, 128, 31, 257, 64, 32, 127, 65, 256, 255 in that order -- kc and with it flat_scratch,
    cap_cand, cap_cand_b and cap_qsplit grow and shrink across 31 | 32 (the re-rank's sort), 64 | 65 (the tail's end), 127 | 128 (radix
    selection -> sorted pool + pair merge) and up to the last k served -- at b = 1, 33 and 130 each.  The image holds two pairs of exact
    duplicates and four blocks of identical rows with a query next to each (ties across the cut wherever k < T), one query IS a stored
    row, and the last query of the b = 33 and b = 130 batches is rejected: ERR_NONFINITE, count 0, neighbours untouched.  f32 rows at
    b = 130 are below the 2^33 work threshold: the VALU scan, the cheapest cross-check of the other two batch sizes."""
    im, ref = image_reference(orc, dtype, metric)
    gix = index(hv, im["data"], metric, dtype)
    for k in fx.SCAN_COUNTS:
        for b in fx.SCAN_BATCHES:
            qs = im["pool"][:1] if b == 1 else with_nan(im["pool"][:b - 1])
            what = f"{dtype} metric {metric} k={k} b={b}"
            out = flat(gix, qs, k)
            check_route(hv, dtype, b, k, route(gix, what), what)
            check(hv, ref, range(b), k, out, what, nan=() if b == 1 else (b - 1,))
    gix.close()


@pytest.mark.parametrize("dtype,metric", [c for c in DTYPE_METRIC if c[0] != "f32"])
def test_filtered_epilogue_and_tile_kernel_end_at_k_127(orc, hv, dtype, metric):
    """1 024-row first chunks without the small-batch kernels, b = 130: k = 127 (kc = 255) is the last result count of the filtered
    epilogue and of the 256 x 256 tile kernel (fp8 rows: the MX build), k = 128 (kc = 257) scores every chunk into the score matrix on
    the 128 x 128 kernel.  A fresh handle per run: a handle whose one-pass attempt missed twice skips it, and the tile kernel with it."""
    im, ref = image_reference(orc, dtype, metric)
    qs = with_nan(im["pool"])
    for k in (127, 128):
        for no_tile in (0, 1):
            gix = index(hv, im["data"], metric, dtype)
            gix.set_option(hv.OPT_FLAT_FIRST_CHUNK, 1024)
            gix.set_option(hv.OPT_FLAT_NO_SMALLB, 1)
            gix.set_option(hv.OPT_FLAT_NO_TILE, no_tile)
            what = f"{dtype} metric {metric} k={k} no_tile={no_tile}"
            out = flat(gix, qs, k)
            path = route(gix, what)
            if k == 127 and path & hv.PATH_PAIR_OVERFLOW_REPEAT:   # (loose thresholds of a short first chunk: check the kernel's OWN answer)
                check(hv, ref, range(130), k, out, what + " (repeated)", nan=(129,))
                gix.set_option(hv.OPT_FLAT_FIRST_CHUNK, 4096)
                out = flat(gix, qs, k)
                path = route(gix, what + " first chunk 4096")
                assert not path & hv.PATH_PAIR_OVERFLOW_REPEAT, f"{what}: {path}"
            if k == 127:
                want, never = (hv.PATH_MFMA_128, hv.PATH_TILE_256) if no_tile else (hv.PATH_TILE_256, 0)
                assert path & (want | hv.PATH_FILTERED) == want | hv.PATH_FILTERED and not path & never, f"{what}: {path}"
            else:
                assert path & hv.PATH_MFMA_128 and not path & (hv.PATH_FILTERED | hv.PATH_TILE_256), f"{what}: {path}"
            assert not path & hv.PATH_SMALL_BATCH
            check(hv, ref, range(130), k, out, what, nan=(129,))
            gix.close()


@pytest.mark.parametrize("dtype,metric", DTYPE_METRIC)
def test_k_512_is_refused_or_scanned_on_the_valu(orc, hv, dtype, metric):
    """k = 512 is past the pipeline (kc would be 1 025): bf16 and fp8 images answer ERR_UNSUPPORTED, f32 images take the VALU scan; the
    handle then serves k = 10 as before"""
    im, ref = image_reference(orc, dtype, metric)
    gix = index(hv, im["data"], metric, dtype)
    qs = im["pool"][:33]
    if dtype == "f32":
        out = flat(gix, qs, 512)
        assert gix.last_scan_path() == hv.PATH_VALU
        check(hv, ref, range(33), 512, out, f"f32 metric {metric} k=512")
    else:
        with pytest.raises(hv.HelixDbError) as e:
            flat(gix, qs, 512)
        assert e.value.status == hv.ERR_UNSUPPORTED, str(e.value)
    out = flat(gix, qs, 10)
    check_route(hv, dtype, 33, 10, gix.last_scan_path(), "after k=512")
    check(hv, ref, range(33), 10, out, f"{dtype} metric {metric} k=10 after k=512")
    gix.close()


@pytest.mark.parametrize("k,sizes", [(32, (31, 32, 64, 65, 66)), (128, (127, 128, 256, 257, 258)), (64, (50, 64, 4097))])
def test_corpora_shorter_than_the_candidate_list(orc, hv, k, sizes):
    """bf16 rows, dim 128, n around k and around kc = max(63, 2 k) + 1 (65, 257; k = 64 on the tail: n = 4 097 leaves its second
    4 096-row slice one row), b = 1 and 33, with the exact tail and with OPT_FLAT_NO_TAIL: min(k, n) results, all n rows in order
    when n <= k"""
    rng = np.random.default_rng(900 + k)
    qs = rng.standard_normal((33, 128)).astype(np.float32)
    for n in sizes:
        data = fx.round_bf16(rng.standard_normal((n, 128)).astype(np.float32))
        ref = reference(orc, ("short", k, n), 1, data, qs, k, "bf16")
        assert ref[0][0].size == min(k, n)
        gix = index(hv, data, 1, "bf16", 64)
        for no_tail in (0, 1):
            gix.set_option(hv.OPT_FLAT_NO_TAIL, no_tail)
            for b in (1, 33):
                what = f"k={k} n={n} b={b} no_tail={no_tail}"
                out = flat(gix, qs[:b], k)
                path = gix.last_scan_path()
                assert path & hv.PATH_SMALL_BATCH and bool(path & hv.PATH_EXACT_TAIL) == (k <= 64 and not no_tail), f"{what}: {path}"
                check(hv, ref, range(b), k, out, what)
        gix.close()


@pytest.mark.parametrize("dtype,metric", DTYPE_METRIC)
def test_ties_across_the_cut(orc, hv, dtype, metric):
    """the nearest rows of every query are T stored-identical rows under scattered ids, k < T: the answer is the k LOWEST ids of the block
    under equal score bits (the reference's (score, id) order), whichever kernel sorts them -- the tail's lanes (k <= 64), the re-rank's
    one-wavefront sort (kc = 64) and its LDS sort (kc = 65 ..), the slices' pools and the pair merge (kc > 256) -- at b = 1 and 33, and
    b = 130 for k >= 128"""
    im = fx.scan_image(dtype)
    gix = index(hv, im["data"], metric, dtype)
    for k, t in fx.TIE_CASES_K_T:
        near = im["near"][t]
        ref = reference(orc, ("ties", dtype, metric, k, t), metric, im["stored"], near, k, dtype)
        for oid, osc in ref:
            assert oid.tolist() == im["blocks"][t][:k].tolist() and np.unique(osc).size == 1
        for no_tail in ((0, 1) if k <= 64 else (0,)):
            gix.set_option(hv.OPT_FLAT_NO_TAIL, no_tail)
            for b in (1, 33) + ((130,) if k >= 128 else ()):
                which = [p % 33 for p in range(b)]
                what = f"{dtype} metric {metric} k={k} T={t} b={b} no_tail={no_tail}"
                out = flat(gix, near[which], k)
                path = gix.last_scan_path()
                if dtype != "fp8" and b <= 128:
                    assert bool(path & hv.PATH_EXACT_TAIL) == (k <= 64 and not no_tail), f"{what}: {path}"
                check(hv, ref, which, k, out, what)
        gix.set_option(hv.OPT_FLAT_NO_TAIL, 0)
    gix.close()


# ---- 2. the attempt ladder ----

def mixed(b, hard, first_easy):
    """reference entries of a batch of b: a hard query at every third position (entries 0 .. hard - 1 in turn), easy ones between"""
    return [(p // 3) % hard if p % 3 == 0 else first_easy + p % 130 for p in range(b)]


def rung1(orc):
    fr = fx.rung1_fixture()
    pool = np.concatenate([fr["hard"][None, :], fr["easy"]])
    return fr, pool, reference(orc, ("rung1",), 1, fr["data"], pool, 10, "bf16")


def test_rung_1_the_full_split_certifies(orc, hv):
    """k rows at one score and 80 rows a gap g = sqrt(E_one E_full) scale above them, every value exact in bf16: the one-pass certificate
    fails on its bound, the full split's holds -- FULL_SPLIT without WIDENED, on the small-batch kernels (OPT_FLAT_NO_TAIL, b = 1 and 33)
    and on the 128 x 128 kernel (b = 130); two of three queries of a batch are easy ones that certified at once"""
    fr, pool, ref = rung1(orc)
    for b, no_tail in ((1, 1), (33, 1), (130, 0)):
        gix = index(hv, fr["data"], 1, "bf16")
        gix.set_option(hv.OPT_FLAT_NO_TAIL, no_tail)
        which = mixed(b, 1, 1)
        out = flat(gix, pool[which], 10)
        path = route(gix, f"rung 1 b={b}")
        assert path & hv.PATH_FULL_SPLIT and not path & (hv.PATH_WIDENED | hv.PATH_EXACT_TAIL), f"b={b}: {path}"
        assert path & (hv.PATH_MFMA_128 if b > 128 else hv.PATH_SMALL_BATCH), f"b={b}: {path}"
        check(hv, ref, which, 10, out, f"rung 1 b={b}")
        gix.close()


def block_case(orc, rung, rows):
    fb = fx.ladder_block(rung, rows)
    pool = np.concatenate([fb["hard"], fb["easy"]])
    return fb, pool, reference(orc, ("block", rung, rows), 1, fb["stored"], pool, 10, rows)


@pytest.mark.parametrize("rows", ["bf16", "fp8"])
def test_rung_2_the_widened_attempt_certifies(orc, hv, rows):
    """500 stored-identical rows nearest, k = 10: 64 candidates never reach past the block, 1 024 do -- FULL_SPLIT | WIDENED without the
    tail, the 10 lowest ids.  bf16 rows at b <= 128 take the sorted-pool selection with kc = 1 024: two slices fill the 2 048-entry
    pool of flat_merge_pairs_kernel"""
    fb, pool, ref = block_case(orc, 2, rows)
    hard = fb["hard"].shape[0]
    for b, no_tail in (((1, 1), (33, 1), (130, 0)) if rows == "bf16" else ((9, 0), (130, 0))):
        gix = index(hv, fb["data"], 1, rows)
        gix.set_option(hv.OPT_FLAT_NO_TAIL, no_tail)
        which = mixed(b, hard, hard)
        out = flat(gix, pool[which], 10)
        path = route(gix, f"rung 2 {rows} b={b}")
        want = hv.PATH_FULL_SPLIT | hv.PATH_WIDENED
        assert path & want == want and not path & hv.PATH_EXACT_TAIL, f"{rows} b={b}: {path}"
        check(hv, ref, which, 10, out, f"rung 2 {rows} b={b}")
        gix.close()


def test_rung_3_bf16_rows_end_on_the_exact_tail(orc, hv):
    """1 500 identical rows: no certificate at m = 1 023 either.  With OPT_FLAT_NO_TAIL (b = 1, 33) the scan is answered by the tail all
    the same, WIDENED | EXACT_TAIL (include/helix_vec.h).  Under default options b = 200 runs the last resort as 128 + 72 queries, every
    output pointer offset by q0 k: hard and easy queries in both halves, and a rejected query at position 150 whose status and zero
    count land in row 150, not 22"""
    fb, pool, ref = block_case(orc, 3, "bf16")
    hard = fb["hard"].shape[0]
    want = hv.PATH_WIDENED | hv.PATH_EXACT_TAIL
    gix = index(hv, fb["data"], 1, "bf16")
    gix.set_option(hv.OPT_FLAT_NO_TAIL, 1)
    for b in (1, 33):
        which = mixed(b, hard, hard)
        out = flat(gix, pool[which], 10)
        assert route(gix, f"rung 3 bf16 b={b}") & want == want, f"b={b}: {gix.last_scan_path()}"
        check(hv, ref, which, 10, out, f"rung 3 b={b}")
    gix.close()
    gix = index(hv, fb["data"], 1, "bf16")
    which = [hard + p % 130 for p in range(200)]
    for j, p in enumerate((3, 64, 127, 128, 140, 199)):
        which[p] = j
    qs = pool[which]
    qs[150, 7] = np.nan
    out = flat(gix, qs, 10)
    assert route(gix, "rung 3 bf16 b=200") & want == want, gix.last_scan_path()
    assert out[3][22] == 0 and out[2][22] == 10
    check(hv, ref, which, 10, out, "rung 3 b=200", nan=(150,))
    gix.close()


def test_rung_3_fp8_rows_report_the_missing_certificate(orc, hv):
    """fp8 rows have neither tail nor VALU scan: ERR_INVARIANT that names the certificate -- never a guess -- and the handle goes on
    answering"""
    fb, pool, ref = block_case(orc, 3, "fp8")
    hard = fb["hard"].shape[0]
    gix = index(hv, fb["data"], 1, "fp8")
    with pytest.raises(hv.HelixDbError) as e:
        flat(gix, pool[mixed(9, hard, hard)], 10)
    assert e.value.status == hv.ERR_INVARIANT and "certificate" in str(e.value), str(e.value)
    which = [hard + p for p in range(9)]
    check(hv, ref, which, 10, flat(gix, pool[which], 10), "fp8 easy batch after the error")
    gix.close()


def test_rung_3_f32_rows_fall_back_to_the_valu_scan(orc, hv):
    """f32 rows (dim 256, 17 500 rows, OPT_FLAT_NO_TAIL, b = 33) never widen: the queries without a certificate after the full split go to
    the VALU scan -- those alone while they are at most a quarter of the batch (VALU_FALLBACK_QUERIES; the other 32 rows keep their
    certified answers), the whole batch otherwise (VALU on top of the earlier attempts' flags)"""
    fb, pool, ref = block_case(orc, 3, "f32")
    hard = fb["hard"].shape[0]
    gix = index(hv, fb["data"], 1, "f32")
    gix.set_option(hv.OPT_FLAT_NO_TAIL, 1)
    which = [hard + p for p in range(33)]
    which[17] = 0
    out = flat(gix, pool[which], 10)
    path = route(gix, "rung 3 f32, 1 hard of 33")
    assert path & hv.PATH_VALU_FALLBACK_QUERIES and not path & hv.PATH_VALU and path & hv.PATH_SMALL_BATCH and path & hv.PATH_FULL_SPLIT, path
    check(hv, ref, which, 10, out, "one hard query of 33")
    which = [p if p < 20 else hard + p for p in range(33)]
    out = flat(gix, pool[which], 10)
    path = route(gix, "rung 3 f32, 20 hard of 33")
    want = hv.PATH_VALU | hv.PATH_SMALL_BATCH | hv.PATH_FULL_SPLIT
    assert path & want == want and not path & hv.PATH_VALU_FALLBACK_QUERIES, path
    check(hv, ref, which, 10, out, "20 hard queries of 33")
    gix.close()


def test_pair_overflow_repeats_the_scan_unfiltered(orc, hv):
    """the deterministic counterpart of the `if` in test_exact_scan_through_the_256_tile_kernel: the 1 024 rows of the first chunk are ten
    times as far from every query as the 4 000 behind them, their thresholds let the whole first filtered slice through, the 1 024-pair
    buffers overflow and the scan runs again without the filter -- PAIR_OVERFLOW_REPEAT and the oracle's answer for every query"""
    data, qs = fx.overflow_fixture()
    ref = reference(orc, ("overflow",), 1, data, qs, 10, "bf16")
    gix = index(hv, data, 1, "bf16")
    gix.set_option(hv.OPT_FLAT_FIRST_CHUNK, fx.OVERFLOW_FIRST_CHUNK)
    gix.set_option(hv.OPT_FLAT_NO_SMALLB, 1)
    out = flat(gix, qs, 10)
    assert route(gix, "pair overflow") & hv.PATH_PAIR_OVERFLOW_REPEAT, gix.last_scan_path()
    check(hv, ref, range(qs.shape[0]), 10, out, "pair overflow")
    gix.close()


def test_a_handle_skips_and_probes_the_one_pass_attempt(orc, hv):
    """hvx_index::m_fast_misses / m_fast_skipped: after two scans whose one-pass attempt missed a certificate, a handle starts with the full
    split and tries the one-pass attempt again on every 32nd scan.  One bf16 handle, b = 130, k = 10: the rung-1 batch twice, then 34 scans
    that alternate an easy batch (certified by one pass on a fresh handle: MFMA_128 alone) with the rung-1 batch.  All 36 answers equal the
    oracle's; the third scan -- an easy batch -- reports MFMA_128 | FULL_SPLIT: its FIRST attempt was the full split.  So does every later
    easy batch: the probe falls on scan 34, a rung-1 batch, whose miss keeps the handle skipping."""
    fr, pool, ref = rung1(orc)
    hard_batch, easy_batch = mixed(130, 1, 1), [1 + p for p in range(130)]
    gix = index(hv, fr["data"], 1, "bf16")
    out = flat(gix, pool[easy_batch], 10)
    assert gix.last_scan_path() == hv.PATH_MFMA_128, gix.last_scan_path()
    check(hv, ref, easy_batch, 10, out, "easy batch, fresh handle")
    gix.close()
    gix = index(hv, fr["data"], 1, "bf16")
    for i in range(36):
        easy = i >= 2 and i % 2 == 0
        which = easy_batch if easy else hard_batch
        out = flat(gix, pool[which], 10)
        path = route(gix, f"handle state, scan {i + 1} ({'easy' if easy else 'rung-1'} batch)")
        if easy:
            assert path == hv.PATH_MFMA_128 | hv.PATH_FULL_SPLIT, f"scan {i + 1}: {path}"
        else:
            assert path & hv.PATH_FULL_SPLIT and not path & hv.PATH_WIDENED, f"scan {i + 1}: {path}"
        check(hv, ref, which, 10, out, f"scan {i + 1}")
    gix.close()
