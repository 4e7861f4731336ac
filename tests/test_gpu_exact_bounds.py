"""The matrix-core exact scan against rows built to defeat an error bound that under-states the one-pass contraction's rounding
(fixtures.py: tail_fixture, certificate_fixture; their arithmetic is checked on the CPU by test_exact_bound_fixtures.py).  The exact
nearest row r is placed so that its approximate score overshoots by as much as bf16 rounding allows while its mirror rows undershoot:
an E below that (hvx_flat_mfma.h, scan_error_bound) lets the exact tail skip r, or the certificate certify an answer without it.
Every case compares ids and score bits with the oracle's exact scan over the stored values."""
import numpy as np
import pytest

import fixtures as fx

pytestmark = pytest.mark.gpu

TAIL_DIMS = [128, 256, 512, 768, 1024, 1536]


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def index(hv, data, metric, dtype, max_batch):
    n = data.shape[0]
    dt = {"bf16": hv.BF16, "f32": hv.F32, "fp8": hv.FP8_E4M3}[dtype]
    return hv.ValidatedVectorReadIndex.managed(dim=data.shape[1], metric=metric, node_ids=np.arange(n, dtype=np.uint64) + 5, vectors=data,
                                               dtype=dt, l0_offsets=np.zeros(n + 1, np.uint64), l0_neighbors=np.zeros(0, np.uint64),
                                               max_batch=max_batch)


def oracle(orc, metric, stored, q, k, dtype):
    kern = {"kernel": orc.K_AVX_FMA_HW} if dtype == "f32" else {}
    rc, oid, osc = orc.flat_matrix(metric, stored, q, k, **kern)
    assert rc == orc.OK
    return oid, osc


def check(orc, metric, stored, qs, k, dtype, gid, gsc, gcnt, id_of=None, what="", nearest=None):
    want_ids, want_sc = oracle(orc, metric, stored, qs[0], k, dtype)
    if nearest is not None:  # the fixture is still a trap on the stored values: its overshooting row is the exact nearest
        assert int(want_ids[0]) == nearest, what
    want = (want_ids if id_of is None else id_of[want_ids.astype(np.int64)]).tolist()
    for qi in range(qs.shape[0]):
        got = (gid[qi, :gcnt[qi]] - (5 if id_of is None else 0)).tolist()
        assert got == want, f"{what} query {qi}: {got[:3]} != {want[:3]}"
        assert bits(gsc[qi, :gcnt[qi]]).tolist() == bits(want_sc).tolist(), f"{what} query {qi}"


def run_tail(orc, hv, gix, metric, data, q, k, dtype, what, rp):
    for b in (1, 33):
        qs = np.repeat(q[None, :], b, axis=0)
        gid, gsc, gcnt, _ = gix.flat_search_batch(qs, k)
        assert gix.last_scan_path() & hv.PATH_EXACT_TAIL, what
        check(orc, metric, data, qs, k, dtype, gid, gsc, gcnt, what=f"{what} b={b} k={k}", nearest=rp)


def rows_for(dim, least, b=1):
    """f32 rows take the matrix cores only from 2^22 row elements on (b <= 128) or from 2^33 query x row elements (hvx_api.hip,
    flat_scan_on_matrix_cores)"""
    return max(least, ((1 << 22) if b <= 128 else (1 << 33) // b) // dim + 1000)


@pytest.mark.parametrize("dtype,dim", [("bf16", d) for d in TAIL_DIMS] + [("f32", d) for d in TAIL_DIMS if d >= 256])  # (f32 at 128: the VALU scan)
@pytest.mark.parametrize("metric", [1, 0])
def test_exact_tail_keeps_the_overshooting_nearest_row(orc, hv, dtype, metric, dim):
    """the one-launch exact tail (hvx_flat_tail.hip) re-scores every row with s~ - E <= T; r's overshoot is ~0.7 of the derived E and
    1.2-1.5 times the bound used before (L2; cosine's bound has a factor two to spare): b = 1 and 33, k = 1 and 10, 9 000 far rows
    or more (three or more 4 096-row slices of the tail; the t's in one wavefront's lanes), then a restricted row list through the same kernel"""
    for k in (1, 10):
        data, q, rp, tp = fx.tail_fixture(dim, dtype, k, rows_for(dim, 9000), seed=31 * dim + k + metric)
        gix = index(hv, data, metric, dtype, 64)
        run_tail(orc, hv, gix, metric, data, q, k, dtype, f"{dtype} metric {metric} dim {dim}", rp)
        # a restricted row list (the restricted scan's shape) with r and the t's in it
        rng = np.random.default_rng(dim + k)
        rest = np.setdiff1d(np.arange(data.shape[0]), [rp] + tp)
        keep = np.sort(np.concatenate([[rp] + tp, rng.choice(rest, rows_for(dim, 6000) - 500, replace=False)]))
        at = int(np.searchsorted(keep, tp[0]))
        keep = np.delete(keep, [i for i in range(at - at % 64, at) if keep[i] != rp])  # the t's from a multiple of 64 in the list too
        allowed = (keep + 5).astype(np.uint64)
        gix.set_option(hv.OPT_RESTRICTED_DIRECT, 1)  # (sets this small would take the one-launch reference-order kernel)
        qs = np.repeat(q[None, :], 33, axis=0)
        rid, rsc, rcnt = gix.search_restricted_batch(qs, hv.SearchParams(k), hv.RestrictedVectorCandidates.from_ids(allowed))
        assert gix.last_scan_path() & hv.PATH_EXACT_TAIL
        check(orc, metric, data[keep], qs, k, dtype, rid, rsc, rcnt, id_of=allowed, what="restricted", nearest=int(np.searchsorted(keep, rp)))
        gix.close()


@pytest.mark.parametrize("dim", [256, 768, 1536])
def test_exact_tail_over_the_bf16_shadow(orc, hv, dim):
    """an f32 index whose image holds the bf16 shadow (built by a large scan, test_small_batch_scan_uses_the_bf16_shadow_once_it_exists)
    streams the shadow in the small-batch contraction: both operands rounded, twice the query-only error"""
    for metric in (1, 0):
        data, q, rp, tp = fx.tail_fixture(dim, "f32", 10, rows_for(dim, 24000, 600), seed=dim + metric)
        gix = index(hv, data, metric, "f32", 600)
        run_tail(orc, hv, gix, metric, data, q, 10, "f32", "f32 rows, before the shadow", rp)
        qs = np.repeat(q[None, :], 600, axis=0)
        gid, gsc, gcnt, _ = gix.flat_search_batch(qs, 10)  # a large scan builds the shadow (certificate path over the shadow)
        assert gix.last_scan_path() & hv.PATH_TILE_256
        check(orc, metric, data, qs, 10, "f32", gid, gsc, gcnt, what="the large scan", nearest=rp)
        for k in (1, 10):
            run_tail(orc, hv, gix, metric, data, q, k, "f32", f"f32 rows over the shadow, metric {metric}", rp)
        gix.close()


@pytest.mark.parametrize("dtype", ["bf16", "f32", "fp8"])
@pytest.mark.parametrize("dim", [256, 768, 1536])
def test_certificate_never_certifies_a_wrong_answer(orc, hv, dtype, dim):
    """the re-rank certificate (hvx_flat_mfma.hip, rerank_bf16_kernel) with the exact tail off: k t's and m + 1 - k accurate fillers take
    the m + 1 candidate slots and r (the exact nearest) overshoots past them.  The answer equals the oracle's (the derived bound fails
    the one-pass certificate and the full split finds r) or the scan reports ERR_INVARIANT -- never r's absence under status 0.
    b = 1 (the small-batch / 128 x 128 kernels) and b = 256 over 40 000 rows or more (the 256 x 256 tile kernels).  fp8 rows are e4m3 code
    points under a power-of-two scale, so the index stores the trap unchanged; at b = 256 the fp8 query is the MX build's trap
    (adversarial_query_mx) and the trap rows lie past the first 16 384-row chunk, in the slices the MX-scaled kernel scores."""
    rows = "fp8" if dtype == "fp8" else ("f32" if dtype == "f32" else "bf16")
    for k, b, n_far in ((1, 1, rows_for(dim, 6000)), (10, 1, rows_for(dim, 6000)), (10, 256, rows_for(dim, 40000, 256))):
        m = max(63, 2 * k)
        mx = dtype == "fp8" and b == 256
        data, q, rp, tp, fp = fx.certificate_fixture(dim, rows, k, m, n_far, seed=dim + k + b, mx=mx, min_pos=20000 if mx else 0)
        stored = fx.quantize_fp8_rows(data) if dtype == "fp8" else data
        gix = index(hv, data, 1, dtype, max(b, 16))
        gix.set_option(hv.OPT_FLAT_NO_TAIL, 1)
        qs = np.repeat(q[None, :], b, axis=0)
        try:
            gid, gsc, gcnt, _ = gix.flat_search_batch(qs, k)
        except hv.HelixDbError as e:
            assert e.status == hv.ERR_INVARIANT, str(e)
            assert oracle(orc, 1, stored, q, k, dtype)[0][0] == rp
            gix.close()
            continue
        if b == 256:
            assert gix.last_scan_path() & hv.PATH_TILE_256
        check(orc, 1, stored, qs, k, dtype, gid, gsc, gcnt, what=f"{dtype} dim {dim} k={k} b={b}", nearest=rp)
        gix.close()
