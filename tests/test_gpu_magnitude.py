"""Scans and searches at the ends of the f32 range (fixtures.py: COSINE_SCALES, L2_SCALES; their arithmetic is checked on the CPU by
test_magnitude_fixtures.py).  Cosine has no component limit and the reference answers any finite magnitude through its f64 fallback, so
queries and rows scaled by exact powers of two up to 2^+-100 (and single outlier rows, rows whose norm exceeds FLT_MAX, products below the
normal range) must give the oracle's ids and score BITS with status OK on every kernel: the approximate cosine of the matrix-core scans
(|q|^2, |x|, an f32 dot product) is worthless there, and so is an error bound drawn around it.  L2 / L1 run at their component limit and
where the scores are tiny or subnormal.  Every case compares with the oracle run on the stored values."""
import functools

import numpy as np
import pytest

import fixtures as fx
from test_gpu_build import oracle_build, rows_of
from test_gpu_delete import assert_same_graph
from test_gpu_parity import assert_hnsw_equal, assert_params_equal, build_oracle

pytestmark = pytest.mark.gpu

ALL = [c[0] for c in fx.COSINE_SCALES]
LARGE = fx.COSINE_SCALES_LARGE
ID0 = 5
STORE = {"bf16": fx.round_bf16, "fp8": fx.quantize_fp8_rows, "f32": lambda x: x}


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=3)
def cosine_corpus(name, dtype, dim, n, src_min=0):
    """(stored rows, scaled query, unit-scale query, source row) of one scale pair: computed once, shared, never written"""
    seed = fx.MAGNITUDE_SEEDS[(dim, n)]
    data, q, src = fx.cosine_case(name, dim, n, seed, src_min=src_min)
    _, uq, _ = fx.cosine_case(name, dim, n, seed, src_min=src_min, unit=True)
    stored = STORE[dtype](data)
    assert np.isfinite(stored).all()
    return frozen(data, stored, q, uq) + (src,)


@functools.lru_cache(maxsize=3)
def l2_corpus(name, dtype, dim, n):
    import orc
    limit = float(orc.lib().orc_component_limit(orc.L2SQ, dim))
    data, q, src = fx.l2_case(name, dim, n, fx.l2_seed(name, dim, n), limit)
    q2 = data[(src * 31 + 7) % n].copy()  # a second query: a stored row itself (score 0 first)
    if dtype == "bf16":
        q2 = fx.round_bf16(q2)
    return frozen(data, STORE[dtype](data), q, q2) + (src,)


_WANT = {}


def want(orc, metric, key, stored, q, k):
    """the oracle's exact scan of `stored` (cached by `key`): (row positions, score bits)"""
    key = key + (metric, k, q.tobytes())
    if key not in _WANT:
        if len(_WANT) >= 64:
            _WANT.clear()
        rc, ids, sc = orc.flat_matrix(metric, stored, q, k, kernel=orc.K_AVX_FMA_HW)
        assert rc == orc.OK, f"the oracle answers every case: rc {rc}"
        _WANT[key] = (ids.astype(np.int64), bits(sc).tolist())
    return _WANT[key]


def image(hv, data, metric, dtype, max_batch):
    n = data.shape[0]
    dt = {"bf16": hv.BF16, "f32": hv.F32, "fp8": hv.FP8_E4M3}[dtype]
    return hv.ValidatedVectorReadIndex.managed(dim=data.shape[1], metric=metric, node_ids=np.arange(n, dtype=np.uint64) + ID0, vectors=data,
                                               dtype=dt, l0_offsets=np.zeros(n + 1, np.uint64), l0_neighbors=np.zeros(0, np.uint64),
                                               max_batch=max_batch)


def batch_of(qa, qb, b):
    """qa, qb alternating; batches of more than one query end with a NaN query (rejected: its flags must not leak to its tile neighbours)"""
    qs = np.stack([qa if i % 2 == 0 else qb for i in range(b)]).astype(np.float32)
    if b > 1:
        qs[b - 1, 3] = np.nan
    return qs


def check(orc, hv, metric, key, stored, qs, k, got, what, id_of=None, src=None, nan_last=True):
    gid, gsc, gcnt, gst = got
    b = qs.shape[0]
    nan_last = nan_last and b > 1
    live = b - 1 if nan_last else b
    if gst is not None:
        assert gst.tolist() == [hv.OK] * live + ([hv.ERR_NONFINITE] if nan_last else []), what
    if nan_last:
        assert gcnt[b - 1] == 0, what
    for qi in range(live):
        pos, sbits = want(orc, metric, key, stored, qs[qi], k)
        if src is not None:
            assert int(pos[0]) == src, what
        ids = (pos + ID0 if id_of is None else id_of[pos]).tolist()
        assert gid[qi, :gcnt[qi]].tolist() == ids, f"{what} query {qi}: ids {gid[qi, :3].tolist()} != {ids[:3]}"
        assert bits(gsc[qi, :gcnt[qi]]).tolist() == sbits, f"{what} query {qi}: score bits differ"


def flat(gix, qs, k):
    gid, gsc, gcnt, _, gst = gix.flat_search_batch(qs, k, per_query_status=True)
    return gid, gsc, gcnt, gst


# ---- exact scans, cosine ----

@pytest.mark.parametrize("dim", [100, 768])
@pytest.mark.parametrize("name", ALL)
def test_valu_scan(orc, hv, name, dim):
    """the f32 reference-order scan (stable_half_cosine behind cosine_finish_fn), a scalar tail of 4 at dim 100"""
    data, stored, q, uq, src = cosine_corpus(name, "f32", dim, 3000)
    gix = image(hv, data, hv.COSINE, "f32", 8)
    qs = batch_of(q, uq, 5)
    got = flat(gix, qs, 10)
    assert gix.last_scan_path() == hv.PATH_VALU
    check(orc, hv, orc.COSINE, (name, "f32", dim, 3000), stored, qs, 10, got, f"VALU {name} dim {dim}", src=src)
    gix.close()


TAIL_ROWS = {"f32": 17500, "bf16": 6000, "fp8": 6000}  # f32 rows take the matrix cores from 2^22 row elements on


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("name", ALL)
def test_small_batch_scan(orc, hv, name, dtype):
    """b = 1 and 33, k = 1 and 10 on the small-batch contraction: with the one-launch exact tail (f32 and bf16 rows; hvx_flat_tail.hip), then
    with the tail off -- sort-free selection, re-rank and certificate (flat_select_radix_kernel, rerank_bf16_kernel); fp8 rows have neither
    kernel: their small batches take the 128 x 128 contraction, its selection and the same certificate.  Where EVERY row is outside
    the trusted norms (r126) no f32 / bf16 row has an approximation: the tail re-scores all rows, and with the tail off the VALU scan
    (f32) resp. the tail as the last resort (bf16) answers; fp8 rows are scored against their codes and keep their approximation."""
    n = TAIL_ROWS[dtype]
    data, stored, q, uq, src = cosine_corpus(name, dtype, 256, n)
    gix = image(hv, data, hv.COSINE, dtype, 64)
    key = (name, dtype, 256, n)
    for no_tail in (0, 1):
        gix.set_option(hv.OPT_FLAT_NO_TAIL, no_tail)
        for b in (1, 33):
            for k in (1, 10):
                qs = batch_of(q, uq, b)
                got = flat(gix, qs, k)
                path = gix.last_scan_path()
                # (fp8 rows have no small-batch kernel: their batches of <= 128 queries run on the 128 x 128 contraction)
                assert path & (hv.PATH_MFMA_128 if dtype == "fp8" else hv.PATH_SMALL_BATCH), path
                if not no_tail:
                    assert bool(path & hv.PATH_EXACT_TAIL) == (dtype != "fp8"), path
                else:  # (the tail may still answer bf16 rows as the last resort, after the widened certificate attempt)
                    assert not path & hv.PATH_EXACT_TAIL or (dtype == "bf16" and path & hv.PATH_WIDENED), path
                check(orc, hv, orc.COSINE, key, stored, qs, k, got, f"{dtype} {name} no_tail={no_tail} b={b} k={k} path={path}", src=src)
    gix.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp8"])
def test_small_batch_scan_of_subnormal_queries(orc, hv, dtype):
    """queries below the normal range, 33 to a batch, tail on and off: every component of one is subnormal with ~19 bits left (2^-130), of
    another with ~9 bits (2^-140; its smallest components are zero).  split_queries_kernel must find their exponent (the device's frexpf on a
    subnormal maximum) and scale them into the normal range exactly (ldexpf).  The scaling by 2^-130 / 2^-140 itself rounds, so the
    oracle scores the rounded queries: ids and bits are its, the source row is not asserted."""
    n = TAIL_ROWS[dtype]
    data, stored, q, uq, src = cosine_corpus("unit", dtype, 256, n)
    tiny = np.finfo(np.float32).tiny
    qa, qb = np.ldexp(uq, -130).astype(np.float32), np.ldexp(uq, -140).astype(np.float32)
    for s in (qa, qb):
        assert 0 < np.abs(s).max() < tiny and np.count_nonzero(s) > 200
    gix = image(hv, data, hv.COSINE, dtype, 64)
    qs = batch_of(qa, qb, 33)
    qs[4] = uq
    for no_tail in (0, 1):
        gix.set_option(hv.OPT_FLAT_NO_TAIL, no_tail)
        got = flat(gix, qs, 10)
        path = gix.last_scan_path()
        assert path & (hv.PATH_MFMA_128 if dtype == "fp8" else hv.PATH_SMALL_BATCH), path
        check(orc, hv, orc.COSINE, ("unit", dtype, 256, n), stored, qs, 10, got, f"{dtype} subnormal queries no_tail={no_tail} path={path}")
    gix.close()


@pytest.mark.parametrize("dtype", ["f32", "bf16"])
@pytest.mark.parametrize("name", ALL)
def test_ring_and_register_builds_of_the_small_batch_scan(orc, hv, name, dtype):
    """the LDS-ring build (<= 32 queries) and the register-fragment build give the same, exact, answer (tail off: the candidates are theirs)"""
    n = TAIL_ROWS[dtype]
    data, stored, q, uq, src = cosine_corpus(name, dtype, 256, n)
    gix = image(hv, data, hv.COSINE, dtype, 32)
    gix.set_option(hv.OPT_FLAT_NO_TAIL, 1)
    for b in (1, 32):
        qs = batch_of(q, uq, b)
        for build in (0, 2):
            gix.set_option(hv.OPT_FLAT_NO_SMALLB, build)
            got = flat(gix, qs, 10)
            assert gix.last_scan_path() & hv.PATH_SMALL_BATCH
            check(orc, hv, orc.COSINE, (name, dtype, 256, n), stored, qs, 10, got, f"{dtype} {name} build {build} b={b}", src=src)
    gix.close()


def tile_scan(orc, hv, name, dtype, n, b, options, tile, src_min):
    data, stored, q, uq, src = cosine_corpus(name, dtype, 256, n, src_min)
    assert src >= src_min
    gix = image(hv, data, hv.COSINE, dtype, b)
    for opt, val in options:
        gix.set_option(opt, val)
    qs = batch_of(q, uq, b)
    got = flat(gix, qs, 10)
    path = gix.last_scan_path()
    assert path & (hv.PATH_TILE_256 if tile else hv.PATH_MFMA_128) and not path & hv.PATH_SMALL_BATCH, path
    if not tile:
        assert not path & hv.PATH_TILE_256, path
    check(orc, hv, orc.COSINE, (name, dtype, 256, n, src_min), stored, qs, 10, got, f"{dtype} {name} b={b} path={path}", src=src)
    gix.close()


@pytest.mark.parametrize("name", LARGE)
def test_128_tile_contraction(orc, hv, name):
    """flat_mfma_bf16_kernel's two epilogues over bf16 rows, 256 queries: the score matrix of a 2 048-row first chunk, then filtered slices
    (the query's source row in one of them)"""
    tile_scan(orc, hv, name, "bf16", 20000, 256, [(hv.OPT_FLAT_NO_TILE, 1), (hv.OPT_FLAT_NO_SMALLB, 1), (hv.OPT_FLAT_FIRST_CHUNK, 2048)], False, 17500)


TILE_CASES = [(name, dtype, build) for name in LARGE for dtype, build in (("bf16", 0), ("fp8", 3), ("fp8", 4))] + \
             [(name, "fp8", 3) for name in fx.COSINE_SCALES_MX]


@pytest.mark.parametrize("name,dtype,build", TILE_CASES)
def test_256_tile_contraction(orc, hv, name, dtype, build):
    """the large-tile filtered kernel (hvx_flat_tile.hip): bf16 rows, fp8 rows on the MX-scaled build (3: the query as two e4m3 pieces under
    an E8M0 block scale) and on the bf16-widening build (4); the query's source row lies past row 17 500 -- behind the first chunk.
    The MX build also takes the queries above 2^100 and below 2^-100: a block exponent clamped to +-100 (as split_queries_mx_kernel's once
    was) saturates every e4m3 piece of the first at 448 and flushes every piece of the second to zero."""
    opts = [(hv.OPT_FLAT_NO_SMALLB, 1), (hv.OPT_FLAT_TILE_BUILD, build)] + ([(hv.OPT_FLAT_FIRST_CHUNK, 2048)] if build != 3 else [])
    tile_scan(orc, hv, name, dtype, 20000, 256, opts, True, 17500)


@pytest.mark.parametrize("name", LARGE)
def test_256_tile_contraction_over_the_bf16_shadow(orc, hv, name):
    """f32 rows reach the matrix cores at b n dim >= 2^33: 512 queries over 66 000 rows, through the bf16 shadow"""
    tile_scan(orc, hv, name, "f32", 66000, 512, [], True, 57750)


# ---- restricted scans ----

@pytest.mark.parametrize("dtype", ["f32", "bf16", "fp8"])
@pytest.mark.parametrize("name", ALL)
def test_restricted_scans(orc, hv, name, dtype):
    """900 and 6 000 allowed ids of the same corpora: the one-launch reference-order kernel (hvx_restricted_exact.hip), the matrix-core /
    VALU pipeline behind OPT_RESTRICTED_DIRECT = 1, and the fused prefilter call over a one-hop CSR.  Which kernel answered is asserted:
    the one-launch kernel serves f32 and bf16 rows (forced, and as the prefilter call's own choice at this size); with it switched off
    f32 sets this small take the VALU scan and bf16 sets the matrix cores.  fp8 rows have no one-launch kernel: every call runs the
    matrix-core scan through the restricted row list, where the rows' code norms (m_rowterm) are indexed through it."""
    n = TAIL_ROWS[dtype]
    data, stored, q, uq, src = cosine_corpus(name, dtype, 256, n)
    gix = image(hv, data, hv.COSINE, dtype, 64)
    p = hv.SearchParams(10)
    matrix = hv.PATH_MFMA_128 | hv.PATH_TILE_256 | hv.PATH_SMALL_BATCH

    def assert_path(direct, what):
        path = gix.last_scan_path()
        if direct and dtype != "fp8":
            assert path == hv.PATH_DIRECT, (what, path)
        elif dtype == "f32":
            assert path == hv.PATH_VALU, (what, path)
        else:
            assert path & matrix and not path & hv.PATH_DIRECT, (what, path)

    qs = batch_of(q, uq, 9)[:8]  # (search_restricted_batch reports one status for the batch: no rejected query here)
    for size in (900, 6000):  # (bf16: 6 000 is every row, still through the restricted row list)
        rng = np.random.default_rng(size)
        keep = np.sort(np.concatenate([[src], rng.choice(np.setdiff1d(np.arange(n), [src]), size - 1, replace=False)]))
        allowed = (keep + ID0).astype(np.uint64)
        sub = np.ascontiguousarray(stored[keep])
        key = (name, dtype, 256, n, "restricted", size)
        at = int(np.searchsorted(keep, src))
        for direct in (2, 1):
            gix.set_option(hv.OPT_RESTRICTED_DIRECT, direct)
            rid, rsc, rcnt = gix.search_restricted_batch(qs, p, hv.RestrictedVectorCandidates.from_ids(allowed))
            assert_path(direct == 2, f"direct={direct} size={size}")
            check(orc, hv, orc.COSINE, key, sub, qs, 10, (rid, rsc, rcnt, None), f"{dtype} {name} direct={direct} size={size}", id_of=allowed, src=at,
                  nan_last=False)
        gix.set_option(hv.OPT_RESTRICTED_DIRECT, 0)
        # node 0 (no vector) points at the allowed ids: one hop from it is the candidate set
        nodes = n + ID0
        off = np.full(nodes + 1, allowed.size, np.uint64)
        off[0] = 0
        g = hv.Graph(nodes, off, allowed)
        fid, fsc, fcnt, ncand, _ = gix.prefilter_search_batch(g, qs, p, [0])
        assert ncand == allowed.size
        assert_path(True, f"prefilter size={size}")
        check(orc, hv, orc.COSINE, key, sub, qs, 10, (fid, fsc, fcnt, None), f"{dtype} {name} prefilter size={size}", id_of=allowed, src=at, nan_last=False)
        g.close()
    gix.close()


# ---- exact scans, L2 ----

@pytest.mark.parametrize("dtype,n", [("f32", 17500), ("bf16", 6000)])
@pytest.mark.parametrize("name", [c[0] for c in fx.L2_SCALES])
def test_l2_scans(orc, hv, name, dtype, n):
    """rows and queries at 0.99 of the component limit, at 2^-60 (scores are tiny normals) and at 2^-72 (subnormal scores with a few bits:
    heavy exact ties, the oracle's (score, id) order decides), b = 33 and 256"""
    data, stored, q, q2, src = l2_corpus(name, dtype, 256, n)
    gix = image(hv, data, hv.EUCLIDEAN, dtype, 256)
    for b in (33, 256):
        qs = batch_of(q, q2, b)
        got = flat(gix, qs, 10)
        check(orc, hv, orc.L2SQ, ("l2", name, dtype, n), stored, qs, 10, got, f"L2 {dtype} {name} b={b} path={gix.last_scan_path()}")
    gix.close()


# ---- HNSW searches over graphs the oracle built at the scaled values ----

HNSW_SCALES = ["q70", "q-80", "q62r62", "q-70r-70", "r126", "outliers"]
HNSW_N = 1200


@functools.lru_cache(maxsize=2)
def hnsw_corpus(name, dim, n=HNSW_N):
    """(rows, 24 queries: rows plus 5 % noise, scaled by 2^sq and -- every other one -- left at unit scale)"""
    _, sq, sr, out, _ = fx.COSINE_SCALE[name]
    data, _, _ = fx.cosine_case(name, dim, n, 40 + dim)
    unit, _, _ = fx.cosine_case(name, dim, n, 40 + dim, unit=True)
    rng = np.random.default_rng(dim)
    pick = rng.choice(n, 24, replace=False)
    q = (unit[pick] + 0.05 * rng.standard_normal((24, dim))).astype(np.float32)
    q[0::2] = np.ldexp(q[0::2], sq)
    assert np.isfinite(q).all() and (np.abs(q[q != 0]) >= np.finfo(np.float32).tiny).all()
    return frozen(data, q)


def hnsw_pair(orc, hv, data, metric, dtype="f32", seed=3):
    lv = fx.draw_levels(data.shape[0], 16, seed=seed)
    stored = STORE[dtype](data)
    oix = build_oracle(orc, stored, metric, lv, efc=64, cached=True)
    ex = oix.export()
    ex["vectors"] = data
    gix = hv.ValidatedVectorReadIndex.from_export(ex, dim=data.shape[1], metric=metric, dtype=hv.BF16 if dtype == "bf16" else hv.F32)
    return oix, gix


def set_hnsw_path(hv, gix, path):
    if path == "general":
        gix.set_option(hv.OPT_HNSW_GENERAL_KERNEL, 1)
    gix.set_option(hv.OPT_HNSW_PAIR, 3 if path == "pair1" else 2 if path == "pair" else 1)
    if path == "wave-spill":
        gix.set_option(hv.OPT_WAVE_LOG2CAP, 8)
    gix.set_occupancy(2 if path == "occ2" else 1)


@pytest.mark.parametrize("dim,path", [(128, p) for p in ("wave", "wave-spill", "general", "pair", "pair1", "occ2")] + [(768, "wave"), (768, "occ2")])
@pytest.mark.parametrize("name", HNSW_SCALES)
def test_hnsw_cosine(orc, hv, name, dim, path):
    """cosine_finish_fn's f64 fallback inside every beam kernel (dim 768: the one-wavefront kernel's 24-chunk build): ids, score bits and
    SearchStats equal the oracle's"""
    data, q = hnsw_corpus(name, dim)
    oix, gix = hnsw_pair(orc, hv, data, orc.COSINE)
    set_hnsw_path(hv, gix, path)
    assert_hnsw_equal(orc, hv, oix, gix, q, 10, 100)
    gix.close()


@pytest.mark.parametrize("name", HNSW_SCALES)
def test_hnsw_cosine_wide_beam_bf16_rows_and_default_params(orc, hv, name):
    """the wide-beam build (ef 500), bf16 rows on the one-wavefront kernel, and the production-default (non-strict) parameters"""
    data, q = hnsw_corpus(name, 128)
    oix, gix = hnsw_pair(orc, hv, data, orc.COSINE)
    assert_hnsw_equal(orc, hv, oix, gix, q, 10, 500)
    if name == "q62r62":
        cfg = hv.SimHashConfig.default()
        oix.set_simhash(int(cfg.seed))
        gix.set_simhash(cfg)
        assert_params_equal(orc, hv, oix, gix, q, hv.SearchParams.new(10), cfg)
    gix.close()
    oix, gix = hnsw_pair(orc, hv, data, orc.COSINE, dtype="bf16")
    gix.set_option(hv.OPT_HNSW_PAIR, 1)
    assert_hnsw_equal(orc, hv, oix, gix, q, 10, 100)
    gix.close()


@pytest.mark.parametrize("name", [c[0] for c in fx.L2_SCALES])
def test_hnsw_l2(orc, hv, name):
    """L2 with the shadow prune at its default (bf16_shadow_kernel's err takes part); at 2^-72 the scores are subnormals with a few bits and a
    tie re-run is legitimate: ids and score bits only"""
    limit = float(orc.lib().orc_component_limit(orc.L2SQ, 128))
    data, _, _ = fx.l2_case(name, 128, HNSW_N, 7, limit)
    rng = np.random.default_rng(5)
    q = data[rng.choice(HNSW_N, 24, replace=False)].copy()
    q[1::2] = (q[1::2] * np.float32(0.97)).astype(np.float32)
    oix, gix = hnsw_pair(orc, hv, data, orc.L2SQ)
    if name != "subnormal":
        assert_hnsw_equal(orc, hv, oix, gix, q, 10, 100)
    else:
        ids, sc, cnt, _ = gix.search_batch(q, hv.SearchParams(10).with_ef(100))
        for qi in range(24):
            rc, oid, osc = oix.search(q[qi], 10, 100)
            assert rc == orc.OK and ids[qi, :cnt[qi]].tolist() == oid.tolist() and bits(sc[qi, :cnt[qi]]).tolist() == bits(osc).tolist(), f"query {qi}"
    gix.close()


def test_hnsw_l1_at_its_limit(orc, hv):
    limit = float(orc.lib().orc_component_limit(orc.L1, 128))
    data, _, _ = fx.limit_case(128, HNSW_N, 7, limit)
    rng = np.random.default_rng(6)
    q = data[rng.choice(HNSW_N, 24, replace=False)].copy()
    q[1::2] = (q[1::2] * np.float32(0.97)).astype(np.float32)
    oix, gix = hnsw_pair(orc, hv, data, orc.L1)
    gix.set_option(hv.OPT_HNSW_GENERAL_KERNEL, 1)
    assert_hnsw_equal(orc, hv, oix, gix, q, 10, 100)
    gix.close()


# ---- device build and writes ----

@pytest.mark.parametrize("name", ["q62r62", "q-70r-70"])
def test_sequential_device_build_and_writes(orc, hv, name):
    """600 rows built one node per batch equal the oracle's insertion row for row; on the 2^62 image one delete and one upsert equal the
    oracle's delete and delete + insert"""
    n, dim, m, m0, efc = 600, 128, 16, 32, 64
    data, q = hnsw_corpus(name, dim)
    extra = data[n]
    data = np.ascontiguousarray(data[:n])
    lv = fx.draw_levels(n, m, seed=9)
    ids = np.arange(n, dtype=np.uint64) * 2 + 11
    oix = oracle_build(orc, data, orc.COSINE, lv, m, m0, efc, ids)
    ex = oix.export()
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=hv.COSINE, node_ids=ids, vectors=data, levels=lv, m=m, m0=m0, ef_construction=efc,
                                                sequential=True, reserve_rows=4)
    assert st["nodes"] == n
    g = gix.export_graph()
    assert g["entry_point"] == ex["entry_point"] and g["max_layer"] == ex["max_layer"] and g["level"].tolist() == ex["level"].tolist()
    gl0, gup = rows_of(g, n)
    ol0, oup = rows_of(ex, n)
    bad = [i for i in range(n) if gl0[i] != ol0[i]]
    assert not bad, f"{len(bad)} layer-0 rows differ, first {bad[:5]}"
    assert gup == oup
    assert_hnsw_equal(orc, hv, oix, gix, q, 10, 64)
    if name == "q62r62":
        ent = oix.entry()[0]
        gone, moved = [int(x) for x in ids if int(x) != ent][100:102]
        assert oix.delete(gone) == (orc.OK, True) and gix.delete_batch([gone])["deleted"] == 1
        assert_same_graph(gix, oix, ids, (gone,))
        level_of = {int(ids[i]): int(lv[i]) for i in range(n)}
        assert oix.delete(moved) == (orc.OK, True) and oix.insert(moved, extra, level_of[moved]) == orc.OK
        assert gix.upsert_batch(np.asarray([moved], np.uint64), extra[None, :], [level_of[moved]], ef_construction=efc)["nodes"] == 1
        assert_same_graph(gix, oix, ids, (gone,))
        gid, gsc, gcnt, _ = gix.search_batch(q, hv.SearchParams(10).with_ef(64))
        for qi in range(q.shape[0]):
            rc, oid, osc = oix.search(q[qi], 10, 64)
            assert rc == orc.OK and gid[qi, :gcnt[qi]].tolist() == oid.tolist() and bits(gsc[qi, :gcnt[qi]]).tolist() == bits(osc).tolist()
    gix.close()


# ---- storage at the edges ----

def from_bits(u, shape):
    return np.full(shape, u, np.uint32).view(np.float32)


def edge_row(kind, dim):
    fmax = np.finfo(np.float32).max
    r = np.ones(dim, np.float32)
    if kind == "fmax":
        r[:] = fmax
    elif kind == "above_bf16_max":      # 0x7F7F8000 is the tie between the largest bf16 and 2^128: RNE goes up -- to inf
        r = from_bits(0x7F7F8000, dim).copy()
    elif kind == "below_bf16_max":      # the largest f32 that still rounds to 0x7F7F
        r = from_bits(0x7F7F7FFF, dim).copy()
    elif kind == "one_ulp":             # the smallest subnormal everywhere
        r = from_bits(1, dim).copy()
    elif kind == "amax_448_ulp":        # fp8: the row scale is one ulp
        r = from_bits(1, dim).copy()
        r[0] = from_bits(448, 1)[0]
    elif kind == "amax_2_127":
        r[:] = 0.5
        r[dim // 2] = np.float32(2.0 ** 127)
    elif kind == "minus_zero":
        r[1] = np.float32(-0.0)
    elif kind == "zero":
        r[:] = 0.0
    return r


@pytest.mark.parametrize("dim", [128, 256])
@pytest.mark.parametrize("kind", ["fmax", "above_bf16_max", "below_bf16_max", "one_ulp", "amax_448_ulp", "amax_2_127", "minus_zero", "zero"])
def test_storage_at_the_edges(orc, hv, kind, dim):
    """one edge row among 63 Gaussian ones, cosine (no component limit): the import's outcome is the oracle's on the values the image would
    hold (bf16: validation sees the rounded row -- above 0x7F7F it is inf, below 2^-134 all zeros); an accepted image holds the numpy twins'
    bits and scans like the oracle, a rejected one leaves the oracle's status and no handle"""
    import torch
    n = 64
    rng = np.random.default_rng(dim)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    data[17] = edge_row(kind, dim)
    q = np.stack([data[3], np.ones(dim, np.float32)])
    ids = np.arange(n, dtype=np.uint64) + ID0
    off = np.zeros(n + 1, np.uint64)
    for dtype in ("f32", "bf16", "fp8"):
        with np.errstate(over="ignore"):
            stored = STORE[dtype](data)
        oix = orc.Index(dim, orc.COSINE)
        rc = oix.seed(ids, stored, off, np.zeros(0, np.uint64))
        try:
            gix = image(hv, data, hv.COSINE, dtype, 8)
        except hv.HelixDbError as e:
            assert rc != orc.OK and e.status == rc, f"{dtype} {kind}: device status {e.status}, oracle {rc}"
            continue
        assert rc == orc.OK, f"{dtype} {kind}: the device accepted what the oracle rejects with {rc}"
        out = torch.empty(n, dim, dtype=torch.float32, device="cuda")
        gix.read_rows_device(0, n, out)
        assert (out.cpu().numpy().view(np.uint32) == stored.view(np.uint32)).all(), f"{dtype} {kind}: stored bits"
        if dtype == "f32" or dim % 128 == 0:
            gid, gsc, gcnt, gst = flat(gix, q, 5)
            for qi in range(2):
                orc_rc, oid, osc = oix.flat(q[qi], 5)
                assert orc_rc == orc.OK and gst[qi] == hv.OK
                assert gid[qi, :gcnt[qi]].tolist() == oid.tolist() and bits(gsc[qi, :gcnt[qi]]).tolist() == bits(osc).tolist(), f"{dtype} {kind} query {qi}"
        gix.close()
