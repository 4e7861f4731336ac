"""The one-launch restricted exact scan at result counts 65 .. 800 = MAX_RESTRICTED_RESULT_COUNT (restricted.rs:55): the builds whose
result list spans 4 / 13 registers per lane (csrc/hvx_toplist.h TopListWide, csrc/hvx_restricted_wide4.hip / _wide13.hip) through the C
ABI against the oracle's restricted_exact_scan -- ids and f32 score BITS -- and against the older pipeline (OPT_RESTRICTED_DIRECT = 1):
register and tier boundaries, every shape class, every query with its own list, ties across register boundaries, duplicates that arrive
after their first copy has moved up a register, many slices and short sets, deleted rows, the batching operator, device-resident lists,
the single-query and fused-hop routes, and what stays refused."""
import threading

import numpy as np
import pytest

import fixtures as fx

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def kernels(orc, hv):
    return {"avx_fma": (orc.K_AVX_FMA, hv.KERNEL_AVX_FMA), "avx": (orc.K_AVX, hv.KERNEL_AVX), "sse": (orc.K_SSE, hv.KERNEL_SSE),
            "neon": (orc.K_NEON, hv.KERNEL_NEON), "scalar": (orc.K_SCALAR, hv.KERNEL_SCALAR)}


def image(orc, hv, ids, data, metric, kernel=None, dtype="f32", max_batch=64):
    """an oracle index and its device image over the given rows (no graph: exact scans never touch it)"""
    n, dim = data.shape
    ok, hk = kernel or (orc.K_AVX_FMA, hv.KERNEL_AVX_FMA)
    oix = orc.Index(dim, metric, kernel=ok)
    off = np.zeros(n + 1, np.uint64)
    assert oix.seed(ids, data, off, np.zeros(0, np.uint64), entry_point=int(ids[0])) == orc.OK
    gix = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=metric, node_ids=ids, vectors=data, l0_offsets=off, l0_neighbors=np.zeros(0, np.uint64),
                                              entry_point=int(ids[0]), float_kernel=hk, max_batch=max_batch,
                                              dtype=hv.BF16 if dtype == "bf16" else hv.F32)
    return oix, gix


def pair(orc, hv, n, dim, metric, kernel=None, dtype="f32", seed=0, sparse_ids=False, max_batch=64):
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((12, dim)).astype(np.float32)
    data = (centres[rng.integers(0, 12, n)] + 0.3 * rng.standard_normal((n, dim))).astype(np.float32)
    if dtype == "bf16":
        data = fx.round_bf16(data)
    ids = (np.sort(rng.choice(np.arange(10 * n, dtype=np.uint64), n, replace=False)) if sparse_ids else np.arange(n, dtype=np.uint64)) + np.uint64(7)
    oix, gix = image(orc, hv, ids, data, metric, kernel, dtype, max_batch)
    queries = (centres[rng.integers(0, 12, 40)] + 0.3 * rng.standard_normal((40, dim))).astype(np.float32)
    return oix, gix, ids, data, queries, rng


def same(got_ids, got_sc, cnt, want_ids, want_sc, what=""):
    assert got_ids[:cnt].tolist() == want_ids.tolist(), what
    assert bits(got_sc[:cnt]).tolist() == bits(want_sc).tolist(), what


def shared_set_checks(orc, hv, oix, gix, q, k, allowed, batches):
    """forced one-launch scan == the oracle == the older pipeline, for every batch size"""
    p = hv.SearchParams(k).with_ef(max(k, 64))
    want = {}
    for b in batches:
        gix.set_option(hv.OPT_RESTRICTED_DIRECT, 2)
        ids_d, sc_d, cnt_d = gix.search_restricted_batch(q[:b], p, allowed)
        assert gix.last_scan_path() == hv.PATH_DIRECT
        gix.set_option(hv.OPT_RESTRICTED_DIRECT, 1)
        ids_o, sc_o, cnt_o = gix.search_restricted_batch(q[:b], p, allowed)
        assert gix.last_scan_path() != hv.PATH_DIRECT
        for i in range(b):
            if i not in want:
                rc, want_ids, want_sc = oix.flat(q[i], k, allowed=allowed)
                assert rc == orc.OK
                want[i] = (want_ids, want_sc)
            same(ids_d[i], sc_d[i], cnt_d[i], *want[i], what=f"one launch, b {b} query {i}")
            same(ids_o[i], sc_o[i], cnt_o[i], *want[i], what=f"older pipeline, b {b} query {i}")
    gix.set_option(hv.OPT_RESTRICTED_DIRECT, 0)


def shuffled_half(rng, ids):
    picked = rng.choice(ids, len(ids) // 2, replace=False)
    allowed = np.concatenate([picked, picked[:50], np.array([1, 2, 3, 10 ** 12], np.uint64)])  # duplicates and ids that hold no vector
    rng.shuffle(allowed)
    return allowed


@pytest.mark.parametrize("k", [65, 128, 129, 256, 257, 512, 513, 800])
def test_register_and_tier_boundaries(orc, hv, k):
    """k on both sides of a register of the list (128 | 129, 512 | 513), of the 4-register build (256 | 257), the narrow build (64 | 65)
    and at the reference's limit; batches of 1 (the single-query route), 3 and 40 (more than max_batch 32 takes in one chunk)"""
    oix, gix, ids, data, q, rng = pair(orc, hv, 2000, 24, 1, kernels(orc, hv)["scalar"], "f32", seed=2024 + k, max_batch=32)
    shared_set_checks(orc, hv, oix, gix, q, k, shuffled_half(rng, ids), (1, 3, 40))
    gix.close()


WIDE_SHAPES = [
    # (n, dim, metric, kernel pair name, dtype, k, sparse ids)
    (3000, 768, 1, "avx_fma", "f32", 100, False),    # unrolled wide build, 24 chunks
    (2500, 1536, 1, "avx_fma", "f32", 300, True),    # unrolled, 48 chunks, 13 registers, ids that need the binary search
    (2000, 128, 0, "avx_fma", "f32", 100, False),    # no unrolled wide build: the any-shape build, cosine
    (1200, 72, 2, "avx_fma", "f32", 100, False),     # Manhattan
    (1500, 100, 1, "avx", "f32", 200, True),         # AVX without FMA, a scalar tail of 4
    (1500, 88, 0, "neon", "f32", 100, False),        # the 128-bit trees
    (1500, 40, 1, "sse", "f32", 70, False),
    (2500, 768, 1, "avx_fma", "bf16", 100, False),   # unrolled, bf16 rows
    (1500, 1536, 0, "avx_fma", "bf16", 300, False),  # unrolled, bf16 rows, cosine, 13 registers
    (1500, 1024, 0, "avx_fma", "bf16", 100, False),  # bf16 rows through the any-shape build
]


@pytest.mark.parametrize("n,dim,metric,kern,dtype,k,sparse", WIDE_SHAPES)
def test_shapes_shared_set(orc, hv, n, dim, metric, kern, dtype, k, sparse):
    oix, gix, ids, data, q, rng = pair(orc, hv, n, dim, metric, kernels(orc, hv)[kern], dtype, seed=dim + n + k, sparse_ids=sparse, max_batch=32)
    shared_set_checks(orc, hv, oix, gix, q, k, shuffled_half(rng, ids), (1, 40))
    gix.close()


@pytest.mark.parametrize("dtype,n", [("f32", 3000), ("bf16", 2500)])
@pytest.mark.parametrize("k", [100, 800])
def test_every_query_with_its_own_candidate_list(orc, hv, dtype, n, k):
    """hvx_search_restricted_batch_params with allowed_offsets at k > 64: ONE launch per chunk of max_batch queries (before: list by list
    through the older path); list lengths around the narrow list's width and around k, duplicates, unknown ids, an empty list, two
    rejected queries (one with a single candidate), under the device plan and the forced exact strategy"""
    dim = 768
    oix, gix, ids, data, q, rng = pair(orc, hv, n, dim, 1, None, dtype, seed=7 * dim + n + k, max_batch=16)
    b = 40
    q = q[:b].copy()
    lens = rng.integers(1, 1500, b)
    lens[[3, 9, 21, 11, 12, 13, 14, 15, 16]] = [0, 4, 1, 63, 64, 65, k - 1, k, k + 1]
    q[5, 0] = np.nan   # rejected (ValidatedMetricVector::try_new)
    q[21] = np.nan     # rejected, single candidate
    lists = []
    for i in range(b):
        own = rng.choice(ids, int(lens[i]), replace=True)  # duplicates
        if i % 4 == 0 and lens[i]:
            own = np.concatenate([own, np.array([0, 10 ** 15], np.uint64)])  # ids that hold no vector
        lists.append(own.astype(np.uint64))
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    flat = np.concatenate(lists)
    ef = max(k, 100)
    for rp in (hv.RestrictedParams.auto(k, ef), hv.RestrictedParams.new(k, ef, strategy=hv.RESTRICTED_EXACT)):
        got_ids, got_sc, got_cnt, got_st, rs, stats = gix.search_restricted_batch_params(q, rp, flat, offsets=off, want_stats=True)
        assert gix.last_scan_path() == hv.PATH_DIRECT
        assert stats["distance_computations"] == int(off[-1]) and stats["device_ms"] > 0.0
        for i in range(b):
            if len(lists[i]) == 0:
                assert got_cnt[i] == 0 and got_st[i] == 0 and rs[i]["strategy"] == 0
                continue
            rc, want_ids, want_sc = oix.flat(q[i], k, allowed=lists[i])
            if i in (5, 21):
                assert rc == orc.ERR_NONFINITE and got_st[i] == hv.ERR_NONFINITE and got_cnt[i] == 0 and rs[i]["strategy"] == 0
                continue
            assert rc == orc.OK and got_st[i] == 0 and rs[i]["strategy"] == hv.RESTRICTED_EXACT
            same(got_ids[i], got_sc[i], got_cnt[i], want_ids, want_sc, what=f"query {i}")
    # the older path (list by list) returns the same rows -- where it serves them: its exact scan over bf16 rows stops at k 511, so a bf16
    # list with more than 511 distinct ids at k 800 had NO device path before (the oracle above is the only witness there)
    gix.set_option(hv.OPT_RESTRICTED_DIRECT, 1)
    older = hv.RestrictedParams.new(k, ef, strategy=hv.RESTRICTED_EXACT)
    if dtype == "bf16" and k > 511:
        with pytest.raises(hv.HelixDbError) as e:
            gix.search_restricted_batch_params(q, older, flat, offsets=off)
        assert e.value.status == hv.ERR_UNSUPPORTED
        gix.close()
        return
    o_ids, o_sc, o_cnt, o_st, _ = gix.search_restricted_batch_params(q, older, flat, offsets=off)
    assert gix.last_scan_path() != hv.PATH_DIRECT
    assert o_cnt.tolist() == got_cnt.tolist() and o_st.tolist() == got_st.tolist()
    for i in range(b):
        assert o_ids[i, : o_cnt[i]].tolist() == got_ids[i, : got_cnt[i]].tolist() and bits(o_sc[i, : o_cnt[i]]).tolist() == bits(got_sc[i, : got_cnt[i]]).tolist()
    gix.close()


@pytest.mark.parametrize("k", [66, 130, 258])
def test_ties_across_register_boundaries(orc, hv, k):
    """every row stored four times under four ids: scores tie in fours and the tied ids come out ascending.  One copy of the nearest
    row is left out of the candidates, so the groups of four start at 3, 7, .. and straddle entries 63 | 64, 127 | 128 and 255 | 256
    (lane 63 of one register, lane 0 of the next).  The list is a permutation followed by its reverse: a duplicate arrives long after
    its first copy has moved into a higher register and counts once."""
    rng = np.random.default_rng(k)
    base = rng.standard_normal((500, 24)).astype(np.float32)
    data = np.tile(base, (4, 1))
    ids = np.arange(2000, dtype=np.uint64) + np.uint64(7)
    oix, gix = image(orc, hv, ids, data, 1, kernels(orc, hv)["scalar"])
    q = rng.standard_normal((1, 24)).astype(np.float32)
    rc, near, _ = oix.flat(q[0], 1)
    perm = rng.permutation(ids[ids != np.uint64(near[0])])
    allowed = np.concatenate([perm, perm[::-1]])
    rc, want_ids, want_sc = oix.flat(q[0], k, allowed=allowed)
    assert rc == orc.OK and len(want_ids) == k
    for forced in (2, 1):
        gix.set_option(hv.OPT_RESTRICTED_DIRECT, forced)
        g_ids, g_sc, g_cnt = gix.search_restricted_batch(q, hv.SearchParams(k).with_ef(k), allowed)
        assert (gix.last_scan_path() == hv.PATH_DIRECT) == (forced == 2)
        assert g_cnt[0] == k
        same(g_ids[0], g_sc[0], g_cnt[0], want_ids, want_sc)
        assert len(set(g_ids[0].tolist())) == k                      # a candidate counts once
        for lo in (63, 127, 255):
            if lo + 1 < k:
                assert bits(g_sc[0, lo]) == bits(g_sc[0, lo + 1]) and g_ids[0, lo] < g_ids[0, lo + 1]
        if k > 65:
            assert bits(g_sc[0, 64]) == bits(g_sc[0, 65]) and g_ids[0, 64] < g_ids[0, 65]
    gix.close()


def test_many_slices_and_short_sets(orc, hv):
    """6 000 candidates are several slices at k 130 and at k 800 (a slice holds 8 k candidates, four at the least); 500 candidates at
    k 800 answer with all of them, sorted; a batch of 40 over the shared set at k 800"""
    oix, gix, ids, data, q, rng = pair(orc, hv, 6000, 24, 1, kernels(orc, hv)["scalar"], "f32", seed=99, max_batch=64)
    everything = np.concatenate([ids, rng.choice(ids, 300)])
    rng.shuffle(everything)
    for k in (130, 800):
        shared_set_checks(orc, hv, oix, gix, q, k, everything, (1,))
    few = rng.choice(ids, 500, replace=False)
    gix.set_option(hv.OPT_RESTRICTED_DIRECT, 2)
    g_ids, g_sc, g_cnt = gix.search_restricted_batch(q[:1], hv.SearchParams(800).with_ef(800), few)
    assert gix.last_scan_path() == hv.PATH_DIRECT and g_cnt[0] == 500
    rc, want_ids, want_sc = oix.flat(q[0], 800, allowed=few)
    same(g_ids[0], g_sc[0], 500, want_ids, want_sc)
    assert sorted(g_ids[0, :500].tolist()) == sorted(few.tolist()) and np.all(np.diff(g_sc[0, :500]) >= 0)
    shared_set_checks(orc, hv, oix, gix, q, 800, everything, (40,))
    gix.close()


def test_deleted_rows_single_query_and_fused_hop(orc, hv):
    """a deleted node is no candidate (mutation.rs:1708-1745) at k 100, and the count shrinks when fewer than k live candidates remain;
    one query with 3 000 ids and the lean expand + scan land on the one-launch kernel at k 100"""
    n, dim, k = 2000, 128, 100
    rng = np.random.default_rng(11)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    lv = fx.draw_levels(n, 16, seed=3)
    ids = np.arange(n, dtype=np.uint64)
    gix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids, vectors=data, levels=lv, m=16, m0=32, ef_construction=64,
                                               sequential=True, search_max_batch=32)
    oix = orc.Index(dim, orc.L2SQ, m=16, m0=32, ef_construction=64)
    for i in range(n):
        assert oix.insert(i, data[i], int(lv[i])) == orc.OK
    gone = rng.choice(ids, 60, replace=False)
    gix.delete_batch(gone)
    for g in gone:
        assert oix.delete(int(g)) == (orc.OK, True)
    q = rng.standard_normal((8, dim)).astype(np.float32)
    lists = [rng.choice(ids, 400, replace=False).astype(np.uint64) for _ in range(8)]
    lists[2] = np.concatenate([lists[2], gone])                                   # deleted ids in the list
    live = np.setdiff1d(ids, gone)
    lists[5] = np.concatenate([rng.choice(live, 70, replace=False), gone[:50]])   # 120 ids, 70 of them live: fewer than k
    off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
    got = gix.search_restricted_batch_params(q, hv.RestrictedParams.auto(k, k), np.concatenate(lists), offsets=off)
    assert gix.last_scan_path() == hv.PATH_DIRECT
    for i in range(8):
        rc, want_ids, want_sc = oix.flat(q[i], k, allowed=lists[i])
        same(got[0][i], got[1][i], got[2][i], want_ids, want_sc, what=f"query {i}")
        assert not set(got[0][i, : got[2][i]].tolist()) & set(gone.tolist())
    assert got[2][5] == 70 and got[2][2] == k
    # one query, 3 000 ids (with duplicates), the device plan; forced: a single list this short is left to the older pipeline otherwise
    many = rng.choice(ids, 3000, replace=True).astype(np.uint64)
    gix.set_option(hv.OPT_RESTRICTED_DIRECT, 2)
    one = gix.search_restricted_batch_params(q[:1], hv.RestrictedParams.auto(k, k), many)
    assert gix.last_scan_path() == hv.PATH_DIRECT
    gix.set_option(hv.OPT_RESTRICTED_DIRECT, 0)
    slow = gix.search_restricted_batch_params(q[:1], hv.RestrictedParams.auto(k, k), many)
    assert gix.last_scan_path() != hv.PATH_DIRECT and slow[0][0].tolist() == one[0][0].tolist()
    rc, want_ids, want_sc = oix.flat(q[0], k, allowed=many)
    same(one[0][0], one[1][0], one[2][0], want_ids, want_sc)
    # fused: node i -> (i + n/2) mod n, sources 0..299 => candidates n/2 .. n/2 + 299
    tgt = ((ids + np.uint64(n // 2)) % np.uint64(n)).astype(np.uint64)
    g = hv.Graph(n, np.arange(n + 1, dtype=np.uint64), tgt)
    src = np.arange(300, dtype=np.uint64)
    # (forced: a shared set scanned once per query is left to the pipeline at k > 64 otherwise)
    gix.set_option(hv.OPT_RESTRICTED_DIRECT, 2)
    f_ids, f_sc, f_cnt, ncand, rs, _ = gix.prefilter_search_batch_params(g, q, hv.RestrictedParams.auto(k, k), src, direction=hv.DIR_OUT)
    assert ncand == 300 and gix.last_scan_path() == hv.PATH_DIRECT and all(s["strategy"] == hv.RESTRICTED_EXACT for s in rs)
    gix.set_option(hv.OPT_RESTRICTED_DIRECT, 0)
    cand = np.arange(n // 2, n // 2 + 300, dtype=np.uint64)
    for i in range(8):
        rc, want_ids, want_sc = oix.flat(q[i], k, allowed=cand)
        same(f_ids[i], f_sc[i], f_cnt[i], want_ids, want_sc, what=f"fused, query {i}")
    gix.close()


@pytest.mark.parametrize("k", [100, 800])
def test_batching_operator(orc, hv, k):
    """hvx_batcher_new_restricted at k > 64 (before: ERR_UNSUPPORTED): 16 threads x 6 calls, each with its own list of 1 .. 1 500 ids; a
    burst of 20 tickets coalesces; every answer is the oracle's"""
    n, dim = 4000, 256
    oix, gix, ids, data, q, rng = pair(orc, hv, n, dim, 1, None, "f32", seed=77 + k, sparse_ids=True, max_batch=64)
    bt = hv.RestrictedBatcher(gix, hv.RestrictedParams.auto(k, max(k, 100)), max_batch=64, max_wait_us=10000, lanes=2, max_ids_per_query=1500)
    threads, per = 16, 6
    jobs = [[(rng.standard_normal(dim).astype(np.float32), rng.choice(ids, int(rng.integers(1, 1500)), replace=True).astype(np.uint64)) for _ in range(per)]
            for _ in range(threads)]
    out = [[None] * per for _ in range(threads)]
    errs = []

    def work(t):
        try:
            for i, (qq, al) in enumerate(jobs[t]):
                out[t][i] = bt.search(qq, al)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    th = [threading.Thread(target=work, args=(t,)) for t in range(threads)]
    [x.start() for x in th]
    [x.join() for x in th]
    assert not errs, errs
    for t in range(threads):
        for i, (qq, al) in enumerate(jobs[t]):
            rc, want_ids, want_sc = oix.flat(qq, k, allowed=al)
            got = out[t][i]
            assert [r.entity_id for r in got] == want_ids.tolist() and bits(np.array([r.score for r in got], np.float32)).tolist() == bits(want_sc).tolist()
    tickets = []
    before = bt.stats()
    for i in range(20):
        tk = bt.submit(q[i], ids[i * 50:(i + 1) * 50 + 1000])
        assert tk is not None
        tickets.append(tk)
    for i, tk in enumerate(tickets):
        got = bt.wait(tk)
        rc, want_ids, want_sc = oix.flat(q[i], k, allowed=ids[i * 50:(i + 1) * 50 + 1000])
        assert [r.entity_id for r in got] == want_ids.tolist()
        assert bits(np.array([r.score for r in got], np.float32)).tolist() == bits(want_sc).tolist()
    after = bt.stats()
    assert after["queries"] - before["queries"] == 20 and after["batches"] - before["batches"] < 20   # twenty tickets in a burst: coalesced
    bt.close()
    gix.close()


def test_device_resident_lists(orc, hv):
    """ValidatedVectorReadIndex.search_restricted_lists_device: queries, fixed-stride id slots, lengths and outputs in HBM (torch
    tensors), k 100 (before: ERR_UNSUPPORTED); lengths 0, 1 and the whole slot among them"""
    import torch
    dev = torch.device("cuda:0")
    b, k, stride = 24, 100, 1024
    oix, gix, ids, data, q, rng = pair(orc, hv, 3000, 768, 1, None, "f32", seed=4242, sparse_ids=True, max_batch=32)
    lens = rng.integers(2, stride, b).astype(np.uint32)
    lens[[0, 1, 2, 3]] = [0, 1, stride, 99]
    slots = np.zeros((b, stride), np.uint64)
    lists = []
    for i in range(b):
        own = rng.choice(ids, int(lens[i]), replace=True).astype(np.uint64)
        if i % 5 == 4:
            own[0] = np.uint64(3)  # an id that holds no vector
        slots[i, : lens[i]] = own
        lists.append(own)
    dq = torch.from_numpy(q[:b].copy()).to(dev)
    d_slots = torch.from_numpy(slots.view(np.int64)).to(dev)
    d_lens = torch.from_numpy(lens.view(np.int32)).to(dev)
    o_ids = torch.zeros(b, k, dtype=torch.int64, device=dev)
    o_sc = torch.zeros(b, k, dtype=torch.float32, device=dev)
    o_cnt = torch.zeros(b, dtype=torch.int32, device=dev)
    o_st = torch.zeros(b, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    gix.search_restricted_lists_device(dq, k, d_slots, stride, d_lens, int(lens.max()), o_ids, o_sc, o_cnt, o_st)
    gix.sync()
    assert gix.last_scan_path() == hv.PATH_DIRECT
    g_ids, g_sc, g_cnt, g_st = o_ids.cpu().numpy().view(np.uint64), o_sc.cpu().numpy(), o_cnt.cpu().numpy(), o_st.cpu().numpy()
    assert g_cnt[0] == 0 and g_cnt[1] == 1 and not g_st.any()
    for i in range(1, b):
        rc, want_ids, want_sc = oix.flat(q[i], k, allowed=lists[i])
        assert rc == orc.OK
        same(g_ids[i], g_sc[i], g_cnt[i], want_ids, want_sc, what=f"query {i}")
    gix.close()


@pytest.mark.parametrize("dim,k", [(768, 800), (320, 100)])
def test_what_the_older_pipeline_refuses_goes_to_the_one_launch_scan(orc, hv, dim, k):
    """over bf16 rows the older exact pipeline stops at k 511 and serves six dimensions: a single list, four lists (fewer than the speed
    rule sends to the one launch) and a shared set of several queries are answered by the wide builds under AUTO routing, not refused"""
    oix, gix, ids, data, q, rng = pair(orc, hv, 2500, dim, 1, None, "bf16", seed=dim + k, max_batch=16)
    rp = hv.RestrictedParams.auto(k, max(k, 100))
    for b in (1, 4):
        lists = [rng.choice(ids, 1200, replace=True).astype(np.uint64) for _ in range(b)]
        off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.uint64)
        got = gix.search_restricted_batch_params(q[:b], rp, np.concatenate(lists), offsets=off)
        assert gix.last_scan_path() == hv.PATH_DIRECT
        for i in range(b):
            rc, want_ids, want_sc = oix.flat(q[i], k, allowed=lists[i])
            assert rc == orc.OK and got[3][i] == 0
            same(got[0][i], got[1][i], got[2][i], want_ids, want_sc, what=f"{b} lists, query {i}")
    allowed = rng.choice(ids, 1200, replace=False).astype(np.uint64)
    for b in (1, 3):  # one list without offsets; one set for three queries
        got = gix.search_restricted_batch_params(q[:b], rp, allowed)
        assert gix.last_scan_path() == hv.PATH_DIRECT
        for i in range(b):
            rc, want_ids, want_sc = oix.flat(q[i], k, allowed=allowed)
            same(got[0][i], got[1][i], got[2][i], want_ids, want_sc, what=f"shared, b {b} query {i}")
    gix.close()


def test_one_long_list_the_older_pipeline_refuses(orc, hv):
    """a single bf16 list at k 800 too long for the single-list route (ids x dim above 2^28: 350 000 ids with repeats over 2 500 rows)
    is deduplicated by the host and still reaches the one launch, as a shared set of one query"""
    oix, gix, ids, data, q, rng = pair(orc, hv, 2500, 768, 1, None, "bf16", seed=31, max_batch=16)
    allowed = rng.choice(ids, 350_000, replace=True).astype(np.uint64)
    got = gix.search_restricted_batch_params(q[:1], hv.RestrictedParams.auto(800, 800), allowed)
    assert gix.last_scan_path() == hv.PATH_DIRECT and got[3][0] == 0
    rc, want_ids, want_sc = oix.flat(q[0], 800, allowed=np.unique(allowed))
    assert rc == orc.OK
    same(got[0][0], got[1][0], got[2][0], want_ids, want_sc)
    gix.close()


def test_rows_at_the_length_limit(orc, hv):
    """13 list registers: the hand-over (26 KiB) and a query row of 9 600 floats are 63.6 KiB of LDS, above the 48 KiB a launch gets
    without asking; rows of 9 760 floats do not fit 64 KiB and are refused"""
    import torch
    dim, n, k = 9600, 400, 300
    oix, gix, ids, data, q, rng = pair(orc, hv, n, dim, 1, None, "f32", seed=96, max_batch=8)
    shared_set_checks(orc, hv, oix, gix, q, k, rng.permutation(ids), (1, 3))
    gix.close()
    dim = 9760
    data = rng.standard_normal((64, dim)).astype(np.float32)
    big = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=1, node_ids=np.arange(64, dtype=np.uint64), vectors=data, max_batch=8,
                                              l0_offsets=np.zeros(65, np.uint64), l0_neighbors=np.zeros(0, np.uint64))
    with pytest.raises(hv.HelixDbError) as e:
        hv.RestrictedBatcher(big, hv.RestrictedParams.auto(k, k), max_batch=8, max_ids_per_query=64)
    assert e.value.status == hv.ERR_UNSUPPORTED and "9 712" in str(e.value)
    bt = hv.RestrictedBatcher(big, hv.RestrictedParams.auto(200, 200), max_batch=8, max_ids_per_query=64)  # 4 registers: up to 14 320 floats
    got = bt.search(data[3], np.arange(64, dtype=np.uint64))
    assert len(got) == 64 and got[0].entity_id == 3
    bt.close()
    big.close()


def test_single_list_line_of_the_speed_rule(orc, hv):
    """ONE list at 64 < k <= 128 takes the one launch from 8 192 ids on (restricted_direct_pays): both sides of the line, of k 128 | 129
    and of k 64 | 65 under AUTO routing, same rows either way"""
    oix, gix, ids, data, q, rng = pair(orc, hv, 9000, 24, 1, kernels(orc, hv)["scalar"], "f32", seed=8192, max_batch=16)
    for k, m, direct in ((100, 8192, True), (100, 8191, False), (128, 8192, True), (129, 8192, False), (64, 500, True), (65, 500, False)):
        allowed = rng.choice(ids, m, replace=False).astype(np.uint64)
        got = gix.search_restricted_batch_params(q[:1], hv.RestrictedParams.auto(k, max(k, 100)), allowed)
        assert (gix.last_scan_path() == hv.PATH_DIRECT) == direct, (k, m)
        rc, want_ids, want_sc = oix.flat(q[0], k, allowed=allowed)
        same(got[0][0], got[1][0], got[2][0], want_ids, want_sc, what=f"k {k}, {m} ids")
    gix.close()


def test_what_stays_refused(orc, hv):
    """k 801 through the batcher constructor and the device-lists call; an fp8 image; OPT_RESTRICTED_DIRECT = 1 keeps the older pipeline"""
    import torch
    dev = torch.device("cuda:0")
    oix, gix, ids, data, q, rng = pair(orc, hv, 1200, 128, 1, None, "f32", seed=5, max_batch=16)
    with pytest.raises(hv.HelixDbError) as e:
        hv.RestrictedBatcher(gix, hv.RestrictedParams.auto(801, 801), max_batch=16, max_ids_per_query=1000)
    assert e.value.status == hv.ERR_UNSUPPORTED

    def device_call(ix, dim, k):
        dq = torch.zeros(2, dim, dtype=torch.float32, device=dev)
        d_slots = torch.from_numpy(np.tile(ids[:64].view(np.int64), (2, 1))).to(dev)
        d_lens = torch.full((2,), 64, dtype=torch.int32, device=dev)
        o_ids = torch.zeros(2, k, dtype=torch.int64, device=dev)
        o_sc = torch.zeros(2, k, dtype=torch.float32, device=dev)
        o_cnt = torch.zeros(2, dtype=torch.int32, device=dev)
        ix.search_restricted_lists_device(dq, k, d_slots, 64, d_lens, 64, o_ids, o_sc, o_cnt)
        ix.sync()

    with pytest.raises(hv.HelixDbError) as e:
        device_call(gix, 128, 801)
    assert e.value.status == hv.ERR_UNSUPPORTED
    gix.set_option(hv.OPT_RESTRICTED_DIRECT, 1)
    allowed = rng.choice(ids, 600, replace=False)
    g_ids, g_sc, g_cnt = gix.search_restricted_batch(q[:2], hv.SearchParams(100).with_ef(100), allowed)
    assert gix.last_scan_path() != hv.PATH_DIRECT
    rc, want_ids, want_sc = oix.flat(q[0], 100, allowed=allowed)
    same(g_ids[0], g_sc[0], g_cnt[0], want_ids, want_sc)
    gix.close()
    n = 1000
    f8 = hv.ValidatedVectorReadIndex.managed(dim=128, metric=1, node_ids=np.arange(n, dtype=np.uint64) + 7, vectors=data[:n], dtype=hv.FP8_E4M3,
                                             l0_offsets=np.zeros(n + 1, np.uint64), l0_neighbors=np.zeros(0, np.uint64), max_batch=16)
    with pytest.raises(hv.HelixDbError) as e:
        hv.RestrictedBatcher(f8, hv.RestrictedParams.auto(100, 100), max_batch=16, max_ids_per_query=500)
    assert e.value.status == hv.ERR_UNSUPPORTED
    with pytest.raises(hv.HelixDbError) as e:
        device_call(f8, 128, 100)
    assert e.value.status == hv.ERR_UNSUPPORTED
    f8.close()
