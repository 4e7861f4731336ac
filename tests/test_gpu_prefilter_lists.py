"""Chains of `expand` hops with PER-QUERY seeds on the device (hvx_expand_path_lists, hvx_prefilter_path_search_lists_params): one launch,
one workgroup per query, every query's final set in its own slot of the one-launch restricted scan.  Frontier sets and per-hop sizes against
the per-query numpy twin (tests/test_prefilter_lists_host.py pins its sizes), result ids and f32 score BITS against the oracle's exact scan
over each query's own set, every row against the shared-seed call run for that query alone."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
from test_gpu_prefilter_path import bits, make_image
from test_prefilter_lists_host import LIST_BATCHES, MANY, clipped, lists_twin, small_groups
from test_prefilter_path_host import OUT, SMALL_LAB, SMALL_OFF, SMALL_TGT, path_union

pytestmark = pytest.mark.gpu

B = len(LIST_BATCHES["plain"][0])   # the mixed batches: 12 queries


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


@pytest.fixture(scope="module")
def g70k(hv):
    n, off, tgt, lab = fx.prefilter_graph("g70k")
    g = hv.Graph(n, off, tgt, lab)
    yield g
    g.close()


class Images:
    def __init__(self, orc, hv):
        rng = np.random.default_rng(66)
        self.q = rng.standard_normal((B, 64)).astype(np.float32)
        self.by_name = {"third": make_image(orc, hv, fx.THIRD_IDS, 64, rng), "contiguous": make_image(orc, hv, fx.CONTIGUOUS_IDS, 64, rng)}
        self._oracle = {}

    def oracle(self, orc, image, qi, key, cand, k):
        """oix.flat of query qi over `cand`, once per (image, query, key, k)"""
        if (image, qi, key, k) not in self._oracle:
            ids, sc = [], []
            if cand.size:
                rc, oid, osc = self.by_name[image][0].flat(self.q[qi], k, allowed=cand)
                assert rc == orc.OK
                ids, sc = oid.tolist(), bits(osc).tolist()
            self._oracle[(image, qi, key, k)] = (ids, sc)
        return self._oracle[(image, qi, key, k)]


@pytest.fixture(scope="module")
def images(orc, hv):
    im = Images(orc, hv)
    yield im
    for _, gix, _ in im.by_name.values():
        gix.close()


def mask_words(n, keep):
    b = np.zeros(((n + 63) // 64) * 64, np.uint8)
    b[:n] = keep
    return np.packbits(b, bitorder="little").view(np.uint64)


def keep_of(n, which):
    return {"none": None, "thirds": np.arange(n) % 3 == 0, "nothing": np.zeros(n, bool)}[which]


def masked(final, keep):
    return final if keep is None else final[keep[final.astype(np.int64)]]


def check_sets(hv, g, name):
    seeds, hops, mf, pinned = LIST_BATCHES[name]
    lists, st, sizes = g.expand_path_lists(seeds, hops, mf)
    twin = lists_twin(name)
    assert sizes.tolist() == pinned, name
    for q, got in enumerate(lists):
        want_sizes, over = clipped([int(f.size) for f in twin[q]], mf)
        assert sizes[q].tolist() == want_sizes and st[q] == (hv.ERR_CANDIDATE_LIMIT if over else hv.OK), (name, q)
        want = [] if over else twin[q][-1].tolist()
        assert got.size == len(set(got.tolist())) == len(want) and sorted(got.tolist()) == want, (name, q)


def check_fused(orc, hv, images, g, name, image, k, which):
    """every query's row == the oracle's exact scan over the twin's set of THAT query; candidates, sizes and statuses the twin's"""
    seeds, hops, mf, pinned = LIST_BATCHES[name]
    oix, gix, image_ids = images.by_name[image]
    keep = keep_of(g.n, which)
    q = images.q[: len(seeds)]
    ids, sc, cnt, st, ncand, _, sizes = gix.prefilter_path_search_lists(g, q, hv.SearchParams(k), seeds, hops, max_frontier=mf, want_sizes=True,
                                                                        node_mask=None if keep is None else mask_words(g.n, keep))
    assert gix.last_scan_path() == hv.PATH_DIRECT
    assert sizes.tolist() == pinned, (name, image, k, which)
    for qi, sets in enumerate(lists_twin(name)):
        over = clipped([int(f.size) for f in sets], mf)[1]
        cand = np.zeros(0, np.uint64) if over else masked(sets[-1], keep)
        assert st[qi] == (hv.ERR_CANDIDATE_LIMIT if over else hv.OK) and ncand[qi] == cand.size, (name, image, k, which, qi)
        assert cnt[qi] == min(k, int(np.isin(cand, image_ids).sum())), (name, image, k, which, qi)
        want = images.oracle(orc, image, qi, (name, which), cand, k)
        assert ids[qi, :cnt[qi]].tolist() == want[0] and bits(sc[qi, :cnt[qi]]).tolist() == want[1], (name, image, k, which, qi)
    return ids, sc, cnt, st, ncand, sizes


# ---- 1. frontier sets
@pytest.mark.parametrize("name", ["plain", "labelled", "both"])
def test_frontier_sets_per_query(hv, g70k, name):
    check_sets(hv, g70k, name)
    check_sets(hv, g70k, name)   # the call before left table, slots and frontier lists dirty


def test_node_mask_on_the_sets(hv, g70k):
    seeds, hops, mf, pinned = LIST_BATCHES["plain"]
    keep = keep_of(g70k.n, "thirds")
    lists, st, sizes = g70k.expand_path_lists(seeds, hops, mf, node_mask=mask_words(g70k.n, keep))
    assert sizes.tolist() == pinned and st.tolist() == [hv.OK] * B   # the sizes are the unmasked ones
    for q, got in enumerate(lists):
        assert sorted(got.tolist()) == masked(lists_twin("plain")[q][-1], keep).tolist(), q


def test_hand_written_graph_grouped_by_chain(hv):
    g = hv.Graph(8, SMALL_OFF, SMALL_TGT, SMALL_LAB)
    try:
        for hops, seeds, finals, want_sizes in small_groups():
            lists, st, sizes = g.expand_path_lists(seeds, hops, 8)
            assert st.tolist() == [hv.OK] * len(seeds) and sizes.tolist() == want_sizes, hops
            assert [sorted(x.tolist()) for x in lists] == finals and all(x.size == len(set(x.tolist())) for x in lists), hops
    finally:
        g.close()


# ---- 2. the fused call against the oracle
@pytest.mark.parametrize("which", ["none", "thirds", "nothing"])
@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("image", ["third", "contiguous"])
def test_fused_call_against_the_oracle(orc, hv, g70k, images, image, k, which):
    check_fused(orc, hv, images, g70k, "plain", image, k, which)


@pytest.mark.parametrize("image,k,which", [("third", 10, "none"), ("contiguous", 100, "thirds")])
def test_fused_call_with_the_largest_slot(orc, hv, g70k, images, image, k, which):
    check_fused(orc, hv, images, g70k, "labelled", image, k, which)


# ---- 3. every row is the shared-seed call's for that query alone
@pytest.mark.parametrize("name,image", [("plain", "third"), ("both", "contiguous")])
def test_rows_equal_the_shared_seed_call(hv, g70k, images, name, image):
    seeds, hops, mf, _ = LIST_BATCHES[name]
    _, gix, _ = images.by_name[image]
    p = hv.SearchParams(10)
    q = images.q[: len(seeds)]
    ids, sc, cnt, st, ncand, _, sizes = gix.prefilter_path_search_lists(g70k, q, p, seeds, hops, max_frontier=mf, want_sizes=True)
    for qi, s in enumerate(seeds):
        i1, s1, c1, n1, _, z1 = gix.prefilter_path_search_batch(g70k, q[qi:qi + 1], p, s, hops, want_sizes=True)
        assert st[qi] == hv.OK and cnt[qi] == c1[0] and ncand[qi] == n1 and sizes[qi].tolist() == z1, (name, qi)
        assert ids[qi, :cnt[qi]].tolist() == i1[0, :c1[0]].tolist() and bits(sc[qi, :cnt[qi]]).tolist() == bits(s1[0, :c1[0]]).tolist(), (name, qi)


# ---- 4. a chain that outgrows its slot
def test_overflow_marks_the_query_and_spares_the_others(orc, hv, g70k, images):
    check_sets(hv, g70k, "overflow")
    for image in ("third", "contiguous"):
        ids, sc, cnt, st, ncand, sizes = check_fused(orc, hv, images, g70k, "overflow", image, 10, "none")
        assert st.tolist() == [hv.ERR_CANDIDATE_LIMIT, hv.OK, hv.OK] and cnt[0] == 0 and sizes[0].tolist() == [1001, 0, 0]
    # a 25 000-arc row against the table's 4 096-slot floor: the call comes back
    check_sets(hv, g70k, "hub")
    _, _, cnt, st, ncand, sizes = check_fused(orc, hv, images, g70k, "hub", "contiguous", 10, "none")
    assert st.tolist() == [hv.ERR_CANDIDATE_LIMIT] and cnt.tolist() == [0] and sizes.tolist() == [[9, 0]]
    # an overflowed query whose vector is invalid as well: the candidate limit wins
    seeds, hops, mf, _ = LIST_BATCHES["overflow"]
    q = images.q[:3].copy()
    q[0, 0] = np.nan
    q[2, 1] = np.inf
    out = images.by_name["third"][1].prefilter_path_search_lists(g70k, q, hv.SearchParams(10), seeds, hops, max_frontier=mf)
    assert out[3].tolist() == [hv.ERR_CANDIDATE_LIMIT, hv.OK, hv.ERR_NONFINITE] and out[2][0] == out[2][2] == 0 and out[2][1] > 0
    # the scratch is clean: the mixed batch answers as before
    check_fused(orc, hv, images, g70k, "plain", "third", 10, "none")
    check_fused(orc, hv, images, g70k, "plain", "contiguous", 100, "thirds")


# ---- 5. more queries than compute units
def test_more_queries_than_compute_units(orc, hv, g70k):
    rng = np.random.default_rng(67)
    data = rng.standard_normal((fx.CONTIGUOUS_IDS.size, 64)).astype(np.float32)
    zeros = np.zeros(fx.CONTIGUOUS_IDS.size + 1, np.uint64)
    oix = orc.Index(64, orc.L2SQ)
    assert oix.seed(fx.CONTIGUOUS_IDS, data, zeros, np.zeros(0, np.uint64)) == orc.OK
    gix = hv.ValidatedVectorReadIndex.managed(dim=64, metric=hv.EUCLIDEAN, node_ids=fx.CONTIGUOUS_IDS, vectors=data, l0_offsets=zeros,
                                              l0_neighbors=np.zeros(0, np.uint64), max_batch=512)
    try:
        q = rng.standard_normal((MANY, 64)).astype(np.float32)
        seeds = [[1000 + i] for i in range(MANY)]
        ids, sc, cnt, st, ncand, _, sizes = gix.prefilter_path_search_lists(g70k, q, hv.SearchParams(10), seeds, [OUT], max_frontier=1024, want_sizes=True)
        _, off, tgt, lab = fx.prefilter_graph("g70k")
        assert st.tolist() == [hv.OK] * MANY
        for qi in range(MANY):
            row = path_union(off, tgt, lab, seeds[qi], [OUT])[0]
            assert ncand[qi] == row.size == sizes[qi, 0], qi
            want_ids, want_sc = [], []
            if row.size:
                rc, oid, osc = oix.flat(q[qi], 10, allowed=row)
                assert rc == orc.OK
                want_ids, want_sc = oid.tolist(), bits(osc).tolist()
            assert ids[qi, :cnt[qi]].tolist() == want_ids and bits(sc[qi, :cnt[qi]]).tolist() == want_sc, qi
    finally:
        gix.close()


# ---- 6. what is refused, before anything runs
def raw_lists_calls(hv, g, gix, q, seeds, soff, dirs, offs, labs, mf, k=10, ef=10, strategy=None, budgets=0, null=None):
    """both entry points through the C ABI with the arrays as given: (status of hvx_expand_path_lists or None, status of the fused call)"""
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    s = np.ascontiguousarray(seeds if len(seeds) else [0], np.uint64)
    soff = np.ascontiguousarray(soff, np.uint64)
    b = soff.size - 1
    dirs = np.ascontiguousarray(dirs if len(dirs) else [0], np.uint32)
    n_hops = len(dirs) if null != "no_hops" else 0
    offs = None if offs is None else np.ascontiguousarray(offs, np.uint32)
    labs = np.ascontiguousarray(labs if len(labs) else [0], np.uint32)
    ids = np.zeros((b, max(mf, 1)), np.uint64); lens = np.zeros(b, np.uint32); st = np.zeros(b, np.uint32)
    rc0 = hv.lib().hvx_expand_path_lists(g._h, b, ptr(s), None if null == "offsets" else ptr(soff), n_hops, None if null == "directions" else ptr(dirs),
                                         ptr(offs), ptr(labs), None, mf, ptr(ids), ptr(lens), None if null == "status" else ptr(st), None)
    rp = hv.RestrictedParams(k=k, ef=ef, strategy=hv.RESTRICTED_EXACT if strategy is None else strategy)
    rp.explicit_budgets = budgets
    kk = max(k, 1)
    oid = np.zeros((b, kk), np.uint64); osc = np.zeros((b, kk), np.float32); cnt = np.zeros(b, np.uint32)
    rc1 = hv.lib().hvx_prefilter_path_search_lists_params(gix._h, g._h, ptr(q[:b]), b, C.byref(rp), ptr(s), None if null == "offsets" else ptr(soff),
                                                          n_hops, None if null == "directions" else ptr(dirs), ptr(offs), ptr(labs), None, mf,
                                                          ptr(oid), ptr(osc), ptr(cnt), None if null == "status" else ptr(st), None, None, None)
    return rc0, rc1


GOOD = dict(seeds=[1000, 1001, 1020], soff=[0, 2, 3], dirs=[OUT, OUT], offs=None, labs=[], mf=64)
# name -> (what differs from GOOD, status of both calls; None = the rule is the fused call's alone)
REFUSED = {
    "null_offsets": (dict(null="offsets"), "ERR_INVARIANT", True),
    "null_directions": (dict(null="directions"), "ERR_INVARIANT", True),
    "null_status": (dict(null="status"), "ERR_INVARIANT", True),
    "no_hops": (dict(null="no_hops"), "ERR_INVARIANT", True),
    "seventeen_hops": (dict(dirs=[OUT] * 17), "ERR_INVARIANT", True),
    "bad_direction": (dict(dirs=[OUT, 3]), "ERR_INVARIANT", True),
    "label_offsets_descend": (dict(offs=[0, 2, 1], labs=[0, 1]), "ERR_INVARIANT", True),
    "seed_offsets_descend": (dict(soff=[0, 3, 2]), "ERR_INVARIANT", True),
    "unknown_seed": (dict(seeds=[1000, 1001, 70001]), "ERR_INVARIANT", True),
    "more_seeds_than_the_slot": (dict(mf=1), "ERR_INVARIANT", True),
    "no_frontier": (dict(mf=0), "ERR_UNSUPPORTED", True),
    "frontier_above_the_table": (dict(mf=16385), "ERR_UNSUPPORTED", True),
    "k_zero": (dict(k=0, ef=0), "ERR_K_RANGE", False),
    "ef_below_k": (dict(k=10, ef=9), "ERR_K_RANGE", False),
    "k_above_800": (dict(k=801, ef=801), "ERR_UNSUPPORTED", False),
    "batch_above_max_batch": (dict(seeds=[1000] * 17, soff=list(range(18))), "ERR_UNSUPPORTED", False),
    "filtered": (dict(strategy="RESTRICTED_FILTERED"), "ERR_UNSUPPORTED", False),
    "reference_plan": (dict(strategy="RESTRICTED_REFERENCE_PLAN"), "ERR_UNSUPPORTED", False),
    "explicit_budgets": (dict(budgets=1), "ERR_UNSUPPORTED", False),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_calls_leave_nothing_behind(orc, hv, g70k, images, name):
    _, gix, _ = images.by_name["third"]
    change, status, both = REFUSED[name]
    kw = dict(GOOD, **change)
    if isinstance(kw.get("strategy"), str):
        kw["strategy"] = getattr(hv, kw["strategy"])
    q = np.tile(images.q, (2, 1))
    good0, good1 = raw_lists_calls(hv, g70k, gix, q, **GOOD)
    assert good0 == good1 == hv.OK
    rc0, rc1 = raw_lists_calls(hv, g70k, gix, q, **kw)
    assert rc1 == getattr(hv, status) and rc0 == (rc1 if both else hv.OK), name
    check_fused(orc, hv, images, g70k, "plain", "third", 10, "none")
    check_sets(hv, g70k, "both")


def test_images_the_scan_does_not_serve(hv, g70k):
    rng = np.random.default_rng(68)
    n = 1000
    f8 = hv.ValidatedVectorReadIndex.managed(dim=128, metric=hv.EUCLIDEAN, node_ids=np.arange(n, dtype=np.uint64) + 5000,
                                             vectors=rng.standard_normal((n, 128)).astype(np.float32), dtype=hv.FP8_E4M3,
                                             l0_offsets=np.zeros(n + 1, np.uint64), l0_neighbors=np.zeros(0, np.uint64), max_batch=16)
    try:
        with pytest.raises(hv.HelixDbError) as e:
            f8.prefilter_path_search_lists(g70k, rng.standard_normal((2, 128)).astype(np.float32), hv.SearchParams(10), [[1000], [1020]], [OUT],
                                           max_frontier=64)
        assert e.value.status == hv.ERR_UNSUPPORTED
    finally:
        f8.close()
