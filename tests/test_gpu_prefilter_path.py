"""Chains of `expand` hops on the device (hvx_expand_path_filter, hvx_prefilter_path_search_batch_params): every hop after the first
reads its frontier from the bitmap the hop before it wrote.  Frontier sets and per-hop sizes against the numpy twin of
tests/test_prefilter_path_host.py (whose sizes are pinned there), result ids and f32 score BITS against the oracle's exact scan over the
twin's final set, on both routes of the last hop, with and without the Filter step's node mask."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
from test_prefilter_path_host import BOTH, IN, OUT, PATH_CASES, norm_hops, path_twin, path_union

pytestmark = pytest.mark.gpu

ROUTES = {"pipeline": 1, "lean": 2}   # HVX_OPT_RESTRICTED_DIRECT: 1 = the bitmap route, 2 = the lean route


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


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def make_image(orc, hv, ids, dim, rng):
    """an oracle index and a device image over the same rows (no HNSW graph: the restricted scans are exact)"""
    data = rng.standard_normal((ids.size, dim)).astype(np.float32)
    zeros = np.zeros(ids.size + 1, np.uint64)
    oix = orc.Index(dim, orc.L2SQ)
    assert oix.seed(ids, data, zeros, np.zeros(0, np.uint64)) == orc.OK
    gix = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids, vectors=data, l0_offsets=zeros,
                                              l0_neighbors=np.zeros(0, np.uint64), max_batch=16)
    return oix, gix, ids


class Images:
    def __init__(self, orc, hv):
        rng = np.random.default_rng(65)
        self.q = rng.standard_normal((5, 64)).astype(np.float32)
        self.by_name = {"third": make_image(orc, hv, fx.THIRD_IDS, 64, rng), "contiguous": make_image(orc, hv, fx.CONTIGUOUS_IDS, 64, rng)}
        self._oracle = {}

    def oracle(self, orc, image, key, cand, k):
        """oix.flat over `cand` for every query, once per (image, key, k)"""
        if (image, key, k) not in self._oracle:
            oix = self.by_name[image][0]
            rows = []
            for qi in range(self.q.shape[0]):
                rc, oid, osc = oix.flat(self.q[qi], k, allowed=cand)
                assert rc == orc.OK
                rows.append((oid.tolist(), bits(osc).tolist()))
            self._oracle[(image, key, k)] = rows
        return self._oracle[(image, key, k)]


@pytest.fixture(scope="module")
def images(orc, hv):
    im = Images(orc, hv)
    yield im
    for _, gix, _ in im.by_name.values():
        gix.close()


def forced(hv, gix, option, call):
    gix.set_option(hv.OPT_RESTRICTED_DIRECT, option)
    try:
        out = call()
        return out, gix.last_scan_path()
    finally:
        gix.set_option(hv.OPT_RESTRICTED_DIRECT, 0)


def check_against_oracle(orc, hv, images, g, image, route, key, seeds, hops, cand, sizes, k=10, mask=None):
    """the fused chain == the twin's candidate count and per-hop sizes and the oracle's exact scan over `cand`"""
    oix, gix, image_ids = images.by_name[image]
    (ids, sc, cnt, ncand, _, got_sizes), path = forced(
        hv, gix, ROUTES[route], lambda: gix.prefilter_path_search_batch(g, images.q, hv.SearchParams(k), seeds, hops, node_mask=mask, want_sizes=True))
    assert ncand == cand.size, (key, image, route)
    assert got_sizes == sizes, (key, image, route)
    held = int(np.isin(cand, image_ids).sum())
    assert cnt.tolist() == [min(k, held)] * images.q.shape[0], (key, image, route)
    want = images.oracle(orc, image, key, cand, k) if cand.size else [([], [])] * images.q.shape[0]
    for qi in range(images.q.shape[0]):
        assert ids[qi, :cnt[qi]].tolist() == want[qi][0] and bits(sc[qi, :cnt[qi]]).tolist() == want[qi][1], (key, image, route, qi)
    if route == "lean":   # hops, row list and scan behind the one-launch scan's single host wait
        assert path == hv.PATH_DIRECT, (key, image)
    elif held:
        assert path != hv.PATH_DIRECT, (key, image)
    return held


# ---- 1. frontier sets and per-hop sizes
@pytest.mark.parametrize("name", list(PATH_CASES))
def test_frontier_sets_and_hop_sizes(hv, g70k, name):
    seeds, hops, sizes = PATH_CASES[name]
    words, got = g70k.expand_path(seeds, hops, want_sizes=True)
    assert got == sizes == [int(f.size) for f in path_twin(name)]
    assert fx.bitmap_ids(words) == set(path_twin(name)[-1].tolist())
    assert fx.bitmap_ids(g70k.expand_path(seeds, hops)) == set(path_twin(name)[-1].tolist())   # the call before left both bitmaps dirty


def test_duplicated_seeds_collapse(hv, g70k):
    seeds, hops, sizes = PATH_CASES["group_oio"]
    words, got = g70k.expand_path(np.concatenate([seeds, seeds]), hops, want_sizes=True)
    assert got == sizes and fx.bitmap_ids(words) == set(path_twin("group_oio")[-1].tolist())


# ---- 2. one hop is the old call
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", ["group", "in", "both_labelled", "sparse"])
def test_one_hop_is_the_one_hop_call(hv, g70k, images, name, route):
    seeds, kw = fx.hop_cases()[name]
    hops = [(kw.get("direction", OUT), kw.get("allowed_labels", ()))]
    p = hv.SearchParams(10)
    for image, (_, gix, _) in images.by_name.items():
        (ids, sc, cnt, ncand, _), path = forced(hv, gix, ROUTES[route], lambda: gix.prefilter_search_batch(g70k, images.q, p, seeds, **kw))
        (ids2, sc2, cnt2, ncand2, _, sizes), path2 = forced(
            hv, gix, ROUTES[route], lambda: gix.prefilter_path_search_batch(g70k, images.q, p, seeds, hops, want_sizes=True))
        assert ncand2 == ncand and sizes == [ncand] and cnt2.tolist() == cnt.tolist(), (image, name)
        assert ids2.tolist() == ids.tolist() and bits(sc2).tolist() == bits(sc).tolist(), (image, name)
        assert path2 == path, (image, name)
        # statuses: with the reference plan's parameters and a status array, through the C ABI of both calls
        rp = hv.RestrictedParams(k=10, ef=10, strategy=hv.RESTRICTED_EXACT)
        st = [np.full(5, 99, np.uint32), np.full(5, 99, np.uint32)]
        out = [(np.zeros((5, 10), np.uint64), np.zeros((5, 10), np.float32), np.zeros(5, np.uint32)) for _ in range(2)]
        s = np.ascontiguousarray(seeds, np.uint64)
        lab = np.asarray(list(kw.get("allowed_labels", ())) or [0], np.uint32)
        n_lab = len(kw.get("allowed_labels", ()))
        dirs, offs = np.array([hops[0][0]], np.uint32), np.array([0, n_lab], np.uint32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        gix.set_option(hv.OPT_RESTRICTED_DIRECT, ROUTES[route])
        try:
            nc = [C.c_uint64(0), C.c_uint64(0)]
            rc0 = hv.lib().hvx_prefilter_search_batch_params(gix._h, g70k._h, ptr(images.q), 5, C.byref(rp), 0, ptr(s), s.size, 1, hops[0][0],
                                                             ptr(lab) if n_lab else None, n_lab, 0, 0, ptr(out[0][0]), ptr(out[0][1]),
                                                             ptr(out[0][2]), ptr(st[0]), C.byref(nc[0]), None, None)
            rc1 = hv.lib().hvx_prefilter_path_search_batch_params(gix._h, g70k._h, ptr(images.q), 5, C.byref(rp), ptr(s), s.size, 1, ptr(dirs),
                                                                  ptr(offs), ptr(lab), None, ptr(out[1][0]), ptr(out[1][1]), ptr(out[1][2]),
                                                                  ptr(st[1]), C.byref(nc[1]), None, None, None)
        finally:
            gix.set_option(hv.OPT_RESTRICTED_DIRECT, 0)
        assert rc0 == rc1 == hv.OK and st[0].tolist() == st[1].tolist() == [hv.OK] * 5 and nc[0].value == nc[1].value == ncand
        assert out[0][2].tolist() == out[1][2].tolist() == cnt.tolist() and out[0][0].tolist() == out[1][0].tolist() == ids.tolist()


# ---- 3. the fused chain against the oracle
@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("name", list(PATH_CASES))
def test_fused_chain_against_the_oracle(orc, hv, g70k, images, name, route):
    seeds, hops, sizes = PATH_CASES[name]
    cand = path_twin(name)[-1]
    for image in (["contiguous"] if name in ("hubrow", "5000") else ["third", "contiguous"]):
        held = check_against_oracle(orc, hv, images, g70k, image, route, name, seeds, hops, cand, sizes)
        if name == "dead_end":
            assert held == 0 and cand.size == 0          # answers nothing, status OK (the call did not raise)
        if name == "vectorless":
            assert held == int(np.isin(cand, images.by_name[image][2]).sum()) and cand.size == 14


@pytest.mark.parametrize("route", list(ROUTES))
def test_fused_chain_with_a_hundred_results(orc, hv, g70k, images, route):
    seeds, hops, sizes = PATH_CASES["group3"]
    for image in ("third", "contiguous"):
        assert check_against_oracle(orc, hv, images, g70k, image, route, "group3", seeds, hops, path_twin("group3")[-1], sizes, k=100) >= 100


# ---- 4. the Filter step
def mask_words(n, keep):
    b = np.zeros(((n + 63) // 64) * 64, np.uint8)
    b[:n] = keep
    return np.packbits(b, bitorder="little").view(np.uint64)


@pytest.mark.parametrize("route", list(ROUTES))
@pytest.mark.parametrize("which", ["thirds", "not_thirds", "nothing"])
def test_filter_mask(orc, hv, g70k, images, which, route):
    seeds, hops, sizes = PATH_CASES["group3"]
    n = g70k.n
    keep = {"thirds": np.arange(n) % 3 == 0, "not_thirds": np.arange(n) % 3 != 0, "nothing": np.zeros(n, bool)}[which]
    final = path_twin("group3")[-1]
    cand = final[keep[final.astype(np.int64)]]
    assert (cand.size == 0) == (which == "nothing") and cand.size < final.size
    for image in ("third", "contiguous"):
        check_against_oracle(orc, hv, images, g70k, image, route, "group3/" + which, seeds, hops, cand, sizes, mask=mask_words(n, keep))
    # the mask of one call is not the next call's
    check_against_oracle(orc, hv, images, g70k, "third", route, "group3", seeds, hops, final, sizes)


# ---- 5. past one pass of the hop kernel's grid, and the candidate limit
RING = 1_200_000   # the hop kernel's grid is capped at 512 workgroups of 1 024 node numbers: one pass covers 524 288 nodes


class Ring:
    def __init__(self, orc, hv):
        n = RING
        self.g = hv.Graph(n, np.arange(n + 1, dtype=np.uint64), (np.arange(n, dtype=np.uint64) + np.uint64(1)) % np.uint64(n))
        rng = np.random.default_rng(12)
        self.first = n - 4096
        self.oix, self.gix, self.ids = make_image(orc, hv, np.arange(self.first, n, dtype=np.uint64), 64, rng)
        self.q = rng.standard_normal((5, 64)).astype(np.float32)


@pytest.fixture(scope="module")
def ring(orc, hv):
    r = Ring(orc, hv)
    yield r
    r.gix.close()
    r.g.close()


def ring_check(orc, hv, ring, route):
    seeds = np.arange(ring.first - 70, ring.first, dtype=np.uint64)
    cand = seeds + np.uint64(3)
    (ids, sc, cnt, ncand, _, sizes), path = forced(
        hv, ring.gix, ROUTES[route], lambda: ring.gix.prefilter_path_search_batch(ring.g, ring.q, hv.SearchParams(10), seeds, [OUT] * 3, want_sizes=True))
    assert ncand == 70 and sizes == [70, 70, 70] and cnt.tolist() == [3] * 5
    assert (path == hv.PATH_DIRECT) == (route == "lean")
    for qi in range(5):
        rc, oid, osc = ring.oix.flat(ring.q[qi], 10, allowed=cand)
        assert rc == orc.OK and ids[qi, :3].tolist() == oid.tolist() and bits(sc[qi, :3]).tolist() == bits(osc).tolist()


@pytest.mark.parametrize("route", list(ROUTES))
def test_frontier_past_one_grid_pass(orc, hv, ring, route):
    assert RING > 512 * 1024
    ring_check(orc, hv, ring, route)
    words, sizes = ring.g.expand_path([RING - 2, 600_000], [OUT, OUT, IN], want_sizes=True)   # across the ring's seam, and the second pass
    assert sizes == [2, 2, 2] and fx.bitmap_ids(words) == {RING - 1, 600_001}


def test_candidate_limit(orc, hv, ring):
    with pytest.raises(hv.HelixDbError) as e:
        ring.gix.prefilter_path_search_batch(ring.g, ring.q, hv.SearchParams(10), np.arange(RING, dtype=np.uint64), [OUT, OUT], want_sizes=True)
    assert e.value.status == hv.ERR_CANDIDATE_LIMIT and e.value.n_candidates == RING and e.value.hop_sizes == [RING, RING]
    ring_check(orc, hv, ring, "lean")
    ring_check(orc, hv, ring, "pipeline")


# ---- 6. argument rules
def raw_path_calls(hv, g, gix, q, seeds, dirs, offs, labs):
    """both entry points through the C ABI with the arrays as given: (status of hvx_expand_path_filter, status of the fused call)"""
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    s = np.ascontiguousarray(seeds, np.uint64)
    dirs = np.ascontiguousarray(dirs, np.uint32)
    offs = None if offs is None else np.ascontiguousarray(offs, np.uint32)
    labs = np.ascontiguousarray(labs if len(labs) else [0], np.uint32)
    words = np.zeros((g.n + 63) // 64, np.uint64)
    sizes = np.full(32, 77, np.uint64)
    rc0 = hv.lib().hvx_expand_path_filter(g._h, ptr(s), s.size, dirs.size, ptr(dirs), ptr(offs), ptr(labs), ptr(words), ptr(sizes))
    rp = hv.RestrictedParams(k=10, ef=10, strategy=hv.RESTRICTED_EXACT)
    ids = np.zeros((q.shape[0], 10), np.uint64); sc = np.zeros((q.shape[0], 10), np.float32); cnt = np.full(q.shape[0], 9, np.uint32)
    nc = C.c_uint64(5)
    sizes1 = np.full(32, 77, np.uint64)
    rc1 = hv.lib().hvx_prefilter_path_search_batch_params(gix._h, g._h, ptr(q), q.shape[0], C.byref(rp), ptr(s), s.size, dirs.size, ptr(dirs), ptr(offs),
                                                          ptr(labs), None, ptr(ids), ptr(sc), ptr(cnt), None, C.byref(nc), ptr(sizes1), None, None)
    return rc0, rc1, words, sizes, cnt, nc.value, sizes1


REFUSED = {
    "no_hops": ([1000], [], [0], []),
    "seventeen_hops": ([1000], [OUT] * 17, None, []),
    "bad_direction": ([1000], [OUT, 3], None, []),
    "offsets_descend": ([1000], [OUT, OUT], [0, 2, 1], [0, 1]),
    "unknown_seed": ([1000, 70001], [OUT, OUT], None, []),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_arguments_leave_nothing_behind(orc, hv, g70k, images, name):
    _, gix, _ = images.by_name["third"]
    seeds, hops, sizes = PATH_CASES["labelled"]
    before = gix.prefilter_path_search_batch(g70k, images.q, hv.SearchParams(10), seeds, hops, want_sizes=True)
    bad_seeds, dirs, offs, labs = REFUSED[name]
    rc0, rc1, _, _, _, _, _ = raw_path_calls(hv, g70k, gix, images.q, bad_seeds, dirs, offs, labs)
    assert rc0 == rc1 == hv.ERR_INVARIANT
    after = gix.prefilter_path_search_batch(g70k, images.q, hv.SearchParams(10), seeds, hops, want_sizes=True)
    assert after[3] == before[3] == sizes[-1] and after[5] == before[5] == sizes
    assert after[0].tolist() == before[0].tolist() and bits(after[1]).tolist() == bits(before[1]).tolist()
    words, got = g70k.expand_path(seeds, hops, want_sizes=True)
    assert got == sizes and fx.bitmap_ids(words) == set(path_twin("labelled")[-1].tolist())


def test_sixteen_hops_and_no_seeds(orc, hv, g70k, images):
    _, gix, _ = images.by_name["third"]
    n, off, tgt, lab = fx.prefilter_graph("g70k")
    hops = [OUT, IN] * 8
    want = path_union(off, tgt, lab, fx.ISLAND_SEEDS, hops)
    words, sizes = g70k.expand_path(fx.ISLAND_SEEDS, hops, want_sizes=True)
    assert sizes == [int(f.size) for f in want] and fx.bitmap_ids(words) == set(want[-1].tolist())
    rc0, rc1, words, sizes, cnt, ncand, sizes1 = raw_path_calls(hv, g70k, gix, images.q, [], [OUT, BOTH], None, [])
    assert rc0 == rc1 == hv.OK and not words.any() and cnt.tolist() == [0] * 5 and ncand == 0
    assert sizes[:3].tolist() == [0, 0, 77] and sizes1[:3].tolist() == [0, 0, 77]
    # NULL label offsets mean every label on every hop
    rc0, rc1, words, sizes, _, ncand, sizes1 = raw_path_calls(hv, g70k, gix, images.q, PATH_CASES["group3"][0], [OUT] * 3, None, [])
    assert rc0 == rc1 == hv.OK and sizes[:3].tolist() == sizes1[:3].tolist() == PATH_CASES["group3"][2] and ncand == PATH_CASES["group3"][2][-1]
    assert norm_hops([OUT, (IN, [1])]) == [(OUT, ()), (IN, (1,))]
