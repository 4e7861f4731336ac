"""repeat(expand).times(n).emit() with PER-QUERY seeds on the device (hvx_expand_repeat_lists, hvx_prefilter_repeat_search_lists_params): one
launch, one workgroup per query, every query's emitted set in its own slot of the one-launch restricted scan.  The kernel walks
breadth-first WITH visited exclusion; the twin (tests/test_prefilter_repeat_host.py, which pins its sizes) is the reference's loop without
it.  Emitted sets, sizes and stop depths against the twin, result ids and f32 score BITS against the oracle's exact scan over each query's
own set, and the sets against the device's own traversal and chain routes."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
from test_gpu_prefilter_lists import B, check_sets as check_chain_sets, g70k, hv, images, keep_of, mask_words, masked  # noqa: F401 (fixtures)
from test_gpu_prefilter_path import bits
from test_prefilter_path_host import BOTH, OUT, SMALL_LAB, SMALL_OFF, SMALL_TGT
from test_prefilter_repeat_host import (AFTER, ALL, BEFORE, HUB, MODES, OVERFLOW_MF, PINNED, REPEAT_BATCHES, SMALL_REPEATS, UNTIL_NODE, UNTIL_SEEDS,
                                        UNTIL_SIZES_ALL, UNTIL_STOPS, repeat_twin, repeat_union, reported)

pytestmark = pytest.mark.gpu


def node_words(n, nodes):
    keep = np.zeros(n, bool)
    keep[list(nodes)] = True
    return mask_words(n, keep)


def check_lists(hv, lists, st, stop, sizes, twins, mf, keep=None, tag=None):
    """every request of one call against its twin as the calls report it: duplicate-free ids, sizes, stop depth, status"""
    assert len(lists) == len(twins)
    for q, t in enumerate(twins):
        emitted, want_sizes, want_stop, over = reported(t, mf)
        assert sizes[q].tolist() == want_sizes and stop[q] == want_stop and st[q] == (hv.ERR_CANDIDATE_LIMIT if over else hv.OK), (tag, q)
        want = masked(emitted, keep).tolist()
        got = lists[q].tolist()
        assert len(got) == len(set(got)) == len(want) and sorted(got) == want, (tag, q)


def check_sets(hv, g, name, mode, which="none", mf=None):
    seeds, direction, allowed, times, mf0 = REPEAT_BATCHES[name]
    mf = mf0 if mf is None else mf
    keep = keep_of(g.n, which)
    out = g.expand_repeat_lists(seeds, times, MODES[mode], direction, allowed, node_mask=None if keep is None else mask_words(g.n, keep),
                                max_frontier=mf)
    check_lists(hv, *out, repeat_twin(name, mode), mf, keep, (name, mode, which))
    return out


# ---- 1. emitted sets and sizes
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(REPEAT_BATCHES))
def test_emitted_sets_per_query(hv, g70k, name, mode):
    for _ in range(2):   # the first call leaves table, slots and level lists dirty
        _, _, stop, sizes = check_sets(hv, g70k, name, mode)
        assert sizes.tolist() == PINNED[name][mode] and stop.tolist() == [0] * B


def test_hand_written_graph_grouped_by_body(hv):
    groups = {}
    for seeds, direction, allowed, times, until, want in SMALL_REPEATS:
        groups.setdefault((direction, allowed, times, until), []).append((seeds, want))
    every = [[0], [0, 0, 0], [1], [4], [5], [6], [7], [3], [0, 4, 6], [], [2, 1, 2]]
    g = hv.Graph(8, SMALL_OFF, SMALL_TGT, SMALL_LAB)
    try:
        for (direction, allowed, times, until), cases in groups.items():
            pw = None if until is None else node_words(8, until)
            for emit in (BEFORE, AFTER, ALL):
                # the cases of this body as one batch, against the values written by hand
                lists, st, stop, sizes = g.expand_repeat_lists([s for s, _ in cases], times, emit, direction, allowed, until_mask=pw, max_frontier=8)
                assert st.tolist() == [hv.OK] * len(cases)
                for q, (_, want) in enumerate(cases):
                    assert (sorted(lists[q].tolist()), sizes[q].tolist(), int(stop[q])) == want[emit], (direction, allowed, times, until, emit, q)
                # ... and every seed list under this body against the twin
                out = g.expand_repeat_lists(every, times, emit, direction, allowed, until_mask=pw, max_frontier=8)
                twins = [repeat_union(SMALL_OFF, SMALL_TGT, SMALL_LAB, s, direction, allowed, times, emit, until) for s in every]
                check_lists(hv, *out, twins, 8, None, (direction, allowed, times, until, emit))
    finally:
        g.close()


# ---- 2. until
@pytest.mark.parametrize("mode", list(MODES))
def test_until_stops_the_loop(hv, g70k, mode):
    pw = node_words(g70k.n, [UNTIL_NODE])
    out = g70k.expand_repeat_lists(UNTIL_SEEDS, 4, MODES[mode], OUT, (), until_mask=pw, max_frontier=16384)
    check_lists(hv, *out, repeat_twin("out3", mode, until=(UNTIL_NODE,), seeds=UNTIL_SEEDS, times=4), 16384, None, mode)
    assert out[2].tolist() == UNTIL_STOPS
    if mode == "all":
        assert out[3].tolist() == UNTIL_SIZES_ALL


def test_until_sees_the_seed_that_comes_back(hv, g70k):
    _, off, tgt, lab = fx.prefilter_graph("g70k")
    pw = node_words(g70k.n, [8191])
    for emit in (BEFORE, AFTER, ALL):
        # under label 1 the seed is an arc target again at iteration 2, among 8 462 nodes: inside the largest slot
        t = repeat_union(off, tgt, lab, [8191], BOTH, (1,), 4, emit, until=(8191,))
        assert t[2] == 2 and (emit != ALL or t[1] == [4, 8462, 8462, 8462])
        out = g70k.expand_repeat_lists([[8191]], 4, emit, BOTH, (1,), until_mask=pw, max_frontier=16384)
        check_lists(hv, *out, [t], 16384, None, emit)
        assert out[2].tolist() == [2]
        # under every label iteration 2 reaches 25 017 nodes: the overflow wins over the predicate that fires in the same iteration
        t = repeat_union(off, tgt, lab, [8191], BOTH, (), 3, emit, until=(8191,))
        assert t[2] == 2 and t[3][1] > 16384
        out = g70k.expand_repeat_lists([[8191]], 3, emit, BOTH, (), until_mask=pw, max_frontier=16384)
        check_lists(hv, *out, [t], 16384, None, emit)
        assert out[1].tolist() == [hv.ERR_CANDIDATE_LIMIT] and out[2].tolist() == [0]
    # a predicate of seeds that no arc reaches again stops nothing
    out = g70k.expand_repeat_lists([[1020], [1021]], 3, ALL, OUT, (), until_mask=node_words(g70k.n, [1020, 1021]), max_frontier=4096)
    assert out[2].tolist() == [0, 0] and out[3].tolist() == [PINNED["out3"]["all"][8], PINNED["out3"]["all"][9]]


# ---- 3. the node mask
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("which", ["thirds", "nothing"])
def test_node_mask_on_the_emitted_sets(hv, g70k, which, mode):
    lists, st, stop, sizes = check_sets(hv, g70k, "out3", mode, which)
    assert sizes.tolist() == PINNED["out3"][mode] and st.tolist() == [hv.OK] * B   # the sizes are the unmasked ones
    if which == "nothing":
        assert all(x.size == 0 for x in lists)


# ---- 4. a reach set that outgrows its slot
def test_overflow_marks_the_query_and_spares_the_others(hv, g70k):
    for _ in range(2):
        lists, st, stop, sizes = check_sets(hv, g70k, "out3", "all", mf=OVERFLOW_MF)
        assert sizes[5].tolist() == [1001, 0, 0] and sizes[11].tolist() == [998, 1001, 0] and sizes[4].tolist() == [13, 20, 41]
        assert [int(s != hv.OK) for s in st] == [0] * 5 + [1] * 3 + [0] * 3 + [1] and lists[4].size == 41
    for mode in ("before", "after"):
        check_sets(hv, g70k, "out3", mode, mf=OVERFLOW_MF)
    # the 25 000-arc row against the table's 4 096-slot floor
    seeds, direction, allowed, times, mf = HUB
    _, off, tgt, lab = fx.prefilter_graph("g70k")
    for emit in (BEFORE, AFTER, ALL):
        out = g70k.expand_repeat_lists(seeds, times, emit, direction, allowed, max_frontier=mf)
        check_lists(hv, *out, [repeat_union(off, tgt, lab, seeds[0], direction, allowed, times, emit)], mf, None, ("hub", emit))
        assert out[1].tolist() == [hv.ERR_CANDIDATE_LIMIT] and out[3].tolist() == [[9, 0]]
    # nothing lands outside the b x max_frontier ids of the output, and an overflowed neighbour leaves a request's slot alone
    seeds = REPEAT_BATCHES["out3"][0]
    s = np.ascontiguousarray(np.concatenate([np.asarray(x, np.uint64) for x in seeds]))
    soff = np.zeros(B + 1, np.uint64)
    soff[1:] = np.cumsum([len(x) for x in seeds])
    sentinel = np.uint64(0xDEADBEEFDEADBEEF)
    ids = np.full(B * OVERFLOW_MF + 4096, sentinel, np.uint64)
    lens = np.zeros(B, np.uint32); st = np.zeros(B, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert hv.lib().hvx_expand_repeat_lists(g70k._h, B, ptr(s), ptr(soff), 3, ALL, OUT, None, 0, None, None, OVERFLOW_MF, ptr(ids), ptr(lens), ptr(st),
                                            None, None) == hv.OK
    assert (ids[B * OVERFLOW_MF:] == sentinel).all()
    for q, t in enumerate(repeat_twin("out3", "all")):
        emitted, _, _, over = reported(t, OVERFLOW_MF)
        assert lens[q] == emitted.size and st[q] == (hv.ERR_CANDIDATE_LIMIT if over else hv.OK)
        assert sorted(ids[q * OVERFLOW_MF: q * OVERFLOW_MF + lens[q]].tolist()) == emitted.tolist(), q


# ---- 5. the fused call against the oracle
def check_fused(orc, hv, images, g, name, mode, image, k, which, mf=None, q=None):
    """every query's row == the oracle's exact scan over the twin's masked emitted set of THAT query; candidates, sizes, stop depths and
    statuses the twin's"""
    seeds, direction, allowed, times, mf0 = REPEAT_BATCHES[name]
    mf = mf0 if mf is None else mf
    oix, gix, image_ids = images.by_name[image]
    keep = keep_of(g.n, which)
    ids, sc, cnt, st, ncand, _, stop, sizes = gix.prefilter_repeat_search_lists(
        g, images.q if q is None else q, hv.SearchParams(k), seeds, times, MODES[mode], direction, allowed,
        node_mask=None if keep is None else mask_words(g.n, keep), max_frontier=mf, want_sizes=True)
    assert gix.last_scan_path() == hv.PATH_DIRECT
    for qi, t in enumerate(repeat_twin(name, mode)):
        emitted, want_sizes, want_stop, over = reported(t, mf)
        cand = masked(emitted, keep)
        assert sizes[qi].tolist() == want_sizes and stop[qi] == want_stop and ncand[qi] == cand.size, (name, mode, image, k, which, qi)
        if q is not None and not np.isfinite(q[qi]).all():
            continue   # (the caller checks these rows)
        assert st[qi] == (hv.ERR_CANDIDATE_LIMIT if over else hv.OK), (name, mode, image, k, which, qi)
        assert cnt[qi] == min(k, int(np.isin(cand, image_ids).sum())), (name, mode, image, k, which, qi)
        want = images.oracle(orc, image, qi, ("repeat", name, mode, which, mf), cand, k)
        assert ids[qi, :cnt[qi]].tolist() == want[0] and bits(sc[qi, :cnt[qi]]).tolist() == want[1], (name, mode, image, k, which, qi)
    return cnt, st, ncand


@pytest.mark.parametrize("which", ["none", "thirds"])
@pytest.mark.parametrize("k", [10, 100])   # 100: above the live rows of the small requests' sets
@pytest.mark.parametrize("image", ["third", "contiguous"])
def test_fused_call_against_the_oracle(orc, hv, g70k, images, image, k, which):
    check_fused(orc, hv, images, g70k, "out3", "all", image, k, which)


@pytest.mark.parametrize("name,mode,image,k,which", [("out3", "before", "third", 10, "none"), ("out3", "after", "contiguous", 100, "thirds"),
                                                     ("both2", "after", "third", 100, "none"), ("in2", "before", "contiguous", 10, "thirds"),
                                                     ("both2", "all", "contiguous", 10, "nothing")])
def test_fused_call_in_the_other_modes(orc, hv, g70k, images, name, mode, image, k, which):
    check_fused(orc, hv, images, g70k, name, mode, image, k, which)


def test_fused_call_statuses(orc, hv, g70k, images):
    q = images.q.copy()
    q[5, 0] = np.nan    # overflows at max_frontier 1 000: the candidate limit wins whatever the vector
    q[0, 3] = np.nan    # no seeds, an empty set: nothing, HVX_OK, before the vector is looked at
    q[8, 1] = np.inf    # candidates and a vector that is not finite: its validation status
    cnt, st, ncand = check_fused(orc, hv, images, g70k, "out3", "all", "third", 10, "none", mf=OVERFLOW_MF, q=q)
    assert st[5] == hv.ERR_CANDIDATE_LIMIT and cnt[5] == 0 and ncand[5] == 0
    assert st[0] == hv.OK and cnt[0] == 0 and ncand[0] == 0
    assert st[8] == hv.ERR_NONFINITE and cnt[8] == 0 and ncand[8] == 256
    assert st[11] == hv.ERR_CANDIDATE_LIMIT and cnt[11] == 0 and st[4] == hv.OK and cnt[4] > 0
    # an empty MASKED set answers nothing as well
    cnt, st, ncand = check_fused(orc, hv, images, g70k, "out3", "all", "third", 10, "nothing", q=q)
    assert st.tolist() == [hv.OK] * B and cnt.tolist() == [0] * B
    check_fused(orc, hv, images, g70k, "out3", "all", "third", 10, "none")   # the scratch is clean


# ---- 6. against the device's own other routes
def test_all_equals_the_traversal_and_one_iteration_the_chain(hv, g70k):
    for seeds, direction, allowed, times in (([1020], OUT, (), 3), (list(range(1000, 1064)), OUT, (), 2), ([8191, 300], BOTH, (1,), 2)):
        lists, st, stop, _ = g70k.expand_repeat_lists([seeds], times, ALL, direction, allowed, max_frontier=16384)
        words, _ = g70k.traverse(seeds, max_depth=times, direction=direction, allowed_labels=allowed, include_seeds=True)
        reached = np.flatnonzero(np.unpackbits(words.view(np.uint8), bitorder="little")[: g70k.n])
        assert st.tolist() == [hv.OK] and reached.size > len(seeds) and sorted(lists[0].tolist()) == reached.tolist(), (seeds, direction, times)
    seeds = REPEAT_BATCHES["out3"][0]
    for direction, allowed in ((OUT, ()), (BOTH, (1,))):
        lists, st, _, sizes = g70k.expand_repeat_lists(seeds, 1, AFTER, direction, allowed, max_frontier=4096)
        chain, cst, csizes = g70k.expand_path_lists(seeds, [(direction, allowed)], 4096)
        assert st.tolist() == cst.tolist() and sizes.tolist() == csizes.tolist()
        assert [sorted(x.tolist()) for x in lists] == [sorted(x.tolist()) for x in chain]


# ---- 7. more requests than compute units
def test_more_requests_than_compute_units(hv, g70k):
    _, off, tgt, lab = fx.prefilter_graph("g70k")
    seeds = [[1000 + i] for i in range(300)]
    out = g70k.expand_repeat_lists(seeds, 2, AFTER, OUT, (), max_frontier=4096)
    check_lists(hv, *out, [repeat_union(off, tgt, lab, s, OUT, (), 2, AFTER) for s in seeds], 4096, None, "many")
    assert out[1].tolist() == [hv.OK] * 300


# ---- 8. what is refused, before anything runs
SENTINEL32, SENTINEL64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5


def raw_repeat_calls(hv, g, gix, q, seeds, soff, times=2, emit=ALL, direction=OUT, labs=(), mf=64, k=10, ef=10, strategy=None, budgets=0, null=None):
    """both entry points through the C ABI with the arrays as given: (status of hvx_expand_repeat_lists, status of the fused call, whether
    the output arrays of the first / of the second still hold what they held)"""
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    s = np.ascontiguousarray(seeds if len(seeds) else [0], np.uint64)
    soff = np.ascontiguousarray(soff, np.uint64)
    b = soff.size - 1
    labs = np.ascontiguousarray(labs, np.uint32)
    n_labels = labs.size
    if null == "labels":
        labs, n_labels = None, 2
    outs = [np.full((b, max(mf, 1)), SENTINEL64, np.uint64)] + [np.full(b, SENTINEL32, np.uint32) for _ in range(3)] + [np.full((b, 16), SENTINEL64, np.uint64)]
    ids, lens, st, stop, sizes = outs
    rc0 = hv.lib().hvx_expand_repeat_lists(g._h, b, None if null == "seeds" else ptr(s), None if null == "offsets" else ptr(soff), times, emit, direction,
                                           ptr(labs), n_labels, None, None, mf, None if null == "ids" else ptr(ids), ptr(lens),
                                           None if null == "status" else ptr(st), ptr(stop), ptr(sizes))
    rp = hv.RestrictedParams(k=k, ef=ef, strategy=hv.RESTRICTED_EXACT if strategy is None else strategy)
    rp.explicit_budgets = budgets
    kk = max(k, 1)
    outs1 = [np.full((b, kk), SENTINEL64, np.uint64), np.full((b, kk), SENTINEL32, np.uint32), np.full(b, SENTINEL32, np.uint32),
             np.full(b, SENTINEL32, np.uint32), np.full(b, SENTINEL64, np.uint64), np.full(b, SENTINEL32, np.uint32), np.full((b, 16), SENTINEL64, np.uint64)]
    oid, osc, cnt, st1, ncand, stop1, sizes1 = outs1
    rc1 = hv.lib().hvx_prefilter_repeat_search_lists_params(gix._h, g._h, ptr(q[:b]), b, C.byref(rp), None if null == "seeds" else ptr(s),
                                                            None if null == "offsets" else ptr(soff), times, emit, direction, ptr(labs), n_labels, None,
                                                            None, mf, None if null == "ids" else ptr(oid), ptr(osc), ptr(cnt),
                                                            None if null == "status" else ptr(st1), ptr(ncand), ptr(stop1), ptr(sizes1), None)
    kept = lambda arrays: all(bool((a == (SENTINEL64 if a.dtype == np.uint64 else SENTINEL32)).all()) for a in arrays)
    return rc0, rc1, kept(outs), kept(outs1)


GOOD = dict(seeds=[1000, 1001, 1020], soff=[0, 2, 3])
# name -> (what differs from GOOD, status, whether both calls refuse it; False = the rule is the fused call's alone)
REFUSED = {
    "null_offsets": (dict(null="offsets"), "ERR_INVARIANT", True),
    "null_seeds": (dict(null="seeds"), "ERR_INVARIANT", True),
    "null_ids": (dict(null="ids"), "ERR_INVARIANT", True),
    "null_status": (dict(null="status"), "ERR_INVARIANT", True),
    "null_labels": (dict(null="labels"), "ERR_INVARIANT", True),
    "no_times": (dict(times=0), "ERR_INVARIANT", True),
    "seventeen_times": (dict(times=17), "ERR_INVARIANT", True),
    "emit_none": (dict(emit=0), "ERR_INVARIANT", True),
    "emit_four": (dict(emit=4), "ERR_INVARIANT", True),
    "bad_direction": (dict(direction=3), "ERR_INVARIANT", True),
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


def test_refused_calls_leave_nothing_behind(orc, hv, g70k, images):
    _, gix, _ = images.by_name["third"]
    q = np.tile(images.q, (2, 1))
    good0, good1, kept0, kept1 = raw_repeat_calls(hv, g70k, gix, q, **GOOD)
    assert good0 == good1 == hv.OK and not kept0 and not kept1
    for name, (change, status, both) in REFUSED.items():
        kw = dict(GOOD, **change)
        if isinstance(kw.get("strategy"), str):
            kw["strategy"] = getattr(hv, kw["strategy"])
        rc0, rc1, kept0, kept1 = raw_repeat_calls(hv, g70k, gix, q, **kw)
        assert rc1 == getattr(hv, status) and rc0 == (rc1 if both else hv.OK), name
        assert kept1 and kept0 == both, name   # a refused call wrote nothing (a rule of the fused call alone: the other call ran)
    check_fused(orc, hv, images, g70k, "both2", "all", "third", 10, "none")
    check_sets(hv, g70k, "in2", "before")


def test_images_and_batches_the_calls_do_not_serve(hv, g70k):
    rng = np.random.default_rng(69)
    n = 1000
    f8 = hv.ValidatedVectorReadIndex.managed(dim=128, metric=hv.EUCLIDEAN, node_ids=np.arange(n, dtype=np.uint64) + 5000,
                                             vectors=rng.standard_normal((n, 128)).astype(np.float32), dtype=hv.FP8_E4M3,
                                             l0_offsets=np.zeros(n + 1, np.uint64), l0_neighbors=np.zeros(0, np.uint64), max_batch=16)
    try:
        with pytest.raises(hv.HelixDbError) as e:
            f8.prefilter_repeat_search_lists(g70k, rng.standard_normal((2, 128)).astype(np.float32), hv.SearchParams(10), [[1000], [1020]], 2, ALL,
                                             max_frontier=64)
        assert e.value.status == hv.ERR_UNSUPPORTED
    finally:
        f8.close()
    # more than 65 535 requests (none of them has a seed: the rule comes before the seeds are looked at)
    with pytest.raises(hv.HelixDbError) as e:
        g70k.expand_repeat_lists([[]] * 65536, 1, ALL, max_frontier=16)
    assert e.value.status == hv.ERR_UNSUPPORTED


def test_an_auto_plan_that_is_not_exact_for_the_slot_is_refused(orc, hv, g70k, images):
    _, gix, _ = images.by_name["third"]
    seeds, direction, allowed, times, _ = REPEAT_BATCHES["both2"]
    auto = hv.RestrictedParams.auto(10, 10)
    gix.set_option(hv.OPT_RESTRICTED_EXACT_MIB, 1)   # the device plan scans exactly up to 1 MiB of rows: 4 096 ids of 64 f32
    try:
        with pytest.raises(hv.HelixDbError) as e:
            gix.prefilter_repeat_search_lists(g70k, images.q, auto, seeds, times, ALL, direction, allowed, max_frontier=4097)
        assert e.value.status == hv.ERR_UNSUPPORTED
        out = gix.prefilter_repeat_search_lists(g70k, images.q, auto, seeds, times, ALL, direction, allowed, max_frontier=4096)
        assert out[3].tolist() == [hv.OK] * B and out[4].tolist() == [r[-1] for r in PINNED["both2"]["all"]]
    finally:
        gix.set_option(hv.OPT_RESTRICTED_EXACT_MIB, 0)
    check_fused(orc, hv, images, g70k, "both2", "all", "third", 10, "none")


# ---- 9. the chain route shares the handle's scratch and answers as before
def test_the_chain_route_is_unchanged_behind_a_repeat_call(hv, g70k):
    check_sets(hv, g70k, "out3", "all")
    check_chain_sets(hv, g70k, "plain")
    check_sets(hv, g70k, "both2", "before")
    check_chain_sets(hv, g70k, "labelled")
