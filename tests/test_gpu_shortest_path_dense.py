"""shortest_path batches of any reach on the device (hvx_shortest_path_batch_dense): 64 requests share one bit-parallel sweep, the per-node
state lives in device memory, groups run in rounds within a scratch budget.  Every comparison is of paths, lengths, statuses and reach sizes
against the literal twin of the reference's loop without a reach limit (tests/shortest_path_twin.py, answers(max_reach=None)); the deep
batches are the ones tests/test_shortest_path_dense_host.py pins as numbers."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import shortest_path_cases as sc
import shortest_path_dense_cases as dc
import shortest_path_twin as twin

pytestmark = pytest.mark.gpu
OUT, IN, BOTH = sc.OUT, sc.IN, sc.BOTH
NODE_GROUP_BYTES = 88


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


@pytest.fixture(scope="module")
def g20k(hv):
    g = hv.Graph(*fx.prefilter_graph("g20k"))
    yield g
    g.close()


@pytest.fixture(scope="module")
def g70k(hv):
    g = hv.Graph(*fx.prefilter_graph("g70k"))
    yield g
    g.close()


def same(got, want, tag=None):
    """one call's (paths, statuses, sizes) against the twin's"""
    paths, st, sizes = got
    wpaths, wst, wsizes = want
    assert len(paths) == len(wpaths), tag
    for q, (p, w) in enumerate(zip(paths, wpaths)):
        assert p.dtype == np.uint64 and p.tolist() == list(w), (tag, q)
    assert st.tolist() == wst.tolist(), tag
    assert sizes.shape == wsizes.shape and sizes.tolist() == wsizes.tolist(), tag


def check(g, t, src, dst, max_depth, direction=OUT, allowed=(), tag=None, **kw):
    want = twin.answers(t, src, dst, max_depth, direction, allowed, max_reach=None)
    same(g.shortest_paths_dense(src, dst, max_depth, direction, allowed, **kw), want, tag)
    return want


def test_hand_graph_every_case_batched_by_plan(hv):
    t = sc.hand_graph()
    g = hv.Graph(*t.arrays())
    try:
        for (max_depth, direction, allowed), cases in sc.HAND_CASES.items():
            for _ in range(2):   # the first call leaves the words' neighbours, the level bytes, dirty
                paths, st, _ = g.shortest_paths_dense([s for s, _, _ in cases], [d for _, d, _ in cases], max_depth, direction, allowed)
                assert st.tolist() == [hv.OK] * len(cases)
                assert [p.tolist() for p in paths] == [w for _, _, w in cases], (max_depth, direction, allowed)
                check(g, t, [s for s, _, _ in cases], [d for _, d, _ in cases], max_depth, direction, allowed, (max_depth, direction, allowed))
    finally:
        g.close()


@pytest.mark.parametrize("max_depth, nodes", [(254, 255), (255, 255), (253, 0)])
def test_chain_end_to_end(hv, max_depth, nodes):
    """one-node levels, the level byte's whole range, 64 runs of levels with a host look between them"""
    n, off, tgt = fx.chain_graph(254)
    t = twin.Graph(n, off, tgt)
    g = hv.Graph(n, off, tgt)
    try:
        (paths, _, _) = check(g, t, [0, 0, 7, 254], [254, 253, 250, 0], max_depth)
        assert len(paths[0]) == nodes and (not nodes or paths[0] == list(range(255)))
        assert len(check(g, t, [254], [0], max_depth, IN)[0][0]) == nodes
    finally:
        g.close()


@pytest.mark.parametrize("name", list(sc.G20K_BATCHES))
def test_g20k_batches_without_the_reach_limit(hv, g20k, name):
    src, dst, max_depth, direction, allowed, _, _ = sc.g20k_batch(name)
    paths, st, _ = check(g20k, sc.g20k(), src, dst, max_depth, direction, allowed, name)
    assert (st == hv.OK).all() and sum(1 for p in paths if len(p)) >= 1


@pytest.mark.parametrize("name", list(dc.DEEP_BATCHES))
def test_deep_batches_the_sibling_refuses(hv, g20k, g70k, name):
    gname, src, dst, max_depth, direction, allowed, want, want16 = dc.deep_batch(name)
    g = g70k if gname == "g70k" else g20k
    # the sibling first: its refused set is the pinned one
    paths16, st16, _ = g.shortest_paths(src, dst, max_depth, direction, allowed, dc.SIBLING_REACH)
    assert st16.tolist() == want16[1].tolist()
    refused = np.flatnonzero(st16 == hv.ERR_CANDIDATE_LIMIT)
    assert refused.size >= 1
    # exactly the refused requests come here and get their paths
    paths, st, sizes = g.shortest_paths_dense(src[refused], dst[refused], max_depth, direction, allowed)
    same((paths, st, sizes), ([want[0][q] for q in refused], want[1][refused], want[2][refused]), (name, "refused"))
    assert sum(1 for p in paths if len(p)) >= 1 and int(sizes.max()) > dc.SIBLING_REACH
    # the whole batch: what the sibling answered gets the same path here
    full = g.shortest_paths_dense(src, dst, max_depth, direction, allowed)
    same(full, want, (name, "whole"))
    for q in np.flatnonzero(st16 == hv.OK):
        assert full[0][q].tolist() == paths16[q].tolist(), (name, q)


def test_group_edges(hv, g20k):
    """1, 63, 64, 65 and 130 requests; one target shared by 70 requests (two groups), one pair repeated, sentinels and source == target mixed in"""
    t = sc.g20k()
    src0, dst0, max_depth, _, _, _, (wpaths, _, _) = sc.g20k_batch("out8")
    hit = next(q for q, p in enumerate(wpaths) if len(p))
    s, d = int(src0[hit]), int(dst0[hit])
    rng = np.random.default_rng(17)
    src = rng.integers(0, t.n, 130).astype(np.uint64)
    dst = rng.integers(0, t.n, 130).astype(np.uint64)
    dst[30:100] = d                              # 70 requests of one target: bits 30 .. 63 of group 0 and 0 .. 35 of group 1
    src[60:68] = s                               # one pair repeated across the group boundary
    src[[3, 64, 129]] = hv.NO_NODE
    dst[[5, 63, 128]] = hv.NO_NODE
    src[[7, 65, 127]] = dst[[7, 65, 127]]        # source == target
    for b in (1, 63, 64, 65, 130):
        paths, _, sizes = check(g20k, t, src[:b], dst[:b], max_depth, tag=b)
        if b == 130:
            assert all(paths[q] == wpaths[hit] for q in (60, 61, 62, 66, 67)) and paths[65] == [d] and paths[3] == paths[63] == []
            assert sizes[64].tolist() == [0] * max_depth and sizes[7].tolist() == [1] * max_depth
    check(g20k, t, [s], [d], max_depth, tag="one found")
    assert len(g20k.shortest_paths_dense([], [], max_depth)[0]) == 0   # b == 0


def test_long_rows_on_g70k(hv, g70k):
    """the 25 000-arc row of node 2000 and the 200-arc incoming row of the sink 3000, in the push and in the walk out"""
    t = dc.graph("g70k")
    assert t.out_off[2001] - t.out_off[2000] == 25000 and t.in_off[3001] - t.in_off[3000] >= 200
    rng = np.random.default_rng(3)
    # sources at the long row: the walk out's first step strides over it; the targets two arcs away lie behind its row
    row = t.out_tgt[t.out_off[2000]:t.out_off[2001]]
    hop2 = np.setdiff1d(t.arcs(row[:50], OUT), row)
    dst = np.concatenate([rng.choice(row, 8), rng.choice(hop2, 8), rng.integers(0, t.n, 8)]).astype(np.uint64)
    paths, _, _ = check(g70k, t, np.full(24, 2000), dst, 6, tag="from the hub")
    assert sum(1 for p in paths if len(p) == 2) >= 8 and sum(1 for p in paths if len(p) == 3) >= 8
    # direction In mirrors it: the push walks the 25 000 arcs from the target in the first level
    paths, _, _ = check(g70k, t, dst, np.full(24, 2000), 6, IN, tag="into the hub")
    assert sum(1 for p in paths if len(p)) >= 16
    # both directions, labels: the long row is walked in either role
    check(g70k, t, np.full(24, 2000), dst, 4, BOTH, (0, 2), tag="hub both labelled")
    # through the sink: its incoming row is the first backward level
    paths, _, _ = check(g70k, t, rng.integers(0, t.n, 24), np.full(24, 3000), 8, tag="sink")
    assert sum(1 for p in paths if len(p)) >= 4
    back = np.unique(t.arcs([3000], IN))
    paths, _, _ = check(g70k, t, rng.choice(back, 8), rng.integers(0, t.n, 8), 8, tag="from the sink's sources")


def test_rounds_within_a_budget(hv, g20k):
    t = sc.g20k()
    rng = np.random.default_rng(23)
    src, dst = rng.integers(0, t.n, 130).astype(np.uint64), rng.integers(0, t.n, 130).astype(np.uint64)
    one_group = t.n * NODE_GROUP_BYTES
    want = check(g20k, t, src, dst, 8, tag="default budget")
    assert sum(1 for p in want[0] if len(p)) >= 8
    same(g20k.shortest_paths_dense(src, dst, 8, scratch_bytes=one_group), want, "three rounds")
    same(g20k.shortest_paths_dense(src, dst, 8, scratch_bytes=2 * one_group + 7), want, "two rounds")
    with pytest.raises(hv.HelixDbError) as err:
        g20k.shortest_paths_dense(src, dst, 8, scratch_bytes=one_group - 1)
    assert err.value.status == hv.ERR_UNSUPPORTED
    same(g20k.shortest_paths_dense(src, dst, 8, scratch_bytes=one_group), want, "after the refusal")


def test_without_sizes(hv, g20k):
    src, dst, max_depth, direction, allowed, _, _ = sc.g20k_batch("both5")
    want = twin.answers(sc.g20k(), src, dst, max_depth, direction, allowed, max_reach=None)
    paths, st, sizes = g20k.shortest_paths_dense(src, dst, max_depth, direction, allowed, sizes=False)
    assert sizes is None and st.tolist() == want[1].tolist()
    assert [p.tolist() for p in paths] == want[0] and sum(1 for p in paths if len(p)) >= 8


def test_answers_follow_an_edit(hv):
    n, off, tgt, lab = fx.prefilter_graph("g20k")
    src, dst, max_depth, _, _, _, (wpaths, _, _) = sc.g20k_batch("out8")
    hit = next(q for q, p in enumerate(wpaths) if len(p))
    path = wpaths[hit]
    u, v = path[2], path[3]
    # every stored copy of the arc u -> v goes (the path is cut there); a shortcut appears elsewhere (another path shortens to one arc)
    row = np.arange(int(off[u]), int(off[u + 1]))
    gone = row[tgt[row] == v]
    other = next(q for q, p in enumerate(wpaths) if len(p) and q != hit)
    add = (np.array([src[other]], np.uint64), np.array([dst[other]], np.uint64), np.array([1], np.uint32))
    g = hv.Graph(n, off, tgt, lab)
    try:
        same(g.shortest_paths_dense(src, dst, max_depth), twin.answers(sc.g20k(), src, dst, max_depth, max_reach=None), "before")
        g.apply_edges(remove=(np.full(gone.size, u, np.uint64), np.full(gone.size, v, np.uint64), lab[gone]), add=add)
        owner = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
        keep = np.ones(tgt.size, bool)
        keep[gone] = False
        edited = twin.Graph.from_edges(n, np.concatenate([owner[keep], add[0].astype(np.int64)]), np.concatenate([tgt[keep].astype(np.int64), add[1].astype(np.int64)]),
                                       np.concatenate([lab[keep], add[2]]))
        paths, _, _ = check(g, edited, src, dst, max_depth, tag="edited")
        assert paths[other] == [int(src[other]), int(dst[other])] and paths[hit] != path
        check(g, edited, src, dst, 5, BOTH, (0, 1), tag="edited both")
    finally:
        g.close()


def test_every_refusal_and_a_good_batch_afterwards(hv, g20k):
    L = hv.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    src, dst = np.array([1, 2], np.uint64), np.array([3, 4], np.uint64)
    paths, lens, st, sizes = np.zeros((2, 300), np.uint64), np.zeros(2, np.uint32), np.zeros(2, np.uint32), np.zeros(2 * 300, np.uint64)
    many = np.zeros(65536, np.uint64)
    base = dict(g=g20k._h, b=2, src=p(src), dst=p(dst), md=8, d=OUT, al=None, nl=0, sb=0, paths=p(paths), lens=p(lens), st=p(st), sizes=p(sizes))
    call = lambda **kw: L.hvx_shortest_path_batch_dense(*[{**base, **kw}[k] for k in ("g", "b", "src", "dst", "md", "d", "al", "nl", "sb", "paths", "lens", "st", "sizes")])
    n = g20k.n
    for bad in (dict(g=None), dict(src=None), dict(dst=None), dict(paths=None), dict(lens=None), dict(st=None), dict(d=3), dict(md=0), dict(nl=1),
                dict(src=p(np.array([1, n], np.uint64))), dict(dst=p(np.array([2 ** 40, 0], np.uint64)))):
        assert call(**bad) == hv.ERR_INVARIANT, bad
    for bad in (dict(md=256), dict(sb=n * NODE_GROUP_BYTES - 1), dict(sb=1), dict(b=65536, src=p(many), dst=p(many))):
        assert call(**bad) == hv.ERR_UNSUPPORTED, bad
    assert call(b=0, src=None, dst=None) == hv.OK
    assert call(sizes=None) == hv.OK and call(md=255) == hv.OK and call(sb=n * NODE_GROUP_BYTES) == hv.OK   # nullable output, largest depth, smallest budget
    src, dst, max_depth, direction, allowed, _, _ = sc.g20k_batch("labelled10")
    check(g20k, sc.g20k(), src, dst, max_depth, direction, allowed, "after the refusals")
