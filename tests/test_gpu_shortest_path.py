"""shortest_path for batches of requests on the device (hvx_shortest_path_batch): one launch, one workgroup per request, levels from the
target over the reversed arcs and then the smallest neighbour one level closer, step by step from the source.  Every comparison is of
paths, lengths, statuses and reach sizes against the literal twin of the reference's loop (tests/shortest_path_twin.py); the g20k batches
are the ones tests/test_shortest_path_host.py pins as numbers."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
import shortest_path_cases as sc
import shortest_path_twin as twin

pytestmark = pytest.mark.gpu
OUT, IN, BOTH = sc.OUT, sc.IN, sc.BOTH


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


@pytest.fixture(scope="module")
def t70k():
    return twin.Graph(*fx.prefilter_graph("g70k"))


def same(got, want, tag=None):
    """one call's (paths, statuses, sizes) against the twin's"""
    paths, st, sizes = got
    wpaths, wst, wsizes = want
    assert len(paths) == len(wpaths), tag
    for q, (p, w) in enumerate(zip(paths, wpaths)):
        assert p.dtype == np.uint64 and p.tolist() == list(w), (tag, q)
    assert st.tolist() == wst.tolist(), tag
    assert sizes.shape == wsizes.shape and sizes.tolist() == wsizes.tolist(), tag


def check(g, t, src, dst, max_depth, direction=OUT, allowed=(), max_reach=16384, tag=None):
    got = g.shortest_paths(src, dst, max_depth, direction, allowed, max_reach)
    want = twin.answers(t, src, dst, max_depth, direction, allowed, max_reach)
    same(got, want, tag)
    return want


def test_hand_graph_every_case_batched_by_plan(hv):
    t = sc.hand_graph()
    g = hv.Graph(*t.arrays())
    try:
        for (max_depth, direction, allowed), cases in sc.HAND_CASES.items():
            for _ in range(2):   # the first call leaves table, list and level bytes dirty
                paths, st, _ = g.shortest_paths([s for s, _, _ in cases], [d for _, d, _ in cases], max_depth, direction, allowed, max_reach=8)
                assert st.tolist() == [hv.OK] * len(cases)
                assert [p.tolist() for p in paths] == [w for _, _, w in cases], (max_depth, direction, allowed)
            check(g, t, [s for s, _, _ in cases], [d for _, d, _ in cases], max_depth, direction, allowed, 8)
        # the overflow rule on the graph whose levels are written out in the host file
        for max_reach in (3, 7, 8):
            check(g, t, [0, 6, 0], [6, 0, 6], 5, OUT, (), max_reach, max_reach)
    finally:
        g.close()


@pytest.mark.parametrize("max_depth, nodes", [(254, 255), (255, 255), (253, 0)])
def test_chain_end_to_end(hv, max_depth, nodes):
    """one-node levels, the level byte's whole range, two barriers a level"""
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
def test_pinned_g20k_batches(hv, g20k, name):
    src, dst, max_depth, direction, allowed, max_reach, want = sc.g20k_batch(name)
    same(g20k.shortest_paths(src, dst, max_depth, direction, allowed, max_reach), want, name)


def test_long_rows_on_g20k(hv, g20k):
    t = sc.g20k()
    n = t.n
    assert t.in_off[778] - t.in_off[777] >= 201 and t.out_off[12346] - t.out_off[12345] == 1000 and t.out_off[6] - t.out_off[5] == 300
    rng = np.random.default_rng(3)
    # the 201-arc incoming row in the first backward level
    paths, _, _ = check(g20k, t, rng.integers(0, n, 24), np.full(24, 777), 8, tag="sink")
    assert sum(1 for p in paths if len(p)) >= 4
    # the hubs' forward rows (983 and 299 distinct targets) walked by Phase B's first step
    src = np.array([12345, 5] * 12)
    paths, _, _ = check(g20k, t, src, rng.integers(0, n, 24), 8, tag="hubs")
    assert {p[0] for p in paths if len(p)} == {12345, 5}
    off, nbr = t.plan(OUT)
    assert off[12346] - off[12345] == 983 and off[6] - off[5] == 299


def test_row_length_group_on_g70k(hv, g70k, t70k):
    """direction In: Phase A walks the OUTGOING rows of 0, 1, 16, 17, 65 and 1 000 arcs, on both sides of the light-row bound and of one
    wavefront step; a source two arcs down every row, one further down, and a random one"""
    t = t70k
    targets = [u for u, _ in fx.G70K_GROUP]
    assert [int(t.out_off[u + 1] - t.out_off[u]) for u in targets] == [0, 1, 16, 17, 65, 1000]
    rng = np.random.default_rng(5)
    src, dst = [], []
    for u in targets:
        hop1 = np.unique(t.arcs([u], OUT))
        hop2 = np.unique(t.arcs(hop1, OUT)) if hop1.size else hop1
        for s in ([int(hop1.max())] if hop1.size else []) + ([int(hop2.max())] if hop2.size else []) + [int(rng.integers(0, t.n))]:
            src.append(s)
            dst.append(u)
    paths, st, _ = check(g70k, t, src, dst, 6, IN, tag="group")
    assert sum(1 for p in paths if len(p)) >= 8 and (st == hv.ERR_CANDIDATE_LIMIT).any()   # (the random sources of the long rows overflow)
    check(g70k, t, src, dst, 6, IN, (0, 2), tag="group labelled")


def test_sentinel_endpoints_and_duplicates(hv, g20k):
    t = sc.g20k()
    src0, dst0, max_depth, direction, allowed, max_reach, (wpaths, _, _) = sc.g20k_batch("out8")
    hit = next(q for q, p in enumerate(wpaths) if len(p))
    s, d = int(src0[hit]), int(dst0[hit])
    src = np.array([s, hv.NO_NODE, s, hv.NO_NODE, s, s, d], np.uint64)
    dst = np.array([d, d, hv.NO_NODE, hv.NO_NODE, d, d, d], np.uint64)
    paths, st, sizes = check(g20k, t, src, dst, max_depth)
    assert paths[0] == paths[4] == paths[5] == wpaths[hit] and paths[1] == paths[2] == paths[3] == [] and paths[6] == [d]
    assert sizes[1].tolist() == [0] * max_depth and sizes[6].tolist() == [1] * max_depth


def test_batch_sizes_one_and_sixty_five(hv, g20k):
    t = sc.g20k()
    src, dst, max_depth, _, _, _, (wpaths, wst, wsizes) = sc.g20k_batch("out8")
    for q in (0, next(q for q, p in enumerate(wpaths) if len(p))):
        same(g20k.shortest_paths(src[q:q + 1], dst[q:q + 1], max_depth), ([wpaths[q]], wst[q:q + 1], wsizes[q:q + 1]), ("b1", q))
    src65, dst65 = np.concatenate([src, src[:1]]), np.concatenate([dst, dst[:1]])
    same(g20k.shortest_paths(src65, dst65, max_depth), (wpaths + wpaths[:1], np.concatenate([wst, wst[:1]]), np.concatenate([wsizes, wsizes[:1]])), "b65")
    assert len(g20k.shortest_paths([], [], max_depth)[0]) == 0   # b == 0


def test_overflow_leaves_its_neighbours_alone_and_runs_repeat(hv, g20k):
    src, dst, max_depth, direction, allowed, max_reach, (wpaths, wst, _) = sc.g20k_batch("out8_small")
    found = [q for q, p in enumerate(wpaths) if len(p)]
    over = next(q for q, s in enumerate(wst) if s == hv.ERR_CANDIDATE_LIMIT)
    pick = [found[0], over, found[1]]
    solo = [g20k.shortest_paths(src[q:q + 1], dst[q:q + 1], max_depth, direction, allowed, max_reach) for q in pick]
    for _ in range(2):   # the same batch twice is identical
        paths, st, sizes = g20k.shortest_paths(src[pick], dst[pick], max_depth, direction, allowed, max_reach)
        assert st.tolist() == [hv.OK, hv.ERR_CANDIDATE_LIMIT, hv.OK] and len(paths[1]) == 0
        for i, (p1, s1, z1) in enumerate(solo):
            assert paths[i].tolist() == p1[0].tolist() and st[i] == s1[0] and sizes[i].tolist() == z1[0].tolist()
        assert paths[0].tolist() == wpaths[pick[0]] and paths[2].tolist() == wpaths[pick[2]]
    a = g20k.shortest_paths(*sc.g20k_batch("both5")[:6])
    b = g20k.shortest_paths(*sc.g20k_batch("both5")[:6])
    same(a, (b[0], b[1], b[2]), "twice")


def test_answers_follow_an_edit(hv):
    n, off, tgt, lab = fx.prefilter_graph("g20k")
    src, dst, max_depth, _, _, _, (wpaths, _, _) = sc.g20k_batch("out8")
    hit = next(q for q, p in enumerate(wpaths) if len(p))
    path = wpaths[hit]
    u, v = path[2], path[3]
    # every stored copy of the arc u -> v goes; a shortcut appears elsewhere: the found path's source now reaches its target in one arc
    row = np.arange(int(off[u]), int(off[u + 1]))
    gone = row[tgt[row] == v]
    other = next(q for q, p in enumerate(wpaths) if len(p) and q != hit)
    add = (np.array([src[other]], np.uint64), np.array([dst[other]], np.uint64), np.array([1], np.uint32))
    g = hv.Graph(n, off, tgt, lab)
    try:
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
    base = dict(g=g20k._h, b=2, src=p(src), dst=p(dst), md=8, d=OUT, al=None, nl=0, mr=16384, paths=p(paths), lens=p(lens), st=p(st), sizes=p(sizes))
    call = lambda **kw: L.hvx_shortest_path_batch(*[{**base, **kw}[k] for k in ("g", "b", "src", "dst", "md", "d", "al", "nl", "mr", "paths", "lens", "st", "sizes")])
    n = g20k.n
    for bad in (dict(g=None), dict(src=None), dict(dst=None), dict(paths=None), dict(lens=None), dict(st=None), dict(d=3), dict(md=0), dict(nl=1),
                dict(src=p(np.array([1, n], np.uint64))), dict(dst=p(np.array([2 ** 40, 0], np.uint64)))):
        assert call(**bad) == hv.ERR_INVARIANT, bad
    for bad in (dict(md=256), dict(mr=0), dict(mr=16385), dict(b=65536, src=p(many), dst=p(many))):
        assert call(**bad) == hv.ERR_UNSUPPORTED, bad
    assert call(b=0, src=None, dst=None) == hv.OK
    assert call(sizes=None) == hv.OK and call(md=255) == hv.OK   # the nullable output, the largest depth
    src, dst, max_depth, direction, allowed, max_reach, want = sc.g20k_batch("labelled10")
    same(g20k.shortest_paths(src, dst, max_depth, direction, allowed, max_reach), want, "after the refusals")
