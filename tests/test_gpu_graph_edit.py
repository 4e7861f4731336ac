"""hvx_csr_apply_edges on the device.  The reference in every case is a fresh hv.Graph import of the arrays the numpy twin
(tests/graph_edit_twin.py) derives: after a batch the handle must be indistinguishable from it."""
import numpy as np
import pytest

import fixtures as fx
import graph_edit_twin as twin

pytestmark = pytest.mark.gpu

# hvx_csr_edit.hip: the copy kernel's grid is at most kCopyBlocks = 2048 workgroups of 4 wavefronts, each moving kCopyUnroll x 64 = 128 arcs
# per step, so one pass of the grid covers 1 048 576 arcs; a graph above twice that makes its wavefronts stride
COPY_ARCS_PER_PASS = 2048 * 4 * 2 * 64


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def fresh(hv, n, arrays):
    return hv.Graph(n, *arrays)


def hold_to_fresh_import(hv, g, n, arrays):
    """export() and sizes() of the edited handle == the twin's arrays == a fresh import's export() and sizes()"""
    want = twin.import_arrays(n, *arrays)
    got = g.export()
    assert twin.same_arrays(got, want)
    ref = fresh(hv, n, arrays)
    try:
        assert twin.same_arrays(ref.export(), got)
        assert g.sizes() == ref.sizes() == twin.sizes(n, arrays[0], arrays[1])
    finally:
        ref.close()


# ---- 1. the eight-node graph
@pytest.mark.parametrize("case", sorted(twin.EIGHT_CASES))
def test_eight_node_graph(hv, case):
    n, off, tgt, lab = twin.eight_graph()
    remove, add, arcs = twin.EIGHT_CASES[case]
    g = hv.Graph(n, off, tgt, lab)
    try:
        g.apply_edges(remove=twin.triples(remove), add=twin.triples(add))
        got = g.export()
        src = np.repeat(np.arange(n), np.diff(got["out_offsets"].astype(np.int64)))
        assert list(zip(src.tolist(), got["out_targets"].tolist(), got["out_labels"].tolist())) == arcs  # the literals
        hold_to_fresh_import(hv, g, n, twin.apply_edges(n, off, tgt, lab, twin.triples(remove), twin.triples(add)))
    finally:
        g.close()


def test_eight_node_graph_all_seven_arrays_as_literals(hv):
    n, off, tgt, lab = twin.eight_graph()
    g = hv.Graph(n, off, tgt, lab)
    try:
        g.apply_edges(remove=twin.triples([(3, 4, 3)]))
        a = g.export()
        assert a["out_offsets"].tolist() == [0, 2, 2, 4, 7, 8, 9, 9, 11]
        assert a["out_targets"].tolist() == [1, 4, 2, 5, 4, 4, 6, 0, 7, 0, 7]
        assert a["out_labels"].tolist() == [1, 2, 7, 1, 3, 5, 2, 9, 4, 6, 8]
        assert a["in_offsets"].tolist() == [0, 2, 3, 4, 4, 7, 8, 9, 11]
        assert a["in_sources"].tolist() == [4, 7, 0, 2, 0, 3, 3, 2, 3, 5, 7]
        assert a["in_edge_index"].tolist() == [7, 9, 0, 2, 1, 4, 5, 3, 6, 8, 10]
        assert a["in_labels"].tolist() == [9, 6, 1, 7, 2, 3, 5, 1, 2, 4, 8]
        assert g.sizes() == dict(n_nodes=8, n_edges=11, max_out_degree=3, max_in_degree=3, rows_sorted=True)
    finally:
        g.close()


# ---- 2. g20k, one seeded batch, every family of calls
def families(hv, g, facts, n):
    hub, sink, many, filled, emptied = facts["hub"], facts["sink"], facts["many"], facts["filled"], facts["emptied"]
    seeds = np.array([hub, 0, filled, n - 1, emptied, many], np.uint64)
    per_query = [[hub], [0, n - 1], [filled, emptied], [many], [sink, 5], [facts["parallel"][0]], [4], [many, hub]]
    hops = [(hv.DIR_OUT, ()), (hv.DIR_BOTH, (1, 2))]
    out = {}
    words, depth = g.traverse(seeds, 3, direction=hv.DIR_BOTH, allowed_labels=(1, 2), hub_degree=100)
    out["traverse"] = (words.tolist(), depth.tolist())
    out["ordered"] = g.traverse_ordered(seeds, 3, direction=hv.DIR_BOTH, allowed_labels=(1, 2), hub_degree=100)
    out["ordered_in"] = g.traverse_ordered(np.array([sink, many], np.uint64), 2, direction=hv.DIR_IN)
    out["dfs"] = g.traverse_depth_first(seeds, 3, direction=hv.DIR_BOTH, allowed_labels=(1, 2), hub_degree=100)
    out["expand"] = g.expand(seeds, direction=hv.DIR_BOTH, allowed_labels=(0, 2)).tolist()
    words, sizes = g.expand_path(seeds, hops, want_sizes=True)
    out["path"] = (words.tolist(), sizes)
    lists, st, sizes = g.expand_path_lists(per_query, hops, 4096)
    out["path_lists"] = ([sorted(l.tolist()) for l in lists], st.tolist(), sizes.tolist())
    lists, st, stop, sizes = g.expand_repeat_lists(per_query, 2, hv.REPEAT_EMIT_ALL, direction=hv.DIR_OUT, max_frontier=4096)
    out["repeat_lists"] = ([sorted(l.tolist()) for l in lists], st.tolist(), stop.tolist(), sizes.tolist())
    return out


def test_g20k_seeded_batch_every_family(hv):
    n, off, tgt, lab = fx.prefilter_graph("g20k")
    remove, add, facts = twin.g20k_batch(n, off, tgt, lab)
    g = hv.Graph(n, off, tgt, lab)
    ref = None
    try:
        # the edge-sized scratch of the ordered traversal and the host mirror of the depth-first one exist at the OLD size
        g.traverse_ordered(np.array([facts["hub"]], np.uint64), 2)
        g.traverse_depth_first(np.array([facts["hub"]], np.uint64), 2)
        g.apply_edges(remove=remove, add=add)
        new = twin.apply_edges(n, off, tgt, lab, remove, add)
        assert new[1].size == tgt.size - remove[0].size + add[0].size
        assert new[0][facts["emptied"] + 1] == new[0][facts["emptied"]] and new[0][facts["filled"] + 1] - new[0][facts["filled"]] == 3
        hold_to_fresh_import(hv, g, n, new)
        ref = fresh(hv, n, new)
        got, want = families(hv, g, facts, n), families(hv, ref, facts, n)
        for name in want:
            assert got[name] == want[name], name
    finally:
        g.close()
        if ref is not None:
            ref.close()


# ---- 3. five successive batches on one handle
def test_five_successive_batches(hv):
    n, off, tgt, lab = fx.prefilter_graph("g20k")
    rng = np.random.default_rng(5)
    g = hv.Graph(n, off, tgt, lab)
    cur = (off, tgt, lab)
    try:
        g.traverse_ordered(np.array([5], np.uint64), 2)  # scratch at the imported size
        def rand_adds(count, rows=None):
            s = rng.integers(0, n, count) if rows is None else rng.choice(rows, count)
            return (s.astype(np.uint64), rng.integers(0, n, count).astype(np.uint64), rng.integers(0, 3, count).astype(np.uint32))
        def stored(count, arrays, rows=None):
            o = arrays[0].astype(np.int64)
            src = np.repeat(np.arange(n), np.diff(o))
            pool = np.arange(arrays[1].size) if rows is None else np.nonzero(np.isin(src, rows))[0]
            pos = rng.choice(pool, count, replace=False)
            return (src[pos].astype(np.uint64), arrays[1][pos], arrays[2][pos])
        e0 = tgt.size
        big = rand_adds(e0 + 5000)                                 # 3: at least doubles e (the spare set and the scratch regrow)
        hub_adds = rand_adds(3000, rows=[4242])                    # 2: node 4242 becomes the largest row ...
        batches = [(stored(200, cur), rand_adds(300)), (None, hub_adds), (None, big), None, None]
        for i in range(5):
            if i == 3:   # 4: ... and shrinks again below hub 12345: the maxima are exact, not bounds
                remove = stored(2900, cur, rows=[4242])
                batch = (remove, rand_adds(10))
            elif i == 4:  # 5: most of what batch 3 added goes
                keep = (rng.random(big[0].size) < 0.1) | (big[0] == 4242)  # (batch 4 drew its removals from row 4242)
                batch = ((big[0][~keep], big[1][~keep], big[2][~keep]), None)
            else:
                batch = batches[i]
            before = g.sizes()
            g.apply_edges(remove=batch[0], add=batch[1])
            cur = twin.apply_edges(n, *cur, remove=batch[0], add=batch[1])
            hold_to_fresh_import(hv, g, n, cur)
            if i == 1:
                assert g.sizes()["max_out_degree"] > 3000
            if i == 2:
                assert g.sizes()["n_edges"] >= 2 * before["n_edges"]
            if i == 3:
                assert g.sizes()["max_out_degree"] < 1100 and before["max_out_degree"] > 3000  # hub 12345 leads again
        visits, edges = g.traverse_ordered(np.array([5, 4242], np.uint64), 2)  # reads in_edge_index and the regrown scratch
        ref = fresh(hv, n, cur)
        try:
            assert (visits, edges) == ref.traverse_ordered(np.array([5, 4242], np.uint64), 2)
        finally:
            ref.close()
    finally:
        g.close()


# ---- 4. the copy kernel at its seams
@pytest.fixture(scope="module")
def wide70k():
    """g70k's shape (its hubs, spelled-out rows and sink) with rows of 0 .. 64 arcs: 2.2 M arcs, so the copy kernel's wavefronts stride
    at least twice (more than 2 x COPY_ARCS_PER_PASS arcs)"""
    n = 70001
    off, tgt, lab = fx.csr_graph(n, seed=70002, avg_row=32, hubs=fx.G70K_GROUP, rows=fx._g70k_rows(), sinks=((3000, 200),), n_labels=3)
    assert tgt.size > 2 * COPY_ARCS_PER_PASS
    return n, off, tgt, lab


def seam_batches(n, off, tgt, lab):
    o = off.astype(np.int64)
    ends = (np.array([0, n - 1, n - 1], np.uint64), np.array([5, 0, n - 1], np.uint64), np.array([1, 2, 0], np.uint32))
    rows = np.arange(96, n, 97)
    rows = rows[np.diff(o)[rows] > 0]
    first = o[rows]
    every97 = ((rows.astype(np.uint64), tgt[first], None if lab is None else lab[first]),
               (rows[::2].astype(np.uint64), (rows[::2] % 1000).astype(np.uint64), None if lab is None else (rows[::2] % 3).astype(np.uint32)))
    return {"ends": (None, ends if lab is not None else ends[:2]), "every97": every97}


@pytest.mark.parametrize("which,labelled", [("ends", True), ("every97", True), ("every97", False)])
def test_copy_kernel_seams(hv, wide70k, which, labelled):
    n, off, tgt, lab = wide70k
    lab = lab if labelled else None
    remove, add = seam_batches(n, off, tgt, lab)[which]
    g = hv.Graph(n, off, tgt, lab)
    try:
        g.apply_edges(remove=remove, add=add)
        hold_to_fresh_import(hv, g, n, twin.apply_edges(n, off, tgt, lab, remove, add))
    finally:
        g.close()


# ---- 5. refusals and atomicity
def test_refusals_leave_the_handle_as_it_was(hv):
    n, off, tgt, lab = twin.eight_graph()
    g = hv.Graph(n, off, tgt, lab)
    plain = hv.Graph(n, off, tgt)
    # row 0 descends: 4 before 1
    unsorted = hv.Graph(n, off, np.array([4, 1] + tgt[2:].tolist(), np.uint64), lab)
    t = twin.triples
    try:
        before, sizes = g.export(), g.sizes()
        refused = {
            "absent": dict(remove=t([(3, 4, 4)])),
            "absent_in_empty_row": dict(remove=t([(1, 0, 0)]), add=t([(0, 0, 0)])),
            "one_too_many": dict(remove=t([(3, 4, 3), (0, 1, 1), (3, 4, 3), (3, 4, 3)])),
            "src_is_n": dict(add=t([(n, 0, 0)])),
            "dst_is_n": dict(remove=t([(0, n, 0)])),
            "no_labels_on_labelled": dict(add=(np.array([0], np.uint64), np.array([1], np.uint64))),
        }
        for name, kw in refused.items():
            with pytest.raises(hv.HelixDbError) as e:
                g.apply_edges(**kw)
            assert e.value.status == hv.ERR_INVARIANT, name
            assert twin.same_arrays(g.export(), before) and g.sizes() == sizes, name
        with pytest.raises(hv.HelixDbError) as e:
            plain.apply_edges(add=t([(0, 1, 1)]))
        assert e.value.status == hv.ERR_INVARIANT
        with pytest.raises(hv.HelixDbError) as e:
            unsorted.apply_edges(add=t([(0, 1, 1)]))
        assert e.value.status == hv.ERR_UNSUPPORTED and not unsorted.sizes()["rows_sorted"]
        g.apply_edges()  # the empty batch
        g.apply_edges(remove=t([]), add=t([]))
        assert twin.same_arrays(g.export(), before) and g.sizes() == sizes
        remove, add = t([(3, 4, 3), (7, 7, 8)]), t([(1, 1, 1), (3, 4, 0)])
        g.apply_edges(remove=remove, add=add)
        hold_to_fresh_import(hv, g, n, twin.apply_edges(n, off, tgt, lab, remove, add))
        plain.apply_edges(remove=(np.array([3], np.uint64), np.array([4], np.uint64)), add=(np.array([6], np.uint64), np.array([2], np.uint64)))
        hold_to_fresh_import(hv, plain, n, twin.apply_edges(n, off, tgt, None, (np.array([3]), np.array([4])), (np.array([6]), np.array([2]))))
    finally:
        g.close(); plain.close(); unsorted.close()


# ---- 6. the fused calls on an edited graph
def test_fused_calls_on_an_edited_g70k(hv):
    n, off, tgt, lab = fx.prefilter_graph("g70k")
    rng = np.random.default_rng(70)
    ids = fx.CONTIGUOUS_IDS
    data = rng.standard_normal((ids.size, 64)).astype(np.float32)
    q = rng.standard_normal((8, 64)).astype(np.float32)
    gix = hv.ValidatedVectorReadIndex.managed(dim=64, metric=hv.EUCLIDEAN, node_ids=ids, vectors=data, l0_offsets=np.zeros(ids.size + 1, np.uint64),
                                              l0_neighbors=np.zeros(0, np.uint64), max_batch=16)
    o = off.astype(np.int64)
    src = np.repeat(np.arange(n), np.diff(o))
    pos = np.unique(np.concatenate([rng.choice(tgt.size, 200, replace=False), np.arange(o[1040], o[1040] + 10), np.arange(o[1020], o[1020] + 3)]))
    remove = (src[pos].astype(np.uint64), tgt[pos], lab[pos])
    a_src = np.concatenate([np.full(20, 1040), np.full(5, 1020), np.full(4, 1003), rng.integers(0, n, 200)])
    add = (a_src.astype(np.uint64), rng.integers(5000, 30000, a_src.size).astype(np.uint64), rng.integers(0, 3, a_src.size).astype(np.uint32))
    new = twin.apply_edges(n, off, tgt, lab, remove, add)
    g, ref = hv.Graph(n, off, tgt, lab), fresh(hv, n, new)
    seeds = [[1000, 1001], [1020], [2002], [300, 301], [1040], [304], [1003, 1010], [3000, 1021]]
    hops = [(hv.DIR_OUT, ()), (hv.DIR_OUT, (1, 2))]
    try:
        g.apply_edges(remove=remove, add=add)
        assert twin.same_arrays(g.export(), twin.import_arrays(n, *new))
        results = []
        for graph in (g, ref):
            r = gix.prefilter_path_search_lists(graph, q, hv.SearchParams(10), seeds, hops, max_frontier=4096, want_sizes=True)
            p1 = gix.last_scan_path()
            s = gix.prefilter_repeat_search_lists(graph, q, hv.SearchParams(10), seeds, 2, hv.REPEAT_EMIT_ALL, max_frontier=4096, want_sizes=True)
            results.append((r, p1, s, gix.last_scan_path()))
        (r0, p0, s0, t0), (r1, p1, s1, t1) = results
        assert p0 == p1 and t0 == t1
        for x, y in ((r0, r1), (s0, s1)):
            cnt = x[2]
            assert cnt.tolist() == y[2].tolist() and x[3].tolist() == y[3].tolist() and np.asarray(x[4]).tolist() == np.asarray(y[4]).tolist()
            assert cnt.sum() > 0
            for qi in range(8):
                assert x[0][qi, :cnt[qi]].tolist() == y[0][qi, :cnt[qi]].tolist()
                assert x[1][qi, :cnt[qi]].view(np.uint32).tolist() == y[1][qi, :cnt[qi]].view(np.uint32).tolist()
            for extra_x, extra_y in zip(x[6:], y[6:]):
                assert np.asarray(extra_x).tolist() == np.asarray(extra_y).tolist()
    finally:
        g.close(); ref.close(); gix.close()
