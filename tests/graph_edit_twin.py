"""The numpy restatement of hvx_csr_apply_edges (include/helix_vec.h) -- a helper, not a test.

E = the stored arcs in out-array order, each (src, dst, label).  A batch: the removals in batch order, each deleting the LAST-stored
arc equal to its triple (a pair for an unlabelled graph); then the additions appended in batch order; then a stable sort by
(src, dst).  import_arrays() derives the incoming side the way hvx_csr_import does: a stable counting sort of the stored arcs by
target, so incoming rows are in (source, out-array position) order and in_edge_index maps a slot back to its stored arc."""
import numpy as np


class Refused(Exception):
    """the batch names a removal with no stored arc left to match, or an endpoint outside the graph"""


def _batch(b, labelled):
    if b is None:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), (np.zeros(0, np.uint32) if labelled else None)
    src, dst = np.asarray(b[0], np.int64), np.asarray(b[1], np.int64)
    lab = np.asarray(b[2], np.uint32) if len(b) > 2 and b[2] is not None else None
    if (lab is not None) != labelled:
        raise Refused("labels on an unlabelled graph, or none on a labelled one")
    return src, dst, lab


def apply_edges(n, offsets, targets, labels=None, remove=None, add=None):
    """(offsets u64 [n + 1], targets u64, labels u32 or None) after the batch"""
    off = np.asarray(offsets, np.int64)
    tgt = np.asarray(targets, np.int64)
    labelled = labels is not None
    lab = np.asarray(labels, np.uint32) if labelled else None
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    ds, dd, dl = _batch(remove, labelled)
    as_, ad, al = _batch(add, labelled)
    for a in (ds, dd, as_, ad):
        if a.size and (a.min() < 0 or a.max() >= n):
            raise Refused("endpoint outside the graph")
    alive = np.ones(tgt.size, bool)
    for i in range(ds.size):
        r0, r1 = off[ds[i]], off[ds[i] + 1]
        hit = alive[r0:r1] & (tgt[r0:r1] == dd[i])
        if labelled:
            hit &= lab[r0:r1] == dl[i]
        where = np.nonzero(hit)[0]
        if where.size == 0:
            raise Refused(f"removal {i} has no stored arc left to match")
        alive[r0 + where[-1]] = False
    src = np.concatenate([src[alive], as_])
    tgt = np.concatenate([tgt[alive], ad])
    if labelled:
        lab = np.concatenate([lab[alive], al])
    order = np.lexsort((tgt, src))  # stable: equal (src, dst) keep stored-then-appended order
    new_off = np.zeros(n + 1, np.uint64)
    new_off[1:] = np.cumsum(np.bincount(src, minlength=n)[:n])
    return new_off, tgt[order].astype(np.uint64), (lab[order] if labelled else None)


def import_arrays(n, offsets, targets, labels=None):
    """dict of the seven arrays hvx_csr_export returns for a fresh import of (offsets, targets, labels)"""
    off = np.asarray(offsets, np.uint64)
    tgt = np.asarray(targets, np.uint64)
    src = np.repeat(np.arange(n, dtype=np.uint64), np.diff(off.astype(np.int64)))
    order = np.argsort(tgt, kind="stable")
    in_off = np.zeros(n + 1, np.uint64)
    in_off[1:] = np.cumsum(np.bincount(tgt.astype(np.int64), minlength=n)[:n])
    lab = None if labels is None else np.asarray(labels, np.uint32)
    return dict(out_offsets=off, out_targets=tgt, out_labels=lab, in_offsets=in_off, in_sources=src[order],
                in_labels=None if lab is None else lab[order], in_edge_index=order.astype(np.uint64))


def sizes(n, offsets, targets):
    off = np.asarray(offsets, np.int64)
    tgt = np.asarray(targets, np.int64)
    return dict(n_nodes=n, n_edges=int(tgt.size), max_out_degree=int(np.diff(off).max()) if n else 0,
                max_in_degree=int(np.bincount(tgt, minlength=max(n, 1)).max()) if tgt.size else 0, rows_sorted=True)


def same_arrays(a, b):
    """two export() / import_arrays() dicts hold the same seven arrays"""
    for key in ("out_offsets", "out_targets", "out_labels", "in_offsets", "in_sources", "in_labels", "in_edge_index"):
        x, y = a[key], b[key]
        if (x is None) != (y is None):
            return False
        if x is not None and (x.shape != y.shape or not np.array_equal(np.asarray(x, np.uint64), np.asarray(y, np.uint64))):
            return False
    return True


# The hand-written eight-node labelled graph.  Row 3 ("d") holds the parallel arcs (d,3) (d,5) (d,3) to node 4, row 2 a self-loop,
# rows 1 and 6 are empty, node 7 is the last one.  Arcs as (src, dst, label), in stored order:
EIGHT_N = 8
EIGHT_ARCS = [(0, 1, 1), (0, 4, 2), (2, 2, 7), (2, 5, 1), (3, 4, 3), (3, 4, 5), (3, 4, 3), (3, 6, 2), (4, 0, 9), (5, 7, 4), (7, 0, 6), (7, 7, 8)]


def eight_graph():
    src = np.array([a[0] for a in EIGHT_ARCS], np.int64)
    off = np.zeros(EIGHT_N + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(src, minlength=EIGHT_N))
    return EIGHT_N, off, np.array([a[1] for a in EIGHT_ARCS], np.uint64), np.array([a[2] for a in EIGHT_ARCS], np.uint32)


def triples(batch):
    """[(src, dst, label)] -> the (src, dst, labels) tuple the calls take"""
    if not batch:
        return None
    return (np.array([t[0] for t in batch], np.uint64), np.array([t[1] for t in batch], np.uint64), np.array([t[2] for t in batch], np.uint32))


# name -> (removals, additions, the arcs afterwards spelled out by hand, in stored order)
EIGHT_CASES = {
    # removing (d,3) takes the LAST (3,4,3): (d,3) (d,5) stay
    "remove_last_parallel": ([(3, 4, 3)], [],
                             [(0, 1, 1), (0, 4, 2), (2, 2, 7), (2, 5, 1), (3, 4, 3), (3, 4, 5), (3, 6, 2), (4, 0, 9), (5, 7, 4), (7, 0, 6), (7, 7, 8)]),
    # an add lands behind the equals already stored, in front of larger targets
    "add_after_equals": ([], [(3, 4, 5), (3, 4, 1)],
                         [(0, 1, 1), (0, 4, 2), (2, 2, 7), (2, 5, 1), (3, 4, 3), (3, 4, 5), (3, 4, 3), (3, 4, 5), (3, 4, 1), (3, 6, 2), (4, 0, 9),
                          (5, 7, 4), (7, 0, 6), (7, 7, 8)]),
    # remove + add of one triple: the stored last (3,4,3) goes, the new one is appended behind (d,5)
    "remove_and_add_same": ([(3, 4, 3)], [(3, 4, 3)],
                            [(0, 1, 1), (0, 4, 2), (2, 2, 7), (2, 5, 1), (3, 4, 3), (3, 4, 5), (3, 4, 3), (3, 6, 2), (4, 0, 9), (5, 7, 4), (7, 0, 6),
                             (7, 7, 8)]),
    # both (d,3) go, (d,5) survives between them
    "remove_both_parallel": ([(3, 4, 3), (3, 4, 3)], [],
                             [(0, 1, 1), (0, 4, 2), (2, 2, 7), (2, 5, 1), (3, 4, 5), (3, 6, 2), (4, 0, 9), (5, 7, 4), (7, 0, 6), (7, 7, 8)]),
    # a removal empties rows 4 and 5; the self-loop of row 2 goes
    "empty_a_row": ([(5, 7, 4), (4, 0, 9), (2, 2, 7)], [],
                    [(0, 1, 1), (0, 4, 2), (2, 5, 1), (3, 4, 3), (3, 4, 5), (3, 4, 3), (3, 6, 2), (7, 0, 6), (7, 7, 8)]),
    # adds into the empty rows 1 and 6 (a self-loop among them)
    "fill_empty_rows": ([], [(6, 6, 2), (1, 7, 3), (6, 0, 1)],
                        [(0, 1, 1), (0, 4, 2), (1, 7, 3), (2, 2, 7), (2, 5, 1), (3, 4, 3), (3, 4, 5), (3, 4, 3), (3, 6, 2), (4, 0, 9), (5, 7, 4),
                         (6, 0, 1), (6, 6, 2), (7, 0, 6), (7, 7, 8)]),
    # node 0 and node n - 1 on both ends of the arrays
    "first_and_last_node": ([(0, 1, 1), (7, 7, 8)], [(0, 0, 5), (7, 7, 1), (7, 3, 2), (0, 7, 4)],
                            [(0, 0, 5), (0, 4, 2), (0, 7, 4), (2, 2, 7), (2, 5, 1), (3, 4, 3), (3, 4, 5), (3, 4, 3), (3, 6, 2), (4, 0, 9), (5, 7, 4),
                             (7, 0, 6), (7, 3, 2), (7, 7, 1)]),
}


def g20k_batch(n, offsets, targets, labels, hub=12345, sink=777, seed=424242):
    """One seeded batch on fixtures.prefilter_graph("g20k"): about 300 removals drawn from DISTINCT stored positions (so every one
    has its arc) and about 500 additions.  It holds: removals from and additions into the hub row; more than 64 additions into one
    ordinary row; a row emptied; an empty row filled; rows 0 and n - 1; an addition that duplicates a stored triple; the removal of
    one of several parallel arcs with distinct labels; an arc into the sink and one removed from it; self-loops.
    Returns (remove, add, facts) -- facts names the rows, for the assertions of the tests."""
    off = np.asarray(offsets, np.int64)
    tgt = np.asarray(targets, np.int64)
    lab = np.asarray(labels, np.uint32)
    src = np.repeat(np.arange(n, dtype=np.int64), np.diff(off))
    deg = np.diff(off)
    rng = np.random.default_rng(seed)
    special = {0, n - 1, hub, sink, 5}
    ordinary = [int(u) for u in np.nonzero(deg >= 2)[0] if int(u) not in special]
    emptied, many = ordinary[len(ordinary) // 3], ordinary[len(ordinary) // 2]
    filled = [int(u) for u in np.nonzero(deg == 0)[0] if int(u) not in special][7]
    # parallel arcs with distinct labels: adjacent stored arcs of one (src, dst) whose labels differ
    par = np.nonzero((src[1:] == src[:-1]) & (tgt[1:] == tgt[:-1]) & (lab[1:] != lab[:-1]))[0]
    assert par.size, "the fixture holds no parallel arcs with distinct labels"
    pos = set(int(p) for p in rng.choice(np.arange(off[hub], off[hub + 1]), 40, replace=False))  # the hub row
    pos |= set(range(int(off[emptied]), int(off[emptied + 1])))                                  # a row emptied
    pos.add(int(par[0]))                                                                         # the first of the parallel pair
    into_sink = np.nonzero(tgt == sink)[0]
    pos.add(int(into_sink[len(into_sink) // 2]))                                                 # out of the sink's long incoming row
    for u in (0, n - 1):
        if deg[u]:
            pos.add(int(off[u]))
    pos |= set(int(p) for p in rng.choice(tgt.size, 250, replace=False))
    pos -= set(range(int(off[many]), int(off[many + 1])))  # (the crowded row keeps its stored arcs)
    pos = np.array(sorted(pos), np.int64)
    rng.shuffle(pos)
    remove = (src[pos].astype(np.uint64), tgt[pos].astype(np.uint64), lab[pos])
    kept = np.setdiff1d(np.arange(tgt.size), pos)
    dup = int(kept[np.nonzero(src[kept] == hub)[0][3]])  # a stored triple of the hub row that stays, added once more
    adds = [(hub, int(t), int(l)) for t, l in zip(rng.integers(0, n, 30), rng.integers(0, 3, 30))]
    adds += [(many, int(t), int(l)) for t, l in zip(rng.integers(0, n, 70), rng.integers(0, 3, 70))]
    adds += [(filled, 9, 1), (filled, filled, 0), (filled, 9, 2)]
    adds += [(0, 3, 1), (0, 0, 2), (n - 1, n - 1, 0), (n - 1, 0, 1), (4, n - 1, 2)]
    adds += [(int(src[dup]), int(tgt[dup]), int(lab[dup]))]
    adds += [(many, sink, 1), (hub, sink, 2), (hub, hub, 0), (sink, sink, 1)]
    adds += [(int(s), int(t), int(l)) for s, t, l in zip(rng.integers(0, n, 390), rng.integers(0, n, 390), rng.integers(0, 3, 390))]
    order = rng.permutation(len(adds))
    adds = [adds[i] for i in order]
    facts = dict(hub=hub, sink=sink, emptied=emptied, many=many, filled=filled, parallel=(int(src[par[0]]), int(tgt[par[0]])), duplicate=dup)
    return remove, triples(adds), facts
