"""Planted graphs for the delete path: one HUB node held by far more rows than any insert-built graph gives a node, on graphs that are
NOT symmetric -- what hvx_index_import accepts on purpose (historical rows, rows of other writers) and reverse_sources_for_target
(mutation.rs:1677) exists for.  Plain numpy: no device, no oracle.  The arrays go into orc.Index.seed(...) and
ValidatedVectorReadIndex.managed(...) alike (the hvx_index_import layout).

One layer, over the layer's node set (the hub is one of them):
  S      `holders` rows that hold the hub
  hub    its own row holds `out_in` members of S and `out_extra` rows OUTSIDE S: mandatory relink sources that do not hold the hub
         (mutation.rs:1833-1837); the holders outside the hub's row are the other asymmetric half
  rel    S + the out_extra rows: the relink sources.  Their other neighbours come from a set U >= rel with |U| = n_cand only, and every
         member of U \\ rel is planted in at least one rel row (ceil(|U \\ rel| / |rel|) per row) -- so the delete's candidate set is U
  rest   random canonical rows (ascending, deduplicated, self-free) that never name the hub, of 4 .. limit ids: about half of them full,
         the reciprocal prunes of a relink that gives one of them a new neighbour
counts() recomputes holders / sources / candidates from the rows alone; the tests assert them before they use a graph."""
import numpy as np

_BIG = np.iinfo(np.int64).max


def _draw_rows(rng, owners, pool, deg, fixed=None):
    """One row per owner: the ids of fixed[i] (a matrix padded with -1; distinct, never the owner) and random members of `pool` up to
    deg[i] distinct ids, never owners[i].  -> (matrix of ascending ids padded with _BIG, ids per row).  Vectorised: every row draws more
    than it needs, duplicates are struck by a sort, the first deg[i] valid draws stay."""
    owners = np.asarray(owners, np.int64)
    deg = np.asarray(deg, np.int64)
    rows = owners.size
    if fixed is None:
        fixed = np.full((rows, 0), -1, np.int64)
    assert (deg >= (fixed >= 0).sum(1)).all() and (deg <= pool.size - 1).all()
    extra = 16
    while True:
        draws = pool[rng.integers(0, pool.size, (rows, int(deg.max(initial=0)) + extra))]
        vals = np.concatenate([fixed, draws], axis=1)
        order = np.argsort(vals, axis=1, kind="stable")                       # (stable: a fixed id sorts before a draw of the same id)
        sv = np.take_along_axis(vals, order, 1)
        dup_sorted = np.zeros(sv.shape, bool)
        dup_sorted[:, 1:] = sv[:, 1:] == sv[:, :-1]
        dup = np.empty_like(dup_sorted)
        np.put_along_axis(dup, order, dup_sorted, 1)
        valid = ~dup & (vals >= 0) & (vals != owners[:, None])
        keep = valid & (np.cumsum(valid, 1) <= deg[:, None])
        got = keep.sum(1)
        if (got == deg).all():
            break
        extra *= 2                                                            # (a row came up short: draw again, wider)
    out = np.where(keep, vals, _BIG)
    out.sort(axis=1)
    return out[:, : max(int(deg.max(initial=0)), 1)], got


def _plant_layer(rng, nodes, hub, limit, holders, out_in, out_extra, n_cand, full_rows, long_rows=0, long_max=60):
    """-> ({row: ascending neighbour array} for every node of the layer, dict of the planted sets)"""
    others = rng.permutation(nodes[nodes != hub])
    assert holders + out_extra <= n_cand <= others.size and out_in <= holders and out_in + out_extra <= limit
    S, E = others[:holders], others[holders: holders + out_extra]
    rel = others[: holders + out_extra]
    U = others[:n_cand]
    cover = U[rel.size:]
    rest = others[rel.size:]                                                   # every row that is no relink source (U \ rel among them)
    quota = -(-cover.size // rel.size)
    assert quota <= limit - 1, "the relink sources' rows cannot hold every candidate"
    fixed = np.full((rel.size, quota + 1), -1, np.int64)
    fixed[:holders, 0] = hub
    for i in range(quota):
        part = cover[i * rel.size: (i + 1) * rel.size]
        fixed[: part.size, 1 + i] = part
    nfixed = (fixed >= 0).sum(1)
    held = np.zeros(rel.size, np.int64)
    held[:holders] = 1
    if full_rows:                                                              # holders: the hub + limit - 1 others; a mandatory source's
        deg = np.full(rel.size, limit, np.int64)                               # row is full WITHOUT the hub (nothing is unlinked from it)
    else:
        deg = np.maximum(rng.integers(min(8, limit // 2), limit, rel.size) + held, nfixed)
    rest_deg = np.minimum(limit, rng.integers(4, 2 * limit, rest.size))
    rest_deg = np.minimum(rest_deg, nodes.size - 2)
    if long_rows:                                                              # rows longer than the degree limit: holders, candidates, untouched ones
        third = long_rows // 3
        deg[rng.choice(holders, third, replace=False)] = rng.integers(limit + 1, long_max + 1, third) + 1
        rest_deg[rng.choice(cover.size, third, replace=False)] = rng.integers(limit + 1, long_max + 1, third)
        far = cover.size + rng.choice(rest.size - cover.size, long_rows - 2 * third, replace=False)
        rest_deg[far] = rng.integers(limit + 1, long_max + 1, long_rows - 2 * third)
    rel_rows, rel_n = _draw_rows(rng, rel, U, deg, fixed)
    rest_rows, rest_n = _draw_rows(rng, rest, others, rest_deg)
    rows = {int(hub): np.sort(np.concatenate([rng.choice(S, out_in, replace=False), E]))}
    for owner, r, k in zip(rel.tolist(), rel_rows, rel_n.tolist()):
        rows[owner] = r[:k]
    for owner, r, k in zip(rest.tolist(), rest_rows, rest_n.tolist()):
        rows[owner] = r[:k]
    return rows, {"holders": np.sort(S), "extra": np.sort(E), "candidates": np.sort(U), "candidate_only": np.sort(cover)}


def planted(n, holders, out_in, out_extra, n_cand, seed, m=16, m0=32, full_rows=True, layers=(), long_rows=0, hub_level=None, island=0):
    """A graph of n nodes with ascending, non-contiguous ids and one planted hub (row n // 2).  `layers`: one dict per upper layer
    (1, 2, ...) with nodes (how many have level >= l, the hub included), holders, out_in, out_extra, n_cand -- upper rows hold at most m
    ids, and only nodes of their layer.  hub_level > len(layers) gives the hub empty rows on layers nobody else reaches.  `island`
    level-0 rows name only each other and are named by nobody else: ordinary nodes whose delete cannot reach the hub's holders (a delete
    NEAR them may prune the hub out of a full holder's row, and the planted count is a count no more).
    -> dict: node_ids, level, l0_offsets, l0_neighbors, up_offsets, up_neighbors (import order: per node, layers 1 .. level), hub (row),
    hub_id, sets (per layer: rows of the holders, extra sources, candidates, candidate-only nodes), quiet (rows no layer planted),
    island (rows)."""
    rng = np.random.default_rng(seed)
    ids = np.arange(n, dtype=np.uint64) * np.uint64(2) + np.uint64(5)
    hub = n // 2
    level = np.zeros(n, np.uint16)
    ranked = rng.permutation(np.delete(np.arange(n, dtype=np.int64), hub))     # the first rows reach the highest layers
    members = [np.arange(n, dtype=np.int64)]
    for l, spec in enumerate(layers, start=1):
        assert spec["nodes"] <= members[-1].size
        level[ranked[: spec["nodes"] - 1]] = l
        members.append(np.sort(np.append(ranked[: spec["nodes"] - 1], hub)))
    level[hub] = len(layers) if hub_level is None else hub_level
    assert level[hub] >= len(layers)
    isl = np.sort(ranked[ranked.size - island:]) if island else np.zeros(0, np.int64)
    assert not level[isl].any()
    rows0, sets0 = _plant_layer(rng, np.setdiff1d(members[0], isl), hub, m0, holders, out_in, out_extra, n_cand, full_rows, long_rows)
    if island:
        isl_rows, isl_n = _draw_rows(rng, isl, isl, np.full(island, min(6, island - 2), np.int64))
        rows0.update({owner: r[:k] for owner, r, k in zip(isl.tolist(), isl_rows, isl_n.tolist())})
    per_layer, sets = [rows0], [sets0]
    for l, spec in enumerate(layers, start=1):
        r, s = _plant_layer(rng, members[l], hub, m, spec["holders"], spec["out_in"], spec["out_extra"], spec["n_cand"], full_rows)
        per_layer.append(r)
        sets.append(s)
    l0 = [rows0[i] for i in range(n)]
    l0_offsets = np.zeros(n + 1, np.uint64)
    l0_offsets[1:] = np.cumsum([r.size for r in l0])
    up = [per_layer[l][i] if l < len(per_layer) else np.zeros(0, np.int64) for i in np.nonzero(level)[0].tolist() for l in range(1, int(level[i]) + 1)]
    up_offsets = np.zeros(len(up) + 1, np.uint64)
    if up:
        up_offsets[1:] = np.cumsum([r.size for r in up])
    planted_rows = np.concatenate([s["candidates"] for s in sets] + [[hub]])
    quiet = np.setdiff1d(np.arange(n), np.concatenate([planted_rows, isl]))
    return {"node_ids": ids, "level": level, "l0_offsets": l0_offsets, "l0_neighbors": ids[np.concatenate(l0)],
            "up_offsets": up_offsets, "up_neighbors": ids[np.concatenate(up)] if up else np.zeros(0, np.uint64),
            "hub": hub, "hub_id": int(ids[hub]), "sets": sets, "quiet": quiet, "island": isl, "m": m, "m0": m0}


def layer_rows(g, layer):
    """{row: neighbour ROWS} of one layer, from the import arrays alone"""
    ids = g["node_ids"]
    out = {}
    if layer == 0:
        nb = np.searchsorted(ids, g["l0_neighbors"])
        off = g["l0_offsets"].astype(np.int64)
        return {i: nb[off[i]: off[i + 1]] for i in range(ids.size)}
    nb = np.searchsorted(ids, g["up_neighbors"])
    off = g["up_offsets"].astype(np.int64)
    r = 0
    for i in np.nonzero(g["level"])[0].tolist():
        lv = int(g["level"][i])
        if lv >= layer:
            out[i] = nb[off[r + layer - 1]: off[r + layer]]
        r += lv
    return out


def counts(rows, hub, layer=0):
    """(holders, relink sources, candidates) of deleting `hub` on one layer, from {row: neighbour rows} (layer_rows) or the dict planted()
    returns: the rows that hold the hub; those and the hub's own out-neighbours; the sources and everything their rows hold, less the hub."""
    if "node_ids" in rows:
        rows = layer_rows(rows, layer)
    holders = {i for i, r in rows.items() if i != hub and hub in set(r.tolist())}
    sources = holders | set(rows.get(hub, np.zeros(0, np.int64)).tolist())
    cands = set(sources)
    for s in sources:
        cands.update(rows[s].tolist())
    cands.discard(hub)
    return len(holders), len(sources), len(cands)


# ---- the cases of tests/test_hub_graphs_host.py (CPU) and tests/test_gpu_delete_hubs.py (device) ----
# plant: planted()'s arguments; counts: (holders, sources, candidates) per layer, asserted before a graph is used; metric 0 cosine / 1 L2
_MID = dict(n=3000, holders=300, out_in=20, out_extra=12, n_cand=2500, seed=11, full_rows=False)
_UPPER = dict(n=3000, holders=100, out_in=20, out_extra=12, n_cand=1500, seed=31, full_rows=False,
              layers=(dict(nodes=1500, holders=200, out_in=10, out_extra=6, n_cand=1000), dict(nodes=60, holders=30, out_in=10, out_extra=4, n_cand=50)))
CASES = {
    "mid": dict(plant=_MID, counts=[(300, 312, 2500)]),
    "mid_cos": dict(plant=_MID, counts=[(300, 312, 2500)], metric=0),
    "mid_bf16": dict(plant=_MID, counts=[(300, 312, 2500)], dim=64, bf16=True),   # (dim 64: the HNSW search kernels do not serve bf16 rows below 128)
    "mid_bf16_128": dict(plant=_MID, counts=[(300, 312, 2500)], dim=128, bf16=True),
    "mid_ties": dict(plant=_MID, counts=[(300, 312, 2500)], points=40),          # 75 exact duplicates of every vector
    # (4 000 candidates need more than 3 000 rows: 4 500 here)
    "mid_wide": dict(plant=dict(n=4500, holders=300, out_in=20, out_extra=12, n_cand=4000, seed=13, m=32, m0=64, full_rows=False), counts=[(300, 312, 4000)]),
    "long_rows": dict(plant=dict(n=3000, holders=100, out_in=20, out_extra=12, n_cand=1500, seed=17, full_rows=False, long_rows=40), counts=[(100, 112, 1500)]),
    "upper": dict(plant=_UPPER, counts=[(100, 112, 1500), (200, 206, 1000), (30, 34, 50)]),
    # the hub alone on a layer of its own above the others: its delete moves the entry point AND lowers the top layer
    "upper_entry": dict(plant=dict(_UPPER, hub_level=3), counts=[(100, 112, 1500), (200, 206, 1000), (30, 34, 50)], hub_is_entry=True),
    "src_boundary": dict(plant=dict(n=40000, holders=4096, out_in=32, out_extra=0, n_cand=4608, seed=19), counts=[(4096, 4096, 4608)]),
    "cand_boundary": dict(plant=dict(n=40000, holders=560, out_in=20, out_extra=12, n_cand=16384, seed=23), counts=[(560, 572, 16384)]),
}
# one past each limit of hvx_index_delete_batch: refused, loudly
REFUSALS = {
    "too_many_holders": dict(plant=dict(n=40000, holders=4097, out_in=32, out_extra=0, n_cand=4609, seed=41, island=12), counts=[(4097, 4097, 4609)],
                             text="more than 4096 rows hold one node"),
    "too_many_sources": dict(plant=dict(n=40000, holders=4090, out_in=20, out_extra=10, n_cand=4608, seed=43), counts=[(4090, 4100, 4608)],
                             text="more than 4096 relink sources"),
    "too_many_candidates": dict(plant=dict(n=40000, holders=560, out_in=20, out_extra=12, n_cand=16385, seed=47), counts=[(560, 572, 16385)],
                                text="more than 16384 relink candidates"),
}


def case_graph(case):
    """the planted graph of a case with its vectors, entry point and the ids its test deletes, in order: the hub, three of its former
    holders (the last one a holder on the hub's TOP planted layer), one node that is only a candidate"""
    g = planted(**case["plant"])
    n, dim = g["node_ids"].size, case.get("dim", 32)
    rng = np.random.default_rng(case["plant"]["seed"] + 1000)
    if case.get("points"):
        vec = rng.standard_normal((case["points"], dim)).astype(np.float32)[rng.integers(0, case["points"], n)]
    else:
        vec = rng.standard_normal((n, dim)).astype(np.float32)
    h0 = g["sets"][0]["holders"]
    order = [g["hub"], int(h0[0]), int(h0[h0.size // 2])]
    order.append(next(int(x) for x in g["sets"][-1]["holders"][::-1] if int(x) not in order))
    order.append(next(int(x) for x in g["sets"][0]["candidate_only"] if int(x) not in order))
    top = len(case["plant"].get("layers", ()))
    if case.get("hub_is_entry"):
        entry, max_layer = g["hub"], int(g["level"][g["hub"]])
    else:
        entry = next(i for i in range(n) if int(g["level"][i]) == top and i not in order)
        max_layer = top
    g.update(vectors=vec, entry_point=int(g["node_ids"][entry]), max_layer=max_layer, delete_ids=[int(g["node_ids"][r]) for r in order],
             quiet_ids=[int(g["node_ids"][r]) for r in g["quiet"][:8] if r != entry], island_ids=[int(x) for x in g["node_ids"][g["island"]]])
    return g


def import_args(g):
    """what orc.Index.seed(**...) and ValidatedVectorReadIndex.managed(**...) both take"""
    return {k: g[k] for k in ("node_ids", "vectors", "l0_offsets", "l0_neighbors", "level", "up_offsets", "up_neighbors", "entry_point", "max_layer")}
