"""Host twin of hvx_index_audit_graph (csrc/hvx_audit.hip), written from the definitions of hvx_graph_audit in include/helix_vec.h:
plain loops over the rows of a graph image as the device holds it.  It is the reference tests/test_gpu_audit.py holds the device audit
to, and tests/test_audit_twin.py pins it on graphs small enough to count by hand.  Test infrastructure only; no GPU.

`raw` is a dict: n, s0, su, l0 [n][s0] u32, up [up_rows][su] u32, level [n], up_base [n], dead (bitmap words, one bit per row, or None),
entry, has_entry, max_layer, m, m0.  An empty slot holds SENTINEL.

What the definitions leave open, and how the audit decides (each is pinned by a hand-counted case):
  * every non-sentinel slot is an edge, whatever else is wrong with it; rows of deleted owners are walked like any other
  * a hole is a non-sentinel slot behind a sentinel; an unsorted entry is one behind a non-sentinel id that is not smaller
  * a self loop is still looked up for its reverse edge (which it finds in its own row, when that row can be searched)
  * an id >= n, or the id of a deleted row, is out of range and is counted in nothing further
  * an upper-layer id whose level is below the row's layer is a level violation and is not also asymmetric
  * the reverse look-up is a LOWER-BOUND BINARY SEARCH over the full stride of the target row, sentinels included; it equals plain
    membership exactly when the target row is canonical.  audit(raw) uses the binary search, audit(raw, reverse="membership") the other
  * a row overflows above m0 (layer 0) / m (upper layers) ids; a limit of 0 means the stride.  max_degree_* runs over all rows
  * the BFS runs over layer 0 from `entry`, follows every id < n (deleted rows are walked, though never counted as unreachable);
    bfs_levels_l0 is the eccentricity of the entry point; without an entry point every live row is unreachable
  * nodes = live rows; up_rows = the sum of `level` over the n rows"""
import numpy as np

SENTINEL = 0xFFFFFFFF

KEYS = ("nodes", "up_rows", "edges_l0", "edges_up", "asymmetric_edges_l0", "asymmetric_edges_up", "unsorted_entries", "self_loops",
        "out_of_range_ids", "holes", "level_violations", "degree_overflow_rows", "unreachable_l0", "max_degree_l0", "max_degree_up",
        "bfs_levels_l0", "max_layer", "has_entry")


def is_dead(raw, v):
    dead = raw.get("dead")
    return dead is not None and bool((int(dead[v >> 5]) >> (v & 31)) & 1)


def lower_bound_has(row, x):
    """what a lower-bound binary search over the whole stride finds (the raw values, sentinels included)"""
    lo, hi = 0, len(row)
    while lo < hi:
        mid = (lo + hi) // 2
        if row[mid] < x:
            lo = mid + 1
        else:
            hi = mid
    return lo < len(row) and row[lo] == x


def is_canonical(row):
    """ascending ids, then nothing but sentinels"""
    ids = [x for x in row if x != SENTINEL]
    return list(row[:len(ids)]) == ids and all(a < b for a, b in zip(ids, ids[1:]))


def audit(raw, reverse="lower_bound"):
    assert reverse in ("lower_bound", "membership")
    has = lower_bound_has if reverse == "lower_bound" else (lambda row, x: x in row)
    n, s0, su = int(raw["n"]), int(raw["s0"]), int(raw["su"])
    out = dict.fromkeys(KEYS, 0)
    out["has_entry"], out["max_layer"] = int(raw["has_entry"]), int(raw["max_layer"])
    if n == 0:
        return out
    l0 = [[int(x) for x in raw["l0"][u][:s0]] for u in range(n)]
    level = [int(x) for x in raw["level"][:n]]
    up_base = [int(x) for x in raw["up_base"][:n]]
    up = [[int(x) for x in r[:su]] for r in raw["up"]]
    lim0, limu = int(raw["m0"]) or s0, int(raw["m"]) or su
    out["nodes"] = sum(1 for u in range(n) if not is_dead(raw, u))
    out["up_rows"] = sum(level)

    def walk(row, owner, layer):
        sfx = "l0" if layer == 0 else "up"
        deg = sum(1 for x in row if x != SENTINEL)
        out["max_degree_" + sfx] = max(out["max_degree_" + sfx], deg)
        if deg > (lim0 if layer == 0 else limu):
            out["degree_overflow_rows"] += 1
        for p, v in enumerate(row):
            if v == SENTINEL:
                continue
            out["edges_" + sfx] += 1
            if p > 0 and row[p - 1] == SENTINEL:
                out["holes"] += 1
            elif p > 0 and row[p - 1] >= v:
                out["unsorted_entries"] += 1
            if v == owner:
                out["self_loops"] += 1
            if v >= n or is_dead(raw, v):
                out["out_of_range_ids"] += 1
                continue
            if layer and level[v] < layer:
                out["level_violations"] += 1
                continue
            back = l0[v] if layer == 0 else up[up_base[v] + layer - 1]
            if not has(back, owner):
                out["asymmetric_edges_" + sfx] += 1

    for u in range(n):
        walk(l0[u], u, 0)
        for layer in range(1, level[u] + 1):
            walk(up[up_base[u] + layer - 1], u, layer)

    dist = {}
    if out["has_entry"]:
        dist[int(raw["entry"])] = 0
        frontier = [int(raw["entry"])]
        while frontier:
            nxt = []
            for u in frontier:
                for v in l0[u]:
                    if v != SENTINEL and v < n and v not in dist:
                        dist[v] = dist[u] + 1
                        nxt.append(v)
            frontier = nxt
        out["bfs_levels_l0"] = max(dist.values())
    out["unreachable_l0"] = sum(1 for u in range(n) if u not in dist and not is_dead(raw, u))
    return out


def make_raw(l0_rows, s0, up_rows=(), su=16, level=None, dead_rows=(), entry=None, max_layer=0, m=0, m0=0):
    """a raw image from rows written out as lists (padded with SENTINEL to the strides; up_base follows `level` in row order)"""
    n = len(l0_rows)
    level = [0] * n if level is None else list(level)
    l0 = np.full((n, s0), SENTINEL, np.uint32)
    for u, r in enumerate(l0_rows):
        l0[u, :len(r)] = r
    up = np.full((len(up_rows), su), SENTINEL, np.uint32)
    for r, ids in enumerate(up_rows):
        up[r, :len(ids)] = ids
    up_base, nxt = np.full(n, SENTINEL, np.uint32), 0
    for u in range(n):
        if level[u]:
            up_base[u], nxt = nxt, nxt + level[u]
    assert nxt == len(up_rows)
    dead = None
    if len(dead_rows):
        dead = np.zeros((n + 31) // 32, np.uint32)
        for d in dead_rows:
            dead[d >> 5] |= np.uint32(1 << (d & 31))
    return {"n": n, "s0": s0, "su": su, "l0": l0, "up": up, "level": np.asarray(level, np.uint16), "up_base": up_base, "dead": dead,
            "entry": 0 if entry is None else entry, "has_entry": 0 if entry is None else 1, "max_layer": max_layer, "m": m, "m0": m0}


def raw_from_export(g, s0, su, m=0, m0=0):
    """the CSR of export_graph() / the oracle's export() in fixed-stride rows; node ids are the row numbers 0 .. n-1"""
    n = len(g["l0_offsets"]) - 1
    cut = lambda off, nb, r: [int(x) for x in nb[int(off[r]):int(off[r + 1])]]
    n_up = len(g["up_offsets"]) - 1
    return make_raw([cut(g["l0_offsets"], g["l0_neighbors"], u) for u in range(n)], s0,
                    [cut(g["up_offsets"], g["up_neighbors"], r) for r in range(n_up)], su, level=[int(x) for x in g["level"][:n]],
                    entry=g["entry_point"], max_layer=int(g["max_layer"]), m=m, m0=m0)
