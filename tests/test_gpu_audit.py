"""hvx_index_audit_graph (csrc/hvx_audit.hip) against its host twin (tests/audit_twin.py) on planted defects of every kind.  The audit is the
only judge of every graph that cannot be compared row for row with the oracle; here it is the one being judged.  Every case is: plant
(tests/native/audit_poke.hip writes single slots of the image on the device), dump, twin(dump) == audit_graph() on EVERY key, exactly --
all counters are integers -- and the counter the case aims at is above 0 on the twin.  The device's reverse look-up is a lower-bound binary
search (the twin's default); where a case keeps the searched rows canonical it says so and asserts that plain membership agrees."""
import numpy as np
import pytest

import audit_harness as ah
import audit_twin as tw

pytestmark = pytest.mark.gpu

S = tw.SENTINEL
DEFECTS = ("asymmetric_edges_l0", "asymmetric_edges_up", "unsorted_entries", "self_loops", "out_of_range_ids", "holes", "level_violations",
           "degree_overflow_rows")


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


# ---- images -------------------------------------------------------------------------------------------------------------------------------

def levels_for(n):
    """every 5th node lives on layer 1, every 10th on layer 2 too: enough nodes per layer to fill an upper row of 32 ids"""
    lv = np.zeros(n, np.uint16)
    lv[::5] = 1
    lv[::10] = 2
    return lv


def base_graph(n, seed, hub=None, hub_degree=0):
    """a symmetric, canonical graph with short rows (room to plant): rings plus random chords on every layer; `hub` gets hub_degree ids"""
    rng = np.random.default_rng(seed)
    lv = levels_for(n)

    def layer(nodes, chords, cap):
        adj = {u: set() for u in nodes}

        def link(a, b):
            if a != b and len(adj[a]) < cap and len(adj[b]) < cap:
                adj[a].add(b), adj[b].add(a)
        k = len(nodes)
        for i, u in enumerate(nodes):
            for step in (1, 2):
                link(u, nodes[(i + step) % k])
            for v in rng.choice(k, size=chords):
                link(u, nodes[int(v)])
        return adj
    everyone = list(range(n))
    l0 = layer(everyone, 2, 12)
    if hub is not None:
        for v in rng.permutation(n)[:hub_degree + 1]:
            if int(v) != hub and len(l0[hub]) < hub_degree:
                l0[hub].add(int(v)), l0[int(v)].add(hub)
    ups = {L: layer([u for u in everyone if lv[u] >= L], 1, 6) for L in (1, 2)}
    l0_rows = [sorted(l0[u]) for u in everyone]
    up_rows = [sorted(ups[L][u]) for u in everyone for L in range(1, int(lv[u]) + 1)]

    def csr(rows):
        off = np.zeros(len(rows) + 1, np.uint64)
        off[1:] = np.cumsum([len(r) for r in rows])
        return off, np.asarray([x for r in rows for x in r], np.uint64)
    l0o, l0n = csr(l0_rows)
    upo, upn = csr(up_rows)
    return {"l0_offsets": l0o, "l0_neighbors": l0n, "level": lv, "up_offsets": upo, "up_neighbors": upn,
            "entry_point": 0 if n else None, "max_layer": int(lv.max()) if n else 0}


IMAGES = {  # name: n, dim, import arguments; (s0, su) the strides they must lead to
    "f32_m16": (1200, 32, dict(m=16, m0=32), (32, 16)),
    "f32_m32": (500, 32, dict(m=32, m0=64), (64, 32)),
    "bf16": (500, 64, dict(m=16, m0=32, dtype="bf16"), (32, 16)),
    "m12": (500, 32, dict(m=12, m0=24), (32, 16)),                              # strides above the limits: rows can overflow
    "wide96": (500, 32, dict(m=0, m0=0, hub=7), (96, 16)),                      # a row of 70 ids, no declared limits: rows straddle blocks
    "reserved": (500, 32, dict(m=16, m0=32, reserve_rows=8, reserve_upper_rows=4), (32, 16)),
}
_IMAGES = {}


def import_graph(hv, g, dim, seed, **kw):
    n = len(g["l0_offsets"]) - 1
    if kw.pop("dtype", None) == "bf16":
        kw["dtype"] = hv.BF16
    data = np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)
    return hv.ValidatedVectorReadIndex.managed(dim=dim, metric=hv.EUCLIDEAN, node_ids=np.arange(n, dtype=np.uint64), vectors=data,
                                               l0_offsets=g["l0_offsets"], l0_neighbors=g["l0_neighbors"], level=g["level"],
                                               up_offsets=g["up_offsets"], up_neighbors=g["up_neighbors"], entry_point=g["entry_point"],
                                               max_layer=g["max_layer"], **kw)


def image(hv, name):
    """one image per name for the module; every test leaves it as it found it (Planter.restore)"""
    if name not in _IMAGES:
        n, dim, kw, strides = IMAGES[name]
        kw = dict(kw)
        hub = kw.pop("hub", None)
        g = base_graph(n, 100 + list(IMAGES).index(name), hub=hub, hub_degree=70)
        gix = import_graph(hv, g, dim, 7, **kw)
        _IMAGES[name] = (gix, g)
    return _IMAGES[name]


class Planter:
    """host mirror of the rows of an image; writes only the slots that change, and puts every one of them back"""

    def __init__(self, gix):
        self.gix = gix
        self.raw = ah.dump(gix)
        self.orig = {k: self.raw[k].copy() for k in ("l0", "up")}
        self.n, self.s0, self.su = self.raw["n"], self.raw["s0"], self.raw["su"]
        self.level = [int(x) for x in self.raw["level"]]

    def stride(self, layer):
        return self.su if layer else self.s0

    def at(self, layer, u):
        """(array, row index) of node u's row on `layer`"""
        if layer == 0:
            return self.raw["l0"], u
        assert 1 <= layer <= self.level[u]
        return self.raw["up"], int(self.raw["up_base"][u]) + layer - 1

    def ids(self, layer, u):
        arr, r = self.at(layer, u)
        return [int(x) for x in arr[r] if x != S]

    def set_row(self, layer, u, values):
        arr, r = self.at(layer, u)
        values = list(values) + [S] * (arr.shape[1] - len(values))
        assert len(values) == arr.shape[1]
        for slot, v in enumerate(values):
            if int(arr[r, slot]) != v:
                ah.write(self.gix, layer != 0, r, slot, v)
                arr[r, slot] = v

    def fill_row(self, layer, u, count=None):
        """node u's row on `layer` grown to `count` ids (default: the whole stride), every new neighbour listing u back: still a canonical,
        symmetric graph.  Returns the row."""
        stride = self.stride(layer)
        count = stride if count is None else count
        cur = self.ids(layer, u)
        cands = [v for v in range(self.n) if v != u and self.level[v] >= layer and v not in cur and len(self.ids(layer, v)) < stride]
        need = count - len(cur)
        assert 0 <= need <= len(cands), (layer, u, count, len(cur), len(cands))
        new = [cands[(i * len(cands)) // need] for i in range(need)] if need else []
        for v in new:
            self.set_row(layer, v, sorted(self.ids(layer, v) + [u]))
        row = sorted(cur + new)
        self.set_row(layer, u, row)
        return row

    def restore(self):
        for key, upper in (("l0", False), ("up", True)):
            for r, slot in np.argwhere(self.raw[key] != self.orig[key]):
                ah.write(self.gix, upper, int(r), int(slot), int(self.orig[key][r, slot]))
            self.raw[key][...] = self.orig[key]


def check(gix, mirror=None):
    """dump, twin(dump) == audit on every key; returns (twin's result, dump)"""
    raw = ah.dump(gix)
    if mirror is not None:  # the writes landed where the mirror says
        assert np.array_equal(raw["l0"], mirror.raw["l0"]) and np.array_equal(raw["up"], mirror.raw["up"])
    want = tw.audit(raw)
    got = gix.audit_graph()
    assert set(got) == set(want) == set(tw.KEYS)
    diff = {k: (got[k], want[k]) for k in tw.KEYS if got[k] != want[k]}
    assert not diff, f"audit (device, twin) differ: {diff}"
    return want, raw


# ---- the layout gate ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(IMAGES))
def test_layout_gate_the_dump_of_an_untouched_image_is_its_export(hv, name):
    """If this fails the helper is wrong, not the audit: the dump of an imported image has the image's rows, converts back to exactly
    export_graph(), has the strides the case is meant to have, and its twin equals the device audit with every defect counter 0."""
    gix, g = image(hv, name)
    n, _, kw, strides = IMAGES[name]
    raw = ah.dump(gix)
    assert raw["n"] == gix.rows() == n and (raw["s0"], raw["su"]) == strides
    assert (raw["m"], raw["m0"]) == (kw["m"], kw["m0"]) and raw["cap_rows"] == n + kw.get("reserve_rows", 0)
    ex, back = gix.export_graph(), ah.csr_of(raw)
    for key in ("l0_offsets", "l0_neighbors", "level", "up_offsets", "up_neighbors"):
        assert np.array_equal(back[key], ex[key]) and np.array_equal(ex[key], g[key]), key
    assert (raw["entry"], raw["has_entry"], raw["max_layer"]) == (ex["entry_point"], 1, ex["max_layer"]) and raw["dead"] is None
    t, _ = check(gix)
    assert all(t[k] == 0 for k in DEFECTS) and t["unreachable_l0"] == 0 and t == tw.audit(raw, reverse="membership")
    assert t["nodes"] == n and t["edges_l0"] == g["l0_neighbors"].size and t["edges_up"] == g["up_neighbors"].size > 0
    assert t["up_rows"] == int(g["level"].sum()) and t["bfs_levels_l0"] >= 2
    if name == "wide96":
        assert t["max_degree_l0"] == 70


# ---- one defect kind at a time ------------------------------------------------------------------------------------------------------------

def plant(P, kind, layer, u, where):
    """one defect of `kind` in node u's row on `layer`, at slot 0 / the middle slot / the last slot of the stride.  Returns the counter it
    aims at.  The row is first grown to the whole stride (symmetrically), so that every slot up to the last one holds an id."""
    stride = P.stride(layer)
    p = {"first": 0, "middle": stride // 2 - 1, "last": stride - 1}[where]
    a = P.fill_row(layer, u)
    q = max(p, 1)  # the defects that need a predecessor sit in slots (0, 1) when they are planted "at slot 0"
    if kind == "duplicate":
        a[q] = a[q - 1]
        aim = "unsorted_entries"
    elif kind == "descending":
        a[q - 1], a[q] = a[q], a[q - 1]
        aim = "unsorted_entries"
    elif kind == "hole":
        a[q - 1] = S
        aim = "holes"
    elif kind == "self_loop":
        a[p] = u
        aim = "self_loops"
    elif kind == "id_n":
        a[p] = P.n
        aim = "out_of_range_ids"
    elif kind == "id_fffffffe":
        a[p] = 0xFFFFFFFE
        aim = "out_of_range_ids"
    elif kind == "one_way":
        v = a[p]
        P.set_row(layer, v, [x for x in P.ids(layer, v) if x != u])  # u -> v stays, v -> u is gone; both rows stay canonical
        return "asymmetric_edges_up" if layer else "asymmetric_edges_l0"
    elif kind == "below_layer":
        a[p] = next(v for v in range(1, P.n) if P.level[v] == layer - 1 and v != u)
        aim = "level_violations"
    else:
        raise AssertionError(kind)
    P.set_row(layer, u, a)
    return aim


def places(P, layer):
    """(node, layer, slot): the first and the last row of the array, a row in the middle; slot 0, the middle slot, the last slot"""
    if layer == 0:
        rows = [(0, 0), (P.n // 2 + 1, 0), (P.n - 1, 0)]
    else:
        last = max(u for u in range(P.n) if P.level[u])
        rows = [(0, 1), (P.n // 2 - P.n // 2 % 10, 2), (last, P.level[last])]  # upper row 0, a layer-2 row, the last upper row
    return [(u, L, where) for u, L in rows for where in ("first", "middle", "last")]


L0_KINDS = ["duplicate", "descending", "hole", "self_loop", "id_n", "id_fffffffe", "one_way"]
UP_KINDS = ["one_way", "below_layer", "duplicate", "hole", "id_n"]


@pytest.mark.parametrize("kind,layer", [(k, 0) for k in L0_KINDS] + [(k, 1) for k in UP_KINDS])
@pytest.mark.parametrize("name", list(IMAGES))
def test_one_planted_defect_is_counted_like_the_twin_counts_it(hv, name, kind, layer):
    gix, _ = image(hv, name)
    P = Planter(gix)
    try:
        for u, L, where in places(P, layer):
            aim = plant(P, kind, L, u, where)
            t, raw = check(gix, P)
            assert t[aim] > 0, (aim, u, L, where, t)
            if kind == "one_way":  # every row is still canonical: the binary search is plain membership, and exactly one edge is one-way
                assert t == tw.audit(raw, reverse="membership") and t[aim] == 1 and t["unsorted_entries"] == t["holes"] == 0
            if name != "m12":
                assert t["degree_overflow_rows"] == 0
            P.restore()
        t, _ = check(gix, P)
        assert all(t[k] == 0 for k in DEFECTS)
    finally:
        P.restore()


@pytest.mark.parametrize("layer", [0, 1])
def test_a_row_of_one_id_above_the_limit_overflows(hv, layer):
    """m = 12, m0 = 24 under strides of 16 / 32: the only image whose rows can hold more ids than the limit.  limit + 1 ids overflow, limit ids
    do not; the rows stay canonical and symmetric."""
    gix, _ = image(hv, "m12")
    P = Planter(gix)
    limit = 12 if layer else 24
    try:
        for u, L, _ in places(P, layer)[::3]:
            P.fill_row(L, u, count=limit)
            t, _ = check(gix, P)
            assert t["degree_overflow_rows"] == 0 and t["max_degree_up" if L else "max_degree_l0"] == limit
            P.fill_row(L, u, count=limit + 1)
            t, raw = check(gix, P)
            assert t["degree_overflow_rows"] == 1 and t["max_degree_up" if L else "max_degree_l0"] == limit + 1
            assert all(t[k] == 0 for k in DEFECTS if k != "degree_overflow_rows") and t == tw.audit(raw, reverse="membership")
            P.restore()
    finally:
        P.restore()


def test_ids_in_the_spare_rows_of_a_reserved_image_change_nothing(hv):
    gix, _ = image(hv, "reserved")
    before, raw = check(gix)
    n, up_rows = raw["n"], raw["up"].shape[0]
    assert raw["cap_rows"] == n + 8 and raw["cap_up_rows"] == up_rows + 4
    spare = [(False, n, 0, 0), (False, n, 1, 0), (False, n + 7, 31, n + 7), (False, n + 3, 5, n), (True, up_rows, 0, 0), (True, up_rows + 3, 15, 0xFFFFFFFE)]
    try:
        for upper, row, slot, value in spare:
            ah.write(gix, upper, row, slot, value)
        after, raw2 = check(gix)
        assert after == before and raw2["n"] == n and np.array_equal(raw2["l0"], raw["l0"]) and np.array_equal(raw2["up"], raw["up"])
    finally:
        for upper, row, slot, _ in spare:
            ah.write(gix, upper, row, slot, S)


# ---- mixed defects ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("name", ["f32_m16", "wide96"])
def test_a_seeded_mix_of_defects_is_counted_like_the_twin_counts_it(hv, name, seed):
    """200 single-slot writes of every kind, on both arrays, near the ids of the rows they hit: the defects overlap (a hole inside an unsorted
    row that is also searched for a reverse edge), so the comparison is with the twin's lower-bound look-up -- membership gives other figures"""
    gix, _ = image(hv, name)
    P = Planter(gix)
    rng = np.random.default_rng(seed)
    owner = {int(P.raw["up_base"][u]) + L - 1: (u, L) for u in range(P.n) for L in range(1, P.level[u] + 1)}
    try:
        for i in range(200):
            kind, upper = i % 8, (i // 8) % 3 == 0
            arr = P.raw["up" if upper else "l0"]
            r = int(rng.integers(arr.shape[0]))
            u, L = owner[r] if upper else (r, 0)
            deg = int((arr[r] != S).sum())
            slot = int(rng.integers(0, min(deg + 2, arr.shape[1])))
            if kind == 0:
                value = int(rng.integers(P.n))
            elif kind == 1:
                value = int(arr[r, slot - 1]) if slot else int(arr[r, 1])           # a duplicate (or, behind the ids, an erased slot)
            elif kind == 2:
                value = S
            elif kind == 3:
                value = u
            elif kind == 4:
                value = P.n
            elif kind == 5:
                value = 0xFFFFFFFE
            elif kind == 6:
                value = int(rng.integers(P.n // 10)) * 10 + 1                        # a node of level 0
            else:
                slot, value = arr.shape[1] - 1, int(rng.integers(P.n))              # the last slot of the stride
            ah.write(gix, upper, r, slot, value)
            arr[r, slot] = value
        t, raw = check(gix, P)
        for key in DEFECTS[:7]:
            assert t[key] > 0, (key, t)
        assert t != tw.audit(raw, reverse="membership")
    finally:
        P.restore()
    t, _ = check(gix, P)
    assert all(t[k] == 0 for k in DEFECTS)


# ---- the smallest images ------------------------------------------------------------------------------------------------------------------

def test_an_empty_image_returns_before_any_launch(hv):
    gix = hv.ValidatedVectorReadIndex.managed(dim=32, metric=hv.EUCLIDEAN, node_ids=np.zeros(0, np.uint64), vectors=np.zeros((0, 32), np.float32),
                                              l0_offsets=np.zeros(1, np.uint64), l0_neighbors=np.zeros(0, np.uint64))
    raw = ah.dump(gix)
    assert raw["n"] == 0 and raw["l0"].shape[0] == 0 and raw["up"].shape[0] == 0 and raw["has_entry"] == 0
    t, _ = check(gix)
    assert t == dict.fromkeys(tw.KEYS, 0)


@pytest.mark.parametrize("n", [1, 2, 9])
def test_images_of_one_two_and_nine_rows(hv, n):
    """n = 9 at stride 32: the last row is the first that starts in a second 256-thread block"""
    g = base_graph(n, 50 + n)
    gix = import_graph(hv, g, 32, 3, m=16, m0=32)
    t, raw = check(gix)
    assert (raw["n"], raw["s0"]) == (n, 32) and t["nodes"] == n and all(t[k] == 0 for k in DEFECTS) and t["unreachable_l0"] == 0
    assert t["bfs_levels_l0"] == {1: 0, 2: 1, 9: 2}[n]                        # (9: a ring with steps of 1 and 2 -- node 4 is two steps from 0)
    P = Planter(gix)
    u = n - 1
    deg = len(P.ids(0, u))
    ah.write(gix, False, u, deg, u)          # a self loop behind the row's ids (above every one of them: the row stays ascending)
    ah.write(gix, False, u, 31, n)           # id == n in the last slot of the stride, behind padding
    t, raw = check(gix)
    assert t["self_loops"] == 1 and t["out_of_range_ids"] == 1 and t["holes"] == 1 and t["unsorted_entries"] == 0 and t["edges_l0"] == g["l0_neighbors"].size + 2
    ah.write(gix, False, u, deg + 1, u)      # ... and the self loop twice
    t, raw = check(gix)
    assert t["self_loops"] == 2 and t["unsorted_entries"] == 1 and t["holes"] == 1 and t["max_degree_l0"] >= deg + 3


# ---- reachability -------------------------------------------------------------------------------------------------------------------------

def path_rows(lo, hi):
    return {u: [v for v in (u - 1, u + 1) if lo <= v < hi] for u in range(lo, hi)}


def ring_rows(lo, hi):
    k = hi - lo
    return {u: sorted({lo + (u - lo - 1) % k, lo + (u - lo + 1) % k}) for u in range(lo, hi)}


def reach_cases():
    n = 300
    one_way = path_rows(0, n - 1)
    one_way[n - 2] = [n - 3, n - 1]
    one_way[n - 1] = []
    empty_entry = path_rows(1, n)
    empty_entry[0] = []
    return {  # name: rows, entry point, then the figures counted by hand: bfs_levels_l0, unreachable_l0, asymmetric_edges_l0
        "path_from_its_end": (path_rows(0, n), 0, 299, 0, 0),
        "path_from_its_middle": (path_rows(0, n), 150, 150, 0, 0),
        "ring": (ring_rows(0, n), 0, 150, 0, 0),
        "two_components": ({**path_rows(0, 200), **ring_rows(200, n)}, 0, 199, 100, 0),
        "behind_a_one_way_edge": (one_way, 0, 299, 0, 1),
        "no_entry_point": (path_rows(0, n), None, 0, 300, 0),
        "entry_point_with_an_empty_row": (empty_entry, 0, 0, 299, 0),
    }


@pytest.mark.parametrize("case", list(reach_cases()))
def test_reachability_of_hand_made_layer0_rows(hv, case):
    rows, entry, levels, unreachable, one_way = reach_cases()[case]
    n = len(rows)
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(rows[u]) for u in range(n)])
    g = {"l0_offsets": off, "l0_neighbors": np.asarray([x for u in range(n) for x in rows[u]], np.uint64), "level": None, "up_offsets": None,
         "up_neighbors": None, "entry_point": entry, "max_layer": 0}
    gix = import_graph(hv, g, 32, 5, m=16, m0=32)
    t, raw = check(gix)
    assert (t["bfs_levels_l0"], t["unreachable_l0"], t["asymmetric_edges_l0"]) == (levels, unreachable, one_way)
    assert t["has_entry"] == (0 if entry is None else 1) and t["nodes"] == n and t == tw.audit(raw, reverse="membership")
    assert t["bfs_levels_l0"] > 0 or t["unreachable_l0"] > 0


# ---- deleted rows -------------------------------------------------------------------------------------------------------------------------

def test_deleted_rows_dangling_edges_and_a_revived_node(hv):
    """An image built on the device, 40 nodes deleted: the twin of the dump equals the audit with nothing planted (nodes, edges_*, max_degree_*
    and unreachable_l0 are the figures that depend on how deleted rows are treated).  Then an edge to a deleted row (out of range, not
    asymmetric), ids in a deleted node's own emptied row (walked like any other row), and an upsert of a deleted id."""
    import fixtures as fx
    n, dim, m, m0 = 600, 64, 16, 32
    rng = np.random.default_rng(8800)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    lv = fx.draw_levels(n, m, seed=88)
    ids = np.arange(n, dtype=np.uint64)
    gix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids, vectors=data, levels=lv, m=m, m0=m0, ef_construction=64)
    t, raw = check(gix)
    assert raw["dead"] is None and t["nodes"] == n and all(t[k] == 0 for k in DEFECTS)
    on_layer1 = [u for u in range(n) if lv[u] == 1]
    gone = on_layer1[:2] + [int(x) for x in rng.permutation(n) if int(x) not in on_layer1[:2]][:38]   # (two of them live on layer 1)
    assert gix.delete_batch(np.asarray(gone, np.uint64))["deleted"] == 40
    t0, raw = check(gix)
    assert raw["dead"] is not None and sorted(u for u in range(n) if tw.is_dead(raw, u)) == sorted(gone)
    print("after 40 deletes:", t0)
    # (rows after deletes equal the oracle's row for row, tests/test_gpu_delete.py, and that file does not hold them to symmetry either:
    # a relink's prune leaves one-way edges behind.  The asymmetric counts of this image are the base the plants below add to.)
    canonical = ("unsorted_entries", "self_loops", "out_of_range_ids", "holes", "level_violations", "degree_overflow_rows")
    assert t0["nodes"] == n - 40 and all(t0[k] == 0 for k in canonical) and t0 == tw.audit(raw, reverse="membership")
    a0, au = t0["asymmetric_edges_l0"], t0["asymmetric_edges_up"]
    assert all(not (raw["l0"][d] != S).any() for d in gone)                    # a deleted node's row is emptied
    P = Planter(gix)
    d1, d2 = gone[0], gone[1]
    # (1) a live node with room lists a deleted one, in ascending order
    u = next(v for v in range(n) if v not in gone and len(P.ids(0, v)) < P.s0)
    P.set_row(0, u, sorted(P.ids(0, u) + [d1]))
    t1, _ = check(gix, P)
    assert t1["out_of_range_ids"] == 1 and t1["asymmetric_edges_l0"] == a0 and t1["edges_l0"] == t0["edges_l0"] + 1 and t1["unsorted_entries"] == 0
    P.restore()
    # ... and the same on layer 1
    w = next(v for v in on_layer1 if v not in gone and len(P.ids(1, v)) < P.su)
    P.set_row(1, w, sorted(P.ids(1, w) + [d1]))
    t1, _ = check(gix, P)
    assert t1["out_of_range_ids"] == 1 and t1["asymmetric_edges_up"] == au and t1["edges_up"] == t0["edges_up"] + 1 and t1["level_violations"] == 0
    P.restore()
    # (2) three live ids in the deleted node's own row: three edges nobody returns; the row counts for max_degree, the node for nothing
    live = [v for v in range(n) if v not in gone][:3]
    P.set_row(0, d1, live)
    t2, _ = check(gix, P)
    assert t2["edges_l0"] == t0["edges_l0"] + 3 and t2["asymmetric_edges_l0"] == a0 + 3 and t2["out_of_range_ids"] == 0 and t2["nodes"] == n - 40
    assert t2["unreachable_l0"] == t0["unreachable_l0"]
    # (3) another deleted id comes back (nobody lists d1, so the insert never meets the planted row)
    gix.upsert_batch([d2], data[d2:d2 + 1], [int(lv[d2])], ef_construction=64)
    t3, raw = check(gix)
    assert t3["nodes"] == n - 39 and not tw.is_dead(raw, d2) and tw.is_dead(raw, d1) and (raw["l0"][d2] != S).any()
    print("after the upsert:", t3)
    assert all(t3[k] == 0 for k in canonical) and t3["edges_l0"] > t2["edges_l0"]
