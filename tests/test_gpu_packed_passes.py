"""The distance passes of the HNSW beam in their packed form (hvx_hnsw_wave.h: fma_chunk on register pairs, gather_consume,
shadow_pass): two elements per subtract and per fused multiply-add.  Element by element these are the component-wise operations, so
nothing may move: ids, score BITS and the four SearchStats counters of every query equal the oracle's.  No tolerance anywhere.

Shapes.  4 096 rows, 16 queries, k 10, ef 48 (the 192-entry beam) and ef 160 (the 384-entry beam); dims 128, 768 and 1536; squared-
Euclidean and cosine; f32 and bf16 rows; one and two queries per SIMD; the pair kernel on and off; for the strict squared-Euclidean f32
builds the bf16 shadow pre-pass on and off.  ONE graph serves everything: the oracle builds it over the rows' first 32 elements (a
second or two; the full rows would take that long per case), and every corpus carries most of its spread in those elements, so the
graph is a fair one for all of them.  What is compared is the search; both sides search the same graph.

Rows.  Gaussian, then planted: elements +0 and -0, subnormals, elements near 2^-60, elements at the largest magnitude near 2^60 the
metric admits (squared-Euclidean: 0.99 of the oracle's component limit, 2^57.2 to 2^59 at these dims; cosine has no limit: 2^60), and
exact copies of rows at other nodes (exact ties under both metrics).  The queries include stored rows, copies, rows moved by one ulp,
the large rows scaled by 0.999, and fresh ones.

Pass widths.  Which pass a frontier takes depends on its length and on whether the beam is full (hvx_hnsw_wave.h: score_frontier,
shadow_prune).  A host replay of the strict search over the same graph, with the oracle's own scores, yields every expansion's
frontier length and beam fill; it is held to the DEVICE's per-query counters (qstats) on every query, so it walked the path the
kernel walked.  From it, at dim 768 with two queries per SIMD: full-beam frontiers of 1-8, 9-16 and 17+ rows (shadow passes of one,
two and three rows per 8-lane group) all occur, and so do frontiers of 1-8 and of 9+ rows (with the pre-pass off every frontier is
scored whole: f32 passes of one and of two rows per group; with it on the same holds until the beam is full).  Run with `-m gpu` on
an MI355X."""
import heapq

import numpy as np
import pytest

import fixtures as fx
from test_gpu_parity import bits, build_oracle

pytestmark = pytest.mark.gpu

N, NQ, K, M, GRAPH_DIM = 4096, 16, 10, 16, 32
EFS = (48, 160)
COUNTERS = ("expansion_steps", "neighbors_examined", "vectors_loaded", "distance_computations")


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


_GRAPH = {}


def shared_graph(orc):
    """the oracle's graph over the rows' first 32 elements: built once, seeded into every index of this file"""
    if not _GRAPH:
        base = np.random.default_rng(4242).standard_normal((N, GRAPH_DIM)).astype(np.float32)
        oix = build_oracle(orc, base, orc.L2SQ, fx.draw_levels(N, M, seed=11), m=M, m0=2 * M, efc=60)
        _GRAPH["base"] = base
        _GRAPH["ex"] = oix.export()
    return _GRAPH["base"], _GRAPH["ex"]


def corpus(orc, base, dim, cosine, rng):
    """rows whose first 32 elements are the graph's (scaled up: most of a distance comes from them), the rest Gaussian; then the
    planted elements and copies.  Returns rows, the nodes of the large rows and the (copy, original) node pairs."""
    data = (rng.standard_normal((N, dim)) * 0.35).astype(np.float32)
    data[:, :GRAPH_DIM] = base * np.float32(1.5)
    big = np.float32(2.0 ** 60) if cosine else np.float32(min(2.0 ** 60, 0.99 * float(orc.lib().orc_component_limit(orc.L2SQ, dim))))
    rows = rng.choice(N, 200, replace=False)
    for t, r in enumerate(rows[:160]):
        cols = rng.choice(dim, 1 + t % 7, replace=False)
        kind = t % 5
        if kind == 0:
            data[r, cols] = np.float32(0.0)
        elif kind == 1:
            data[r, cols] = np.float32(-0.0)
        elif kind == 2:
            data[r, cols] = (rng.integers(1, 1 << 23, cols.size).astype(np.uint32)).view(np.float32) * np.float32(1 - 2 * (t % 2))  # subnormals
        elif kind == 3:
            data[r, cols] = np.float32(2.0 ** -60) * rng.uniform(0.5, 2.0, cols.size).astype(np.float32)
        else:
            data[r, cols] = big * np.float32(1 - 2 * (t % 2))
    large = rows[4:160:5]
    pairs = [(int(rows[160 + i]), int(rows[180 + i])) for i in range(20)]
    for dst, src in pairs:
        data[dst] = data[src]
    return data, large, pairs


def queries(stored, large, pairs, dim, rng):
    q = np.vstack([stored[[pairs[0][1], pairs[1][0], int(rng.integers(0, N)), int(rng.integers(0, N))]],
                   np.nextafter(stored[rng.integers(0, N, 2)], np.float32(np.inf)),
                   stored[large[:2]] * np.float32(0.999),
                   (rng.standard_normal((8, dim)) * 0.35).astype(np.float32)]).astype(np.float32)
    q[8:, :GRAPH_DIM] = (rng.standard_normal((8, GRAPH_DIM)) * 1.5).astype(np.float32)
    assert q.shape[0] == NQ
    return q


def replay(ex, score, ef):
    """The strict search on the exported graph with the oracle's scores of one query (score[node], f32): greedy descent, then the
    layer-0 beam ordered by (score, id) -- node == id here.  Returns the four counters and, per expansion with a non-empty frontier,
    (frontier rows, beam full at that point)."""
    off, nb, level = ex["l0_offsets"].astype(np.int64), ex["l0_neighbors"].astype(np.int64), ex["level"].astype(np.int64)
    uoff, unb = ex["up_offsets"].astype(np.int64), ex["up_neighbors"].astype(np.int64)
    ubase = np.concatenate([[0], np.cumsum(level)])
    cur = int(ex["entry_point"])
    for layer in range(int(ex["max_layer"]), 0, -1):
        seen, cur_d = {cur}, score[cur]
        while True:
            changed = False
            row = []
            if level[cur] >= layer:
                r = ubase[cur] + layer - 1
                row = unb[uoff[r]:uoff[r + 1]]
            for x in row:  # the list loaded for the node current at loop entry
                x = int(x)
                if x in seen:
                    continue
                seen.add(x)
                if score[x] < cur_d:
                    cur, cur_d, changed = x, score[x], True
            if not changed:
                break
    st = dict.fromkeys(COUNTERS, 0)
    st["distance_computations"] = 1
    cand, beam, seen, passes = [(score[cur], cur)], [(-score[cur], -cur)], {cur}, []  # min-heap; max-heap of (score, id)
    while cand:
        st["expansion_steps"] += 1
        d, c = heapq.heappop(cand)
        if len(beam) >= ef and d > -beam[0][0]:
            break
        row = nb[off[c]:off[c + 1]]
        st["neighbors_examined"] += len(row)
        fr = [int(x) for x in row if int(x) not in seen]
        if not fr:
            continue
        seen.update(fr)
        st["vectors_loaded"] += len(fr)
        st["distance_computations"] += len(fr)
        passes.append((len(fr), len(beam) >= ef))
        for x in fr:
            if score[x] < -beam[0][0] or len(beam) < ef:
                heapq.heappush(cand, (score[x], x))
                heapq.heappush(beam, (-score[x], -x))
                if len(beam) > ef:
                    heapq.heappop(beam)
    return st, passes


CASES = [(dim, metric, dtype) for dim in (128, 768, 1536) for metric in ("l2", "cosine") for dtype in ("f32", "bf16")]


@pytest.mark.parametrize("dim,metric,dtype", CASES, ids=[f"{d}-{m}-{t}" for d, m, t in CASES])
def test_packed_passes_equal_the_oracle(orc, hv, dim, metric, dtype):
    cosine, bf = metric == "cosine", dtype == "bf16"
    base, gex = shared_graph(orc)
    rng = np.random.default_rng(8800 + dim + 2 * cosine + bf)
    data, large, pairs = corpus(orc, base, dim, cosine, rng)
    stored = fx.round_bf16(data) if bf else data
    for dst, src in pairs:
        assert stored[dst].tobytes() == stored[src].tobytes()
    ometric, hmetric = (orc.COSINE, hv.COSINE) if cosine else (orc.L2SQ, hv.EUCLIDEAN)
    oix = orc.Index(dim, ometric, kernel=orc.K_AVX_FMA, m=M, m0=2 * M, ef_construction=60)
    assert oix.seed(gex["node_ids"], stored, gex["l0_offsets"], gex["l0_neighbors"], level=gex["level"], up_offsets=gex["up_offsets"],
                    up_neighbors=gex["up_neighbors"], entry_point=gex["entry_point"], max_layer=gex["max_layer"]) == orc.OK
    ex = dict(gex)
    ex["vectors"] = stored
    gix = hv.ValidatedVectorReadIndex.from_export(ex, dim=dim, metric=hmetric, m=M, m0=2 * M, dtype=hv.BF16 if bf else hv.F32)
    q = queries(stored, large, pairs, dim, rng)
    strict_l2_f32 = not cosine and not bf

    for ef in EFS:
        want = [oix.search(q[qi], K, ef, with_stats=True) for qi in range(NQ)]  # computed once, shared by every launch below
        assert all(w[0] == orc.OK for w in want)
        first = None
        for occ in (1, 2):
            for pair_off in (0, 1):
                for prune_off in ((0, 1) if strict_l2_f32 else (0,)):
                    gix.set_occupancy(occ)
                    gix.set_option(hv.OPT_HNSW_PAIR, pair_off)
                    gix.set_option(hv.OPT_HNSW_SHADOW_PRUNE, prune_off)
                    ids, sc, cnt, st, per_query, tot = gix.search_batch_with_stats(q, hv.SearchParams(K).with_ef(ef))
                    where = f"ef {ef} occupancy {occ} pair_off {pair_off} prune_off {prune_off}"
                    for qi, (rc, oid, osc, ost) in enumerate(want):
                        c = int(cnt[qi])
                        assert st[qi] == 0 and c == oid.size, f"{where} query {qi}: status {st[qi]}, count {c} vs {oid.size}"
                        assert ids[qi, :c].tolist() == oid.tolist(), f"{where} query {qi}: ids differ from the oracle"
                        assert bits(sc[qi, :c]).tolist() == bits(osc).tolist(), f"{where} query {qi}: score bits differ from the oracle"
                        for key in COUNTERS:
                            assert per_query[qi][key] == ost[key], f"{where} query {qi}: {key} {per_query[qi][key]} vs {ost[key]}"
                    for key in COUNTERS:
                        assert tot[key] == sum(w[3][key] for w in want), f"{where}: {key}"
                    assert tot["tie_overflow_queries"] == 0, where
                    if first is None:
                        first = per_query
        if dim == 768 and strict_l2_f32:
            # the pass widths this corpus reaches, from the replay held to the device's counters
            shadow, plain = set(), set()
            for qi in range(NQ):
                _, aid, asc = oix.flat(q[qi], N)
                score = np.empty(N, np.float32)
                score[aid.astype(np.int64)] = asc
                rst, passes = replay(gex, score, ef)
                for key in COUNTERS:
                    assert rst[key] == first[qi][key], f"ef {ef} query {qi}: the replay's {key} {rst[key]} vs the device's {first[qi][key]}"
                for nf, full in passes:
                    plain.add(min((nf + 7) // 8, 2))
                    if full:
                        shadow.add(min((nf + 7) // 8, 3))
            print(f"dim {dim} ef {ef}: shadow passes of {sorted(shadow)} rows per group, f32 passes of {sorted(plain)}")
            assert shadow == {1, 2, 3}, f"ef {ef}: full-beam frontiers reach shadow passes of {sorted(shadow)} rows per group only"
            assert plain == {1, 2}, f"ef {ef}: the frontiers reach f32 passes of {sorted(plain)} rows per group only"
    gix.set_option(hv.OPT_HNSW_PAIR, 0)
    gix.set_option(hv.OPT_HNSW_SHADOW_PRUNE, 0)
    gix.close()
