"""Every build of the HNSW search kernels that plan_wave() (helix-db_amd/csrc/hvx_hnsw_plan.h) can pick runs here once and is held to
the oracle: ids, score BITS, the SearchStats counters, `tie_overflow_queries == 0`.  No tolerance anywhere.  The cases are the table
tests/hnsw_cover_cases.py; tests/test_hnsw_cover_ledger.py shows without a GPU that they reach all 566 instantiations, and
tests/hnsw_cover_table.txt says which case runs which.  One test per GROUP (an index shape): one oracle graph serves its ~30 launches.

Per group: n = 1 500 clustered rows (bf16 groups: the oracle holds the rounded rows, the device rounds), inserted by the oracle with
efc 60; 16 queries per launch -- 4 stored rows, 4 stored rows moved by one ulp, 8 fresh ones; every launch is repeated on half the
batch, which only agrees if the first launch handed the visited state back clean.

The re-run with the wider beam.  The re-run kernel launches after every search whose beam has a wider sibling and leaves at once when
nobody is listed, so equal results alone do not show that it ever worked.  Its cases search a second corpus over the SAME graph:
sparse 0/1 rows of one weight, and 0/1 queries built so that ~100 (or ~200) rows score strictly better than all the others, which
tie exactly (integer dot products: every summation order gives the same bits, under each metric).  The graph knows nothing of these
rows, so a search meets the mass of tied rows first and the better ones later, one by one; each pushes a tied, unexpanded candidate
off a beam that is full of them: the beam's slack overflows, the query is listed, and the re-run's beam (ef + b < 384 resp. 832
entries) holds them all.  That the first rung really overflows is shown on the device: the general kernel has the same 192-entry
beam at ef 128, no re-run, and reports the flags (`tie_overflow_queries > 0`; bf16 groups: over an f32 image of the same values).
The release library has no such witness for the 384 -> 832 (generic: 448 -> 832) hop: that hop rests on the corpus alone, and on a
host model of the capped beam (`capped_beam_overflows`) that is itself held to the device's count at the first rung.

(Exact copies of a few vectors, the corpus of the older re-run tests, do not do this: an oracle graph over 70 copies of each of 40
vectors falls apart into cliques of 33 copies, a search computes 33 distances and no beam ever fills.)"""
import bisect

import numpy as np
import pytest

import fixtures as fx
import hnsw_cover_cases as cc
from test_gpu_parity import _oracle_params, assert_hnsw_equal, assert_params_equal, bits, build_oracle

pytestmark = pytest.mark.gpu

N = 1500


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def clustered_rows(n, dim, rng, centres):
    return (centres[rng.integers(0, centres.shape[0], n)] + 0.6 * rng.standard_normal((n, dim))).astype(np.float32)


def tie_rows(n, dim, rng):
    """0/1 rows of one weight"""
    w = max(3, int(round((dim / 12) ** 0.5)))
    idx = np.argsort(rng.random((n, dim)), axis=1)[:, :w]
    out = np.zeros((n, dim), np.float32)
    np.put_along_axis(out, idx, np.float32(1.0), axis=1)
    return out


def tie_query(rows, better, rng):
    """a 0/1 query whose support meets `better` rows or a few more: they score strictly better than all the others, which tie"""
    q = np.zeros(rows.shape[1], np.float32)
    hit = np.zeros(rows.shape[0], bool)
    for c in rng.permutation(rows.shape[1]):
        if hit.sum() >= better:
            break
        q[c] = 1.0
        hit |= rows[:, c] > 0
    return q


def capped_beam_overflows(ex, rows, q, ef, cap):
    """Host model of a strict search whose (score, id) beam holds `cap` entries (the layer-0 loop of hvx_hnsw.hip): True when an
    unexpanded candidate leaves the end of the full beam with a score that is not worse than the ef-th best.  `rows` are the 0/1
    rows of one weight: -dot orders them as every metric's score does, and exactly."""
    sc = -(rows @ q).astype(np.int64)
    off, nb, level = ex["l0_offsets"].astype(np.int64), ex["l0_neighbors"].astype(np.int64), ex["level"].astype(np.int64)
    uoff, unb = ex["up_offsets"].astype(np.int64), ex["up_neighbors"].astype(np.int64)
    base = np.concatenate([[0], np.cumsum(level)])
    cur = int(ex["entry_point"])
    for layer in range(int(ex["max_layer"]), 0, -1):   # greedy descent: the row's first minimum, if it improves
        seen, changed = {cur}, True
        while changed:
            changed = False
            if level[cur] < layer:
                break
            r = base[cur] + layer - 1
            fresh = [int(x) for x in unb[uoff[r]:uoff[r + 1]] if int(x) not in seen]
            seen.update(fresh)
            if fresh:
                best = min(fresh, key=lambda x: sc[x])   # (min keeps the first of equal scores)
                if sc[best] < sc[cur]:
                    cur, changed = best, True
    beam, expanded, visited, flagged = [(int(sc[cur]), cur)], set(), {cur}, False
    while True:
        pos = next((i for i, e in enumerate(beam) if e[1] not in expanded), None)
        if pos is None:
            break
        wl = min(len(beam), ef)
        wmax = beam[wl - 1][0]
        if wl >= ef and beam[pos][0] > wmax:
            break
        c = beam[pos][1]
        expanded.add(c)
        for x in nb[off[c]:off[c + 1]]:
            x = int(x)
            if x in visited:
                continue
            visited.add(x)
            e = (int(sc[x]), x)
            if e[0] < wmax or min(len(beam), ef) < ef:
                p = bisect.bisect_left(beam, e)
                drop = None
                if len(beam) == cap:
                    drop = e if p == cap else beam.pop()
                if drop is not e:
                    beam.insert(p, e)
                wmax = beam[min(len(beam), ef) - 1][0]
                if drop is not None and drop[1] not in expanded and drop[0] <= wmax:
                    flagged = True
    return flagged


def assert_params_equal_without_stats(orc, hv, oix, gix, queries, p, cfg):
    """the diagnostics-free build of the non-strict arms: ids, score bits, counts and status against the oracle"""
    ids, sc, cnt, stats, st = gix.search_batch(queries, p, per_query_status=True)
    op = _oracle_params(orc, p, cfg)
    for qi in range(queries.shape[0]):
        rc, oid, osc = oix.search_params(queries[qi], op)
        assert rc == orc.OK and st[qi] == 0, f"query {qi}: status {st[qi]}"
        assert cnt[qi] == oid.size, f"query {qi}: count {cnt[qi]} vs oracle {oid.size}"
        assert ids[qi, :cnt[qi]].tolist() == oid.tolist(), f"query {qi}: ids differ"
        assert bits(sc[qi, :cnt[qi]]).tolist() == bits(osc).tolist(), f"query {qi}: score bits differ"
    assert stats["tie_overflow_queries"] == 0


def run_case(orc, hv, c, oix, gix, q, cfg, shadow_pairs):
    gix.set_occupancy(c.occupancy)
    gix.set_option(hv.OPT_HNSW_PAIR, c.pair)
    gix.set_option(hv.OPT_WAVE_LOG2CAP, c.log2cap)
    gix.set_option(hv.OPT_HNSW_SHADOW_PRUNE, c.prune_off)
    for batch in (q, q[: q.shape[0] // 2]):   # the second launch: the visited state was handed back clean
        if c.arm == "strict":
            assert_hnsw_equal(orc, hv, oix, gix, batch, c.k, c.ef)
        else:
            p = hv.SearchParams.new(c.k).with_ef(c.ef)
            (assert_params_equal if c.stats else assert_params_equal_without_stats)(orc, hv, oix, gix, batch, p, cfg)
    if shadow_pairs is not None and c.arm == "strict" and c.occupancy == 2 and c.log2cap == 0 and c.corpus == "clustered":
        # with the bf16-shadow pre-pass and without it: everything identical, per query
        got = gix.search_batch_with_stats(q, hv.SearchParams(c.k).with_ef(c.ef))
        other = shadow_pairs.setdefault((c.ef, c.k), got)
        if other is not got:
            for a, b in zip(other[:4], got[:4]):
                assert bits(a).tolist() == bits(b).tolist() if a.dtype == np.float32 else a.tolist() == b.tolist()
            assert other[4] == got[4]
            for key in ("expansion_steps", "neighbors_examined", "vectors_loaded", "distance_computations", "tie_overflow_queries", "queries"):
                assert other[5][key] == got[5][key], key
            shadow_pairs[(c.ef, c.k)] = None


@pytest.mark.parametrize("group", [g.name for g in cc.GROUPS])
def test_every_build_the_plan_can_pick_equals_the_oracle(orc, hv, group):
    g = cc.group_named(group)
    cases = cc.cases_of(group)
    rng = np.random.default_rng(7100 + cc.GROUPS.index(g))
    bf = g.dtype == cc.BF16
    okernel = {cc.TREE_AVX: orc.K_AVX, cc.TREE_AVX_FMA: orc.K_AVX_FMA}[g.tree]
    kw = dict(dim=g.dim, metric=g.metric, m=g.m, m0=g.m0, float_kernel=g.tree)
    cfg = hv.SimHashConfig.default()

    # the clustered corpus and the group's one oracle graph
    centres = rng.standard_normal((24, g.dim)).astype(np.float32)
    data = clustered_rows(N, g.dim, rng, centres)
    stored = fx.round_bf16(data) if bf else data
    oix = build_oracle(orc, stored, g.metric, fx.draw_levels(N, g.m, seed=g.dim + g.metric), m=g.m, m0=g.m0, efc=60, kernel=okernel, cached=False)
    oix.set_simhash(int(cfg.seed))
    ex = oix.export()
    ex["vectors"] = data   # (bf16 groups: the device does the rounding)
    gix = hv.ValidatedVectorReadIndex.from_export(ex, dtype=hv.BF16 if bf else hv.F32, **kw)
    gix.set_simhash(cfg)
    at = rng.integers(0, N, 8)
    q = np.vstack([stored[at[:4]], np.nextafter(stored[at[4:]], np.float32(np.inf)), clustered_rows(8, g.dim, rng, centres)]).astype(np.float32)

    # the tie-heavy corpus over the same graph
    rows = tie_rows(N, g.dim, rng)
    tix = orc.Index(g.dim, g.metric, kernel=okernel, m=g.m, m0=g.m0, ef_construction=60)
    assert tix.seed(ex["node_ids"], rows, ex["l0_offsets"], ex["l0_neighbors"], level=ex["level"], up_offsets=ex["up_offsets"],
                    up_neighbors=ex["up_neighbors"], entry_point=ex["entry_point"], max_layer=ex["max_layer"]) == orc.OK
    tix.set_simhash(int(cfg.seed))
    tex = dict(ex)
    # bf16 groups: rows the device has to round (1.001 -> 1), the oracle holds the rounded ones
    tex["vectors"] = rows * np.float32(1.001) if bf else rows
    assert not bf or fx.round_bf16(tex["vectors"]).tobytes() == rows.tobytes()
    tgix = hv.ValidatedVectorReadIndex.from_export(tex, dtype=hv.BF16 if bf else hv.F32, **kw)
    tgix.set_simhash(cfg)
    tq = np.stack([tie_query(rows, 100 if i < 8 else 200, rng) for i in range(16)])

    shadow_pairs = {} if any(c.prune_off for c in cases) else None
    for c in cases:
        if c.corpus == "clustered":
            run_case(orc, hv, c, oix, gix, q, cfg, shadow_pairs)
        else:
            run_case(orc, hv, c, tix, tgix, tq, cfg, None)
    assert shadow_pairs is None or (shadow_pairs and all(v is None for v in shadow_pairs.values())), "a shadow case without its twin"

    # the witness: the first launch of the tie cases overflows its beam's slack, so their re-run launches had queries to search
    wgix = tgix
    if bf:
        wex = dict(ex)
        wex["vectors"] = rows
        wgix = hv.ValidatedVectorReadIndex.from_export(wex, dtype=hv.F32, **kw)
    wgix.set_option(hv.OPT_HNSW_GENERAL_KERNEL, 1)
    first_ef = min(c.ef for c in cases if c.corpus == "ties")
    assert first_ef + 32 <= 192
    _, _, _, wstats = wgix.search_batch(tq, hv.SearchParams(10).with_ef(first_ef))
    wgix.set_option(hv.OPT_HNSW_GENERAL_KERNEL, 0)
    model = sum(capped_beam_overflows(ex, rows, tq[i], first_ef, 192) for i in range(16))
    print(f"{group}: first rung, ef {first_ef}: the device flags {wstats['tie_overflow_queries']} of 16 queries, the host model {model}")
    assert wstats["tie_overflow_queries"] > 0
    assert model == wstats["tie_overflow_queries"]
    # the wider hop (no device witness): the host model of its beam
    for ef, cap in sorted({(c.ef, 448 if g in cc.GENERIC_GROUPS else 384) for c in cases if c.corpus == "ties" and c.ef != first_ef}):
        wide = sum(capped_beam_overflows(ex, rows, tq[i], ef, cap) for i in range(16))
        print(f"{group}: ef {ef}: the host model of the {cap}-entry beam flags {wide} of 16 queries")
        assert wide > 0
