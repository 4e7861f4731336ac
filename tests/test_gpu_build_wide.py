"""Device build, insert, upsert and link step for M = 32 / M0 = 64, the reference's scale configuration (scale_contracts.rs:167-173;
csrc/hvx_build_wide.hip), against the oracle's restatement of the reference's sequential insertion.  Every test first asserts on the
ORACLE's export that its case holds full rows: an append to a full row goes through the 65-id (33-id) prune, and a graph without full
rows would pass a row-for-row comparison without running the wide kernels."""
import numpy as np
import pytest

import fixtures as fx
from test_gpu_build import oracle_build, rows_of, _rows_dict
from test_gpu_delete import assert_same_graph, bits

pytestmark = pytest.mark.gpu

M, M0 = 32, 64


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def wide_inputs(n, dim, metric, lm):
    rng = np.random.default_rng(6400 + dim + metric)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64) * 2 + 3
    lv = fx.draw_levels(n, lm, seed=n + 1)
    return rng, data, ids, lv


def full_rows(ex, n, m=M, m0=M0):
    """(layer-0 rows with m0 ids, upper rows with m ids, upper rows) of an export"""
    l0, up = rows_of(ex, n)
    return sum(len(r) == m0 for r in l0), sum(len(r) == m for r in up), len(up)


def assert_rows_equal(g, ex, n):
    assert g["entry_point"] == ex["entry_point"] and g["max_layer"] == ex["max_layer"]
    assert g["level"].tolist() == ex["level"].tolist()
    gl0, gup = rows_of(g, n)
    ol0, oup = rows_of(ex, n)
    bad = [i for i in range(n) if gl0[i] != ol0[i]]
    assert not bad, f"{len(bad)} layer-0 rows differ, first {bad[:5]}: device {gl0[bad[0]]} oracle {ol0[bad[0]]}"
    badu = [r for r in range(len(oup)) if gup[r] != oup[r]]
    assert len(gup) == len(oup) and not badu, f"{len(badu)} upper rows differ, first {badu[:5]}"


def assert_searches_equal(hv, gix, oix, q, ef=64):
    gid, gsc, gcnt, _ = gix.search_batch(q, hv.SearchParams(10).with_ef(ef))
    for qi in range(q.shape[0]):
        rc, oid, osc = oix.search(q[qi], 10, ef)
        assert gid[qi, :gcnt[qi]].tolist() == oid.tolist()
        assert bits(gsc[qi, :gcnt[qi]]).tolist() == bits(osc).tolist()


SHAPES = [(900, 64, 1, 120, 4, True), (800, 128, 0, 120, 4, True), (1200, 128, 1, 100, 3, True), (600, 768, 1, 100, 32, False)]


@pytest.mark.parametrize("link_mode", [0, 1])
@pytest.mark.parametrize("n,dim,metric,efc,lm,upper", SHAPES)
def test_sequential_wide_build_equals_the_oracles_insertion_row_for_row(orc, hv, n, dim, metric, efc, lm, upper, link_mode):
    """sequential=True at M 32 / M0 64: every layer-0 row, every upper row, the entry point and the top layer equal the oracle's, with
    the default one-node steps and with link_mode=1 (the one-wavefront kernels); then 16 searches, ids and score bits."""
    rng, data, ids, lv = wide_inputs(n, dim, metric, lm)
    oix = oracle_build(orc, data, metric, lv, M, M0, efc, ids)
    ex = oix.export()
    f0, fu, nu = full_rows(ex, n)
    print(f"oracle: {f0} layer-0 rows with {M0} ids, {fu} of {nu} upper rows with {M} ids")
    assert f0 >= 100 and (fu >= 50 or not upper), (f0, fu, nu)
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids, vectors=data, levels=lv, m=M, m0=M0,
                                                ef_construction=efc, sequential=True, link_mode=link_mode)
    assert st["nodes"] == n and st["batches"] == n - 1
    assert_rows_equal(gix.export_graph(), ex, n)
    assert_searches_equal(hv, gix, oix, rng.standard_normal((16, dim)).astype(np.float32))
    gix.close()


GENERIC_N = 700


def test_sequential_wide_build_of_a_generic_shape_equals_the_oracle(orc, hv):
    """A shape outside the unrolled kernels: dim 100 (96 + a scalar tail of 4) under the scalar summation tree -- the generic build of
    the search kernel, the one-wavefront select and link kernels."""
    n, dim, metric, efc = GENERIC_N, 100, 1, 100
    rng, data, ids, lv = wide_inputs(n, dim, metric, 32)
    oix = oracle_build(orc, data, metric, lv, M, M0, efc, ids, kernel=orc.K_SCALAR)
    ex = oix.export()
    f0, fu, nu = full_rows(ex, n)
    print(f"oracle: {f0} layer-0 rows with {M0} ids, {fu} of {nu} upper rows with {M} ids")
    assert f0 >= 100, f0
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids, vectors=data, levels=lv, m=M, m0=M0,
                                                ef_construction=efc, sequential=True, float_kernel=hv.KERNEL_SCALAR)
    assert_rows_equal(gix.export_graph(), ex, n)
    assert_searches_equal(hv, gix, oix, rng.standard_normal((16, dim)).astype(np.float32))
    gix.close()


@pytest.mark.parametrize("n,dim,metric,efc,lm", [(900, 64, 1, 120, 4), (800, 128, 0, 120, 4)])
def test_sequential_wide_inserts_and_upserts_into_a_live_image_equal_the_oracle(orc, hv, n, dim, metric, efc, lm):
    """The first 2/3 built on the device with room to grow, the rest appended by insert_batch(sequential=True), then 40 live ids (the
    entry point among them) upserted with new vectors: rows, entry point and searches equal the oracle's insert / delete + insert."""
    rng, data, ids, lv = wide_inputs(n, dim, metric, lm)
    newv = rng.standard_normal((40, dim)).astype(np.float32)
    n0 = n * 2 // 3
    gix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids[:n0], vectors=data[:n0], levels=lv[:n0], m=M, m0=M0,
                                               ef_construction=efc, sequential=True, reserve_rows=n - n0, reserve_upper_rows=int(lv[n0:].sum()))
    oix = oracle_build(orc, data[:n0], metric, lv[:n0], M, M0, efc, ids[:n0])
    assert_rows_equal(gix.export_graph(), oix.export(), n0)
    for i in range(n0, n):
        assert oix.insert(int(ids[i]), data[i], int(lv[i])) == orc.OK
    ex = oix.export()
    f0, fu, nu = full_rows(ex, n)
    assert f0 >= 100 and fu >= 50, (f0, fu, nu)
    cuts = [n0, n0 + (n - n0) // 2, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        st = gix.insert_batch(ids[a:b], data[a:b], lv[a:b], ef_construction=efc, sequential=True)
        assert st["nodes"] == b - a and gix.rows() == b
    assert_rows_equal(gix.export_graph(), ex, n)
    ent = oix.entry()[0]
    targets = [int(x) for x in ids[rng.permutation(n)[:60]] if int(x) != ent][:39] + [ent]
    level_of = {int(ids[i]): int(lv[i]) for i in range(n)}
    for t, nid in enumerate(targets):
        assert oix.delete(nid) == (orc.OK, True)
        assert oix.insert(nid, newv[t], level_of[nid]) == orc.OK
    st = gix.upsert_batch(np.asarray(targets, np.uint64), newv, ef_construction=efc)
    assert st["nodes"] == len(targets) == 40 and gix.live_rows() == n == oix.count
    assert_same_graph(gix, oix, ids, ())
    assert_searches_equal(hv, gix, oix, np.vstack([rng.standard_normal((12, dim)).astype(np.float32), newv[:4]]))
    gix.close()


@pytest.mark.parametrize("metric", [1, 0])
def test_wide_inserts_and_upserts_into_a_bf16_image_equal_the_oracle_on_the_rounded_rows(orc, hv, metric):
    """A bf16 image with rows of 64 ids (an oracle graph over the rounded rows, imported with spare rows) takes one-node inserts and
    upserts: rows, entry point and searches equal the oracle's on the ROUNDED vectors."""
    n, dim, efc, lm = 800, 128, 120, 4
    rng, data, ids, lv = wide_inputs(n, dim, metric, lm)
    newv = rng.standard_normal((24, dim)).astype(np.float32)
    rounded, newr = fx.round_bf16(data), fx.round_bf16(newv)
    n0 = n * 2 // 3
    oix = oracle_build(orc, rounded[:n0], metric, lv[:n0], M, M0, efc, ids[:n0])
    ex0 = oix.export()
    ex0["vectors"] = data[:n0]
    gix = hv.ValidatedVectorReadIndex.from_export(ex0, dim=dim, metric=metric, dtype=hv.BF16, m=M, m0=M0, reserve_rows=n - n0,
                                                  reserve_upper_rows=int(lv[n0:].sum()))
    for i in range(n0, n):
        assert oix.insert(int(ids[i]), rounded[i], int(lv[i])) == orc.OK
    f0, fu, nu = full_rows(oix.export(), n)
    assert f0 >= 100 and fu >= 50, (f0, fu, nu)
    gix.insert_batch(ids[n0:], data[n0:], lv[n0:], ef_construction=efc)
    assert gix.live_rows() == n == oix.count
    assert_same_graph(gix, oix, ids, ())
    ent = oix.entry()[0]
    targets = [int(x) for x in ids[rng.permutation(n)[:40]] if int(x) != ent][:23] + [ent]
    level_of = {int(ids[i]): int(lv[i]) for i in range(n)}
    for t, nid in enumerate(targets):
        assert oix.delete(nid) == (orc.OK, True)
        assert oix.insert(nid, newr[t], level_of[nid]) == orc.OK
    st = gix.upsert_batch(np.asarray(targets, np.uint64), newv, ef_construction=efc)
    assert st["nodes"] == len(targets) and gix.live_rows() == n == oix.count
    assert_same_graph(gix, oix, ids, ())
    assert_searches_equal(hv, gix, oix, np.vstack([rng.standard_normal((12, dim)).astype(np.float32), newr[:4]]))
    gix.close()


@pytest.mark.parametrize("dim,metric,n", [(128, 1, 1500), (768, 1, 900), (1536, 1, 500), (128, 0, 1500), (768, 0, 900), (1536, 0, 500)])
def test_wide_link_workgroup_kernel_equals_the_oracles_prune_link_by_link(orc, hv, dim, metric, n):
    """The wide twin of test_link_workgroup_kernel_equals_the_oracles_prune_link_by_link: build_link_wide_wg_kernel driven one link at a
    time through hvx_index_link_rows against a host model whose every prune is the oracle's prune_candidates(to, row + [from], 64).
    Only targets whose row already holds 64 ids: every link prunes a list of 65.  Duplicate vectors (equal distances), repeated targets,
    links whose new node is itself dropped."""
    rng = np.random.default_rng(9100 + dim + metric)
    efc = 64
    centres = rng.standard_normal((12, dim)).astype(np.float32)
    data = (centres[rng.integers(0, 12, n)] + 0.35 * rng.standard_normal((n, dim))).astype(np.float32)
    for t in range(0, n, 9):          # duplicate vectors: ties in every distance that involves them
        data[t] = data[(t * 7 + 3) % n]
    lv = np.zeros(n, np.uint16)        # layer 0 only: the probe links layer-0 rows
    ids = np.arange(n, dtype=np.uint64) * 2 + 7
    oix = oracle_build(orc, data, metric, lv, M, M0, efc, ids)
    ex = oix.export()
    gix = hv.ValidatedVectorReadIndex.from_export(ex, dim=dim, metric=metric, m=M, m0=M0)
    rows = _rows_dict(ex, ids)
    full = [nid for nid in ids.tolist() if len(rows[nid]) == M0]
    assert len(full) >= 60, "the fixture must hold full rows (every link to one prunes)"
    links = []
    targets = [full[int(x)] for x in rng.choice(len(full), 200, replace=len(full) < 200)]
    targets += targets[:40]                                           # the same row again, after its first prune
    for to in targets:
        if len(rows[to]) != M0:                                       # (an earlier prune elsewhere took an id from it)
            continue
        while True:
            frm = int(ids[int(rng.integers(0, n))])
            if frm != to and frm not in rows[to]:
                break
        row = rows[to] + [frm]
        rc, keep = oix.prune_candidates(to, np.array(row, np.uint64), M0)
        assert rc == orc.OK
        keep = keep.tolist()
        for x in row:
            if x not in keep and to in rows[x]:                       # remove_edge_from_neighbor (mutation.rs:1890-1908)
                rows[x].remove(to)
        rows[to] = sorted(keep)
        links.append((frm, to))
    assert len(links) >= 150
    gix.link_rows([f for f, _ in links], [t for _, t in links], concurrent=False)
    got = _rows_dict(gix.export_graph(), ids)
    bad = [nid for nid in ids.tolist() if got[nid] != rows[nid]]
    assert not bad, f"{len(bad)} rows differ after {len(links)} links, first {bad[0]}: device {got[bad[0]]} model {rows[bad[0]]}"
    # the same links in ONE launch (the batched build's situation: undefined order): the row invariants hold afterwards
    gix2 = hv.ValidatedVectorReadIndex.from_export(ex, dim=dim, metric=metric, m=M, m0=M0)
    gix2.link_rows([f for f, _ in links], [t for _, t in links], concurrent=True)
    a = gix2.audit_graph()
    for key in ("unsorted_entries", "self_loops", "out_of_range_ids", "holes", "degree_overflow_rows", "level_violations"):
        assert a[key] == 0, (key, a)
    assert a["max_degree_l0"] <= M0
    gix.close()
    gix2.close()


def batched_wide_build(hv, n, dim, metric):
    rng = np.random.default_rng(8100 + dim)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    q = rng.standard_normal((1000, dim)).astype(np.float32)
    lv = fx.draw_levels(n, 32, seed=3)
    ids = np.arange(n, dtype=np.uint64)
    efc = 100
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids, vectors=data, levels=lv, m=M, m0=M0,
                                                ef_construction=efc, max_batch=512, batch_divisor=16)
    assert st["batches"] < n // 4
    g = gix.export_graph()
    top = int(lv.max())
    assert g["max_layer"] == top and lv[g["entry_point"]] == top
    l0, up = rows_of(g, n)
    edges = [set() for _ in range(top + 1)]
    for i in range(n):
        r = l0[i]
        assert r == sorted(set(r)) and i not in r and len(r) <= M0
        edges[0].update((i, t) for t in r)
    r_idx = 0
    for i in range(n):
        for layer in range(1, int(lv[i]) + 1):
            r = up[r_idx]
            r_idx += 1
            assert r == sorted(set(r)) and i not in r and len(r) <= M
            assert all(lv[t] >= layer for t in r)
            edges[layer].update((i, t) for t in r)
    for layer, es in enumerate(edges):
        asym = [(a, b) for (a, b) in es if (b, a) not in es]
        assert not asym, f"layer {layer}: {len(asym)} one-directional edges, e.g. {asym[:3]}"
    assert sum(len(r) == M0 for r in l0) >= 100                      # rows that went through the 65-id prune
    a = gix.audit_graph()
    for key in ("asymmetric_edges_l0", "asymmetric_edges_up", "unsorted_entries", "self_loops", "out_of_range_ids", "holes",
                "level_violations", "degree_overflow_rows"):
        assert a[key] == 0, (key, a)
    assert a["nodes"] == n and a["max_degree_l0"] <= M0 and a["max_degree_up"] <= M
    return gix, data, q, lv, ids, efc


def test_batched_wide_build_invariants_and_graph_quality(orc, hv):
    """8 000 x 128 L2 Gaussian rows in batches (one workgroup per link, build_link_wide_wg_kernel): rows canonical, degree-bounded and
    symmetric on every layer, entry on the top layer, audit clean; and the graph is as good as the oracle's sequential one: recall@10
    against the exact scan over 1 000 Gaussian queries, the device's graph searched on the device, the oracle's by the oracle, at ef 32
    and ef 64 (where the oracle's graph is below 1: a worse graph shows) -- recall_device >= recall_oracle - 0.01, the margin the
    project grants batching on narrow graphs (nodes of a batch do not see each other)."""
    n, dim, metric = 8000, 128, 1
    gix, data, q, lv, ids, efc = batched_wide_build(hv, n, dim, metric)
    tid, _, _, _ = gix.flat_search_batch(q, 10)
    oix = oracle_build(orc, data, metric, lv, M, M0, efc, ids)
    for ef in (32, 64):
        gid, _, gcnt, st = gix.search_batch(q, hv.SearchParams(10).with_ef(ef))
        rec = fx.recall_at_k(gid, tid)
        hits, odc = 0, 0
        for qi in range(q.shape[0]):
            rc, oid, _, ost = oix.search(q[qi], 10, ef, with_stats=True)
            hits += len(set(oid.tolist()) & set(tid[qi].tolist()))
            odc += ost["distance_computations"]
        orec = hits / (10.0 * q.shape[0])
        print(f"ef {ef}: recall@10 device {rec:.4f} oracle {orec:.4f}; distance evaluations per query device "
              f"{st['distance_computations'] / q.shape[0]:.0f} oracle {odc / q.shape[0]:.0f}")
        assert rec >= orec - 0.01, (ef, rec, orec)
    gix.close()


def test_batched_wide_build_of_a_cosine_shape_keeps_the_invariants(hv):
    """6 000 x 256 cosine, same recipe: invariants and the audit."""
    gix, *_ = batched_wide_build(hv, 6000, 256, 0)
    gix.close()


def test_degree_limits_above_64_are_refused_with_nothing_changed(orc, hv):
    n, dim = 300, 64
    rng, data, ids, lv = wide_inputs(n, dim, 1, 32)
    for m, m0 in ((32, 96), (40, 80)):
        with pytest.raises(hv.HelixDbError) as e:
            hv.ValidatedVectorReadIndex.build(dim=dim, metric=1, node_ids=ids, vectors=data, levels=lv, m=m, m0=m0, ef_construction=64)
        assert e.value.status == hv.ERR_UNSUPPORTED
    oix = oracle_build(orc, data[:200], 1, lv[:200], 48, 96, 64, ids[:200])
    ex = oix.export()
    try:
        gix = hv.ValidatedVectorReadIndex.from_export(ex, dim=dim, metric=1, m=48, m0=96, reserve_rows=100, reserve_upper_rows=int(lv[200:].sum()))
    except hv.HelixDbError as e:
        print(f"the import refuses an image that declares m0 = 96 (status {e.status}): nothing to insert into")
        return
    before = gix.export_graph()
    with pytest.raises(hv.HelixDbError) as e:
        gix.insert_batch(ids[200:], data[200:], lv[200:], ef_construction=64, sequential=True)
    assert e.value.status == hv.ERR_UNSUPPORTED
    after = gix.export_graph()
    assert gix.rows() == 200
    for key in ("l0_offsets", "l0_neighbors", "level", "up_offsets", "up_neighbors"):
        assert before[key].tolist() == after[key].tolist(), key
    assert (before["entry_point"], before["max_layer"]) == (after["entry_point"], after["max_layer"])
    with pytest.raises(hv.HelixDbError) as e:
        gix.upsert_batch(ids[:2], data[200:202], ef_construction=64)
    assert e.value.status == hv.ERR_UNSUPPORTED
    assert gix.export_graph()["l0_neighbors"].tolist() == before["l0_neighbors"].tolist() and gix.live_rows() == 200
    gix.close()
