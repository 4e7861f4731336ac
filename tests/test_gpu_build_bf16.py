"""hvx_index_build / hvx_index_insert_batch / hvx_index_link_rows over bf16 images (csrc/hvx_build.hip: the BF builds of the select / link
kernels) against the oracle fed the ROUNDED rows (fixtures.round_bf16): a bf16 index IS the graph of the rounded vectors."""
import numpy as np
import pytest

import fixtures as fx

pytestmark = pytest.mark.gpu

# every defect counter of hvx_index_audit_graph (the counters below `bfs_levels_l0`; the rest are sizes)
AUDIT_KEYS = ("asymmetric_edges_l0", "asymmetric_edges_up", "unsorted_entries", "self_loops", "out_of_range_ids", "holes", "level_violations",
              "degree_overflow_rows", "unreachable_l0")


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def oracle_build(orc, rounded, metric, levels, m, m0, efc, ids):
    oix = orc.Index(rounded.shape[1], metric, kernel=orc.K_AVX_FMA, m=m, m0=m0, ef_construction=efc)
    for i in range(rounded.shape[0]):
        assert oix.insert(int(ids[i]), rounded[i], int(levels[i])) == orc.OK
    return oix


def rows_of(g, n):
    l0 = [g["l0_neighbors"][int(g["l0_offsets"][i]):int(g["l0_offsets"][i + 1])].tolist() for i in range(n)]
    up = [g["up_neighbors"][int(g["up_offsets"][r]):int(g["up_offsets"][r + 1])].tolist() for r in range(len(g["up_offsets"]) - 1)]
    return l0, up


def assert_rows_equal(g, ex, n):
    assert g["entry_point"] == ex["entry_point"] and g["max_layer"] == ex["max_layer"]
    assert g["level"].tolist() == ex["level"].tolist()
    gl0, gup = rows_of(g, n)
    ol0, oup = rows_of(ex, n)
    bad = [i for i in range(n) if gl0[i] != ol0[i]]
    assert not bad, f"{len(bad)} layer-0 rows differ, first {bad[:5]}: device {gl0[bad[0]]} oracle {ol0[bad[0]]}"
    assert gup == oup


def assert_audit_clean(a, n, m, m0, unreachable_max=0):
    """Every defect counter 0 -- unreachable_l0 among them: a batch that cut nodes off from the entry point would not show in the recall
    of 200 queries --, and the degrees bounded on layer 0 and above.  unreachable_max: HNSW does not guarantee connectivity (a prune's
    reverse-edge removals can leave a node without an edge in a graph the reference could have written: include/helix_vec.h,
    hvx_index_audit_graph); the builds are held to 0 as tests/test_gpu_build.py holds the batched f32 build, appends to a live image to
    what that file grants batched f32 inserts."""
    print("audit:", a)
    assert a["nodes"] == n and a["has_entry"] == 1
    for key in AUDIT_KEYS:
        assert a[key] <= (unreachable_max if key == "unreachable_l0" else 0), (key, a)
    assert a["max_degree_l0"] <= m0 and a["max_degree_up"] <= m, a


def oracle_recall(oix, q, true_ids, k, ef):
    hits = 0
    for qi in range(q.shape[0]):
        _, oid, _ = oix.search(q[qi], k, ef)
        hits += len(set(oid.tolist()) & set(true_ids[qi].tolist()))
    return hits / float(q.shape[0] * k)


def clustered(rng, n, dim, nc=64, spread=0.5):
    centres = rng.standard_normal((nc, dim)).astype(np.float32)
    draw = lambda cnt: (centres[rng.integers(0, nc, cnt)] + spread * rng.standard_normal((cnt, dim))).astype(np.float32)
    return draw(n), draw


# ------------------------------------------------------------------------------------------------------------------------
# 1. sequential build == the oracle's insertion of the rounded rows
# ------------------------------------------------------------------------------------------------------------------------
SEQ_SHAPES = [(1000, 128, 1, 16, 32, 80), (800, 256, 0, 16, 32, 80), (500, 768, 1, 8, 16, 64)]
_seq_cache = {}


def seq_case(orc, shape):
    """(data, levels, ids, the oracle's index over the rounded rows, its export, queries): computed once per shape"""
    if shape not in _seq_cache:
        n, dim, metric, m, m0, efc = shape
        rng = np.random.default_rng(7600 + dim + metric + n)
        data = rng.standard_normal((n, dim)).astype(np.float32)
        lv = fx.draw_levels(n, m, seed=n + 1)
        ids = np.arange(n, dtype=np.uint64) * 2 + 11
        oix = oracle_build(orc, fx.round_bf16(data), metric, lv, m, m0, efc, ids)
        _seq_cache[shape] = (data, lv, ids, oix, oix.export(), rng.standard_normal((16, dim)).astype(np.float32))
    return _seq_cache[shape]


@pytest.mark.parametrize("shape,link_mode", [(s, 0) for s in SEQ_SHAPES] + [(SEQ_SHAPES[0], 1)])
def test_sequential_bf16_build_equals_the_oracles_insertion_of_the_rounded_rows(orc, hv, shape, link_mode):
    """build(dtype=BF16, sequential=True): one node per batch over the packed bf16 rows == insert_hnsw of the ROUNDED vectors in node-id
    order: entry point, top layer, every layer-0 and upper row, and 16 searches (ids and score bits).  link_mode=1 runs the
    one-wavefront bf16 builds of build_select_kernel / build_link_kernel instead of the many-workgroup one-node steps."""
    n, dim, metric, m, m0, efc = shape
    data, lv, ids, oix, ex, q = seq_case(orc, shape)
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids, vectors=data, levels=lv, m=m, m0=m0,
                                                ef_construction=efc, sequential=True, dtype=hv.BF16, link_mode=link_mode)
    assert st["nodes"] == n and st["batches"] == n - 1
    assert_rows_equal(gix.export_graph(), ex, n)
    gid, gsc, gcnt, _ = gix.search_batch(q, hv.SearchParams(10).with_ef(64))
    for qi in range(16):
        rc, oid, osc = oix.search(q[qi], 10, 64)
        assert gid[qi, :gcnt[qi]].tolist() == oid.tolist()
        assert gsc[qi, :gcnt[qi]].view(np.uint32).tolist() == osc.view(np.uint32).tolist()
    gix.close()


# ------------------------------------------------------------------------------------------------------------------------
# 2. build_link_wg_kernel<.., BF> link by link
# ------------------------------------------------------------------------------------------------------------------------
def _rows_dict(g, ids):
    return {nid: g["l0_neighbors"][int(g["l0_offsets"][i]):int(g["l0_offsets"][i + 1])].tolist() for i, nid in enumerate(ids.tolist())}


# column blocks of <= 8 chunks: dim 128 = one block of 4, dim 384 = 8 + 4 chunks (the last block partial), dim 1536 = six blocks
@pytest.mark.parametrize("dim,metric,n", [(128, 1, 1500), (384, 0, 1200), (1536, 1, 500)])
def test_bf16_link_workgroup_kernel_equals_the_oracles_prune_link_by_link(orc, hv, dim, metric, n):
    """The bf16 twin of test_gpu_build.py::test_link_workgroup_kernel_equals_the_oracles_prune_link_by_link: the kernel that links every
    batched bf16 build (bf16 column blocks widened into LDS), one link at a time through hvx_index_link_rows, against a host model
    whose every prune is the oracle's select_diverse + backfill on the ROUNDED rows -- full rows, duplicate vectors (ties), repeated
    targets: after >= 220 links every layer-0 row equals the model's; then the same links in one launch keep the row invariants."""
    rng = np.random.default_rng(9400 + dim + metric)
    m, m0, efc = 16, 32, 64
    centres = rng.standard_normal((12, dim)).astype(np.float32)
    data = (centres[rng.integers(0, 12, n)] + 0.35 * rng.standard_normal((n, dim))).astype(np.float32)
    for t in range(0, n, 9):          # duplicate vectors: ties in every distance that involves them
        data[t] = data[(t * 7 + 3) % n]
    lv = np.zeros(n, np.uint16)        # layer 0 only: the probe links layer-0 rows
    ids = np.arange(n, dtype=np.uint64) * 2 + 7
    oix = oracle_build(orc, fx.round_bf16(data), metric, lv, m, m0, efc, ids)
    ex = oix.export()
    gix = hv.ValidatedVectorReadIndex.from_export(ex, dim=dim, metric=metric, dtype=hv.BF16)
    rows = _rows_dict(ex, ids)
    full = [nid for nid in ids.tolist() if len(rows[nid]) == m0]
    assert len(full) >= 60, "the fixture must hold full rows (every link to one prunes)"
    links = []
    targets = [full[int(x)] for x in rng.choice(len(full), 150, replace=len(full) < 150)]
    targets += [int(ids[int(x)]) for x in rng.integers(0, n, 60)]      # rows of any degree
    targets += targets[:25]                                           # the same row again, after its first prune
    for to in targets:
        while True:
            frm = int(ids[int(rng.integers(0, n))])
            if frm != to and frm not in rows[to]:
                break
        row = rows[to] + [frm]                                        # host model of add_bidirectional_link(from, to) on layer 0
        if len(row) > m0:
            rc, keep = oix.prune_candidates(to, np.array(row, np.uint64), m0)
            assert rc == orc.OK
            keep = keep.tolist()
            for x in row:
                if x not in keep and to in rows[x]:                   # remove_edge_from_neighbor (mutation.rs:1890-1908)
                    rows[x].remove(to)
            rows[to] = sorted(keep)
        else:
            rows[to] = sorted(row)
        links.append((frm, to))
    assert len(links) >= 220
    gix.link_rows([f for f, _ in links], [t for _, t in links], concurrent=False)
    got = _rows_dict(gix.export_graph(), ids)
    bad = [nid for nid in ids.tolist() if got[nid] != rows[nid]]
    assert not bad, f"{len(bad)} rows differ after {len(links)} links, first {bad[0]}: device {got[bad[0]]} model {rows[bad[0]]}"
    gix.close()
    gix2 = hv.ValidatedVectorReadIndex.from_export(ex, dim=dim, metric=metric, dtype=hv.BF16)
    gix2.link_rows([f for f, _ in links], [t for _, t in links], concurrent=True)
    a = gix2.audit_graph()
    for key in ("unsorted_entries", "self_loops", "out_of_range_ids", "holes", "degree_overflow_rows", "level_violations"):
        assert a[key] == 0, (key, a)
    assert a["max_degree_l0"] <= m0
    gix2.close()


# ------------------------------------------------------------------------------------------------------------------------
# 3. batched build
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [1, 0])
def test_batched_bf16_build_invariants_and_recall(orc, hv, metric):
    """The default (batched) bf16 build: few batches, a graph the audit passes (symmetric, canonical, degree-bounded rows), and
    recall@10 at ef 100 no more than 0.01 (the margin batching is granted) under that of the ORACLE's sequential graph
    over the rounded rows, both scored against the exact answer on the same image."""
    n, dim, m, m0, efc = 6000, 128, 16, 32, 100
    rng = np.random.default_rng(8200 + metric)
    data, draw = clustered(rng, n, dim)
    lv = fx.draw_levels(n, m, seed=3)
    ids = np.arange(n, dtype=np.uint64)
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids, vectors=data, levels=lv, m=m, m0=m0,
                                                ef_construction=efc, max_batch=256, batch_divisor=16, dtype=hv.BF16)
    assert st["nodes"] == n and st["batches"] < n // 4
    assert_audit_clean(gix.audit_graph(), n, m, m0)
    g = gix.export_graph()
    top = int(lv.max())
    assert g["max_layer"] == top and lv[g["entry_point"]] == top
    l0, up = rows_of(g, n)
    assert max(len(r) for r in l0) <= m0 and min(len(r) for r in l0) >= 1 and max([len(r) for r in up] + [0]) <= m
    q = draw(200)
    gid, _, _, _ = gix.search_batch(q, hv.SearchParams(10).with_ef(100))
    tid, _, _, _ = gix.flat_search_batch(q, 10)
    rec = fx.recall_at_k(gid, tid)
    ref = oracle_recall(oracle_build(orc, fx.round_bf16(data), metric, lv, m, m0, efc, ids), q, tid, 10, 100)
    print(f"bf16 batched build, metric {metric}: {st['batches']} batches, recall@10 {rec:.4f}, oracle sequential {ref:.4f}")
    assert rec >= ref - 0.01, (rec, ref)
    gix.close()


def test_scattered_bf16_build_gathers_its_queries_in_insertion_order(orc, hv):
    """scatter=True inserts position i = row (i x stride) mod n: the build searches' f32 queries are gathered from the bf16 rows over the
    permuted node list.  Rows sorted by cluster (consecutive rows are each other's nearest neighbours -- what scatter is for), dim 256
    (four pieces per lane); a query taken from the wrong row would link nodes next to strangers: audit and the recall criterion."""
    n, dim, metric, m, m0, efc = 3000, 256, 1, 16, 32, 100
    rng = np.random.default_rng(8250)
    centres = rng.standard_normal((32, dim)).astype(np.float32)
    lab = np.sort(rng.integers(0, 32, n))
    data = (centres[lab] + 0.5 * rng.standard_normal((n, dim))).astype(np.float32)
    lv = fx.draw_levels(n, m, seed=6)
    ids = np.arange(n, dtype=np.uint64)
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids, vectors=data, levels=lv, m=m, m0=m0,
                                                ef_construction=efc, max_batch=256, batch_divisor=16, dtype=hv.BF16, scatter=True)
    assert st["nodes"] == n and st["batches"] < n // 4
    assert_audit_clean(gix.audit_graph(), n, m, m0)
    q = (centres[rng.integers(0, 32, 200)] + 0.5 * rng.standard_normal((200, dim))).astype(np.float32)
    gid, _, _, _ = gix.search_batch(q, hv.SearchParams(10).with_ef(100))
    tid, _, _, _ = gix.flat_search_batch(q, 10)
    rec = fx.recall_at_k(gid, tid)
    ref = oracle_recall(oracle_build(orc, fx.round_bf16(data), metric, lv, m, m0, efc, ids), q, tid, 10, 100)
    print(f"bf16 scattered build: {st['batches']} batches, recall@10 {rec:.4f}, oracle sequential (id order) {ref:.4f}")
    assert rec >= ref - 0.01, (rec, ref)
    gix.close()


# ------------------------------------------------------------------------------------------------------------------------
# 4. batched inserts by opt-in; the default stays one node per step
# ------------------------------------------------------------------------------------------------------------------------
def test_bf16_inserts_batch_by_opt_in_and_stay_sequential_by_default(orc, hv):
    """A bf16 image hydrated with spare rows (60 % of 3 000 x 128).  insert_batch(sequential=BUILD_BATCHED) links the rest in batches:
    audit clean, live_rows right, recall as the batched build's criterion.  The same rows with the default: one node per step, rows
    equal the oracle's insertion of the rounded rows (the contract hvx_index_insert_batch documents for bf16 images)."""
    n, dim, metric, m, m0, efc = 3000, 128, 1, 16, 32, 100
    rng = np.random.default_rng(8300)
    data, draw = clustered(rng, n, dim)
    rounded = fx.round_bf16(data)
    lv = fx.draw_levels(n, m, seed=9)
    ids = np.arange(n, dtype=np.uint64) * 2 + 1
    n0 = n * 6 // 10
    oix = oracle_build(orc, rounded[:n0], metric, lv[:n0], m, m0, efc, ids[:n0])
    ex = oix.export()
    ex["vectors"] = data[:n0]
    hydrate = lambda: hv.ValidatedVectorReadIndex.from_export(ex, dim=dim, metric=metric, dtype=hv.BF16, m=m, m0=m0, reserve_rows=n - n0,
                                                              reserve_upper_rows=int(lv[n0:].sum()))
    for i in range(n0, n):
        assert oix.insert(int(ids[i]), rounded[i], int(lv[i])) == orc.OK
    # -- batches
    gix = hydrate()
    st = gix.insert_batch(ids[n0:], data[n0:], lv[n0:], ef_construction=efc, sequential=hv.BUILD_BATCHED, max_batch=128, batch_divisor=16)
    assert st["nodes"] == n - n0 and st["batches"] < (n - n0) // 4
    assert gix.live_rows() == n and gix.rows() == n
    # (unreachable_l0 <= 10: the bound of test_gpu_build.py::test_batched_inserts_keep_the_graph_invariants_... -- 1 200 links into full
    # rows of a live graph, every one a prune with reverse-edge removals, in an order that varies from run to run)
    assert_audit_clean(gix.audit_graph(), n, m, m0, unreachable_max=10)
    q = draw(200)
    gid, _, _, _ = gix.search_batch(q, hv.SearchParams(10).with_ef(100))
    tid, _, _, _ = gix.flat_search_batch(q, 10)
    rec, ref = fx.recall_at_k(gid, tid), oracle_recall(oix, q, tid, 10, 100)
    print(f"bf16 batched insert: {st['batches']} batches, recall@10 {rec:.4f}, oracle sequential {ref:.4f}")
    assert rec >= ref - 0.01, (rec, ref)
    gix.close()
    # -- the default
    gix = hydrate()
    st = gix.insert_batch(ids[n0:], data[n0:], lv[n0:], ef_construction=efc)
    assert st["nodes"] == n - n0 and st["batches"] == n - n0
    assert_rows_equal(gix.export_graph(), oix.export(), n)
    gix.close()


# ------------------------------------------------------------------------------------------------------------------------
# 5. degree limits above 32
# ------------------------------------------------------------------------------------------------------------------------
def test_batched_bf16_build_with_wide_rows(orc, hv):
    """M 32 / M0 64 over bf16 rows: the wide select kernel and the one-wavefront wide link kernel for every batch."""
    n, dim, metric, m, m0, efc = 2000, 128, 1, 32, 64, 100
    rng = np.random.default_rng(8400)
    data, draw = clustered(rng, n, dim)
    lv = fx.draw_levels(n, m, seed=4)
    ids = np.arange(n, dtype=np.uint64)
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids, vectors=data, levels=lv, m=m, m0=m0,
                                                ef_construction=efc, max_batch=256, batch_divisor=16, dtype=hv.BF16)
    assert st["nodes"] == n and st["batches"] < n // 4
    assert_audit_clean(gix.audit_graph(), n, m, m0)
    q = draw(200)
    gid, _, _, _ = gix.search_batch(q, hv.SearchParams(10).with_ef(64))
    tid, _, _, _ = gix.flat_search_batch(q, 10)
    rec = fx.recall_at_k(gid, tid)
    ref = oracle_recall(oracle_build(orc, fx.round_bf16(data), metric, lv, m, m0, efc, ids), q, tid, 10, 64)
    print(f"bf16 wide batched build: {st['batches']} batches, recall@10 {rec:.4f}, oracle sequential {ref:.4f}")
    assert rec >= ref - 0.01, (rec, ref)
    gix.close()


# ------------------------------------------------------------------------------------------------------------------------
# 6. refusals
# ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what,dim,metric,efc,dtype", [("dim 192", 192, 1, 64, "BF16"), ("Manhattan", 128, 2, 64, "BF16"),
                                                       ("ef_construction 400", 128, 1, 400, "BF16"), ("fp8", 128, 1, 64, "FP8_E4M3")])
def test_bf16_build_refuses_what_it_does_not_serve(hv, what, dim, metric, efc, dtype):
    n = 64
    data = np.random.default_rng(1).standard_normal((n, dim)).astype(np.float32)
    with pytest.raises(hv.HelixDbError) as e:
        hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=np.arange(n, dtype=np.uint64), vectors=data, m=16, m0=32,
                                          ef_construction=efc, dtype=getattr(hv, dtype))
    assert e.value.status == hv.ERR_UNSUPPORTED, what
