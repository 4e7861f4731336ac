"""hvx_index_delete_batch (csrc/hvx_delete.hip) against the oracle on graphs no insert produces: planted hubs (tests/hub_graphs.py) held
by hundreds to 4 096 rows, on ASYMMETRIC graphs -- holders the hub's own row does not name, out-neighbours that do not hold the hub
(mandatory relink sources, mutation.rs:1833-1837), full rows of nodes that are no sources (reciprocal prunes), rows longer than the
degree limit, hubs on the upper layers -- up to the last source and candidate counts the kernels accept, and one past each of the three
limits, where the delete is refused loudly.  Every graph the other delete tests use came out of an insert: at most m0 relink sources
and ~760 candidates before any delete, 291 sources and 1 292 candidates at the most once their own relinks have broken the symmetry
(counted with the oracle over test_gpu_delete.py's 1 600 x 128 sequence; tests/test_hub_graphs_host.py holds the planted counts).
Deletes are deterministic and the device promises the oracle's rows exactly: no tolerance anywhere."""
import time

import numpy as np
import pytest

import fixtures as fx
import hub_graphs as hg
from test_gpu_delete import assert_same_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


def both(orc, hv, case, g):
    """the planted graph on the device (hvx_index_import) and in the oracle (seeded with the same arrays; the rounded rows for bf16)"""
    dim, metric = g["vectors"].shape[1], case.get("metric", 1)
    gix = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=metric, m=g["m"], m0=g["m0"], dtype=hv.BF16 if case.get("bf16") else hv.F32,
                                              **hg.import_args(g))
    oix = orc.Index(dim, metric, kernel=orc.K_AVX_FMA, m=g["m"], m0=g["m0"], ef_construction=100)
    vec = fx.round_bf16(g["vectors"]) if case.get("bf16") else g["vectors"]
    assert oix.seed(**dict(hg.import_args(g), vectors=vec)) == orc.OK
    return gix, oix


@pytest.mark.parametrize("name", list(hg.CASES))
def test_a_hub_delete_equals_the_oracles_row_for_row(orc, hv, name):
    """One delete_batch call: the hub, three of its former holders (sequential semantics on the relinked graph), one node that was only a
    candidate, an unknown id.  Every layer-0 and upper row, the entry point and the top layer equal the oracle's; the statistics count
    what happened; the audit's row invariants hold (rows over the limit: exactly the ones the oracle still has -- planted long rows no
    delete touched); the HNSW search and the exact scan equal the oracle's ids and score bits on the relinked graph.
      mid            312 sources > the ranking's 64 workgroups (each loops ~5 times over its LDS), both asymmetric branches of the
                     prep kernel, 2 500 candidates through the sixteen-wavefront merge; _cos: the cosine headers; _bf16 (dim 64, where
                     both searches refuse bf16 rows: rows, statistics and audit only) and _bf16_128 (every check): the BF builds;
                     _ties: 40 distinct points, 75 exact duplicates each -- ties broken by id on lists far longer than the tie tests'
      mid_wide       M 32 / M0 64: the wide step with more than 64 sources
      long_rows      M 16 / M0 32 with 40 rows of 33 .. 60 ids: stride 64, so the WIDE step with degree limit 32 -- rows that start over it
      upper[_entry]  200 / 30 holders on layers 1 / 2 (> m sources on the per-layer workgroups, three layers in one step launch);
                     _entry: the hub is the entry point, alone on a layer above -- the entry moves and the top layer drops
      src_boundary   4 096 holders = 4 096 sources, the last count accepted; 1.28 M layer-0 slots: the scan's second grid-stride pass
      cand_boundary  16 384 candidates, the last count accepted"""
    case = hg.CASES[name]
    g = hg.case_graph(case)
    assert [hg.counts(g, g["hub"], layer) for layer in range(len(case["counts"]))] == case["counts"]
    ids = g["node_ids"]
    gix, oix = both(orc, hv, case, g)
    assert_same_graph(gix, oix, ids, ())
    dels = g["delete_ids"]
    t0 = time.perf_counter()
    for d in dels:
        assert oix.delete(d) == (orc.OK, True)
    t_orc = time.perf_counter() - t0
    st = gix.delete_batch(np.asarray(dels + [10 ** 12], np.uint64))
    print(f"{name}: counts {case['counts']} device {st['seconds']:.3f} s oracle {t_orc:.2f} s relinked rows {st['relinked_rows']}")
    assert st["requested"] == len(dels) + 1 and st["deleted"] == len(dels) and st["missing"] == 1
    assert st["relinked_rows"] >= sum(c[1] for c in case["counts"]) and st["entry_moves"] == int(bool(case.get("hub_is_entry")))
    assert gix.live_rows() == ids.size - len(dels) == oix.count
    assert_same_graph(gix, oix, ids, dels)
    ex = oix.export()
    over = int((np.diff(ex["l0_offsets"].astype(np.int64)) > g["m0"]).sum())
    assert (over > 0) == (name == "long_rows")                                  # (upper rows are planted within m)
    audit = gix.audit_graph()
    assert audit["out_of_range_ids"] == 0 and audit["unsorted_entries"] == 0 and audit["self_loops"] == 0 and audit["nodes"] == ids.size - len(dels)
    assert audit["degree_overflow_rows"] == over
    rng = np.random.default_rng(5)
    q = rng.standard_normal((8, g["vectors"].shape[1])).astype(np.float32)
    if name == "mid_bf16":       # bf16 rows of dim 64: the exact scan and the HNSW search refuse them by contract (dim >= 128: mid_bf16_128)
        for refused in (lambda: gix.flat_search_batch(q, 10), lambda: gix.search_batch(q, hv.SearchParams(10).with_ef(64))):
            with pytest.raises(hv.HelixDbError) as e:
                refused()
            assert e.value.status == hv.ERR_UNSUPPORTED
        gix.close()
        return
    fid, fsc, fcnt, _ = gix.flat_search_batch(q, 10)
    gid, gsc, gcnt, _ = gix.search_batch(q, hv.SearchParams(10).with_ef(64))
    for qi in range(q.shape[0]):
        rc, oid, osc = oix.search(q[qi], 10, 64)
        assert rc == orc.OK and gid[qi, :gcnt[qi]].tolist() == oid.tolist() and bits(gsc[qi, :gcnt[qi]]).tolist() == bits(osc).tolist()
        rc, tid, tsc = oix.flat(q[qi], 10)
        assert rc == orc.OK and fid[qi, :fcnt[qi]].tolist() == tid.tolist() and bits(fsc[qi, :fcnt[qi]]).tolist() == bits(tsc).tolist()
        assert not (set(gid[qi, :gcnt[qi]].tolist()) | set(fid[qi, :fcnt[qi]].tolist())) & set(dels)
    gix.close()


@pytest.mark.parametrize("name", list(hg.REFUSALS) + ["refusal_mid_batch"])
def test_one_past_a_limit_is_refused_loudly_and_the_next_handle_is_sound(orc, hv, name):
    """The boundary graphs plus one row: 4 097 holders, 4 100 relink sources (of 4 090 holders), 16 385 candidates -- HVX_ERR_UNSUPPORTED,
    the message names the limit and says the image is partially relinked.  refusal_mid_batch: the 4 097-holder hub between two ordinary
    nodes of one batch (the host goes on launching for the rest with the flag set) -- nodes of a planted island: the delete of a node
    NEAR the holders may prune the hub out of a full holder's row, and a hub of 4 096 holders is rightly accepted.
    Afterwards the handle is closed, the same arrays are imported into a fresh one, and an ordinary delete there equals the oracle's: a refusal poisons neither the process nor the next
    handle's scratch.  (A status from the host, not a fault.)"""
    case = hg.REFUSALS["too_many_holders" if name == "refusal_mid_batch" else name]
    g = hg.case_graph(case)
    assert [hg.counts(g, g["hub"])] == case["counts"]
    ids = g["node_ids"]
    gix, oix = both(orc, hv, case, g)
    quiet = g["quiet_ids"]
    batch = [g["island_ids"][0], g["hub_id"], g["island_ids"][1]] if name == "refusal_mid_batch" else [g["hub_id"]]
    with pytest.raises(hv.HelixDbError) as e:
        gix.delete_batch(np.asarray(batch, np.uint64))
    assert e.value.status == hv.ERR_UNSUPPORTED
    assert case["text"] in str(e.value) and "partially relinked" in str(e.value)
    gix.close()
    gix = hv.ValidatedVectorReadIndex.managed(dim=32, metric=1, m=16, m0=32, **hg.import_args(g))
    assert oix.delete(quiet[2]) == (orc.OK, True)
    st = gix.delete_batch(np.asarray(quiet[2:3], np.uint64))
    assert st["deleted"] == 1 and st["missing"] == 0 and st["relinked_rows"] > 0
    assert_same_graph(gix, oix, ids, quiet[2:3])
    gix.close()
