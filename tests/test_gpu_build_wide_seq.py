"""One node at a time into an image with degree limits above 32 (M 32 / M0 64): the two many-workgroup steps of
csrc/hvx_build_wide_seq.hip -- select and links with every prune's distance matrix evaluated up front -- against the oracle's restatement
of the reference's sequential insertion, and hvx_index_last_write_path, which says which kernels a write ran.

ef_construction = 160 > 128: the layer-0 select hydrates the full 128 candidates (the two-ids-per-lane replay of the select).  Every test
first asserts on the ORACLE alone that its case exercises what the kernels can get wrong: layer-0 rows with 64 ids (an append goes
through the 65-id prune) and inserts in which two of the new node's linked neighbours lose their mutual layer-0 edge -- an earlier link
of the node took an id out of a later link's row (the `alive` replay) or out of another link's row (the removal pass)."""
import numpy as np
import pytest

import fixtures as fx
from test_gpu_build import oracle_build, _rows_dict
from test_gpu_delete import assert_same_graph
from test_gpu_build_wide import M, M0, wide_inputs, full_rows, assert_rows_equal, assert_searches_equal

pytestmark = pytest.mark.gpu

EFC = 160
SHAPES = [(700, 64, 1, EFC, 4), (700, 128, 0, EFC, 4), (500, 768, 1, EFC, 32)]


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


_ORACLE = {}


def oracle_of(orc, n, dim, metric, efc, lm, m=M, m0=M0):
    """The oracle's sequential build of a shape (once per module; nobody changes it) and, counted on its exports before and after each
    insert, the inserts in which two of the new node's linked neighbours (an id in the node's new row, or an id whose row now holds the
    node) lose their mutual layer-0 edge."""
    key = (n, dim, metric, efc, lm, m, m0)
    if key not in _ORACLE:
        rng, data, ids, lv = wide_inputs(n, dim, metric, lm)
        oix = orc.Index(dim, metric, kernel=orc.K_AVX_FMA, m=m, m0=m0, ef_construction=efc)
        before, cross = {}, 0
        for i in range(n):
            assert oix.insert(int(ids[i]), data[i], int(lv[i])) == orc.OK
            after = _rows_dict(oix.export(), ids[:i + 1])
            me = int(ids[i])
            linked = set(after[me]) | {x for x, r in after.items() if me in r}
            cross += any((set(before.get(a, ())) - set(after[a])) & linked for a in linked)
            before = after
        _ORACLE[key] = (oix, oix.export(), cross, rng, data, ids, lv)
    return _ORACLE[key]


def assert_case_is_hard(ex, n, cross, upper):
    f0, fu, nu = full_rows(ex, n)
    print(f"oracle: {f0} layer-0 rows with {M0} ids, {fu} of {nu} upper rows with {M} ids, {cross} inserts whose links cross")
    assert f0 >= 100 and cross >= 100 and (fu >= 50 or not upper), (f0, cross, fu, nu)


@pytest.mark.parametrize("n,dim,metric,efc,lm", SHAPES)
def test_sequential_wide_build_runs_the_eager_steps_and_equals_the_oracle_row_for_row(orc, hv, n, dim, metric, efc, lm):
    """sequential=True, default link_mode: rows, entry point, top layer and levels equal the oracle's, 16 searches equal ids and score
    bits, and the path word says the two many-workgroup steps ran on the two-ids-per-lane kernels -- not the one-wavefront ones."""
    oix, ex, cross, rng, data, ids, lv = oracle_of(orc, n, dim, metric, efc, lm)
    assert_case_is_hard(ex, n, cross, upper=lm == 4)
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids, vectors=data, levels=lv, m=M, m0=M0,
                                                ef_construction=efc, sequential=True)
    assert st["nodes"] == n and st["batches"] == n - 1
    assert_rows_equal(gix.export_graph(), ex, n)
    assert_searches_equal(hv, gix, oix, np.random.default_rng(n + dim).standard_normal((16, dim)).astype(np.float32))
    path = gix.last_write_path()
    assert path & (hv.WRITE_EAGER_STEPS | hv.WRITE_WIDE) == hv.WRITE_EAGER_STEPS | hv.WRITE_WIDE and not path & hv.WRITE_ONE_WAVE, path
    gix.close()


@pytest.mark.parametrize("n,dim,metric,efc,lm", SHAPES)
def test_sequential_wide_build_with_link_mode_1_keeps_the_one_wavefront_kernels(orc, hv, n, dim, metric, efc, lm):
    """link_mode=1: the same rows from the one-wavefront kernels, and the path word says so."""
    oix, ex, cross, rng, data, ids, lv = oracle_of(orc, n, dim, metric, efc, lm)
    assert_case_is_hard(ex, n, cross, upper=lm == 4)
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids, vectors=data, levels=lv, m=M, m0=M0,
                                                ef_construction=efc, sequential=True, link_mode=1)
    assert_rows_equal(gix.export_graph(), ex, n)
    path = gix.last_write_path()
    assert path & (hv.WRITE_ONE_WAVE | hv.WRITE_WIDE) == hv.WRITE_ONE_WAVE | hv.WRITE_WIDE and not path & hv.WRITE_EAGER_STEPS, path
    gix.close()


def test_one_node_inserts_and_upserts_into_a_live_wide_image_equal_the_oracle(orc, hv):
    """The first 2/3 built on the device with room to grow, the rest appended by insert_batch(sequential=True) in two calls, then 40 live
    ids (the entry point among them) upserted with new vectors: rows, entry point and searches equal the oracle's insert / delete +
    insert, every write through the eager steps."""
    n, dim, metric, efc, lm = SHAPES[0]
    _, ex_full, cross, _, data, ids, lv = oracle_of(orc, n, dim, metric, efc, lm)
    assert_case_is_hard(ex_full, n, cross, upper=True)
    rng = np.random.default_rng(77)
    newv = rng.standard_normal((40, dim)).astype(np.float32)
    n0 = n * 2 // 3
    want = hv.WRITE_EAGER_STEPS | hv.WRITE_WIDE
    gix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids[:n0], vectors=data[:n0], levels=lv[:n0], m=M, m0=M0,
                                               ef_construction=efc, sequential=True, reserve_rows=n - n0, reserve_upper_rows=int(lv[n0:].sum()))
    oix = oracle_build(orc, data, metric, lv, M, M0, efc, ids)   # (a copy this test may change)
    cuts = [n0, n0 + (n - n0) // 2, n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        st = gix.insert_batch(ids[a:b], data[a:b], lv[a:b], ef_construction=efc, sequential=True)
        assert st["nodes"] == b - a and gix.rows() == b
        assert gix.last_write_path() == want, gix.last_write_path()
    assert_rows_equal(gix.export_graph(), ex_full, n)
    ent = oix.entry()[0]
    targets = [int(x) for x in ids[rng.permutation(n)[:60]] if int(x) != ent][:39] + [ent]
    level_of = {int(ids[i]): int(lv[i]) for i in range(n)}
    for t, nid in enumerate(targets):
        assert oix.delete(nid) == (orc.OK, True)
        assert oix.insert(nid, newv[t], level_of[nid]) == orc.OK
    st = gix.upsert_batch(np.asarray(targets, np.uint64), newv, ef_construction=efc)
    assert st["nodes"] == len(targets) == 40 and gix.live_rows() == n == oix.count
    assert gix.last_write_path() == want, gix.last_write_path()
    assert_same_graph(gix, oix, ids, ())
    assert_searches_equal(hv, gix, oix, np.vstack([rng.standard_normal((12, dim)).astype(np.float32), newv[:4]]))
    gix.close()


@pytest.mark.parametrize("metric", [1, 0])
def test_one_node_inserts_and_upserts_into_a_wide_bf16_image_equal_the_oracle_on_the_rounded_rows(orc, hv, metric):
    """A bf16 image with rows of 64 ids (an oracle graph over the rounded rows, imported with spare rows) takes one-node inserts, then 24
    upserts, through the eager steps: rows, entry point and searches equal the oracle's on the ROUNDED vectors."""
    n, dim, efc, lm = 800, 128, EFC, 4
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
    want = hv.WRITE_EAGER_STEPS | hv.WRITE_WIDE
    gix.insert_batch(ids[n0:], data[n0:], lv[n0:], ef_construction=efc)
    assert gix.last_write_path() == want, gix.last_write_path()
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
    assert gix.last_write_path() == want, gix.last_write_path()
    assert_same_graph(gix, oix, ids, ())
    assert_searches_equal(hv, gix, oix, np.vstack([rng.standard_normal((12, dim)).astype(np.float32), newr[:4]]))
    gix.close()


def test_sequential_wide_build_of_a_generic_manhattan_shape_equals_the_oracle(orc, hv):
    """Manhattan at dim 100 (96 + a scalar tail of 4) under the scalar summation tree: the generic build of the search kernel.  The
    route of the one-node steps is a matter of the degree limits alone (wide_seq_geom, csrc/hvx_build_dev.h: it fits whenever
    32 < max(m, m0), m0 <= 64 and m <= 32, on every metric, tree and dimension), so this shape takes the eager steps too."""
    n, dim, metric, efc = 700, 100, 2, 100
    rng, data, ids, lv = wide_inputs(n, dim, metric, 32)
    oix = oracle_build(orc, data, metric, lv, M, M0, efc, ids, kernel=orc.K_SCALAR)
    ex = oix.export()
    f0, fu, nu = full_rows(ex, n)
    assert f0 >= 100, f0
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=metric, node_ids=ids, vectors=data, levels=lv, m=M, m0=M0,
                                                ef_construction=efc, sequential=True, float_kernel=hv.KERNEL_SCALAR)
    assert_rows_equal(gix.export_graph(), ex, n)
    fits = 32 < max(M, M0) and M0 <= 64 and M <= 32
    want = hv.WRITE_WIDE | (hv.WRITE_EAGER_STEPS if fits else hv.WRITE_ONE_WAVE)
    assert gix.last_write_path() == want, gix.last_write_path()
    gix.close()


def test_the_path_word_on_a_narrow_image(hv):
    """M 16 / M0 32, code this change does not touch: a sequential build reports the eager steps without the wide flag, a batched build
    of the same rows the workgroup link kernel; an insert of nothing reports 0."""
    n, dim = 1200, 128
    rng = np.random.default_rng(51)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    ids = np.arange(n, dtype=np.uint64)
    lv = fx.draw_levels(n, 16, seed=2)
    gix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=1, node_ids=ids, vectors=data, levels=lv, m=16, m0=32, ef_construction=100,
                                               sequential=True, reserve_rows=8)
    assert gix.last_write_path() == hv.WRITE_EAGER_STEPS, gix.last_write_path()
    gix.insert_batch(ids[:0], data[:0], lv[:0])
    assert gix.last_write_path() == 0
    gix.close()
    gix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=1, node_ids=ids, vectors=data, levels=lv, m=16, m0=32, ef_construction=100)
    assert st["batches"] < n // 4
    path = gix.last_write_path()
    assert path & hv.WRITE_LINK_WG and not path & hv.WRITE_WIDE, path
    gix.close()
