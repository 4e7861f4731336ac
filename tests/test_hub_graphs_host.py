"""The planted hub graphs (tests/hub_graphs.py) are what their cases say they are, and the oracle takes them: the counts the delete
kernels size their loops by are recomputed from the rows alone and must equal each case's stated triple -- conditions of the cases of
tests/test_gpu_delete_hubs.py, kept honest here when someone retunes the generator.  No device."""
import time

import numpy as np
import pytest

import hub_graphs as hg
from test_oracle_delete import rows_by_id


def kernel_counts(g, case):
    return [hg.counts(g, g["hub"], layer) for layer in range(len(case["counts"]))]


@pytest.mark.parametrize("name", list(hg.CASES))
def test_a_planted_case_has_its_counts_and_the_oracle_deletes_its_hub(orc, name):
    """holders / relink sources / candidates per layer equal the case's; the rows are canonical and, on the upper layers, hold nodes of
    their layer only; orc.Index.seed takes the arrays; the oracle deletes the hub and the follow-up ids (three former holders, one node
    that was only a candidate) with (OK, True); afterwards every row the deletes rewrote is within its degree limit, every other row is
    the planted one, and no live row names a deleted id.  Prints the oracle's seconds for the hub delete (run with -s)."""
    case = hg.CASES[name]
    g = hg.case_graph(case)
    assert kernel_counts(g, case) == case["counts"]
    ids, m, m0 = g["node_ids"], g["m"], g["m0"]
    level_of = dict(zip(ids.tolist(), g["level"].tolist()))
    before = rows_by_id(g)
    for nid, (lv, l0, up) in before.items():
        for layer, row in enumerate([l0] + up):
            assert row == sorted(set(row)) and nid not in row and all(level_of[x] >= layer for x in row)
            assert layer == 0 or len(row) <= m
    longest = max(len(l0) for _, l0, _ in before.values())
    assert (longest > m0) == bool(case["plant"].get("long_rows")) and longest <= max(m0, 61)          # (import serves rows of up to 64 ids)
    metric = case.get("metric", orc.L2SQ)
    vec = g["vectors"]
    if case.get("bf16"):
        import fixtures as fx
        vec = fx.round_bf16(vec)
    oix = orc.Index(vec.shape[1], metric, m=m, m0=m0, ef_construction=100)
    assert oix.seed(**dict(hg.import_args(g), vectors=vec)) == orc.OK
    assert oix.entry() == (g["entry_point"], g["max_layer"])
    for t, d in enumerate(g["delete_ids"]):
        t0 = time.perf_counter()
        assert oix.delete(d) == (orc.OK, True)
        if t == 0:
            print(f"{name}: oracle hub delete {time.perf_counter() - t0:.2f} s, counts {case['counts']}")
    gone = set(g["delete_ids"])
    after = rows_by_id(oix.export())
    assert set(after) == set(before) - gone
    changed = 0
    for nid, (lv, l0, up) in after.items():
        assert lv == before[nid][0]
        for layer, row in enumerate([l0] + up):
            assert not gone & set(row)
            was = before[nid][1] if layer == 0 else before[nid][2][layer - 1]
            if row != was:
                changed += 1
                assert len(row) <= (m0 if layer == 0 else m), f"node {nid} layer {layer}: {len(row)} ids after its relink"
    assert changed >= case["counts"][0][1]                                       # (every relink source of layer 0 at least)
    ent = oix.entry()
    assert ent is not None and ent[0] not in gone
    if case.get("hub_is_entry"):                                               # the hub sat alone on the top layer: the entry moved one layer down
        top = g["max_layer"] - 1
        assert ent == (min(nid for nid in after if level_of[nid] == top), top)
    else:
        assert ent == (g["entry_point"], g["max_layer"])


@pytest.mark.parametrize("name", list(hg.REFUSALS))
def test_a_refusal_graph_is_one_past_its_limit(orc, name):
    """the graphs hvx_index_delete_batch must refuse are the boundary graphs plus one: exactly one of the three quantities is past its
    limit (4 096 holders, 4 096 relink sources, 16 384 candidates), the other two are within theirs; the oracle takes the arrays"""
    case = hg.REFUSALS[name]
    g = hg.case_graph(case)
    (holders, sources, cands), = kernel_counts(g, case)
    assert [(holders, sources, cands)] == case["counts"]
    over = {"too_many_holders": holders > 4096, "too_many_sources": holders <= 4096 < sources, "too_many_candidates": sources <= 4096 and cands == 16385}
    assert over[name]
    oix = orc.Index(32, orc.L2SQ, m=16, m0=32, ef_construction=100)
    assert oix.seed(**hg.import_args(g)) == orc.OK


def test_counts_on_a_graph_written_out_by_hand():
    """counts() itself, on five rows: 0 is the hub; 1 and 2 hold it; its own row names 2 and 3 (3 does not hold it); 4 holds nobody's
    attention but is named by 3 -> 2 holders, 3 sources, candidates {1, 2, 3, 4, 5} less nothing = 5 (5 is named by 1)"""
    rows = {0: np.array([2, 3]), 1: np.array([0, 5]), 2: np.array([0, 1]), 3: np.array([4]), 4: np.array([1]), 5: np.array([4])}
    assert hg.counts(rows, 0) == (2, 3, 5)
    assert hg.counts(rows, 4) == (2, 3, 4)                                      # held by 3 and 5; out-neighbour 1; candidates {1, 3, 5, 0}
