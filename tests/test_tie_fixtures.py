"""The tie-heavy corpora of fixtures.py (lattice_rows, duplicate_groups) on the ORACLE alone: its sequential insertion is deterministic
on them, every summation tree gives the same rows (arithmetic is exact, so a difference would be an order-of-decision bug in the oracle
itself), and the cases tests/test_gpu_build_ties.py builds on the device reach what they are there for -- inserts whose ties a
192-entry register beam cannot hold, full rows where the prune is the point, unreachable nodes in the reference's own graph of the
duplicate corpus."""
import numpy as np
import pytest

import fixtures as fx


def exports_equal(a, b):
    return (a["entry_point"], a["max_layer"]) == (b["entry_point"], b["max_layer"]) and all(
        np.array_equal(a[k], b[k]) for k in ("node_ids", "l0_offsets", "l0_neighbors", "level", "up_offsets", "up_neighbors"))


def test_lattice_rows_are_distinct_exact_and_bf16_values():
    for n, dim, nz in [(1200, 128, 2), (1200, 128, 3), (600, 100, 3)]:
        x = fx.lattice_rows(n, dim, nz, 1)
        assert x.shape == (n, dim) and x.dtype == np.float32
        assert ((x != 0).sum(axis=1) == nz).all() and set(np.unique(x).tolist()) == {-1.0, 0.0, 1.0}
        assert len({r.tobytes() for r in x}) == n
        assert np.array_equal(fx.round_bf16(x), x)
        d = ((x[:64, None, :].astype(np.float64) - x[None, :64, :]) ** 2).sum(axis=2)
        assert set(np.unique(d).tolist()) <= set(range(0, 4 * nz + 1, 2))


def test_duplicate_groups_hold_exact_copies_and_distinct_filler():
    x, label = fx.duplicate_groups(2, [20, 80], 280, 128, 5)
    assert x.shape == (380, 128) and [(label == g).sum() for g in (0, 1, -1)] == [20, 80, 280]
    for g in (0, 1):
        assert len({r.tobytes() for r in x[label == g]}) == 1
    assert len({r.tobytes() for r in x}) == 282
    assert np.array_equal(fx.round_bf16(x), x)
    # shuffled: a group is not one run of consecutive rows
    assert np.ptp(np.flatnonzero(label == 0)) > 100


@pytest.mark.parametrize("name", list(fx.TIE_CASES))
def test_the_oracle_reaches_the_ties_each_device_case_is_there_for(orc, name):
    """tie_case asserts >= 100 tie-prone inserts (and >= 100 full rows where the prune is the point); the duplicate corpus leaves
    unreachable nodes in the oracle's own graph -- the number the batched device build is held to."""
    c = fx.tie_case(orc, name)
    n = fx.TIE_CASES[name][1]
    assert c["oix"].count == n and c["prone"] >= 100
    if name.startswith("dup"):
        print(f"{name}: {c['unreachable']} of {n} nodes unreachable in the oracle's graph")
        assert c["unreachable"] > 0


@pytest.mark.parametrize("name", ["l2_small", "dup", "l1_prune"])
def test_two_oracle_builds_of_a_tie_corpus_are_identical(orc, name):
    c = fx.tie_case(orc, name)
    oix = fx.tie_oracle_factory(orc, name)()
    for i in range(c["data"].shape[0]):
        assert oix.insert(int(c["ids"][i]), c["data"][i], int(c["levels"][i])) == orc.OK
    assert exports_equal(oix.export(), c["ex"])


@pytest.mark.parametrize("metric", [1, 0])
def test_every_summation_tree_builds_the_same_rows_on_a_lattice(orc, metric):
    name = "l2_small" if metric == 1 else "cos_small"
    c = fx.tie_case(orc, name)
    _, n, dim, _, _, m, m0, efc, _, _, _, _ = fx.TIE_CASES[name]
    for kern in (orc.K_SCALAR, orc.K_AVX, orc.K_SSE, orc.K_NEON):  # (the case itself is K_AVX_FMA)
        oix = orc.Index(dim, metric, kernel=kern, m=m, m0=m0, ef_construction=efc)
        for i in range(n):
            assert oix.insert(int(c["ids"][i]), c["data"][i], int(c["levels"][i])) == orc.OK
        assert exports_equal(oix.export(), c["ex"]), f"summation tree {kern} links other rows than AVX+FMA on exact arithmetic"


def test_header_library_and_python_report_the_flagged_build_searches():
    """include/helix_vec.h declares hvx_index_last_write_tie_overflows next to hvx_index_last_write_path, the comments of the build, insert
    and upsert calls name it as the precondition of their row-for-row promise, hvx_build_stats keeps its three words (the struct is ABI),
    the library exports the accessor (0 for a null handle) and pyhvx exposes it."""
    import ctypes
    import os
    import re
    import pyhvx as hv
    text = open(os.path.join(fx.ROOT, "include", "helix_vec.h")).read()
    assert re.search(r"uint32_t\s+hvx_index_last_write_path\s*\(\s*const\s+hvx_index\s*\*\s*\)\s*;\s*/\*.*?\*/\s*"
                     r"uint32_t\s+hvx_index_last_write_tie_overflows\s*\(\s*const\s+hvx_index\s*\*\s*\)\s*;", text, flags=re.S)
    for call in ("hvx_index_build", "hvx_index_insert_batch", "hvx_index_upsert_batch"):
        decl = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:enum[^;]*;\s*|typedef struct[^}]*\}[^;]*;\s*|void[^;]*;\s*|/\*(?:(?!\*/).)*\*/\s*|uint32_t[^;]*;\s*)*int\s+"
                         + call + r"\s*\(", text, flags=re.S)
        assert decl and "hvx_index_last_write_tie_overflows" in decl.group(1), f"the comment of {call} does not state the precondition"
    stats = re.search(r"typedef struct hvx_build_stats \{(.*?)\} hvx_build_stats;", text, flags=re.S).group(1)
    assert re.sub(r"\s+", " ", stats).strip() == "uint64_t nodes, batches, single_node_batches;"
    fn = hv.lib().hvx_index_last_write_tie_overflows
    fn.restype, fn.argtypes = ctypes.c_uint32, [ctypes.c_void_p]
    assert fn(None) == 0
    assert callable(hv.ValidatedVectorReadIndex.last_write_tie_overflows)
