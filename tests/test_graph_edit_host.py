"""hvx_csr_apply_edges without a GPU: the numpy twin of its contract (tests/graph_edit_twin.py) on a hand-written graph, and the host
plan (helix-db_amd/csrc/hvx_csr_edit_plan.h) held to the twin through tests/native/csr_edit_plan_probe.cpp."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import fixtures as fx
import graph_edit_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arrays_of(arcs):
    src = np.array([a[0] for a in arcs], np.int64)
    off = np.zeros(twin.EIGHT_N + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(src, minlength=twin.EIGHT_N))
    return off, np.array([a[1] for a in arcs], np.uint64), np.array([a[2] for a in arcs], np.uint32)


@pytest.mark.parametrize("case", sorted(twin.EIGHT_CASES))
def test_twin_equals_the_arcs_spelled_out_by_hand(case):
    n, off, tgt, lab = twin.eight_graph()
    remove, add, want = twin.EIGHT_CASES[case]
    got = twin.apply_edges(n, off, tgt, lab, twin.triples(remove), twin.triples(add))
    w_off, w_tgt, w_lab = _arrays_of(want)
    assert got[0].tolist() == w_off.tolist() and got[1].tolist() == w_tgt.tolist() and got[2].tolist() == w_lab.tolist()


def test_twin_incoming_arrays_spelled_out_by_hand():
    """after removing (d,3) from the eight-node graph: all seven arrays as literals"""
    n, off, tgt, lab = twin.eight_graph()
    new = twin.apply_edges(n, off, tgt, lab, twin.triples([(3, 4, 3)]), None)
    a = twin.import_arrays(n, *new)
    assert a["out_offsets"].tolist() == [0, 2, 2, 4, 7, 8, 9, 9, 11]
    assert a["out_targets"].tolist() == [1, 4, 2, 5, 4, 4, 6, 0, 7, 0, 7]
    assert a["out_labels"].tolist() == [1, 2, 7, 1, 3, 5, 2, 9, 4, 6, 8]
    assert a["in_offsets"].tolist() == [0, 2, 3, 4, 4, 7, 8, 9, 11]
    assert a["in_sources"].tolist() == [4, 7, 0, 2, 0, 3, 3, 2, 3, 5, 7]
    assert a["in_edge_index"].tolist() == [7, 9, 0, 2, 1, 4, 5, 3, 6, 8, 10]
    assert a["in_labels"].tolist() == [9, 6, 1, 7, 2, 3, 5, 1, 2, 4, 8]
    assert twin.sizes(n, new[0], new[1]) == dict(n_nodes=8, n_edges=11, max_out_degree=3, max_in_degree=3, rows_sorted=True)


def test_twin_refuses_what_the_call_refuses():
    n, off, tgt, lab = twin.eight_graph()
    for remove in ([(3, 4, 4)], [(3, 4, 5), (3, 4, 5)], [(1, 0, 0)], [(8, 0, 0)]):
        with pytest.raises(twin.Refused):
            twin.apply_edges(n, off, tgt, lab, twin.triples(remove), None)
    with pytest.raises(twin.Refused):
        twin.apply_edges(n, off, tgt, lab, None, (np.array([0]), np.array([1])))


def test_header_states_the_contract():
    text = open(os.path.join(ROOT, "include", "helix_vec.h")).read()
    for name in ("hvx_csr_apply_edges", "hvx_csr_sizes", "hvx_csr_export"):
        assert re.search(r"\bint %s\(" % name, text), name
    flat = " ".join(text.split()).replace(" * ", " ")
    assert "LAST-stored arc" in flat
    assert "Edits are exclusive with every other call on the handle; there are no snapshots or generations for graphs" in flat


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("csr_edit") / "csr_edit_plan_probe"
    out = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "csr_edit_plan_probe.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def _run_probe(exe, tmp_path, n, remove, add, labelled=True):
    none = (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    remove, add = remove or none, add or none
    lines = [f"{n} {1 if labelled else 0} {remove[0].size} {add[0].size}"]
    for b in (remove, add):
        labs = b[2] if len(b) > 2 and b[2] is not None else np.zeros(b[0].size, np.uint32)
        lines += [f"{int(s)} {int(d)} {int(l)}" for s, d, l in zip(b[0], b[1], labs)]
    path = tmp_path / "batch.txt"
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    sides, cur = {}, None
    for line in run.stdout.splitlines():
        w = line.split()
        if w[0] == "side":
            cur = sides[w[1]] = dict(rows=[], dels=[], adds=[], cum=[])
        elif w[0] == "row":
            cur["rows"].append(int(w[1])); cur["dels"].append((int(w[3]), int(w[4]))); cur["adds"].append((int(w[6]), int(w[7]))); cur["cum"].append(int(w[9]))
        elif w[0] == "total":
            cur["cum"].append(int(w[1]))
        elif w[0] in ("dels", "adds"):
            cur[w[0] + "_list"] = [tuple(int(x) for x in p.split(":")) for p in w[1:]]
    return sides


def _hold_plan_to_twin(sides, n, off, tgt, lab, remove, add):
    """touched rows, per-row change of degree, the offsets after the edit and the order of each row's segments, for both adjacencies"""
    none = (np.zeros(0, np.uint64), np.zeros(0, np.uint64), np.zeros(0, np.uint32))
    remove, add = remove or none, add or none
    new = twin.apply_edges(n, off, tgt, lab, remove, add)
    old_a, new_a = twin.import_arrays(n, off, tgt, lab), twin.import_arrays(n, *new)
    for side, key, row_i, nbr_i in (("out", "out_offsets", 0, 1), ("in", "in_offsets", 1, 0)):
        p = sides[side]
        old_off, new_off = old_a[key].astype(np.int64), new_a[key].astype(np.int64)
        rows = np.array(p["rows"], np.int64)
        assert rows.tolist() == sorted(set(remove[row_i].tolist()) | set(add[row_i].tolist()))
        change = np.diff(new_off) - np.diff(old_off)
        per_row = np.array([(a1 - a0) - (d1 - d0) for (d0, d1), (a0, a1) in zip(p["dels"], p["adds"])], np.int64)
        assert per_row.tolist() == change[rows].tolist()
        assert np.count_nonzero(change) == np.count_nonzero(per_row)  # untouched rows keep their degree
        cum = np.array(p["cum"], np.int64)
        assert cum.tolist() == np.concatenate([[0], np.cumsum(per_row)]).tolist()
        # new_off[u] = old_off[u] + cum[touched rows below u]: what the device's offsets kernel computes
        below = np.searchsorted(rows, np.arange(n + 1), side="left")
        assert (old_off + cum[below]).tolist() == new_off.tolist()
        # segments: removals by (row, neighbour, label); additions by (row, neighbour), equal ones in batch order
        dr, dn, dl = remove[row_i].astype(np.int64), remove[nbr_i].astype(np.int64), remove[2].astype(np.int64)
        order = np.lexsort((dl, dn, dr))
        assert p["dels_list"] == list(zip(dn[order].tolist(), dl[order].tolist()))
        ar, an, al = add[row_i].astype(np.int64), add[nbr_i].astype(np.int64), add[2].astype(np.int64)
        order = np.lexsort((an, ar))
        assert p["adds_list"] == list(zip(an[order].tolist(), al[order].tolist()))
        assert [d1 - d0 for d0, d1 in p["dels"]] == [int(np.count_nonzero(dr == r)) for r in rows]
        assert [a1 - a0 for a0, a1 in p["adds"]] == [int(np.count_nonzero(ar == r)) for r in rows]


@pytest.mark.parametrize("case", sorted(twin.EIGHT_CASES))
def test_plan_of_the_hand_written_batches(probe, tmp_path, case):
    n, off, tgt, lab = twin.eight_graph()
    remove, add, _ = twin.EIGHT_CASES[case]
    remove, add = twin.triples(remove), twin.triples(add)
    _hold_plan_to_twin(_run_probe(probe, tmp_path, n, remove, add), n, off, tgt, lab, remove, add)


def test_plan_of_the_seeded_batch_on_g20k(probe, tmp_path):
    n, off, tgt, lab = fx.prefilter_graph("g20k")
    remove, add, facts = twin.g20k_batch(n, off, tgt, lab)
    assert 250 <= remove[0].size <= 350 and 450 <= add[0].size <= 550
    sides = _run_probe(probe, tmp_path, n, remove, add)
    _hold_plan_to_twin(sides, n, off, tgt, lab, remove, add)
    out = sides["out"]
    k = out["rows"].index(facts["hub"])
    assert out["dels"][k][1] - out["dels"][k][0] >= 40 and out["adds"][k][1] - out["adds"][k][0] >= 30  # the heavy row, many edits
    k = out["rows"].index(facts["many"])
    assert out["adds"][k][1] - out["adds"][k][0] > 64
    assert 0 in out["rows"] and n - 1 in out["rows"] and facts["sink"] in sides["in"]["rows"]


def test_plan_refuses_an_endpoint_outside_the_graph(probe, tmp_path):
    exe = probe
    (tmp_path / "b.txt").write_text("8 1 1 1\n3 4 3\n2 8 0\n")
    run = subprocess.run([str(exe), str(tmp_path / "b.txt")], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.split() == ["out", "of", "range", "1"]
