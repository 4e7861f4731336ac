"""shortest_path without a GPU (hvx_shortest_path_host, and what hvx_shortest_path_batch refuses before it touches a device): the literal
twin of the reference's loop (tests/shortest_path_twin.py) on a hand-written graph, the lexicographic characterisation the device kernel
rests on held to that loop on random multigraphs, the library's host loop and the stand-alone sanitized probe held to the twin, and the
g20k batches of tests/test_gpu_shortest_path.py pinned as numbers, so that the GPU file cannot pass by comparing nothing."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import shortest_path_cases as sc
import shortest_path_twin as twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT, IN, BOTH = sc.OUT, sc.IN, sc.BOTH


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def random_multigraph(rng):
    """2 .. 14 nodes, parallel edges and self-loops allowed, three labels, three in ten symmetrised"""
    n = int(rng.integers(2, 15))
    m = int(rng.integers(0, 3 * n + 1))
    src, dst = rng.integers(0, n, m), rng.integers(0, n, m)
    if rng.random() < 0.3:
        src, dst = np.concatenate([src, dst]), np.concatenate([dst, src])
    return twin.Graph.from_edges(n, src, dst, rng.integers(0, 3, src.size))


# ---- 1. the twin itself
def test_hand_written_graph():
    g = sc.hand_graph()
    for (max_depth, direction, allowed), cases in sc.HAND_CASES.items():
        for source, target, want in cases:
            assert twin.literal(g, source, target, max_depth, direction, allowed) == want, (max_depth, direction, allowed, source, target)


def test_hand_graph_traps_the_other_searches():
    """0 -> 6: what a depth-first search (smallest neighbour first) and a smallest-predecessor search from the target would return are
    both paths of the graph, and neither is the answer"""
    g = sc.hand_graph()
    off, nbr = g.plan(OUT)
    arcs = {(u, int(v)) for u in range(g.n) for v in nbr[off[u]:off[u + 1]]}
    for other in ([0, 1, 4, 7, 6], [0, 2, 3, 6]):
        assert all(a in arcs for a in zip(other, other[1:]))
    assert twin.literal(g, 0, 6, 8, OUT) == [0, 1, 5, 6]


def test_reach_sizes_and_overflow_rule_by_hand():
    g = sc.hand_graph()
    # from 6 backwards under Out: {6} -> {3, 5, 7} -> {1, 2, 4} -> {0}: the source is reached in level 3, which completes
    assert twin.answer(g, 0, 6, 5, OUT) == ([0, 1, 5, 6], twin.OK, [4, 7, 8, 8, 8])
    assert twin.answer(g, 0, 6, 2, OUT) == ([], twin.OK, [4, 7])
    assert twin.answer(g, 0, 6, 5, OUT, max_reach=7) == ([], twin.ERR_CANDIDATE_LIMIT, [4, 7, 8, 0, 0])   # overflow wins over the source found
    assert twin.answer(g, 0, 6, 5, OUT, max_reach=8) == ([0, 1, 5, 6], twin.OK, [4, 7, 8, 8, 8])
    assert twin.answer(g, 0, 6, 5, OUT, max_reach=3) == ([], twin.ERR_CANDIDATE_LIMIT, [4, 0, 0, 0, 0])
    assert twin.answer(g, 6, 0, 4, OUT) == ([], twin.OK, [1, 1, 1, 1])          # nothing enters 0: the first level is empty
    assert twin.answer(g, 2, 2, 3, OUT) == ([2], twin.OK, [1, 1, 1])
    assert twin.answer(g, twin.NO_NODE, 2, 3, OUT) == ([], twin.OK, [0, 0, 0])
    assert twin.answer(g, 2, twin.NO_NODE, 3, OUT) == ([], twin.OK, [0, 0, 0])


def test_lexicographic_characterisation_on_random_multigraphs():
    rng = np.random.default_rng(2024)
    longer = 0
    for i in range(2500):
        g = random_multigraph(rng)
        direction = int(rng.integers(0, 3))
        allowed = [(), (), (0,), (0, 2)][int(rng.integers(0, 4))]
        max_depth = int(rng.integers(1, g.n + 2))
        for _ in range(4):
            s, t = int(rng.integers(0, g.n)), int(rng.integers(0, g.n))
            want = twin.literal(g, s, t, max_depth, direction, allowed)
            assert twin.lexicographic(g, s, t, max_depth, direction, allowed) == want, (i, s, t, max_depth, direction, allowed)
            longer += len(want) >= 3
    assert longer >= 1000   # (the comparison is not of empty paths)


# ---- 2. the g20k batches of the GPU file, by the twin alone
PINNED = {
    "out8": dict(found=21, overflowed=0, lengths=[7, 8, 9], largest_reach=12190),
    "both5": dict(found=37, overflowed=13, lengths=[4, 5, 6], largest_reach=15755),
    "out8_small": dict(found=2, overflowed=56, lengths=[7], largest_reach=780),
    "labelled10": dict(found=5, overflowed=0, lengths=[10, 11], largest_reach=5342),
}


@pytest.mark.parametrize("name", list(sc.G20K_BATCHES))
def test_g20k_batches_are_pinned(name):
    src, dst, max_depth, direction, allowed, max_reach, (paths, status, sizes) = sc.g20k_batch(name)
    f = sc.facts(paths, status, sizes, max_reach)
    assert f == PINNED[name]
    b = src.size
    not_found = sum(1 for p, s in zip(paths, status) if not len(p) and s == twin.OK)
    if name == "out8":
        assert f["found"] * 4 >= b and len(f["lengths"]) >= 3 and f["overflowed"] == 0
    elif name == "both5":
        assert f["found"] >= 8 and f["overflowed"] >= 8 and not_found >= 1
    elif name == "out8_small":
        assert f["overflowed"] * 2 >= b and f["found"] >= 1
    else:
        assert f["found"] >= 1
    for p, s, t in zip(paths, src, dst):
        assert not len(p) or (p[0] == s and p[-1] == t and len(p) <= max_depth + 1)


# ---- 3. the library's host loop
def test_library_host_loop_on_the_hand_graph(hv):
    g = sc.hand_graph()
    n, off, tgt, lab = g.arrays()
    for (max_depth, direction, allowed), cases in sc.HAND_CASES.items():
        for source, target, want in cases:
            got = hv.shortest_path_host(n, off, tgt, lab, source, target, max_depth, direction, allowed)
            assert got.dtype == np.uint64 and got.tolist() == want, (max_depth, direction, allowed, source, target)
    assert hv.shortest_path_host(n, off, tgt, None, 0, 6, 8, OUT, (0, 2)).tolist() == [0, 1, 5, 6]   # unlabelled: every arc passes
    assert hv.shortest_path_host(n, off, tgt, lab, hv.NO_NODE, 6, 8).size == 0
    assert hv.shortest_path_host(n, off, tgt, lab, 0, hv.NO_NODE, 8).size == 0


@pytest.mark.parametrize("name", list(sc.G20K_BATCHES))
def test_library_host_loop_on_the_g20k_batches(hv, name):
    src, dst, max_depth, direction, allowed, _, _ = sc.g20k_batch(name)
    g = sc.g20k()
    n, off, tgt, lab = g.arrays()
    found = 0
    for s, t in zip(src.tolist(), dst.tolist()):
        want = twin.literal(g, s, t, max_depth, direction, allowed)   # the literal loop: max_reach is the device's matter
        assert hv.shortest_path_host(n, off, tgt, lab, s, t, max_depth, direction, allowed).tolist() == want, (s, t)
        found += len(want) > 0
    assert found >= 1


# ---- 4. refusals, before any device is touched
def test_null_handles_and_bad_arguments(hv):
    L = hv.lib()
    one = np.zeros(1, np.uint64)
    paths, lens, st = np.zeros(9, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.hvx_shortest_path_batch(None, 1, p(one), p(one), 8, OUT, None, 0, 16384, p(paths), p(lens), p(st), None) == hv.ERR_INVARIANT
    assert L.hvx_shortest_path_batch(None, 0, None, None, 8, OUT, None, 0, 16384, p(paths), p(lens), p(st), None) == hv.ERR_INVARIANT
    g = sc.hand_graph()
    n, off, tgt, lab = g.arrays()
    ln = C.c_uint32(7)
    host = lambda **kw: L.hvx_shortest_path_host(*[{**dict(n=n, e=tgt.size, off=p(off), tgt=p(tgt), lab=p(lab), s=0, t=6, md=8, d=OUT, al=None, nl=0,
                                                           out=p(paths), ln=C.byref(ln)), **kw}[k]
                                                   for k in ("n", "e", "off", "tgt", "lab", "s", "t", "md", "d", "al", "nl", "out", "ln")])
    assert host() == hv.OK and ln.value == 4
    for bad in (dict(off=None), dict(tgt=None), dict(out=None), dict(ln=None), dict(d=3), dict(md=0), dict(s=8), dict(t=8), dict(t=2 ** 63),
                dict(nl=2), dict(e=tgt.size - 1), dict(n=7)):
        assert host(**bad) == hv.ERR_INVARIANT, bad
    with pytest.raises(hv.HelixDbError):
        hv.shortest_path_host(n, off, tgt, lab, 0, 6, 0)


# ---- 5. the host header alone, under the sanitizers
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path_factory.mktemp("shortest_path") / "shortest_path_host_probe"
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "shortest_path_host_probe.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def run_probe(exe, path, g, requests):
    lines = [f"{g.n} {g.out_tgt.size} {0 if g.out_lab is None else 1}"]
    owner = np.repeat(np.arange(g.n), np.diff(g.out_off))
    labs = np.zeros(g.out_tgt.size, np.int64) if g.out_lab is None else g.out_lab
    lines += [f"{u} {v} {l}" for u, v, l in zip(owner.tolist(), g.out_tgt.tolist(), labs.tolist())]
    lines.append(str(len(requests)))
    lines += [" ".join(str(x) for x in (s, t, md, d, len(al), *al)) for s, t, md, d, al in requests]
    path.write_text("\n".join(lines) + "\n")
    run = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = [[int(x) for x in line.split()] for line in run.stdout.splitlines()]
    assert len(got) == len(requests) and all(row[0] == len(row) - 1 for row in got)
    return [row[1:] for row in got]


def test_sanitized_probe_on_the_hand_graph(probe, tmp_path):
    g = sc.hand_graph()
    requests = [(s, t, md, d, al) for (md, d, al), cases in sc.HAND_CASES.items() for s, t, _ in cases]
    want = [w for cases in sc.HAND_CASES.values() for _, _, w in cases]
    assert run_probe(probe, tmp_path / "hand.txt", g, requests) == want


def test_sanitized_probe_on_a_random_graph(probe, tmp_path):
    rng = np.random.default_rng(11)
    n = 300
    src, dst = rng.integers(0, n, 900), rng.integers(0, n, 900)
    g = twin.Graph.from_edges(n, src, dst, rng.integers(0, 3, 900))
    requests = [(int(rng.integers(0, n)), int(rng.integers(0, n)), int(rng.integers(1, 12)), int(rng.integers(0, 3)), [(), (1,), (0, 2)][int(rng.integers(0, 3))])
                for _ in range(200)]
    want = [twin.literal(g, *r) for r in requests]
    assert sum(1 for w in want if len(w) >= 3) >= 50
    assert run_probe(probe, tmp_path / "random.txt", g, requests) == want
