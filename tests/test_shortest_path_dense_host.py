"""hvx_shortest_path_batch_dense without a GPU: the plain-Python twin of the bit-parallel sweep (tests/shortest_path_dense_twin.py, written
as the kernels run it) held to the literal twin of the reference's loop and to twin.answers(max_reach=None) on random multigraphs and the
hand-written graph, the deep batches of tests/test_gpu_shortest_path_dense.py pinned as numbers from the existing twin, the export, what
the call refuses before it touches a device, and the round plan (csrc/hvx_shortest_path_dense_plan.h) as a stand-alone sanitized program."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import shortest_path_cases as sc
import shortest_path_dense_cases as dc
import shortest_path_dense_twin as dense
import shortest_path_twin as twin
from test_shortest_path_host import random_multigraph

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT, IN, BOTH = sc.OUT, sc.IN, sc.BOTH


def same(got, want, tag=None):
    paths, st, sizes = got
    wpaths, wst, wsizes = want
    assert [list(p) for p in paths] == [list(w) for w in wpaths], tag
    assert st.tolist() == wst.tolist(), tag
    assert sizes.shape == wsizes.shape and sizes.tolist() == wsizes.tolist(), tag


# ---- 1. the sweep's twin against the literal loop
def test_sweep_twin_on_the_hand_graph():
    g = sc.hand_graph()
    for (max_depth, direction, allowed), cases in sc.HAND_CASES.items():
        src, dst = [s for s, _, _ in cases], [d for _, d, _ in cases]
        got = dense.answers(g, src, dst, max_depth, direction, allowed)
        assert got[0] == [w for _, _, w in cases], (max_depth, direction, allowed)
        same(got, twin.answers(g, src, dst, max_depth, direction, allowed, max_reach=None), (max_depth, direction, allowed))
    # the levels written out in tests/test_shortest_path_host.py: the source is reached in level 3, which completes
    paths, st, sizes = dense.answers(g, [0, 6, 2, twin.NO_NODE, 2], [6, 0, 2, 2, twin.NO_NODE], 5, OUT)
    assert paths == [[0, 1, 5, 6], [], [2], [], []] and st.tolist() == [twin.OK] * 5
    assert sizes.tolist() == [[4, 7, 8, 8, 8], [1, 1, 1, 1, 1], [1, 1, 1, 1, 1], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0]]


BATCH_SIZES = (1, 2, 7, 63, 64, 65, 128, 129, 130)


def test_sweep_twin_on_random_multigraphs():
    """2 400 seeded multigraphs (tests/test_shortest_path_host.py's corpus), a batch each: a pool of pairs drawn with repeats, so targets
    and whole pairs repeat inside a group, with source == target and sentinel endpoints mixed in; one, two or three groups; budgets of one
    group (rounds) and of all of them"""
    rng = np.random.default_rng(2025)
    longer = multi_round = repeated_targets = 0
    for i in range(2400):
        g = random_multigraph(rng)
        direction = int(rng.integers(0, 3))
        allowed = [(), (), (0,), (0, 2)][int(rng.integers(0, 4))]
        max_depth = int(rng.integers(1, g.n + 2))
        b = int(BATCH_SIZES[int(rng.integers(0, len(BATCH_SIZES)))]) if rng.random() < 0.15 else int(rng.integers(1, 12))
        if i % 400 == 0:
            b = int(rng.integers(66, 131))
        pool = [(int(rng.integers(0, g.n)), int(rng.integers(0, g.n))) for _ in range(int(rng.integers(1, 9)))]
        pool += [(pool[0][1], pool[0][1]), (twin.NO_NODE, pool[0][1]), (pool[0][0], twin.NO_NODE)]
        weights = np.array([4.0] * (len(pool) - 3) + [1.0, 0.5, 0.5])
        pick = rng.choice(len(pool), b, p=weights / weights.sum())
        src, dst = [pool[k][0] for k in pick], [pool[k][1] for k in pick]
        known = {p: twin.answer(g, p[0], p[1], max_depth, direction, allowed, None) for p in set(pool)}
        want = ([known[pool[k]][0] for k in pick], np.array([known[pool[k]][1] for k in pick], np.uint32),
                np.array([known[pool[k]][2] for k in pick], np.uint64).reshape(b, max_depth))
        for p, (path, _, _) in known.items():   # the literal loop itself (answer() goes through it; said once more on purpose)
            if twin.NO_NODE not in p:
                assert path == twin.literal(g, p[0], p[1], max_depth, direction, allowed)
        one_group = g.n * dense.NODE_GROUP_BYTES
        stats = {}
        same(dense.answers(g, src, dst, max_depth, direction, allowed, scratch_bytes=one_group, stats=stats), want, (i, "one group a round"))
        assert stats["rounds"] == (b + 63) // 64 and all(w <= -(-max_depth // dense.RUN) + 1 for w in stats["waits"])
        if stats["rounds"] > 1:
            multi_round += 1
            same(dense.answers(g, src, dst, max_depth, direction, allowed), want, (i, "one round"))
        longer += sum(1 for p in want[0] if len(p) >= 3)
        repeated_targets += len(set(dst[:64])) < len(dst[:64])
    assert longer >= 1000 and multi_round >= 100 and repeated_targets >= 1000   # (the comparison is not of empty paths or lone requests)


def test_check_order_found_before_empty():
    """0 -> 1 and nothing else: from the target 1 the level that reaches the source 0 is also the last one that grows.  The request is found
    in level 1; one that asked the empty-first way round would call it 'no path' a level later or never"""
    g = twin.Graph.from_edges(2, [0], [1])
    paths, _, sizes = dense.answers(g, [0, 1], [1, 0], 3, OUT)
    assert paths == [[0, 1], []] and sizes.tolist() == [[2, 2, 2], [1, 1, 1]]


# ---- 2. the deep batches of the GPU file, by the existing twin alone
PINNED = {   # (the first four columns are the 64 random pairs' alone; refused_found counts the constructed requests too)
    "g70k_both6": dict(found=64, lengths=[3, 4, 5, 6], largest_reach=69594, refused=64, refused_found=64),
    "g70k_out8": dict(found=9, lengths=[7, 8, 9], largest_reach=24610, refused=7, refused_found=1),
    "g70k_in8": dict(found=6, lengths=[7, 9], largest_reach=30275, refused=9, refused_found=2),
    "g70k_out12_labelled": dict(found=5, lengths=[11, 12, 13], largest_reach=20490, refused=5, refused_found=1),
    "g20k_both6": dict(found=56, lengths=[3, 4, 5, 6, 7], largest_reach=19822, refused=33, refused_found=28),
}


@pytest.mark.parametrize("name", list(dc.DEEP_BATCHES))
def test_deep_batches_are_pinned(name):
    gname, src, dst, max_depth, direction, allowed, (paths, status, sizes), (paths16, status16, _) = dc.deep_batch(name)
    f = dc.facts(name)
    assert f == PINNED[name]
    assert f["refused_found"] >= 1        # a request the sibling refuses and this call answers with a path
    assert f["largest_reach"] > dc.SIBLING_REACH and (status == twin.OK).all()
    for q, (p, s, t) in enumerate(zip(paths, src, dst)):
        assert not len(p) or (p[0] == s and p[-1] == t and len(p) <= max_depth + 1)
        if status16[q] == twin.OK:       # what the sibling answers, this call answers alike
            assert paths16[q] == p
    sibling_found = sum(1 for p in paths16 if len(p))   # paths the sibling does return
    assert sibling_found == {"g70k_both6": 0, "g70k_out8": 9, "g70k_in8": 4, "g70k_out12_labelled": 5, "g20k_both6": 28}[name]


def test_g20k_out8_is_not_a_deep_batch():
    _, _, _, _, _, _, (_, status, _) = sc.g20k_batch("out8")
    assert (status == twin.OK).all()


# ---- 3. the export
def test_header_declares_and_library_exports_the_call():
    header = open(os.path.join(ROOT, "include", "helix_vec.h")).read()
    m = re.search(r"int hvx_shortest_path_batch_dense\(([^;]*)\);", header)
    assert m and "uint64_t scratch_bytes" in m.group(1) and m.group(1).count(",") == 12
    lib = os.path.join(ROOT, "helix-db_amd", "libhelix_vec_gfx950.so")
    if os.path.exists(lib):
        L = C.CDLL(lib)
        assert hasattr(L, "hvx_shortest_path_batch_dense")
    for doc in ("INTEGRATION.md", "README.md"):
        text = open(os.path.join(ROOT, doc)).read()
        assert "120" in text and "hvx_shortest_path_batch_dense" in text, doc


def test_refusals_that_need_no_device():
    import pyhvx as hv
    L = hv.lib()
    one = np.zeros(1, np.uint64)
    paths, lens, st = np.zeros(9, np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.hvx_shortest_path_batch_dense(None, 1, p(one), p(one), 8, OUT, None, 0, 0, p(paths), p(lens), p(st), None) == hv.ERR_INVARIANT
    assert L.hvx_shortest_path_batch_dense(None, 0, None, None, 8, OUT, None, 0, 0, p(paths), p(lens), p(st), None) == hv.ERR_INVARIANT


# ---- 4. the round plan alone, under the sanitizers
@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++") or "/opt/rocm/lib/llvm/bin/clang++"
    exe = tmp_path_factory.mktemp("sp_dense") / "sp_dense_plan_probe"
    out = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "sp_dense_plan_probe.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return exe


def plan_line(n, b, scratch):
    plan = dense.plan_rounds(n, b, scratch)
    if plan is None:
        return "refused"
    rounds = [dense.round_of(plan, b, r) for r in range(plan["rounds"])]
    head = [plan[k] for k in ("groups", "groups_per_round", "rounds", "words", "seen_off", "cur_off", "next_off", "lvl_off", "bytes")]
    return " ".join(str(x) for x in head + [sum(r[k] for r in rounds) for k in range(4)] + list(rounds[-1]))


def test_sanitized_plan_probe(probe, tmp_path):
    big = 2 ** 31 - 1
    cases = [(1, 1, 0), (1, 65535, 88), (1, 64, 87),                       # n = 1; one group exactly; one byte less
             (70001, 130, 70001 * 88), (70001, 130, 70001 * 88 - 1),       # exactly one group: three rounds; one byte less: refused
             (70001, 130, 2 * 70001 * 88 + 5), (70001, 130, 0), (20011, 65535, 0),
             (big, 65535, 0), (big, 65535, big * 88), (big, 65535, big * 88 - 1), (big, 65535, big * 88 * 1024), (big, 65535, 2 ** 64 - 1),
             (2 ** 20, 4096, 2 ** 40), (0, 3, 0)]
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{n} {b} {s}\n" for n, b, s in cases))
    run = subprocess.run([str(probe), str(path)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    got = run.stdout.splitlines()
    assert got == [plan_line(*c) for c in cases]
    by = dict(zip(cases, got))
    assert by[(1, 64, 87)] == by[(70001, 130, 70001 * 88 - 1)] == by[(big, 65535, 0)] == by[(big, 65535, big * 88 - 1)] == "refused"
    assert by[(70001, 130, 70001 * 88)].split()[:3] == ["3", "1", "3"]
    # b = 65 535 at n = 2^31 - 1 does not wrap: 1 024 groups of 88 x (2^31 - 1) bytes
    whole = [int(x) for x in by[(big, 65535, big * 88 * 1024)].split()]
    assert whole[:4] == [1024, 1024, 1, big * 1024] and whole[7] == big * 1024 * 24 and whole[8] == big * 1024 * 88 > 2 ** 47
    assert whole[-4:] == [0, 1024, 0, 65535]
    one = [int(x) for x in by[(big, 65535, big * 88)].split()]
    assert one[:4] == [1024, 1, 1024, big] and one[-4:] == [1023, 1, 1023 * 64, 63]
