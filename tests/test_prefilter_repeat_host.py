"""repeat(expand).times(n).emit() with PER-QUERY seeds (hvx_expand_repeat_lists, hvx_prefilter_repeat_search_lists_params): the literal
numpy twin of the reference's loop (control/repeat.rs:24-99, on sets) and the batches the GPU tests of tests/test_gpu_prefilter_repeat.py
run on fixtures.prefilter_graph("g70k").  The twin iterates fixtures.row_union WITHOUT visited exclusion -- the kernel walks breadth-first
with exclusion and must give the same sets --; its sizes are pinned here as numbers, so that a twin and a kernel that drift together are
caught."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
from test_prefilter_lists_host import MIXED_SEEDS
from test_prefilter_path_host import BOTH, IN, OUT, SMALL_LAB, SMALL_OFF, SMALL_TGT

BEFORE, AFTER, ALL = 1, 2, 3
MODES = {"before": BEFORE, "after": AFTER, "all": ALL}
_NONE = np.zeros(0, np.uint64)


def repeat_union(off, tgt, lab, seeds, direction, allowed, times, emit, until=None):
    """The loop of repeat.rs on sets: (emitted, |emitted| after every iteration, stop depth, |reach set| after every iteration).
    The reach set is the seeds (BEFORE / ALL) and every nxt so far: what max_frontier bounds.  Iterations the loop never ran repeat the
    last size."""
    cur = np.unique(np.asarray(seeds, np.uint64))
    emitted = _NONE
    reach = cur if emit in (BEFORE, ALL) else _NONE
    p = None if until is None else np.asarray(list(until), np.uint64)
    sizes, reach_sizes, stop_depth = [], [], 0
    for i in range(1, times + 1):
        if emit in (BEFORE, ALL):
            emitted = np.union1d(emitted, cur)
        nxt = fx.row_union(off, tgt, cur, lab, allowed, direction) if cur.size else _NONE   # no visited exclusion
        if emit in (AFTER, ALL):
            emitted = np.union1d(emitted, nxt)
        reach = np.union1d(reach, nxt)
        stop = p is not None and bool(np.isin(nxt, p).any())   # only nxt is tested: the seeds themselves never stop the loop
        cur = nxt
        sizes.append(int(emitted.size))
        reach_sizes.append(int(reach.size))
        if stop:
            stop_depth = i
        if cur.size == 0 or stop:
            break
    sizes += [sizes[-1]] * (times - len(sizes))
    reach_sizes += [reach_sizes[-1]] * (times - len(reach_sizes))
    return emitted.astype(np.uint64), sizes, stop_depth, reach_sizes


def reported(twin, max_frontier):
    """what the calls report for one request of the twin: (emitted ids, sizes, stop depth, overflowed).  The first iteration whose reach
    set exceeds max_frontier reports max_frontier + 1, later ones 0, no id and stop depth 0 -- also when `until` fired in it."""
    emitted, sizes, stop_depth, reach = twin
    over = [r > max_frontier for r in reach]
    if not any(over):
        return emitted, sizes, stop_depth, False
    at = over.index(True)
    return _NONE, sizes[:at] + [max_frontier + 1] + [0] * (len(sizes) - at - 1), 0, True


def small(seeds, direction, times, emit, allowed=(), until=None):
    e, sizes, stop, reach = repeat_union(SMALL_OFF, SMALL_TGT, SMALL_LAB, seeds, direction, allowed, times, emit, until)
    return e.tolist(), sizes, stop, reach


# ---- the hand-written graph: 0 -> 1, 2;  1 -> 1 (a self loop), 3;  2 -> 3;  4 <-> 5 (a two-cycle);  6 -> 7;  3 and 7 have no row
# seeds, direction, labels, times, until, then per mode (emitted, sizes, stop depth), worked out by hand from the loop
SMALL_REPEATS = [
    ([4], BOTH, (), 3, None, {BEFORE: ([4, 5], [1, 2, 2], 0), AFTER: ([4, 5], [1, 2, 2], 0), ALL: ([4, 5], [2, 2, 2], 0)}),
    ([1], OUT, (), 2, None, {BEFORE: ([1, 3], [1, 2], 0), AFTER: ([1, 3], [2, 2], 0), ALL: ([1, 3], [2, 2], 0)}),   # the self loop emits its seed
    ([6], OUT, (), 3, None, {BEFORE: ([6, 7], [1, 2, 2], 0), AFTER: ([7], [1, 1, 1], 0), ALL: ([6, 7], [2, 2, 2], 0)}),
    ([7], OUT, (), 3, None, {BEFORE: ([7], [1, 1, 1], 0), AFTER: ([], [0, 0, 0], 0), ALL: ([7], [1, 1, 1], 0)}),    # a seed without arcs
    # the two-cycle hands its seed back at iteration 2: `until` {4} fires there, never on the seed itself
    ([4], OUT, (), 5, (4,), {BEFORE: ([4, 5], [1, 2, 2, 2, 2], 2), AFTER: ([4, 5], [1, 2, 2, 2, 2], 2), ALL: ([4, 5], [2, 2, 2, 2, 2], 2)}),
    ([0, 0, 0], OUT, (), 2, None, {BEFORE: ([0, 1, 2], [1, 3], 0), AFTER: ([1, 2, 3], [2, 3], 0), ALL: ([0, 1, 2, 3], [3, 4], 0)}),
    ([0], OUT, (), 3, (3,), {BEFORE: ([0, 1, 2], [1, 3, 3], 2), AFTER: ([1, 2, 3], [2, 3, 3], 2), ALL: ([0, 1, 2, 3], [3, 4, 4], 2)}),
    ([0], OUT, (1,), 3, None, {BEFORE: ([0, 2], [1, 2, 2], 0), AFTER: ([2], [1, 1, 1], 0), ALL: ([0, 2], [2, 2, 2], 0)}),   # label 1: 0 -> 2, 2 has none
    ([3], IN, (), 2, None, {BEFORE: ([1, 2, 3], [1, 3], 0), AFTER: ([0, 1, 2], [2, 3], 0), ALL: ([0, 1, 2, 3], [3, 4], 0)}),
    ([0, 4, 6], BOTH, (), 1, None, {BEFORE: ([0, 4, 6], [3], 0), AFTER: ([1, 2, 5, 7], [4], 0), ALL: ([0, 1, 2, 4, 5, 6, 7], [7], 0)}),
    ([5], OUT, (), 4, (5,), {BEFORE: ([4, 5], [1, 2, 2, 2], 2), AFTER: ([4, 5], [1, 2, 2, 2], 2), ALL: ([4, 5], [2, 2, 2, 2], 2)}),
]


@pytest.mark.parametrize("case", range(len(SMALL_REPEATS)))
def test_twin_on_the_hand_written_graph(case):
    seeds, direction, allowed, times, until, want = SMALL_REPEATS[case]
    for emit, (emitted, sizes, stop) in want.items():
        assert small(seeds, direction, times, emit, allowed, until)[:3] == (emitted, sizes, stop), (case, emit)


def test_the_cases_the_loop_is_known_for():
    assert small([4], BOTH, 3, AFTER)[0] == [4, 5] and small([4], BOTH, 3, BEFORE)[0] == [4, 5]
    assert small([1], OUT, 2, AFTER)[0] == [1, 3]
    assert small([6], OUT, 3, ALL)[0] == [6, 7] and small([6], OUT, 3, BEFORE)[0] == [6, 7] and small([6], OUT, 3, AFTER)[0] == [7]
    assert small([7], OUT, 3, BEFORE)[0] == [7] and small([7], OUT, 3, AFTER)[0] == []
    assert [small([4], OUT, 5, m, until=(4,))[2] for m in (BEFORE, AFTER, ALL)] == [2, 2, 2]
    # the reach set counts the seeds for BEFORE and ALL only, and for BEFORE the last level although it is not emitted
    assert small([6], OUT, 1, BEFORE)[0] == [6] and small([6], OUT, 1, BEFORE)[3] == [2] and small([6], OUT, 1, AFTER)[3] == [1]


# ---- the batches on "g70k": name -> (seeds per query, direction, labels, times, max_frontier)
REPEAT_BATCHES = {
    "out3": (MIXED_SEEDS, OUT, (), 3, 16384),    # 32 768 table slots (128 KiB of LDS, opted in), more than half full
    "both2": (MIXED_SEEDS, BOTH, (1,), 2, 4096),  # both passes of the body; 8 192 slots (32 KiB)
    "in2": (MIXED_SEEDS, IN, (), 2, 4096),
}
# name -> mode -> pinned [query][iteration] sizes of the emitted set as the calls report them
PINNED = {
    "out3": {
        "all": [[0, 0, 0], [7, 28, 75], [1, 1, 1], [6, 23, 71], [13, 20, 41], [1319, 4904, 14273], [1233, 4565, 13384], [1319, 4904, 14273],
                [17, 74, 256], [18, 70, 220], [66, 260, 851], [998, 3862, 11677]],
        "after": [[0, 0, 0], [5, 26, 73], [0, 0, 0], [5, 22, 70], [9, 16, 37], [1255, 4843, 14218], [1169, 4504, 13334], [1255, 4843, 14218],
                  [16, 73, 255], [17, 69, 219], [65, 259, 850], [997, 3861, 11677]],
        "before": [[0, 0, 0], [2, 7, 28], [1, 1, 1], [1, 6, 23], [4, 13, 20], [64, 1319, 4904], [64, 1233, 4565], [64, 1319, 4904], [1, 17, 74],
                   [1, 18, 70], [1, 66, 260], [1, 998, 3862]],
    },
    "both2": {
        "all": [[0, 0], [8, 17], [2, 4], [4, 10], [9, 17], [562, 1593], [511, 1547], [562, 1593], [9, 37], [7, 28], [25, 78], [329, 987]],
        "after": [[0, 0], [6, 16], [1, 4], [3, 10], [5, 16], [498, 1584], [447, 1537], [498, 1584], [8, 37], [6, 28], [24, 78], [328, 987]],
        "before": [[0, 0], [2, 8], [1, 2], [1, 4], [4, 9], [64, 562], [64, 511], [64, 562], [1, 9], [1, 7], [1, 25], [1, 329]],
    },
    "in2": {
        "all": [[0, 0], [8, 23], [8, 26], [6, 24], [16, 63], [281, 972], [265, 887], [281, 972], [7, 25], [6, 19], [5, 21], [6, 19]],
        "after": [[0, 0], [6, 21], [7, 25], [5, 23], [12, 59], [217, 910], [201, 825], [217, 910], [6, 24], [5, 18], [4, 20], [5, 18]],
        "before": [[0, 0], [2, 8], [1, 8], [1, 6], [4, 16], [64, 281], [64, 265], [64, 281], [1, 7], [1, 6], [1, 5], [1, 6]],
    },
}

_TWIN = {}


def repeat_twin(name, mode, until=None, seeds=None, times=None):
    """[per query: repeat_union's tuple] of REPEAT_BATCHES[name] (other seeds / times on request), once per process; nobody changes the arrays"""
    key = (name, mode, until, None if seeds is None else tuple(map(tuple, seeds)), times)
    if key not in _TWIN:
        _, off, tgt, lab = fx.prefilter_graph("g70k")
        s, direction, allowed, t, _ = REPEAT_BATCHES[name]
        _TWIN[key] = [repeat_union(off, tgt, lab, x, direction, allowed, t if times is None else times, MODES[mode], until)
                      for x in (s if seeds is None else seeds)]
    return _TWIN[key]


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(REPEAT_BATCHES))
def test_pinned_sizes_per_query(name, mode):
    seeds, _, _, times, mf = REPEAT_BATCHES[name]
    got = [reported(t, mf)[1] for t in repeat_twin(name, mode)]
    assert got == PINNED[name][mode], (name, mode)
    assert all(len(s) <= mf for s in seeds) and all(len(r) == times for r in got)
    assert all(r == sorted(r) for r in got)   # without overflow a row is monotone


def test_pinned_rows_of_the_other_modes():
    assert repeat_twin("out3", "after")[5][1] == [1255, 4843, 14218]
    assert repeat_twin("out3", "before")[5][1] == [64, 1319, 4904]


# `until` = {1491}: requests, then stop depths and ALL sizes (Out, every label, times 4)
UNTIL_NODE = 1491
UNTIL_SEEDS = [[1020], [1021], [8191], list(range(1000, 1064))]
UNTIL_STOPS = [2, 0, 0, 2]
UNTIL_SIZES_ALL = [[17, 74, 74, 74], [18, 70, 220, 631], [3, 5, 10, 23], [1319, 4904, 4904, 4904]]


def test_until_on_g70k():
    twin = repeat_twin("out3", "all", until=(UNTIL_NODE,), seeds=UNTIL_SEEDS, times=4)
    assert [t[2] for t in twin] == UNTIL_STOPS and [t[1] for t in twin] == UNTIL_SIZES_ALL
    for mode in ("before", "after"):
        assert [t[2] for t in repeat_twin("out3", mode, until=(UNTIL_NODE,), seeds=UNTIL_SEEDS, times=4)] == UNTIL_STOPS


def test_the_seed_that_comes_back():
    """8191 <-> 8190 / 8192 under Both: the seed is an arc target again at iteration 2 -- already in the visited set of a walk with
    exclusion, so a test on fresh nodes only would miss it"""
    _, off, tgt, lab = fx.prefilter_graph("g70k")
    e, sizes, stop, _ = repeat_union(off, tgt, lab, [8191], BOTH, (), 3, ALL)
    assert sizes == [6, 25017, 64126] and stop == 0
    e, sizes, stop, _ = repeat_union(off, tgt, lab, [8191], BOTH, (), 3, ALL, until=(8191,))
    assert sizes == [6, 25017, 25017] and stop == 2
    # a predicate that holds only seeds which no arc reaches again stops nothing
    assert [repeat_union(off, tgt, lab, [s], OUT, (), 3, ALL, until=(1020, 1021))[2] for s in (1020, 1021)] == [0, 0]


# the batch of the overflow test: max_frontier 1 000 on "out3"; the hub's 25 000-arc row against the 4 096-slot floor
OVERFLOW_MF = 1000
HUB = ([[2000]], OUT, (), 2, 8)


def test_what_the_batches_are_for():
    _, off, tgt, lab = fx.prefilter_graph("g70k")
    off = off.astype(np.int64)
    rows = {1020: 16, 1021: 17, 1030: 65, 1040: 1000, 2000: 25000}   # the light / heavy split 16 | 17, a wavefront's width, a long row, the hub
    assert {u: int(off[u + 1] - off[u]) for u in rows} == rows
    assert [MIXED_SEEDS[i] for i in (8, 9, 10, 11)] == [[1020], [1021], [1030], [1040]]
    assert MIXED_SEEDS[0] == [] and len(set(MIXED_SEEDS[1])) < len(MIXED_SEEDS[1])          # no seeds; duplicated seeds
    assert repeat_twin("out3", "after")[2][0].size == 0 and repeat_twin("out3", "all")[2][0].tolist() == [8000]   # a dead end emits its seed at most
    # the table: more than half full at the largest slot, and a slot under the 48 KiB a workgroup gets without asking
    assert max(max(t[3]) for t in repeat_twin("out3", "all")) == 14273 > 8192 and REPEAT_BATCHES["out3"][4] * 2 * 4 == 128 * 1024
    assert REPEAT_BATCHES["both2"][4] * 2 * 4 < 48 * 1024
    # nothing of the three batches overflows; at max_frontier 1 000 request 5 does at iteration 1, request 11 at iteration 2, the island never
    for name in REPEAT_BATCHES:
        for mode in MODES:
            assert not any(reported(t, REPEAT_BATCHES[name][4])[3] for t in repeat_twin(name, mode)), (name, mode)
    rep = [reported(t, OVERFLOW_MF) for t in repeat_twin("out3", "all")]
    assert rep[5][1] == [1001, 0, 0] and rep[11][1] == [998, 1001, 0] and rep[4][1] == [13, 20, 41] and not rep[4][3]
    assert [r[3] for r in rep] == [False] * 5 + [True] * 3 + [False] * 3 + [True]
    # BEFORE overflows on its reach set although what it emits would fit: [1040] at iteration 1 holds 998 nodes and emits one
    t = repeat_twin("out3", "before")[11]
    assert t[1][0] == 1 and t[3][0] == 998 and reported(repeat_union(off, tgt, lab, [1040], OUT, (), 1, BEFORE), 997)[3]
    hub = repeat_union(off, tgt, lab, HUB[0][0], OUT, (), 2, ALL)
    assert hub[3][0] == 25001 and reported(hub, HUB[4])[1] == [9, 0]


def test_null_handles_are_refused_before_the_device_is_touched():
    import pyhvx as hv
    assert (hv.REPEAT_EMIT_BEFORE, hv.REPEAT_EMIT_AFTER, hv.REPEAT_EMIT_ALL) == (BEFORE, AFTER, ALL)
    L = hv.lib()
    one = np.zeros(4, np.uint64)
    u32 = np.zeros(4, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.hvx_expand_repeat_lists(None, 1, ptr(one), ptr(one), 1, ALL, OUT, None, 0, None, None, 16, ptr(one), ptr(u32), ptr(u32), None,
                                     None) == hv.ERR_INVARIANT
    rp = hv.RestrictedParams(k=1, ef=1, strategy=hv.RESTRICTED_EXACT)
    assert L.hvx_prefilter_repeat_search_lists_params(None, None, None, 0, C.byref(rp), ptr(one), ptr(one), 1, ALL, OUT, None, 0, None, None, 16,
                                                      ptr(one), ptr(u32), ptr(u32), ptr(u32), None, None, None, None) == hv.ERR_INVARIANT
