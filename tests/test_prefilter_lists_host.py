"""Chains of `expand` hops with PER-QUERY seeds (hvx_expand_path_lists, hvx_prefilter_path_search_lists_params): the batches the GPU tests
of tests/test_gpu_prefilter_lists.py run on fixtures.prefilter_graph("g70k").  The per-query twin is path_union of
tests/test_prefilter_path_host.py called once per query; every query's per-hop sizes are pinned here as numbers, so that a twin and a
kernel that drift together are caught."""
import ctypes as C

import numpy as np
import pytest

import fixtures as fx
from test_prefilter_path_host import BOTH, IN, OUT, SMALL_CASES, norm_hops, path_union


def _run(a, b):
    return list(range(a, b))


# one seed list per query: the empty list, duplicated seeds, a dead end, a vectorless intermediate set, the island, two overlapping groups,
# the first group a second time, and the single rows on both sides of the light / heavy split (16 | 17) and of a wavefront's width (65)
MIXED_SEEDS = [[], [1000, 1000, 1010, 1010, 1000], [8000], [2001], list(fx.ISLAND_SEEDS), _run(1000, 1064), _run(1032, 1096), _run(1000, 1064),
               [1020], [1021], [1030], [1040]]

# name -> (seeds per query, hops, max_frontier, pinned per-query per-hop sizes of the twin)
LIST_BATCHES = {
    # 8 192 table slots (32 KiB of LDS)
    "plain": (MIXED_SEEDS, [OUT, OUT], 4096,
              [[0, 0], [5, 21], [0, 0], [5, 17], [9, 9], [1255, 3657], [1169, 3386], [1255, 3657], [16, 58], [17, 52], [65, 194], [997, 2903]]),
    # a label set per hop, the largest slot there is: 32 768 table slots (128 KiB of LDS, opted in)
    "labelled": (MIXED_SEEDS, [(OUT, (0, 1)), (IN, (2,)), (OUT, (1,))], 16384,
                 [[0, 0, 0], [4, 2, 72], [0, 0, 0], [4, 2, 1], [6, 9, 8464], [810, 800, 9607], [746, 811, 9512], [810, 800, 9607], [13, 9, 8463],
                  [9, 7, 8462], [44, 48, 8497], [630, 636, 9073]]),
    # both passes of a hop; 3000 has a long INCOMING row, 2002 is 300 parallel edges to five nodes
    "both": ([_run(1000, 1700), _run(1000, 1064), [3000], [2002]], [(BOTH, (1,)), (OUT, (2,))], 4096, [[1759, 2189], [498, 476], [80, 63], [8, 9]]),
    # the first query outgrows its slot at the first hop (reported as max_frontier + 1, later hops 0), the others are exact
    "overflow": ([_run(1000, 1064), list(fx.ISLAND_SEEDS), [1020]], [OUT, OUT, OUT], 1000, [[1001, 0, 0], [9, 9, 23], [16, 58, 188]]),
    # a 25 000-arc row against the 4 096-slot floor of the table
    "hub": ([[2000]], [OUT, OUT], 8, [[9, 0]]),
}
MANY = 300   # more queries than the chip has compute units: seeds 1000 .. 1299, one hop OUT

_TWIN = {}


def lists_twin(name):
    """[per query: every hop's set] of LIST_BATCHES[name] by the twin, once per process; nobody changes the arrays"""
    if name not in _TWIN:
        _, off, tgt, lab = fx.prefilter_graph("g70k")
        seeds, hops, _, _ = LIST_BATCHES[name]
        _TWIN[name] = [path_union(off, tgt, lab, s, hops) for s in seeds]
    return _TWIN[name]


def clipped(sizes, max_frontier):
    """what the calls report for a chain of these sizes: the first set above max_frontier as max_frontier + 1, later hops as 0"""
    out, over = [], False
    for s in sizes:
        out.append(0 if over else (max_frontier + 1 if s > max_frontier else s))
        over = over or s > max_frontier
    return out, over


def small_groups():
    """SMALL_CASES of the hand-written graph grouped by chain: [(hops, [seeds per query], [final set per query], [sizes per query])]"""
    groups = {}
    for seeds, hops, want in SMALL_CASES:
        groups.setdefault(tuple(norm_hops(hops)), []).append((seeds, want))
    return [(list(h), [s for s, _ in g], [w[-1] for _, w in g], [[len(f) for f in w] for _, w in g]) for h, g in groups.items()]


@pytest.mark.parametrize("name", list(LIST_BATCHES))
def test_pinned_sizes_per_query(name):
    seeds, hops, max_frontier, pinned = LIST_BATCHES[name]
    assert len(pinned) == len(seeds)
    for q, sets in enumerate(lists_twin(name)):
        assert clipped([int(f.size) for f in sets], max_frontier)[0] == pinned[q], (name, q)
        assert len(seeds[q]) <= max_frontier


def test_what_the_batches_are_for():
    _, off, tgt, _ = fx.prefilter_graph("g70k")
    off = off.astype(np.int64)
    rows = {1020: 16, 1021: 17, 1030: 65, 1040: 1000, 2000: 25000}
    assert {u: int(off[u + 1] - off[u]) for u in rows} == rows
    plain = lists_twin("plain")
    a, b = set(plain[5][-1].tolist()), set(plain[6][-1].tolist())
    assert len(a & b) == 3127 and a - b and b - a                       # two frontiers that really overlap: each query owes its FULL set
    assert MIXED_SEEDS[5] == MIXED_SEEDS[7] and MIXED_SEEDS[5] != MIXED_SEEDS[6]
    assert plain[0][-1].size == 0 and plain[2][0].size == 0             # no seeds; a dead end
    assert plain[3][0].tolist() == sorted(fx.VECTORLESS)                # an intermediate set without a vector in either image
    assert len(set(MIXED_SEEDS[1])) < len(MIXED_SEEDS[1])
    # the two slot sizes: under and over the 48 KiB a workgroup gets without asking, the second the largest there is
    assert LIST_BATCHES["plain"][2] * 2 * 4 < 48 * 1024 < LIST_BATCHES["labelled"][2] * 2 * 4 == 128 * 1024
    assert max(max(s) for s in LIST_BATCHES["labelled"][3]) > 8192      # ... and more than half full
    # overflow: the first query only, at its first hop; the hub against the smallest table
    assert [clipped([int(f.size) for f in s], 1000)[1] for s in lists_twin("overflow")] == [True, False, False]
    assert [int(f.size) for f in lists_twin("hub")[0]] == [25000, 45945]
    # more queries than compute units, every set inside its slot
    _, off64, tgt64, lab = fx.prefilter_graph("g70k")
    assert MANY > 256 and max(path_union(off64, tgt64, lab, [s], [OUT])[0].size for s in range(1000, 1000 + MANY)) == 997


def test_small_cases_group_by_chain():
    groups = small_groups()
    assert sum(len(g[1]) for g in groups) == len(SMALL_CASES) and max(len(g[1]) for g in groups) >= 4
    assert any(h == [(BOTH, ()), (BOTH, ())] for h, _, _, _ in groups) and any(h == [(IN, ()), (IN, ())] for h, _, _, _ in groups)


def test_null_handles_are_refused_before_the_device_is_touched():
    import pyhvx as hv
    L = hv.lib()
    one = np.zeros(4, np.uint64)
    u32 = np.zeros(4, np.uint32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    assert L.hvx_expand_path_lists(None, 1, ptr(one), ptr(one), 1, ptr(u32), None, None, None, 16, ptr(one), ptr(u32), ptr(u32), None) == hv.ERR_INVARIANT
    rp = hv.RestrictedParams(k=1, ef=1, strategy=hv.RESTRICTED_EXACT)
    assert L.hvx_prefilter_path_search_lists_params(None, None, None, 0, C.byref(rp), ptr(one), ptr(one), 1, ptr(u32), None, None, None, 16, ptr(one),
                                                    ptr(u32), ptr(u32), ptr(u32), None, None, None) == hv.ERR_INVARIANT
