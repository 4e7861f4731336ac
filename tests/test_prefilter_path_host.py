"""The numpy twin of a chain of `expand` hops (access/expand.rs:16-80, node output, set semantics) and the cases the GPU tests of
tests/test_gpu_prefilter_path.py run on fixtures.prefilter_graph("g70k").  The twin iterates fixtures.row_union; its per-hop sizes on
those cases are pinned here as numbers, so that a twin and a kernel that drift together are caught."""
import numpy as np
import pytest

import fixtures as fx

OUT, IN, BOTH = 0, 1, 2


def norm_hops(hops):
    """[(direction, allowed labels) or a bare direction] -> [(direction, tuple of labels)]"""
    return [(int(h), ()) if isinstance(h, (int, np.integer)) else (int(h[0]), tuple(int(x) for x in h[1])) for h in hops]


def path_union(off, tgt, lab, seeds, hops):
    """F(1) .. F(n_hops) of the chain from `seeds`: F(i + 1) = row_union(F(i)) under hop i's direction and allow-set.  No visited
    exclusion; an empty frontier stays empty.  Returns a list of ascending uint64 arrays, one per hop."""
    front = np.unique(np.asarray(seeds, np.uint64))
    out = []
    for direction, allowed in norm_hops(hops):
        front = fx.row_union(off, tgt, front, lab, allowed, direction) if front.size else np.zeros(0, np.uint64)
        out.append(front)
    return out


# ---- the hand-written graph: 0 -> 1, 2;  1 -> 1 (a self loop), 3;  2 -> 3;  4 <-> 5 (a two-cycle);  6 -> 7;  3 and 7 have no row
SMALL_OFF = np.array([0, 2, 4, 5, 5, 6, 7, 8, 8], np.uint64)
SMALL_TGT = np.array([1, 2, 1, 3, 3, 5, 4, 7], np.uint64)
SMALL_LAB = np.array([0, 1, 0, 1, 0, 0, 1, 0], np.uint32)

SMALL_CASES = [
    # seeds, hops, every hop's set
    ([0], [OUT, OUT], [[1, 2], [1, 3]]),
    ([0, 0, 0], [OUT, OUT], [[1, 2], [1, 3]]),                       # duplicated seeds collapse
    ([1], [OUT], [[1, 3]]),                                          # the self loop keeps 1
    ([1], [OUT, OUT, OUT], [[1, 3], [1, 3], [1, 3]]),
    ([4], [BOTH, BOTH], [[5], [4]]),                                 # the two-cycle hands its seed back
    ([4], [OUT, OUT, OUT], [[5], [4], [5]]),
    ([3], [IN, IN], [[1, 2], [0, 1]]),
    ([0], [(OUT, [0]), (OUT, [1])], [[1], [3]]),                     # a label per hop
    ([0], [(OUT, [1]), (OUT, [1])], [[2], []]),
    ([0], [(OUT, [0, 1]), (IN, [])], [[1, 2], [0, 1]]),              # an empty allow-set means every label
    ([6], [OUT, OUT], [[7], []]),                                    # a node without arcs drops out
    ([7], [OUT, OUT], [[], []]),
    ([1], [BOTH], [[0, 1, 3]]),
    ([0, 4, 6], [OUT, BOTH], [[1, 2, 5, 7], [0, 1, 3, 4, 6]]),
]


@pytest.mark.parametrize("seeds,hops,want", SMALL_CASES)
def test_twin_on_the_hand_written_graph(seeds, hops, want):
    got = path_union(SMALL_OFF, SMALL_TGT, SMALL_LAB, seeds, hops)
    assert [f.tolist() for f in got] == want


def test_two_cycle_seed_comes_back():
    assert 4 in path_union(SMALL_OFF, SMALL_TGT, SMALL_LAB, [4], [BOTH, BOTH])[1].tolist()


# ---- the cases on "g70k": name -> (seeds, hops, pinned per-hop sizes)
def _run(a, b):
    return np.arange(a, b, dtype=np.uint64)


PATH_CASES = {
    "island2": (np.array(fx.ISLAND_SEEDS, np.uint64), [OUT, OUT], [9, 9]),
    "group_oio": (_run(1000, 1064), [OUT, IN, OUT], [1255, 3953, 33529]),
    "group3": (_run(1000, 1064), [OUT, OUT, OUT], [1255, 3657, 10316]),
    "labelled": (_run(1000, 1700), [(BOTH, (1,)), (OUT, (2,))], [1759, 2189]),
    "label_then_any": (_run(1000, 1064), [(OUT, (0,)), (IN, ())], [395, 1233]),
    "hubrow": (np.array([2000], np.uint64), [OUT, OUT], [25000, 45945]),
    "5000": (_run(1000, 6000), [OUT, OUT], [34165, 53748]),
    "dead_end": (np.array([8000], np.uint64), [OUT, OUT], [0, 0]),
    "vectorless": (np.array([2001], np.uint64), [OUT, IN], [5, 14]),
    "cycle": (np.array([8191], np.uint64), [BOTH, BOTH], [5, 25016]),
}

_TWIN = {}


def path_twin(name):
    """every hop's set of PATH_CASES[name] by the twin, computed once per process; nobody changes the arrays"""
    if name not in _TWIN:
        _, off, tgt, lab = fx.prefilter_graph("g70k")
        seeds, hops, _ = PATH_CASES[name]
        _TWIN[name] = path_union(off, tgt, lab, seeds, hops)
    return _TWIN[name]


@pytest.mark.parametrize("name", list(PATH_CASES))
def test_pinned_sizes_on_g70k(name):
    assert [int(f.size) for f in path_twin(name)] == PATH_CASES[name][2]


def test_what_the_cases_are_for():
    _, off, tgt, _ = fx.prefilter_graph("g70k")
    off = off.astype(np.int64)
    final = path_twin("island2")[-1]
    assert fx.bitmap_blocks(final) == [0, 1, 2, 3, 6] and fx.has_empty_block_between(final)
    # F(2) of group_oio -- a frontier the kernel reads from a BITMAP -- holds rows on both sides of the light / heavy split (16 | 17)
    # and of one wavefront's width (65), a long row and the hub
    f2 = set(path_twin("group_oio")[1].tolist())
    rows = {1010: 1, 1020: 16, 1021: 17, 1030: 65, 1040: 1000, 2000: 25000}
    assert set(rows) <= f2
    assert {u: int(off[u + 1] - off[u]) for u in rows} == rows
    assert 8191 in path_twin("cycle")[1].tolist()
    assert path_twin("dead_end")[0].size == 0
    # vectorless: the intermediate frontier is the five ids that hold no vector in either image
    assert path_twin("vectorless")[0].tolist() == sorted(fx.VECTORLESS)
