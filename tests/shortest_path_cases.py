"""The shortest-path cases the CPU and the GPU tests share: the hand-written eight-node graph with its expectations, and the g20k batches
(tests/test_shortest_path_host.py pins what the twin says about them, tests/test_gpu_shortest_path.py runs them on the device).  The twin's
answers are computed once per process and nobody changes them."""
import numpy as np

import fixtures as fx
import shortest_path_twin as twin

OUT, IN, BOTH = twin.DIR_OUT, twin.DIR_IN, twin.DIR_BOTH

# Eight nodes.  From 0 to 6 there are two shortest paths, 0 1 5 6 and 0 2 3 6: the reference returns the first.  A depth-first search that
# takes the smallest neighbour first runs 0 1 4 7 6; a search that gives every node its smallest predecessor, from the target back, returns
# 0 2 3 6.  2 <-> 3 is a two-cycle, 5 -> 5 a self-loop, 0 -> 2 and 1 -> 5 are parallel edges with different labels; both arcs into 6 on the
# short paths carry label 1, so the allow-set (0, 2) leaves only 0 1 4 7 6.  Nothing leaves 6.
HAND_N = 8
HAND_EDGES = [  # (source, target, label)
    (0, 1, 0), (0, 2, 1), (0, 2, 2), (1, 4, 0), (1, 5, 0), (1, 5, 1), (2, 3, 0), (3, 2, 0), (3, 6, 1), (4, 7, 2), (5, 5, 0), (5, 6, 1), (7, 6, 0),
]
# (max_depth, direction, allowed labels) -> [(source, target, the path written by hand)]
HAND_CASES = {
    (3, OUT, ()): [(0, 6, [0, 1, 5, 6]),      # max_depth = the distance; the smaller of two equal paths
                   (2, 2, [2]),               # source == target
                   (3, 2, [3, 2]), (2, 3, [2, 3]),   # the two-cycle
                   (5, 6, [5, 6]),            # past the self-loop
                   (5, 5, [5]),
                   (6, 0, []),                # nothing leaves 6
                   (0, 7, [0, 1, 4, 7]),
                   (1, 3, [])],               # 1 never reaches 3
    (2, OUT, ()): [(0, 6, []), (0, 5, [0, 1, 5]), (0, 3, [0, 2, 3])],   # one below the distance
    (8, OUT, (0, 2)): [(0, 6, [0, 1, 4, 7, 6]), (0, 2, [0, 2]), (1, 5, [1, 5]), (3, 6, [])],   # the allow-set removes the short paths
    (3, OUT, (0, 2)): [(0, 6, [])],
    (4, OUT, (1,)): [(1, 6, [1, 5, 6]), (0, 6, [])],   # one label, as the reference's plan has it
    (3, IN, ()): [(6, 0, [6, 3, 2, 0]),       # against the arcs: 6 3 2 0 is smaller than 6 5 1 0
                  (0, 6, []), (7, 0, [7, 4, 1, 0]), (5, 5, [5])],
    (3, BOTH, ()): [(4, 3, [4, 7, 6, 3]), (6, 0, [6, 3, 2, 0]), (7, 5, [7, 6, 5])],
    (2, BOTH, ()): [(4, 3, []), (4, 6, [4, 7, 6]), (6, 1, [6, 5, 1])],
}


def hand_graph() -> twin.Graph:
    e = np.array(HAND_EDGES, np.int64)
    return twin.Graph.from_edges(HAND_N, e[:, 0], e[:, 1], e[:, 2])


_CACHE = {}


def g20k() -> twin.Graph:
    if "g20k" not in _CACHE:
        _CACHE["g20k"] = twin.Graph(*fx.prefilter_graph("g20k"))
    return _CACHE["g20k"]


# name -> (pair seed, requests, max_depth, direction, allowed labels, max_reach)
G20K_BATCHES = {
    "out8": (7, 64, 8, OUT, (), 16384),
    "both5": (7, 64, 5, BOTH, (), 16384),
    "out8_small": (7, 64, 8, OUT, (), 1000),
    "labelled10": (7, 64, 10, OUT, (0, 2), 16384),
}


def g20k_batch(name):
    """(sources u64, targets u64, max_depth, direction, allowed, max_reach, the twin's (paths, statuses, sizes))"""
    if name not in _CACHE:
        seed, b, max_depth, direction, allowed, max_reach = G20K_BATCHES[name]
        g = g20k()
        pairs = np.random.default_rng(seed).integers(0, g.n, (b, 2)).astype(np.uint64)
        src, dst = pairs[:, 0].copy(), pairs[:, 1].copy()
        _CACHE[name] = (src, dst, max_depth, direction, allowed, max_reach, twin.answers(g, src, dst, max_depth, direction, allowed, max_reach))
    return _CACHE[name]


def facts(paths, status, sizes, max_reach):
    """the numbers the host file pins for a batch"""
    ok = sizes[status == twin.OK]
    return dict(found=sum(1 for p in paths if len(p)), overflowed=int((status == twin.ERR_CANDIDATE_LIMIT).sum()),
                lengths=sorted(set(len(p) for p in paths if len(p))), largest_reach=int(ok.max()) if ok.size else 0)
