"""The deep shortest-path batches the CPU and the GPU tests of hvx_shortest_path_batch_dense share: requests whose backward reach outgrows
hvx_shortest_path_batch's 16 384 nodes (tests/test_shortest_path_dense_host.py pins what the existing twin says about them,
tests/test_gpu_shortest_path_dense.py runs them on the device).  The twin's answers are computed once per process and nobody changes them."""
import numpy as np

import fixtures as fx
import shortest_path_cases as sc
import shortest_path_twin as twin

OUT, IN, BOTH = twin.DIR_OUT, twin.DIR_IN, twin.DIR_BOTH
SIBLING_REACH = 16384

# name -> (graph, max_depth, direction, allowed labels, extra requests).  Every batch is the 64 pairs default_rng(11).integers(0, n, (64, 2))
# followed by the extra ones.  The 64 random pairs of the two Out batches on g70k hold no request that the sibling refuses AND that has a
# path (its refused ones have none), so each gets one by construction: a refused request's target and the smallest node of the last
# level of its backward search -- a path of exactly max_depth arcs whose reach set has passed 16 384 nodes before the source is in it.
DEEP_BATCHES = {
    "g70k_both6": ("g70k", 6, BOTH, (), ()),
    "g70k_out8": ("g70k", 8, OUT, (), ((2, 68664),)),
    "g70k_in8": ("g70k", 8, IN, (), ()),
    "g70k_out12_labelled": ("g70k", 12, OUT, (0, 2), ((1, 64975),)),
    "g20k_both6": ("g20k", 6, BOTH, (), ()),
}

_CACHE = {}


def graph(name) -> twin.Graph:
    if name == "g20k":
        return sc.g20k()
    if name not in _CACHE:
        _CACHE[name] = twin.Graph(*fx.prefilter_graph(name))
    return _CACHE[name]


def deep_batch(name):
    """(graph name, sources u64, targets u64, max_depth, direction, allowed, the twin's (paths, statuses, sizes) without a reach limit,
    the twin's (paths, statuses, sizes) at the sibling's max_reach of 16 384)"""
    key = ("batch", name)
    if key not in _CACHE:
        gname, max_depth, direction, allowed, extra = DEEP_BATCHES[name]
        g = graph(gname)
        pairs = np.random.default_rng(11).integers(0, g.n, (64, 2)).astype(np.uint64)
        if extra:
            pairs = np.concatenate([pairs, np.array(extra, np.uint64)])
        src, dst = pairs[:, 0].copy(), pairs[:, 1].copy()
        _CACHE[key] = (gname, src, dst, max_depth, direction, allowed, twin.answers(g, src, dst, max_depth, direction, allowed, None),
                       twin.answers(g, src, dst, max_depth, direction, allowed, SIBLING_REACH))
    return _CACHE[key]


def facts(name):
    """the numbers the host file pins for a deep batch (the first 64 requests are the issue's table row; `refused_found` counts every request)"""
    _, src, _, _, _, _, (paths, _, sizes), (_, st16, _) = deep_batch(name)
    refused = st16 == twin.ERR_CANDIDATE_LIMIT
    return dict(found=sum(1 for p in paths[:64] if len(p)), lengths=sorted(set(len(p) for p in paths if len(p))), largest_reach=int(sizes.max()),
                refused=int(refused[:64].sum()), refused_found=sum(1 for q in range(src.size) if refused[q] and len(paths[q])))
