"""The graphs of tests/test_gpu_prefilter_scale.py, held on the CPU to what that file says of them -- from the oracle's own output
(orc.breadth_first / orc.depth_first) and the CSR arrays: frontiers wider than the level kernels' fixed grid of 4 096 wavefronts and
than one 1 024-entry chunk of ord_scan_kernel, discovery arcs in several 64-arc chunks of one row and in both rows of one node,
candidate bitmaps with ids on both sides of a block edge and an empty block between populated ones, one wavefront's seeds with light
and heavy rows.  These are conditions of the fixtures: where a generator seed stops meeting one, the seed changes, not the assertion.
Then the host traversal (hvx_traverse_host: breadth first and depth first) against the oracle on the 20 011-node graph."""
from collections import Counter, defaultdict

import numpy as np
import pytest

import fixtures as fx

G20K_CASES = ["out1", "in1", "both1", "many", "twice", "labelled", "hubs"]
ORDERED_CASES = ["out1", "in1", "both1", "labelled", "hubs"]


def row_positions(graph):
    """per stored edge: its position in its source's outgoing row and in its target's incoming row (sources ascending, parallel
    edges in outgoing-row order: model.rs:376-417)"""
    n, off, tgt, _ = fx.prefilter_graph(graph)
    off, tgt = off.astype(np.int64), tgt.astype(np.int64)
    owner = np.repeat(np.arange(n), np.diff(off))
    pos_out = np.arange(tgt.size) - off[owner]
    order = np.argsort(tgt, kind="stable")
    in_off = np.zeros(n + 1, np.int64)
    in_off[1:] = np.cumsum(np.bincount(tgt, minlength=n))
    pos_in = np.empty(tgt.size, np.int64)
    pos_in[order] = np.arange(tgt.size) - in_off[tgt[order]]
    return pos_out, pos_in


def test_generators_give_the_reference_form():
    for graph in ("g20k", "g70k"):
        n, off, tgt, lab = fx.prefilter_graph(graph)
        assert off.dtype == np.uint64 and tgt.dtype == np.uint64 and lab.dtype == np.uint32
        assert off[0] == 0 and off[-1] == tgt.size == lab.size and off.size == n + 1 and int(tgt.max()) < n
        owner = np.repeat(np.arange(n), np.diff(off.astype(np.int64)))
        same_row = owner[1:] == owner[:-1]
        assert (tgt[1:][same_row] >= tgt[:-1][same_row]).all()                       # every row ascends by target
        assert (tgt[1:][same_row] == tgt[:-1][same_row]).any() and (tgt == owner).any()   # parallel edges and self-loops occur
        assert n % 64 != 0 and n % 32 != 0
    n, off, tgt, lab = fx.prefilter_graph("g20k")
    deg = np.diff(off.astype(np.int64))
    assert deg[list(fx.G20K_HUBS)].tolist() == [300, 1000] and np.bincount(tgt.astype(np.int64))[fx.G20K_SINK] >= 200
    assert sorted(set(deg.tolist()) - {300, 1000}) == list(range(7))
    assert fx.csr_graph(500, 3)[1].tolist() == fx.csr_graph(500, 3)[1].tolist() != fx.csr_graph(500, 4)[1].tolist()
    assert fx.csr_graph(200, 1, avg_row=10)[0][-1] > 3 * fx.csr_graph(200, 1, avg_row=2)[0][-1] and fx.csr_graph(9, 1)[2] is None
    n, off, tgt = fx.chain_graph(7)
    assert n == 8 and off.tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 7] and tgt.tolist() == [1, 2, 3, 4, 5, 6, 7]
    assert fx.bitmap_ids(np.array([1 | 1 << 63, 2], np.uint64)) == {0, 63, 65}
    assert fx.bitmap_ids(np.array([1 << 31, 0, 5], np.uint32)) == {31, 64, 66}


@pytest.mark.parametrize("name", G20K_CASES)
def test_frontiers_are_wider_than_the_fixed_grid_and_one_scan_chunk(orc, name):
    """bfs_level_kernel / ord_claim / ord_count / ord_emit stride (more than 1024 x 4 frontier positions) and ord_scan_kernel carries
    across 1 024-entry chunks (level 0 of `many` and `twice` is the level-0 grid of more than 4 096 wavefronts)"""
    visits, edges = fx.prefilter_oracle(orc, name)
    sizes = Counter(d for _, d in visits)
    print(name, [sizes[d] for d in sorted(sizes)])
    assert max(sizes.values()) > 4096 and sum(1 for s in sizes.values() if s > 1024) >= (1 if name == "twice" else 2)
    assert len(visits) == len(edges) + sizes[0] and len(set(v for v, _ in visits)) == len(visits)
    seeds = fx.prefilter_traversals()[name][1]
    assert sizes[0] == np.unique(seeds).size
    if name in ("many", "twice", "labelled"):
        assert seeds.size > sizes[0] and (np.diff(seeds.astype(np.int64)) < 0).any()  # duplicates, not ascending
    if name in ("many", "twice"):
        assert seeds.size > 4096                                                      # the pinned seed buffer regrows
        words = np.unique(seeds) // 32
        assert np.bincount(words.astype(np.int64)).max() > 1                          # several seeds share one bitmap word
    if name == "twice":
        assert seeds.size > fx.G20K["n"]                                              # the de-duplication branch


@pytest.mark.parametrize("name", ORDERED_CASES)
def test_discovery_arcs_span_chunks_and_rows(orc, name):
    """ord_count_kernel's running count across the 64-arc steps of one row, and ord_emit_kernel's rank across the two rows of a node"""
    visits, edges = fx.prefilter_oracle(orc, name)
    pos_out, pos_in = row_positions("g20k")
    chunks, sides = defaultdict(set), defaultdict(set)
    for parent, arc, against in edges:
        chunks[(parent, against)].add(int((pos_in if against else pos_out)[arc]) // 64)
        sides[parent].add(against)
    assert any(len(c) > 1 for c in chunks.values()), "no expanded node has discovery arcs in two 64-arc chunks of one row"
    direction = fx.prefilter_traversals()[name][3]
    assert set(a for _, _, a in edges) == {0: {0}, 1: {1}, 2: {0, 1}}[direction]
    if direction == 2:
        assert any(len(s) == 2 for s in sides.values()), "no expanded node has discovery arcs in both of its rows"
        assert any(len(chunks[(p, 0)]) > 1 and (p, 1) in chunks for p in sides)   # the rank of an incoming arc past a long outgoing row
    parents = set(p for p, _, _ in edges)
    if name == "hubs":   # the hub that is a seed is expanded, the one that is met is emitted and never expanded
        small, big = fx.G20K_HUBS
        assert big in parents and small in set(v for v, _ in visits) and small not in parents and fx.G20K_SINK not in parents
    if name == "labelled":
        lab = fx.prefilter_graph("g20k")[3]
        assert set(int(lab[a]) for _, a, _ in edges) == {1, 2} and set(fx.G20K_HUBS) <= parents


def test_single_seed_traversals_end_on_both_sides_of_a_level_batch(orc):
    """levels are enqueued eight at a time: the unbounded traversals from one seed end inside the first, second and third batch"""
    last = {name: max(d for _, d in fx.prefilter_oracle(orc, name)[0]) for name in ("out1", "in1", "both1")}
    print(last)
    assert last["both1"] <= 8 < last["out1"] <= 16 < last["in1"]


def test_fused_bitmaps_straddle_block_edges_and_skip_blocks(orc):
    n, off, tgt, lab = fx.prefilter_graph("g70k")
    island = set(v for v, _ in fx.prefilter_oracle(orc, "island")[0])
    sparse_seeds, _ = fx.hop_cases()["sparse"]
    sparse = set(fx.row_union(off, tgt, sparse_seeds).tolist())
    for ids in (island, sparse):
        assert {8191, 8192, 24575, 24576} <= ids and fx.has_empty_block_between(ids)
        assert fx.bitmap_blocks(ids) == [0, 1, 2, 3, 6]
    assert len(sparse) > 256
    edge_ids = {8191, 8192, 24575, 24576}   # next to the block edges: with a vector in one image, mostly without in the other
    assert edge_ids <= set(fx.CONTIGUOUS_IDS.tolist()) and edge_ids & set(fx.THIRD_IDS.tolist()) == {24576}
    dense = np.array(sorted(v for v, _ in fx.prefilter_oracle(orc, "dense")[0]))
    assert fx.bitmap_blocks(dense) == list(range(9)) and dense.size > 50000
    assert np.unique(dense // 32).size > 0.95 * ((n + 31) // 32)       # next to no empty word
    woff, wtgt, wsrc = fx.walk_hop_graph(fx.WALK_NODES, 5)
    assert woff[-1] == wtgt.size == wsrc.size == 1500 and np.diff(woff.astype(np.int64)).max() == 1
    assert fx.bitmap_blocks(wtgt) == [0, 2] and {8190, 8191, 16384, 16385} <= set(wtgt.tolist()) and np.unique(wtgt).size > 256
    assert 8191 % 3 == 1 and 16384 % 3 == 1 and 8190 % 3 != 1 and 16385 % 3 != 1   # ids 3 i + 1 hold a vector
    assert 0.5 < float((wtgt % 3 != 1).mean()) < 0.8                               # most candidates hold no vector: the ranks count them


def test_hop_seeds_mix_light_and_heavy_rows_in_one_wavefront():
    n, off, tgt, lab = fx.prefilter_graph("g70k")
    deg = np.diff(off.astype(np.int64))
    indeg = np.bincount(tgt.astype(np.int64), minlength=n)
    cases = fx.hop_cases()
    assert [cases[c][0].size for c in ("one", "group", "65", "1024", "1025", "5000")] == [1, 64, 65, 1024, 1025, 5000]
    for name in ("group", "65", "1024", "1025", "5000", "duplicates", "in"):
        first = deg[cases[name][0][:64].astype(np.int64)]                 # one wavefront takes 64 consecutive seeds
        assert {0, 1, 16, 17, 65, 1000} <= set(first.tolist()), name
        assert (first > 64).sum() >= 2 and ((first > 0) & (first < 16)).sum() > 30
    s = cases["duplicates"][0]
    assert np.unique(s).size == 64 < s.size
    assert indeg[3000] > 64 and 3000 in cases["in"][0].tolist() and indeg[cases["in"][0][:64].astype(np.int64)].max() <= 16
    row = tgt[int(off[2002]):int(off[2003])]
    assert row.size == 300 and np.unique(row).size == 5
    both = fx.row_union(off, tgt, cases["both_labelled"][0], lab, [1], 2)
    assert 0 < both.size < fx.row_union(off, tgt, cases["both_labelled"][0], direction=2).size
    # bound = seeds x the longest row exceeds both images; one hop reaches every row of the contiguous one
    assert cases["5000"][0].size * deg.max() > n > fx.THIRD_IDS.size
    assert np.isin(fx.CONTIGUOUS_IDS, fx.row_union(off, tgt, cases["every_row"][0])).all()
    vless = fx.row_union(off, tgt, cases["vectorless"][0])
    assert vless.size == 5 and not np.isin(vless, fx.THIRD_IDS).any() and not np.isin(vless, fx.CONTIGUOUS_IDS).any()


@pytest.mark.parametrize("depth_first", [False, True])
@pytest.mark.parametrize("name", ["out1", "in1", "both1", "labelled", "hubs"])
def test_host_traversal_equals_the_oracle_at_scale(orc, name, depth_first):
    """hvx_traverse_host (no device): both strategies, the three directions, labels, many seeds and the hub policy"""
    import pyhvx as hv
    graph, seeds, md, direction, allowed, hub = fx.prefilter_traversals()[name]
    n, off, tgt, lab = fx.prefilter_graph(graph)
    if depth_first:
        want = orc.depth_first(n, off.astype(np.int64), tgt, lab, seeds, md, direction, allowed, hub)
    else:
        want = fx.prefilter_oracle(orc, name)
    visits, edges = hv.traverse_host(n, off, tgt, lab, seeds, md, direction, allowed, hub, depth_first=depth_first)
    assert visits == want[0], f"{name}: visit order differs"
    assert edges == want[1], f"{name}: discovery edges differ"
