"""The graph prefilter (csrc/hvx_prefilter.hip) where its kernels split their work -- traversals whose frontiers exceed the fixed grid
of the level kernels and one chunk of the ordered traversal's scan, level counts on both sides of the eight-level batches, seed lists
past the pinned buffer and past the node count, the fused hop over many workgroups with light and heavy rows in one wavefront, candidate
bitmaps with ids on both sides of a block edge and empty blocks between populated ones -- against the oracle: visited sets, depths,
visit order, discovery edges, candidate counts, result ids and f32 score BITS, all by equality.  tests/test_prefilter_fixtures.py proves
on the CPU that the graphs of tests/fixtures.py meet every one of these conditions."""
import numpy as np
import pytest

import fixtures as fx
import walk_harness as wh
from test_gpu_walk import assert_equal, device_index

pytestmark = pytest.mark.gpu

UNREACHED = 0xFFFFFFFF


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


@pytest.fixture(scope="module")
def g20k(hv):
    n, off, tgt, lab = fx.prefilter_graph("g20k")
    return hv.Graph(n, off, tgt, lab)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def depths_of(n, visits):
    want = np.full(n, UNREACHED, np.uint32)
    want[[v for v, _ in visits]] = [d for _, d in visits]
    return want


# ---- a. the visited-set traversal
@pytest.mark.parametrize("name", ["out1", "in1", "both1", "many", "twice", "labelled", "hubs"])
def test_visited_set_and_depths_on_wide_frontiers(orc, hv, g20k, name):
    """bfs_level_kernel striding over frontiers of more than 4 096 nodes, a level-0 grid of more than 4 096 wavefronts (`many`), the
    regrown seed buffer, the de-duplication of a seed list longer than the graph (`twice`), labels, and the hub policy"""
    _, seeds, md, direction, allowed, hub = fx.prefilter_traversals()[name]
    visits, _ = fx.prefilter_oracle(orc, name)
    words, depth = g20k.traverse(seeds, md, direction, allowed, hub)
    assert fx.bitmap_ids(words) == set(v for v, _ in visits)
    assert np.array_equal(depth, depths_of(g20k.n, visits))
    if name in ("many", "hubs"):   # clear_bits_kernel over many blocks, several seeds inside one bitmap word
        words, depth = g20k.traverse(seeds, md, direction, allowed, hub, include_seeds=False)
        assert fx.bitmap_ids(words) == set(v for v, _ in visits) - set(seeds.tolist())
        assert np.array_equal(depth, depths_of(g20k.n, visits))


def test_expand_over_5000_rows_is_the_union_of_the_rows(hv, g20k):
    n, off, tgt, lab = fx.prefilter_graph("g20k")
    rows = fx.prefilter_traversals()["many"][1]
    for direction, allowed in ((hv.DIR_OUT, ()), (hv.DIR_IN, ()), (hv.DIR_BOTH, (0, 2))):
        words = g20k.expand(rows, direction, allowed)
        assert fx.bitmap_ids(words) == set(fx.row_union(off, tgt, rows, lab, allowed, direction).tolist()), (direction, allowed)


# ---- b. levels are enqueued eight at a time
@pytest.mark.parametrize("length", [7, 8, 9, 15, 16, 17])
def test_chains_that_end_next_to_a_level_batch(hv, length):
    n, off, tgt = fx.chain_graph(length)
    g = hv.Graph(n, off, tgt)
    words, depth = g.traverse([0], 1000, hv.DIR_OUT)
    assert fx.bitmap_ids(words) == set(range(n)) and depth.tolist() == list(range(n))
    visits, edges = g.traverse_ordered([0], 1000, hv.DIR_OUT)
    assert visits == [(i, i) for i in range(n)] and edges == [(i, i, 0) for i in range(length)]
    visits, edges = g.traverse_ordered([length], 1000, hv.DIR_BOTH)   # the same chain walked back, against every edge
    assert visits == [(length - i, i) for i in range(n)] and edges == [(length - i, length - i - 1, 1) for i in range(length)]
    g.close()


@pytest.mark.parametrize("max_depth", [7, 8, 9, 16, 17])
def test_depth_caps_next_to_a_level_batch(hv, max_depth):
    n, off, tgt = fx.chain_graph(40)
    g = hv.Graph(n, off, tgt)
    words, depth = g.traverse([0], max_depth, hv.DIR_OUT)
    assert fx.bitmap_ids(words) == set(range(max_depth + 1))
    assert depth.tolist() == list(range(max_depth + 1)) + [UNREACHED] * (40 - max_depth)
    visits, edges = g.traverse_ordered([0], max_depth, hv.DIR_OUT)
    assert visits == [(i, i) for i in range(max_depth + 1)] and edges == [(i, i, 0) for i in range(max_depth)]
    g.close()


# ---- c. the ordered traversal
@pytest.mark.parametrize("name", ["out1", "in1", "both1", "labelled", "hubs"])
def test_visit_order_and_discovery_edges_on_wide_frontiers(orc, hv, g20k, name):
    """ord_claim / ord_count / ord_emit striding over more than 4 096 frontier positions, ord_scan_kernel carrying across its
    1 024-entry chunks, rows of several 64-arc steps, ranks across the two rows of one node; where two parallel edges reach the same
    node the oracle's rule (the outgoing one first) is the contract, as in test_ordered_traversal_... of test_gpu_parity.py"""
    _, seeds, md, direction, allowed, hub = fx.prefilter_traversals()[name]
    want_visits, want_edges = fx.prefilter_oracle(orc, name)
    visits, edges = g20k.traverse_ordered(seeds, md, direction, allowed, hub)
    assert len(visits) == len(want_visits)
    assert visits == want_visits, f"{name}: visit order differs"
    assert edges == want_edges, f"{name}: discovery edges differ"


# ---- d / e. the fused call
class Fused:
    def __init__(self, orc, hv):
        n, off, tgt, lab = fx.prefilter_graph("g70k")
        self.csr = (off, tgt, lab)
        self.g = hv.Graph(n, off, tgt, lab)
        rng = np.random.default_rng(64)
        self.q = rng.standard_normal((8, 64)).astype(np.float32)
        self.images = []
        for ids in (fx.THIRD_IDS, fx.CONTIGUOUS_IDS):   # the binary-search id map and the contiguous one
            data = rng.standard_normal((ids.size, 64)).astype(np.float32)
            zeros = np.zeros(ids.size + 1, np.uint64)
            oix = orc.Index(64, orc.L2SQ)
            assert oix.seed(ids, data, zeros, np.zeros(0, np.uint64)) == orc.OK
            gix = hv.ValidatedVectorReadIndex.managed(dim=64, metric=hv.EUCLIDEAN, node_ids=ids, vectors=data, l0_offsets=zeros,
                                                      l0_neighbors=np.zeros(0, np.uint64), max_batch=16)
            self.images.append((oix, gix, ids))

    def check(self, orc, hv, seeds, kw, cand, k=10, option=0):
        """the fused call == candidate count, the two-call form and the oracle's exact scan over `cand`, on both images"""
        p = hv.SearchParams(k)
        for oix, gix, image_ids in self.images:
            gix.set_option(hv.OPT_RESTRICTED_DIRECT, option)
            try:
                ids, sc, cnt, ncand, _ = gix.prefilter_search_batch(self.g, self.q, p, seeds, **kw)
                path = gix.last_scan_path()
            finally:
                gix.set_option(hv.OPT_RESTRICTED_DIRECT, 0)
            assert ncand == cand.size
            if not kw.get("traverse"):
                assert (path == hv.PATH_DIRECT) == (option != 1), "one hop: the lean route unless the pipeline is asked for"
            if kw.get("traverse"):
                words, _ = self.g.traverse(seeds, kw["max_depth"], kw["direction"], include_seeds=kw.get("include_seeds", True))
            else:
                words = self.g.expand(seeds, kw.get("direction", hv.DIR_OUT), kw.get("allowed_labels", ()))
            assert fx.bitmap_ids(words) == set(cand.tolist())
            ids2, sc2, cnt2 = gix.search_restricted_batch(self.q, p, hv.RestrictedVectorCandidates.from_bitmap_words(words))
            assert cnt.tolist() == cnt2.tolist() and ids.tolist() == ids2.tolist() and bits(sc).tolist() == bits(sc2).tolist()
            held = int(np.isin(cand, image_ids).sum())
            assert cnt.tolist() == [min(k, held)] * self.q.shape[0]
            for qi in range(self.q.shape[0]):
                rc, oid, osc = oix.flat(self.q[qi], k, allowed=cand)
                assert rc == orc.OK and ids[qi, :cnt[qi]].tolist() == oid.tolist() and bits(sc[qi, :cnt[qi]]).tolist() == bits(osc).tolist()
        return int(cnt[0])


@pytest.fixture(scope="module")
def fused(orc, hv):
    f = Fused(orc, hv)
    yield f
    for _, gix, _ in f.images:
        gix.close()
    f.g.close()


# in file order on the same two handles: small, 5 000 seeds (the pinned seed buffer regrows), small again -- the bitmap the call
# before left behind and the regrown buffer are part of every case
HOP_SEQUENCE = ["one", "group", "65", "1024", "1025", "5000", "one", "duplicates", "parallel", "in", "both_labelled", "every_row",
                "vectorless", "sparse", "group"]


@pytest.mark.parametrize("step,name", list(enumerate(HOP_SEQUENCE)))
def test_fused_hop_on_the_lean_route(orc, hv, fused, step, name):
    """expand_collect_kernel + the one-launch scan: 1 / 64 / 65 / 1 024 / 1 025 / 5 000 seeds (one wavefront, one workgroup, several),
    rows of 0, 1, 16, 17, 65 and 1 000 arcs in one wavefront, duplicated seeds, parallel edges, a long incoming row, both rows with
    labels, a bound above the image (the row list's capacity is the image), every row of an image, no row at all"""
    seeds, kw = fx.hop_cases()[name]
    off, tgt, lab = fused.csr
    cand = fx.row_union(off, tgt, seeds, lab, kw.get("allowed_labels", ()), kw.get("direction", 0))
    found = fused.check(orc, hv, seeds, kw, cand)
    if name == "vectorless":
        assert found == 0 and cand.size == len(fx.VECTORLESS)
    if name == "every_row":
        assert np.isin(fx.CONTIGUOUS_IDS, cand).all()


def test_fused_hop_with_a_hundred_results(orc, hv, fused):
    """k > 64 takes the lean route when asked to (a shared set scanned once per query is the pipeline's otherwise)"""
    seeds, kw = fx.hop_cases()["1025"]
    off, tgt, lab = fused.csr
    assert fused.check(orc, hv, seeds, kw, fx.row_union(off, tgt, seeds), k=100, option=2) == 100


@pytest.mark.parametrize("name,include_seeds", [("island", True), ("island", False), ("dense", True)])
def test_fused_traversal_on_the_bitmap_pipeline(orc, hv, fused, name, include_seeds):
    """bitmap_count / block_scan / bitmap_compact over nine blocks: candidates at 8191 | 8192 and 24575 | 24576, blocks 4 and 5 empty
    between populated ones (`island`), and nearly every word populated (`dense`)"""
    _, seeds, md, direction, _, _ = fx.prefilter_traversals()[name]
    visits, _ = fx.prefilter_oracle(orc, name)
    cand = np.array(sorted(set(v for v, _ in visits) - (set() if include_seeds else set(seeds.tolist()))), np.uint64)
    fused.check(orc, hv, seeds, dict(traverse=True, max_depth=md, direction=direction, include_seeds=include_seeds), cand)


@pytest.mark.parametrize("name", ["sparse", "group", "5000"])
def test_fused_hop_on_the_bitmap_pipeline(orc, hv, fused, name):
    """the same hops through the level kernel + count / scan / compact (OPT_RESTRICTED_DIRECT = 1, restored afterwards)"""
    seeds, kw = fx.hop_cases()[name]
    off, tgt, lab = fused.csr
    fused.check(orc, hv, seeds, kw, fx.row_union(off, tgt, seeds, lab, kw.get("allowed_labels", ()), kw.get("direction", 0)), option=1)


# ---- f. the sampled walk
def test_sampled_walk_over_a_bitmap_with_an_empty_middle_block(orc, hv):
    """bitmap_select_kernel: the deterministic sample's ranks resolved against a three-block bitmap whose middle block is empty (two
    equal prefixes under the binary search), candidates on both block edges, ids without a vector counted by the ranks.  The image
    holds fixtures.WALK_ROWS rows, not 9 000: the oracle's inserts of 9 000 rows take ten seconds."""
    oix, ids, vec = wh.random_graph(orc, fx.WALK_ROWS, 32, orc.L2SQ, 9000, id_gap=True)
    assert int(ids[-1]) + 3 == fx.WALK_NODES
    gix = device_index(hv, oix, 32, orc.L2SQ)
    off, tgt, src = fx.walk_hop_graph(fx.WALK_NODES, 5)
    g = hv.Graph(fx.WALK_NODES, off, tgt)
    q = np.random.default_rng(1).standard_normal((3, 32)).astype(np.float32)
    for seeds in (src, src[:700]):
        allowed = np.unique(tgt[: seeds.size])
        out_ids, sc, cnt, ncand, rs, _ = gix.prefilter_search_batch_params(g, q, hv.RestrictedParams.new(10, 100), seeds)
        assert ncand == allowed.size
        for i in range(3):
            assert rs[i]["strategy"] == hv.RESTRICTED_FILTERED
            assert_equal(out_ids[i], sc[i], int(cnt[i]), rs[i], oix.search_restricted(q[i], 10, 100, allowed))
    gix.close()
    g.close()
