"""The bf16 shadow pre-pass of the strict squared-Euclidean beam at every dimension the wave kernel is built for, on both graph
widths (hvx_hnsw_wave.h: shadow_pass / shadow_prune; test_gpu_shadow_prune.py holds the corpora that stress the bound itself).

What differs from dimension to dimension is the shape of a pass, and every shape is its own code:
  * rows per 8-lane group and shadow pass of the two-per-SIMD builds: 4 at dim 128 / 256, 3 at dim 384 / 512 / 768, 1 at dim 1024 / 1536
    (kSWmax), with the narrower passes 2 and 1 for the frontiers that do not fill the widest one;
  * whether a shadow pass ties each step's reads and widening behind the previous step's FMAs (three rows at dim 768) or not;
  * M0 64 rows hold up to 64 unvisited neighbours: more than the 32 / 24 / 8 rows of one widest pass, so a frontier takes two or more;
    late expansions of any graph leave frontiers of 1 to 8 rows (one narrow pass, most groups idle and pointed at the pass's first row).
ef 32 fills the beam after two or three expansions, so the wide frontiers of the first hops already run the pre-pass; ef 200 is the
384-entry beam.  With the pre-pass on and off, at one and two queries per SIMD: ids, score bits, counts, statuses and the four
SearchStats counters are identical, and equal the oracle's.  Run with `-m gpu` on an MI355X."""
import numpy as np
import pytest

import fixtures as fx
from test_gpu_shadow_prune import assert_oracle_ids, search_both

pytestmark = pytest.mark.gpu

DIMS = [128, 256, 384, 512, 768, 1024, 1536]


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


def queries_for(data, rng, dim):
    """24 queries: 8 rows, 8 rows moved by one ulp, 8 random"""
    n = data.shape[0]
    rows = data[rng.choice(n, 8, replace=False)]
    ulp = np.nextafter(data[rng.choice(n, 8, replace=False)], np.float32(np.inf))
    return np.vstack([rows, ulp, rng.standard_normal((8, dim)).astype(np.float32)]).astype(np.float32)


def device_built_pair(orc, hv, data, m, efc, seed):
    """The graph is built on the device and the oracle is seeded with its export, so both search the same graph (what these tests
    compare is the search; the oracle's own sequential build of an M0 64 graph takes 10 to 30 s per case on one core)."""
    n, dim = data.shape
    ids = np.arange(n, dtype=np.uint64)
    gix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids, vectors=data, levels=fx.draw_levels(n, m, seed=seed),
                                               m=m, m0=2 * m, ef_construction=efc)
    gix.sync()
    g = gix.export_graph()
    oix = orc.Index(dim, orc.L2SQ, kernel=orc.K_AVX_FMA, m=m, m0=2 * m, ef_construction=efc)
    assert oix.seed(ids, data, g["l0_offsets"], g["l0_neighbors"], g["level"], g["up_offsets"], g["up_neighbors"],
                    entry_point=g["entry_point"], max_layer=g["max_layer"]) == orc.OK
    return oix, gix


@pytest.mark.parametrize("m", [16, 32])
@pytest.mark.parametrize("dim", DIMS)
def test_every_pass_shape(orc, hv, dim, m):
    rng = np.random.default_rng(9000 + dim + m)
    n = 1500 if dim >= 1024 else 2500 if dim <= 256 else 2000
    efc = 64 if dim >= 1024 else 100 if dim <= 256 else 80
    data = rng.standard_normal((n, dim)).astype(np.float32)
    oix, gix = device_built_pair(orc, hv, data, m, efc, seed=dim + m)
    q = queries_for(data, rng, dim)
    for ef in (32, 200):
        res = search_both(hv, gix, q, 10, ef)
        assert_oracle_ids(orc, oix, res, q, 10, ef)
    gix.close()


def test_rows_at_the_largest_magnitude_are_always_scored(orc, hv):
    """A row with an element beyond the bf16 range has shadow_err = inf and no bound (kNoBound): it is always scored in f32.  The
    oracle accepts no such row under squared-Euclidean -- its component limit (orc_component_limit, the range test_gpu_magnitude.py
    works in) lies far below the largest bf16 value, which this test first confirms -- so the rows here sit at 0.99 of that limit, the
    largest magnitude it takes.  Their sums of squares are near the top of the f32 range: the finiteness test of the bound refuses
    them (kNoBound again), and the queries next to them find them."""
    dim, n, m = 128, 2000, 16
    limit = float(orc.lib().orc_component_limit(orc.L2SQ, dim))
    assert limit < 3.3e38, "the oracle takes rows beyond the bf16 range: this test must use them"
    probe = orc.Index(dim, orc.L2SQ, kernel=orc.K_AVX_FMA, m=m, m0=2 * m, ef_construction=64)
    over = np.zeros(dim, np.float32)
    over[0] = np.float32(3.3962e38)  # rounds to +inf in bf16
    assert probe.insert(0, over, 0) != orc.OK, "the oracle takes a row beyond the bf16 range: this test must use it"
    rng = np.random.default_rng(77)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    big = rng.choice(n, 6, replace=False)
    lim = np.float32(0.99) * np.float32(limit)
    for t, r in enumerate(big):  # a few elements, every element, alternating signs
        if t % 3 == 0:
            data[r, rng.choice(dim, 3, replace=False)] = lim
        elif t % 3 == 1:
            data[r] = (rng.uniform(-1.0, 1.0, dim).astype(np.float32) * lim).astype(np.float32)
        else:
            data[r, ::2] = lim
            data[r, 1::2] = -lim
    oix, gix = device_built_pair(orc, hv, data, m, 80, seed=3)
    near = (data[big] * np.float32(0.999)).astype(np.float32)
    q = np.vstack([data[big], near, data[rng.choice(n, 6, replace=False)], rng.standard_normal((6, dim)).astype(np.float32)]).astype(np.float32)
    for ef in (32, 200):
        res = search_both(hv, gix, q, 10, ef)
        assert_oracle_ids(orc, oix, res, q, 10, ef)
    gix.close()
