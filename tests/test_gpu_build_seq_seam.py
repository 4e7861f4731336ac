"""The seam between the two builds of the many-workgroup one-node steps (csrc/hvx_build.hip: one id per lane; csrc/hvx_build_wide_seq.hip:
two): the largest shape the one-id-per-lane kernels serve, M 16 / M0 32 -- rows of 32 ids, so an append to a full row is the 33-id list,
two short of the 35 the narrow lists hold --, and the smallest the two-ids-per-lane kernels serve -- the layer-0 select matrix is 128 wide
but holds 66 - 68 candidates, so replay_rows2 runs with its upper word nearly empty: M 17 / M0 33, which the degree limits' own rule
m0 = max(m0, 2 m) (mutation.rs:178-196) makes 17 / 34 on the device and in the oracle alike, and M 16 / M0 33, which stays 33.
Sequential builds, default link_mode, L2, dim 32, held to the oracle row for row as tests/test_gpu_build_wide_seq.py holds M 32 / M0 64,
with that file's oracle_of and full_rows.

Each case first asserts on the ORACLE alone that it exercises what the kernels can get wrong: dozens of layer-0 rows at their limit (an
append goes through the prune) and inserts in which two of the new node's linked neighbours lose their mutual layer-0 edge (the `alive`
replay or the removal pass)."""
import numpy as np
import pytest

from test_gpu_build_wide import full_rows, assert_rows_equal, assert_searches_equal
from test_gpu_build_wide_seq import oracle_of

pytestmark = pytest.mark.gpu

N, DIM, METRIC, EFC, LM = 600, 32, 1, 80, 4   # (ef_construction >= 2 m0: the layer-0 select hydrates its full 2 m0 candidates)


@pytest.fixture(scope="module")
def hv():
    import pyhvx
    pyhvx.lib()
    return pyhvx


@pytest.mark.parametrize("m,m0,wide", [(16, 32, False), (17, 33, True), (16, 33, True)])
def test_sequential_build_at_the_seam_between_the_row_widths_equals_the_oracle_row_for_row(orc, hv, m, m0, wide):
    """Rows, entry point, top layer and levels equal the oracle's, 16 searches equal ids and score bits, and the path word says the two
    many-workgroup steps ran: without the wide flag at 16 / 32, with it above."""
    oix, ex, cross, rng, data, ids, lv = oracle_of(orc, N, DIM, METRIC, EFC, LM, m, m0)
    lim0 = max(m0, 2 * m)   # the limit in force on layer 0
    f0, fu, nu = full_rows(ex, N, m, lim0)
    print(f"oracle: {f0} layer-0 rows with {lim0} ids, {fu} of {nu} upper rows with {m} ids, {cross} inserts whose links cross")
    assert f0 >= 36 and cross >= 1, (f0, cross)
    gix, st = hv.ValidatedVectorReadIndex.build(dim=DIM, metric=METRIC, node_ids=ids, vectors=data, levels=lv, m=m, m0=m0,
                                                ef_construction=EFC, sequential=True)
    assert st["nodes"] == N and st["batches"] == N - 1
    assert_rows_equal(gix.export_graph(), ex, N)
    assert_searches_equal(hv, gix, oix, np.random.default_rng(m0).standard_normal((16, DIM)).astype(np.float32))
    assert gix.last_write_path() == hv.WRITE_EAGER_STEPS | (hv.WRITE_WIDE if wide else 0), gix.last_write_path()
    gix.close()
