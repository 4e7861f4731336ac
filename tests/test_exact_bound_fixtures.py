"""Self-checks of the adversarial rounding fixtures (fixtures.py: tail_fixture, certificate_fixture) that the GPU tests of the exact
scan's error bound use (test_gpu_exact_bounds.py).  An f64 model of the matrix-core arithmetic (bf16 RNE query, bf16 RNE f32 rows,
the full hi + lo split) checks, on the CPU, that each fixture (a) has the intended exact top-k in the reference's order, (b) is
adversarial: its rounding error defeats the bound the library used before scan_error_bound, and (c) stays within scan_error_bound."""
import ctypes

import numpy as np
import pytest

import fixtures as fx

TAIL_DIMS = [128, 256, 512, 768, 1024, 1536]
ONE_PASS = {"bf16": fx.ERR_BF16_ONE_PASS, "f32": fx.ERR_F32_SHADOW_ONE_PASS, "fp8": fx.ERR_FP8_ONE_PASS}
FULL = {"bf16": fx.ERR_BF16_FULL, "f32": fx.ERR_F32_FULL, "fp8": fx.ERR_FP8_FULL}


def oracle_top(orc, metric, data, q, k):
    rc, ids, sc = orc.flat_matrix(metric, data, q, k, kernel=orc.K_AVX_FMA_HW)
    assert rc == orc.OK
    return ids.tolist(), sc


@pytest.mark.parametrize("rows", ["bf16", "f32"])
@pytest.mark.parametrize("metric", [1, 0])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("dim", TAIL_DIMS)
def test_tail_fixture(orc, rows, metric, k, dim):
    data, q, rp, tp = fx.tail_fixture(dim, rows, k, 300, seed=dim + k)
    if rows == "bf16":
        assert (fx.round_bf16(data).view(np.uint32) == data.view(np.uint32)).all()  # the stored values ARE the fixture
    # (a) r, then the copies of t by id, in the reference's order
    ids, _ = oracle_top(orc, metric, data, q, k)
    assert ids == [rp] + sorted(tp)[: k - 1]
    ap = fx.one_pass_scores(metric, data, q, rows)
    ex = fx.exact_scores(metric, data, q)
    scale = fx.error_scale(metric, data, q)
    e_old = fx.scan_error_bound_before_fix(True, rows == "f32", metric == 1, dim) * scale
    e_new = fx.scan_error_bound(ONE_PASS[rows], metric == 1, dim) * scale
    gap = ap[rp] - ap[tp[0]]  # the tail skips r iff its approximation - E is above t's approximation + E
    err = np.abs(ap - ex).max()
    if metric == 1:
        # (b) with the old bound the tail would never re-score r and return the t's with status 0
        assert gap > 2.0 * e_old and err > e_old
    else:
        # cosine's bound keeps a factor two over the worst case ((1 - c) / 2 halves the error of c): near that worst case, not past it
        assert gap > 0.6 * e_old and err > 0.35 * e_new
    # (c) the derived bound covers the fixture, and r is re-scored
    assert err <= e_new and gap <= 2.0 * e_new


@pytest.mark.parametrize("rows,mx", [("bf16", False), ("f32", False), ("fp8", False), ("fp8", True)])
@pytest.mark.parametrize("k", [1, 10])
@pytest.mark.parametrize("dim", [256, 768, 1536])
def test_certificate_fixture(orc, rows, mx, k, dim):
    m = max(63, 2 * k)
    data, q, rp, tp, fp = fx.certificate_fixture(dim, rows, k, m, 300, seed=7 * dim + k, mx=mx, min_pos=100 if mx else 0)
    if rows == "fp8":  # the fixture's rows are e4m3 code points under a power-of-two row scale: the fp8 index stores them unchanged
        stored = fx.quantize_fp8_rows(data)
        for i in [rp] + tp + fp:
            assert stored[i].view(np.uint32).tolist() == data[i].view(np.uint32).tolist()
        data = stored
    if mx:
        assert min([rp] + tp + fp) >= 100
    ids, _ = oracle_top(orc, 1, data, q, k)  # (a)
    assert ids == [rp] + sorted(tp)[: k - 1]
    ap = fx.one_pass_scores(1, data, q, rows, mx=mx)
    ex = fx.exact_scores(1, data, q)
    scale = fx.error_scale(1, data, q)
    order = np.lexsort((np.arange(len(ap)), ap))
    cand = order[: m + 1]
    assert set(cand.tolist()) == set(tp) | set(fp) and rp == order[m + 1]  # r is the first row the one-pass selection leaves out
    thr = ap[order[m]]
    kth = np.sort(ex[cand])[k - 1]
    e_trap = fx.certificate_trap_bound(rows, dim, mx) * scale
    e_new = fx.scan_error_bound(fx.ERR_MX_FP8 if mx else ONE_PASS[rows], True, dim) * scale
    assert kth < thr - e_trap                                  # (b) the trap bound (the old one; MX: a quarter) certifies without r
    assert not kth < thr - e_new                               # (c) the derived one sends the query to the full split ...
    err = np.abs(ap - ex).max()
    assert err <= e_new
    if mx:
        assert err > 0.4 * e_new  # the two-piece split's worst case is half the bound: the fixture is near it
    full = fx.one_pass_scores(1, data, q, rows, full=True)     # ... which selects r and certifies
    e_full = fx.scan_error_bound(FULL[rows], True, dim) * scale
    assert np.abs(full - ex).max() <= e_full
    order = np.lexsort((np.arange(len(full)), full))
    assert rp in order[: m + 1].tolist()
    assert np.sort(ex[order[: m + 1]])[k - 1] < full[order[m]] - e_full


def test_mx_query_split_error():
    """mx_query (the model of split_queries_mx_kernel) over random queries: normal pieces within 2^-9 |q| (the bound takes 2^-8), the
    adversarial query at that worst case, every element within 2^-9 |q| + 2^-21 max |q|"""
    rng = np.random.default_rng(11)
    worst = 0.0
    for _ in range(50):
        q = (rng.standard_normal(1536) * rng.uniform(0.01, 100.0)).astype(np.float32)
        err = np.abs(fx.mx_query(q) - q.astype(np.float64))
        assert (err <= 2.0 ** -9 * np.abs(q) + 2.0 ** -21 * np.abs(q).max()).all()
        worst = max(worst, float((err / np.abs(q))[np.abs(q) > np.abs(q).max() * 2.0 ** -6].max()))
    assert 2.0 ** -9.2 < worst <= 2.0 ** -9
    q = fx.adversarial_query_mx(768)
    rel = (fx.mx_query(q) - q.astype(np.float64)) / q
    A, B = np.arange(384), np.arange(384, 768)
    assert (rel[A] < -2.0 ** -9.1).all() and (rel[B] > 2.0 ** -9.1).all()


def test_full_split_bound_covers_its_residuals():
    """the full split's constant against its worst case, element by element: the query's hi + lo residual <= 2^-17 |q_i| (bf16 rows);
    for f32 rows also the row's residual and the dropped q_lo x_lo, 2 x 2^-16 per dot product in all -- 2^-14 in the L2 score"""
    rng = np.random.default_rng(5)
    v = (rng.uniform(1.0, 2.0, 200000) * np.exp2(rng.integers(-20, 20, 200000))).astype(np.float32)
    hi = fx.round_bf16(v)
    lo = fx.round_bf16((v - hi).astype(np.float32))
    res = np.abs(v.astype(np.float64) - hi - lo) / np.abs(v)
    assert res.max() <= 2.0 ** -17 and res.max() > 0.9 * 2.0 ** -17
    rel1 = np.abs(v.astype(np.float64) - hi) / np.abs(v)
    assert rel1.max() <= 2.0 ** -8 and rel1.max() > 0.99 * 2.0 ** -8  # bf16's unit roundoff: 2^-8, not 2^-9
    # f32 rows: q x - (qh xh + ql xh + qh xl), worst case over pairs of elements, relative to |q||x|
    q, x = v[:100000], v[100000:]
    qh, ql, xh, xl = hi[:100000], lo[:100000], hi[100000:], lo[100000:]
    d = q.astype(np.float64) * x - (qh.astype(np.float64) * xh + ql.astype(np.float64) * xh + qh.astype(np.float64) * xl)
    assert (np.abs(d) / (q.astype(np.float64) * x)).max() <= 2.0 ** -15 + 2.0 ** -23


def test_twin_matches_the_header():
    """the numpy twin equals scan_error_bound as the library computes it (hvxi_scan_error_bound: the header's function, host-compiled),
    for every kind, both metrics and every dimension the exact scan takes"""
    import pyhvx
    f = pyhvx.lib().hvxi_scan_error_bound
    f.restype = ctypes.c_float
    f.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    kinds = [fx.ERR_BF16_ONE_PASS, fx.ERR_BF16_FULL, fx.ERR_F32_SHADOW_ONE_PASS, fx.ERR_F32_REG_ONE_PASS, fx.ERR_F32_FULL, fx.ERR_FP8_ONE_PASS,
             fx.ERR_FP8_FULL, fx.ERR_MX_FP8]
    assert kinds == list(range(8))
    for kind in kinds:
        for l2 in (True, False):
            for dim in (128, 256, 384, 512, 768, 1024, 1536):
                got = f(kind, int(l2), dim)
                want = fx.scan_error_bound(kind, l2, dim)
                assert abs(got - want) <= 1e-6 * want, (kind, l2, dim, got, want)
    assert f(8, 1, 768) >= 1.0  # an unknown kind certifies nothing
