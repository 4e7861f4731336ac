"""Self-checks of the corpora that hold the exact scan along its result count and its attempt ladder (fixtures.py: scan_image,
rung1_fixture, ladder_block, overflow_fixture; used by test_gpu_scan_result_counts.py).  The oracle and the f64 model of the matrix-core
arithmetic (one_pass_scores, exact_scores, scan_error_bound) check, on the CPU, that the stored values are the fixture, that the exact
top-k is the intended one, and that the modelled certificate kth < t - E fails and holds at the rungs each corpus is built for.  These
are conditions on the inputs: a failure here means a fixture is wrong, not a kernel."""
import numpy as np
import pytest

import fixtures as fx

ONE_PASS = {"bf16": fx.ERR_BF16_ONE_PASS, "f32": fx.ERR_F32_REG_ONE_PASS, "fp8": fx.ERR_FP8_ONE_PASS}
FULL = {"bf16": fx.ERR_BF16_FULL, "f32": fx.ERR_F32_FULL, "fp8": fx.ERR_FP8_FULL}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def oracle_top(orc, metric, stored, q, k):
    rc, ids, sc = orc.flat_matrix(metric, stored, q, k, kernel=orc.K_AVX_FMA_HW)
    assert rc == orc.OK
    return ids.tolist(), sc


def is_bf16(x):
    return bool((bits(fx.round_bf16(x)) == bits(x)).all())


def is_fp8(stored):
    """every value is an e4m3fn code point times its row's scale max |x| / 448 (up to the f32 rounding of scale x code)"""
    s = stored.astype(np.float64)
    v = s / (np.abs(s).max(axis=1, keepdims=True) / 448.0)
    return bool((np.abs(fx.e4m3_rne(v) - v) <= 2.0 ** -20 * np.abs(v)).all())


def certificates(rows, stored, qs, k):
    """the modelled certificate of every query at the ladder's three attempts: [(one pass, full split, full split with m = 1023)]"""
    dim = stored.shape[1]
    ex, ap1, ap2 = fx.l2_model_scores(stored, qs, rows)
    scale = fx.l2_error_scales(stored, qs)
    e1 = fx.scan_error_bound(ONE_PASS[rows], True, dim) * scale
    e2 = fx.scan_error_bound(FULL[rows], True, dim) * scale
    # the model stays within the bounds it is judged by
    assert (np.abs(ap1 - ex).max(axis=1) <= e1).all() and (np.abs(ap2 - ex).max(axis=1) <= e2).all()
    m = max(63, 2 * k)
    return [(fx.certificate_holds(ap1[i], ex[i], k, m, e1[i]), fx.certificate_holds(ap2[i], ex[i], k, m, e2[i]),
             fx.certificate_holds(ap2[i], ex[i], k, fx.LADDER_M_WIDE, e2[i])) for i in range(qs.shape[0])]


@pytest.mark.parametrize("rows", ["bf16", "f32"])
def test_batched_model_is_the_per_query_model(rows):
    """l2_model_scores against exact_scores / one_pass_scores, query by query"""
    rng = np.random.default_rng(3)
    data = rng.standard_normal((500, 128)).astype(np.float32)
    stored = fx.stored_rows(rows, data)
    qs = (stored[:4] + 0.05 * rng.standard_normal((4, 128))).astype(np.float32)
    ex, ap1, ap2 = fx.l2_model_scores(stored, qs, rows)
    for i, q in enumerate(qs):
        assert np.abs(ex[i] - fx.exact_scores(1, stored, q)).max() <= 1e-10
        assert np.abs(ap1[i] - fx.one_pass_scores(1, stored, q, rows)).max() <= 1e-10
        assert np.abs(ap2[i] - fx.one_pass_scores(1, stored, q, rows, full=True)).max() <= 1e-10
        assert fx.l2_error_scales(stored, qs)[i] == pytest.approx(fx.error_scale(1, stored, q), rel=1e-12)


@pytest.mark.parametrize("rows", ["bf16", "fp8", "f32"])
def test_scan_image_ties_and_duplicates(orc, rows):
    """the blocks are stored-identical rows, and the oracle alone answers a query next to block T with the k lowest ids of the block
    under equal score bits, for every (k, T) the device test runs and both metrics"""
    im = fx.scan_image(rows)
    data, stored = im["data"], im["stored"]
    assert stored.shape == fx.SCAN_SHAPES[rows] and im["pool"].shape == (129, stored.shape[1])
    if rows == "bf16":
        assert is_bf16(data)
    if rows != "fp8":
        assert (bits(stored) == bits(data)).all()
    else:
        assert is_fp8(stored) and not is_fp8(data)
    for a, b in im["dups"]:
        assert a != b and (bits(stored[a]) == bits(stored[b])).all()
    taken = np.concatenate(list(im["blocks"].values()))
    assert np.unique(taken).size == sum(fx.TIE_BLOCKS)
    for t, bp in im["blocks"].items():
        assert bp.size == t and (np.diff(bp) > 0).all() and (bits(stored[bp]) == bits(stored[bp[0]])).all()
        assert np.diff(bp).max() > 1   # scattered, not a run of ids
    assert (bits(im["pool"][0]) == bits(stored)).all(axis=1).any()   # one query IS a stored row
    for metric in (1, 0):
        for k, t in fx.TIE_CASES_K_T:
            for q in im["near"][t][[0, 1, 32]]:
                ids, sc = oracle_top(orc, metric, stored, q, k)
                assert ids == im["blocks"][t][:k].tolist() and np.unique(bits(sc)).size == 1
                ids, sc = oracle_top(orc, metric, stored, q, t + 1)   # ... and the block ends where it should
                assert ids[:t] == im["blocks"][t].tolist() and bits(sc)[t] != bits(sc)[0]
        for j, (a, b) in enumerate(im["dups"]):
            ids, sc = oracle_top(orc, metric, stored, im["pool"][1 + j], 2)
            assert ids == sorted((a, b)) and bits(sc)[0] == bits(sc)[1]


def test_rung1_fixture(orc):
    """rung 1: no modelled error, k rows at one score, m + 1 or more rows at a gap between the two bounds: the one-pass certificate fails
    on its bound alone, the full split's holds; every easy query certifies at the first attempt"""
    k = 10
    fxr = fx.rung1_fixture(k=k)
    data, q = fxr["data"], fxr["hard"]
    dim = data.shape[1]
    assert is_bf16(data) and is_bf16(q)
    ids, sc = oracle_top(orc, 1, data, q, k + fxr["ring"].size)
    assert ids[:k] == fxr["near"].tolist() and ids[k:] == fxr["ring"].tolist()
    assert bits(sc[:k]).tolist() == [bits(np.float32(0.25))] * k
    assert bits(sc[k:]).tolist() == [bits(np.float32(0.25 + fxr["gap"]))] * fxr["ring"].size
    assert fxr["ring"].size >= max(63, 2 * k) + 1
    ex = fx.exact_scores(1, data, q)
    rest = np.setdiff1d(np.arange(data.shape[0]), np.concatenate([fxr["near"], fxr["ring"]]))
    assert ex[rest].min() > 200 * 0.25
    scale = fx.error_scale(1, data, q)
    e1 = fx.scan_error_bound(fx.ERR_BF16_ONE_PASS, True, dim) * scale
    e2 = fx.scan_error_bound(fx.ERR_BF16_FULL, True, dim) * scale
    assert 4 * e2 < fxr["gap"] < e1 / 4 and 0.7 * fxr["g"] < fxr["gap"] < 1.4 * fxr["g"]
    ap = fx.one_pass_scores(1, data, q, "bf16")
    assert np.abs(ap - ex).max() <= e2 and np.abs(ap - ex).max() <= 2.0 ** -20 * scale   # (the row norm's f32 rounding is all there is)
    assert certificates("bf16", data, q[None, :], k) == [(False, True, True)]
    assert all(c[0] for c in certificates("bf16", data, fxr["easy"], k))


@pytest.mark.parametrize("rows", ["bf16", "fp8"])
def test_rung2_fixture(orc, rows):
    """rung 2: 500 stored-identical rows nearest, the rest ten times as far or more: no certificate at m = 63, one at m = 1023"""
    k = 10
    fb = fx.ladder_block(2, rows)
    stored, bp = fb["stored"], fb["block"]
    assert bp.size == 500 and stored.shape[0] >= 2048 and (bits(stored[bp]) == bits(stored[bp[0]])).all()
    if rows == "bf16":
        assert is_bf16(fb["data"]) and (bits(stored) == bits(fb["data"])).all()
    else:
        assert is_fp8(stored)
    far = np.setdiff1d(np.arange(stored.shape[0]), bp)
    for q in fb["hard"]:
        ids, sc = oracle_top(orc, 1, stored, q, k)
        assert ids == bp[:k].tolist() and np.unique(bits(sc)).size == 1
    ex = fx.l2_model_scores(stored, fb["hard"], rows)[0]
    assert (ex[:, far].min(axis=1) >= 10.0 * ex[:, bp[0]]).all()
    assert certificates(rows, stored, fb["hard"], k) == [(False, False, True)] * fb["hard"].shape[0]
    assert all(c[0] for c in certificates(rows, stored, fb["easy"], k))


@pytest.mark.parametrize("rows", ["bf16", "fp8", "f32"])
def test_rung3_fixture(orc, rows):
    """rung 3: 1 500 identical rows: no certificate at m = 63 nor at m = 1023"""
    k = 10
    fb = fx.ladder_block(3, rows)
    stored, bp = fb["stored"], fb["block"]
    assert bp.size == 1500 and (bits(stored[bp]) == bits(stored[bp[0]])).all()
    assert {"bf16": is_bf16, "fp8": is_fp8, "f32": lambda x: True}[rows](stored) and (rows == "fp8" or (bits(stored) == bits(fb["data"])).all())
    far = np.setdiff1d(np.arange(stored.shape[0]), bp)
    for q in fb["hard"]:
        ids, sc = oracle_top(orc, 1, stored, q, k)
        assert ids == bp[:k].tolist() and np.unique(bits(sc)).size == 1
    ex = fx.l2_model_scores(stored, fb["hard"], rows)[0]
    assert (ex[:, far].min(axis=1) >= 10.0 * ex[:, bp[0]]).all()
    assert certificates(rows, stored, fb["hard"], k) == [(False, False, False)] * fb["hard"].shape[0]
    assert all(c[0] for c in certificates(rows, stored, fb["easy"], k))


def test_overflow_fixture():
    """the first filtered slice (rows 1 024 .. 4 095) holds more rows below the first chunk's 64th modelled score than a query's pair
    buffer takes, for every query"""
    data, qs = fx.overflow_fixture()
    assert is_bf16(data) and data.shape[0] >= 4 * fx.OVERFLOW_FIRST_CHUNK
    c = fx.OVERFLOW_FIRST_CHUNK
    for q in qs:
        ap = fx.one_pass_scores(1, data, q, "bf16")
        ex = fx.exact_scores(1, data, q)
        assert ex[:c].min() >= 10.0 * ex[c:].max()
        thr = np.sort(ap[:c])[63]
        assert int((ap[c:4 * c] < thr).sum()) > fx.OVERFLOW_PAIR_CAP
