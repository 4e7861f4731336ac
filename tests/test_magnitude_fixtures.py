"""Self-checks of the magnitude fixtures (fixtures.py: scaled_case, COSINE_SCALES, L2_SCALES) that the GPU tests at the ends of the f32
range use (test_gpu_magnitude.py).  For every case, on the CPU: the oracle answers it, its top-k is the f64 ranking's with a clear gap
behind rank k, a scaled cosine case ranks like its unit-scale twin (the scaling is exact), and a numpy twin of the UNGUARDED f32
approximation of the matrix-core scans (approx_half_cosine_model) breaks scan_error_bound exactly on the cases marked as traps."""
import ctypes

import numpy as np
import pytest

import fixtures as fx

N, DIM, K = 3000, 256, 10
SEED = fx.MAGNITUDE_SEEDS[(DIM, N)]
GAP = 2.0 ** -12


def oracle_top(orc, metric, data, q, k):
    rc, ids, sc = orc.flat_matrix(metric, data, q, k, kernel=orc.K_AVX_FMA_HW)
    assert rc == orc.OK
    return ids.tolist(), sc


def f64_top(scores, k):
    order = np.lexsort((np.arange(len(scores)), scores))
    return order[:k].tolist(), float(scores[order[k]] - scores[order[k - 1]])


@pytest.mark.parametrize("name", [c[0] for c in fx.COSINE_SCALES])
def test_cosine_case(orc, name):
    _, sq, sr, out, trap = fx.COSINE_SCALE[name]
    data, q, src = fx.cosine_case(name, DIM, N, SEED)
    ud, uq, _ = fx.cosine_case(name, DIM, N, SEED, unit=True)
    unit_ids = oracle_top(orc, orc.COSINE, ud, uq, K)[0]
    ids, sc = oracle_top(orc, orc.COSINE, data, q, K)
    ex = fx.f64_half_cosine(data, q)
    want, gap = f64_top(ex, K)
    print(f"{name}: f64 gap behind rank {K} = {gap:.3e}")
    assert ids == want and ids[0] == src
    assert gap >= GAP
    assert ids == unit_ids  # cosine is scale-invariant and the scaling exact
    assert np.abs(sc.astype(np.float64) - ex[ids]).max() <= 2.0 ** -20  # the oracle's f32 scores are the f64 ones, rounded
    bound = fx.scan_error_bound(fx.ERR_BF16_ONE_PASS, False, DIM)  # the smallest one-pass bound; the f32 / MX ones are < 2.1 times it
    errs = []
    for flush in (False, True):
        ap = fx.approx_half_cosine_model(data, q, flush=flush).astype(np.float64)
        errs.append(float(np.where(np.isfinite(ap), np.abs(ap - ex), np.inf).max()))
    print(f"{name}: model error {errs[0]:.3e} (subnormals kept), {errs[1]:.3e} (flushed); bound {bound:.3e}")
    if trap:
        assert max(errs) > 2.1 * bound
    else:
        assert max(errs) <= bound
    # the guarded expression (the query scaled by an exact power of two, no approximation for rows outside the trusted norms) keeps the
    # bound on every row it scores, whether or not a matrix core flushes subnormals, and gives up exactly the rows it should
    for flush in (False, True):
        ap, has = fx.guarded_half_cosine_model(data, q, flush=flush)
        assert np.abs(ap[has].astype(np.float64) - ex[has]).max(initial=0.0) <= 2.0 ** -18, (name, flush)
        assert (ap[~has] == 0).all()
        assert (~has).sum() == {"r126": N, "outliers": fx.N_OUTLIERS}.get(name, 0), (name, int((~has).sum()))


def test_unit_scale_twin_of_every_row_scaling():
    """the scaled rows ARE the unit rows times a power of two, bit for bit after undoing it"""
    for name, sq, sr, out, _ in fx.COSINE_SCALES:
        base, q0, src0 = fx.cosine_case(name, DIM, N, SEED, unit=True)
        data, q, src = fx.cosine_case(name, DIM, N, SEED)
        assert src == src0
        with np.errstate(divide="ignore"):
            e = np.round(np.log2(np.abs(data[:, 0].astype(np.float64)) / np.abs(base[:, 0].astype(np.float64)))).astype(np.int32)
        assert (np.ldexp(base, e[:, None]).view(np.uint32) == data.view(np.uint32)).all()
        assert (np.ldexp(q0, sq).view(np.uint32) == q.view(np.uint32)).all()
        if out is not None:
            assert (e != 0).sum() == fx.N_OUTLIERS and e[src] == out


@pytest.mark.parametrize("dim,n", sorted(fx.MAGNITUDE_SEEDS))
def test_every_shape_of_the_gpu_tests_keeps_the_gap(orc, dim, n):
    """the rank-10 / rank-11 gap of every (dim, rows) the device tests scan, cosine and L2, on the unit-scale rows (the scalings are exact
    powers of two: the cosine scores do not move, the L2 scores move together), with the source row moved as the tile tests move it"""
    seed = fx.MAGNITUDE_SEEDS[(dim, n)]
    for src_min in (0, n - n // 8):
        data, q, src = fx.scaled_case(dim, n, seed, 0, 0, src_min=src_min)
        assert src >= src_min
        ex = fx.f64_half_cosine(data, q)
        want, gap = f64_top(ex, K)
        assert want[0] == src and gap >= GAP, (dim, n, gap)
        l2 = fx.f64_l2sq(data, q)
        want2, gap2 = f64_top(l2, K)
        assert want2[0] == src and gap2 / l2[want2[K - 1]] >= GAP
        if dim % 4 == 0 and src_min == 0:
            assert oracle_top(orc, orc.COSINE, data, q, K)[0] == want


@pytest.mark.parametrize("metric_name,dim,n", [("l2", 256, 3000), ("l2", 256, 6000), ("l2", 256, 17500), ("l1", 256, 3000)])
@pytest.mark.parametrize("name", [c[0] for c in fx.L2_SCALES])
def test_l2_l1_case(orc, metric_name, dim, n, name):
    metric = orc.L2SQ if metric_name == "l2" else orc.L1
    limit = float(orc.lib().orc_component_limit(metric, dim))
    assert np.isfinite(limit) and limit > 0
    data, q, src = fx.l2_case(name, dim, n, fx.l2_seed(name, dim, n), limit)
    if name == "limit":
        assert np.abs(data).max() <= 0.99 * limit and np.abs(data).max() > 0.98 * limit
    rc, ids, sc = orc.flat_matrix(metric, data, q, K)
    assert rc == orc.OK and len(ids) == K
    assert np.isfinite(sc).all()
    if metric_name == "l1":
        x = data.astype(np.float64)
        ex = np.abs(x - q.astype(np.float64)).sum(axis=1)
    else:
        ex = fx.f64_l2sq(data, q)
    if name == "subnormal" and metric_name == "l2":  # L2 scores are subnormals with a few bits: heavy exact ties, compared with the oracle alone
        assert 0 < sc.max() < np.finfo(np.float32).tiny
        return
    want, gap = f64_top(ex, K)
    rel = gap / ex[want[K - 1]]
    print(f"{metric_name} {name}: relative f64 gap behind rank {K} = {rel:.3e}")
    assert ids.tolist() == want and int(ids[0]) == src
    assert rel >= GAP  # (L2 / L1 scores scale with the data: the gap is relative to the k-th score)


def test_cosine_query_scaling_and_trusted_norms():
    """the magnitude precondition as the library evaluates it (hvx_flat_mfma.h, host-compiled): every finite non-zero maximum, subnormals
    included, is scaled into [2^12, 2^13) by an exact power of two; a row norm is trusted on [2^-100, 2^107] and nowhere else -- with
    |q^| < 2^13 sqrt(1536) the products stay below 2^126, and the rows of every case of COSINE_SCALES fall on the side its comment says"""
    import pyhvx
    L = pyhvx.lib()
    L.hvxi_cosine_query_exponent.restype = ctypes.c_int
    L.hvxi_cosine_query_exponent.argtypes = [ctypes.c_float]
    L.hvxi_cosine_term_trusted.restype = ctypes.c_uint32
    L.hvxi_cosine_term_trusted.argtypes = [ctypes.c_float]
    rng = np.random.default_rng(1)
    u = np.concatenate([rng.integers(1, 0x7F800000, 4000, dtype=np.int64), [1, 2, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x3F800000, 0x3FFFFFFF]]).astype(np.uint32)
    for v in u.view(np.float32):
        e = L.hvxi_cosine_query_exponent(float(v))
        assert 2.0 ** 12 <= np.ldexp(np.float64(v), -e) < 2.0 ** 13, (v, e)
    assert L.hvxi_cosine_query_exponent(0.0) == 0
    trusted = lambda x: bool(L.hvxi_cosine_term_trusted(float(np.float32(x))))
    assert trusted(2.0 ** -100) and trusted(2.0 ** 107) and trusted(1.0)
    assert not trusted(np.nextafter(np.float32(2.0 ** -100), np.float32(0))) and not trusted(np.nextafter(np.float32(2.0 ** 107), np.float32(np.inf)))
    assert not trusted(0.0) and not trusted(np.inf) and not trusted(np.nan) and not trusted(np.finfo(np.float32).max)
    assert 2.0 ** 13 * np.sqrt(1536.0) * 2.0 ** 107 < 2.0 ** 126
    for name, sq, sr, out, _ in fx.COSINE_SCALES:
        data, q, src = fx.cosine_case(name, DIM, N, SEED)
        xs, ex = fx._pow2_normalised(data, axis=1)
        norms = np.ldexp(np.linalg.norm(xs, axis=1), ex[:, 0])  # f64: no overflow
        ok = np.array([trusted(min(x, np.finfo(np.float32).max)) for x in norms])
        # fp8 rows are scored against their CODES (cos(q, scale codes) = cos(q, codes)): the codes' norm is trusted on every case
        stored = fx.quantize_fp8_rows(data).astype(np.float64)
        amax = np.abs(data).max(axis=1).astype(np.float32)
        codes = stored / (amax / np.float32(448.0)).astype(np.float64)[:, None]
        cn = np.linalg.norm(codes, axis=1)
        assert (cn >= 447.9).all() and (cn <= 448.1 * np.sqrt(DIM)).all() and all(trusted(x) for x in cn[::97])
        if name == "r126":
            assert not ok.any()
        elif name == "outliers":
            assert (~ok).sum() == fx.N_OUTLIERS and not ok[src]
        else:
            assert ok.all(), name
