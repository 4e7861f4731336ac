"""Deterministic fixtures restated from the reference's own tests (no reference code is imported).

Each generator cites the reference file:line it follows (paths under /root/reference/crates/db/).
"""
from __future__ import annotations

import math

import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MASK64 = (1 << 64) - 1


def lifecycle_vector(entity_id: int, dim: int = 128) -> np.ndarray:
    """tests/production_support/index_lifecycle_scale.rs:410-421 `vector(entity_id)`:
    xorshift(13,7,17) seeded id+0x9e3779b97f4a7c15, component = ((s & 0xffff) - 32768)/32768."""
    state = (entity_id + 0x9E3779B97F4A7C15) & MASK64
    out = np.empty(dim, np.float32)
    for i in range(dim):
        state ^= (state << 13) & MASK64
        state ^= state >> 7
        state ^= (state << 17) & MASK64
        centered = (state & 0xFFFF) - 32768
        out[i] = np.float32(centered) / np.float32(32768.0)
    return out


def lifecycle_matrix(n: int, dim: int = 128) -> np.ndarray:
    """Vectorised `lifecycle_vector` for ids 0..n-1 (bit-identical)."""
    state = (np.arange(n, dtype=np.uint64) + np.uint64(0x9E3779B97F4A7C15))
    out = np.empty((n, dim), np.float32)
    for i in range(dim):
        state ^= state << np.uint64(13)
        state ^= state >> np.uint64(7)
        state ^= state << np.uint64(17)
        centered = (state & np.uint64(0xFFFF)).astype(np.int64) - 32768
        out[:, i] = centered.astype(np.float32) / np.float32(32768.0)
    return out


def circle_vector(entity_id: int, entity_count: int, dim: int = 2) -> np.ndarray:
    """src/search/vector/scale_contracts.rs:45-49 vector_for (dim 2); the 8-D variant used by
    tests/production_support/vector/restricted.rs pads harmonics -- see circle_vector_nd."""
    angle = math.tau * entity_id / entity_count
    return np.array([np.float32(math.cos(angle)), np.float32(math.sin(angle))], np.float32)


def skip_neighbors(entity_id: int, entity_count: int) -> list[int]:
    """src/search/vector/scale_contracts.rs:52-72: power-of-two ring links, sorted, deduped."""
    out = []
    offset = 1
    while offset < entity_count:
        forward = (entity_id - 1 + offset) % entity_count + 1
        backward = (entity_id - 1 + entity_count - offset % entity_count) % entity_count + 1
        if forward != entity_id:
            out.append(forward)
        if backward != entity_id:
            out.append(backward)
        offset *= 2
    return sorted(set(out))


def circle_index_arrays(entity_count: int):
    """Seed arrays of the scale fixture (scale_contracts.rs:95-155): ids 1..N, entry=1, layer 0 only."""
    ids = np.arange(1, entity_count + 1, dtype=np.uint64)
    ang = (math.tau * ids.astype(np.float64)) / float(entity_count)
    vec = np.stack([np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)], axis=1)
    offs = [0]
    nbrs = []
    for i in range(1, entity_count + 1):
        nb = skip_neighbors(i, entity_count)
        nbrs.extend(nb)
        offs.append(len(nbrs))
    return ids, vec, np.array(offs, np.uint64), np.array(nbrs, np.uint64)


def circle_queries(entity_count: int, query_count: int = 24):
    """scale_contracts.rs:175-180."""
    return [circle_vector(1 + qi * (entity_count // query_count), entity_count) for qi in range(query_count)]


def draw_levels(n: int, m: int, seed: int) -> np.ndarray:
    """Layer draws for synthetic builds: uniform f32 from PCG64(seed) pushed through the reference's
    select_layer_from_uniform (src/search/vector/mod.rs:776-796) -- vectorised restatement."""
    rng = np.random.Generator(np.random.PCG64(seed))
    u = rng.random(n, dtype=np.float32)
    ml = np.float32(1.0) / np.log(np.float32(max(m, 2)))
    u = np.clip(u, np.finfo(np.float32).tiny, np.float32(1.0) - np.finfo(np.float32).eps)
    s = np.floor(-np.log(u).astype(np.float32) * ml)
    s = np.where(np.isfinite(s) & (s > 0), s, 0)
    return np.minimum(s, 63).astype(np.uint16)


def recall_at_k(got_ids, true_ids) -> float:
    hit = 0
    tot = 0
    for g, t in zip(got_ids, true_ids):
        ts = set(int(x) for x in t)
        hit += sum(1 for x in g if int(x) in ts)
        tot += len(t)
    return hit / max(tot, 1)


def merge_topk_reference(ids, scores, counts, k):
    """Checker for the multi-shard merge: per query, the k smallest of the gathered per-shard lists by
    the reference's Candidate order (score asc, then id asc; model.rs:55-61).
    ids/scores [g,b,k'], counts [g,b] -> (ids [b,k] u64, scores [b,k] f32, counts [b])."""
    ids = np.asarray(ids).astype(np.uint64)
    scores = np.asarray(scores, np.float32)
    counts = np.asarray(counts).astype(np.int64)
    g, b, _ = ids.shape
    out_i = np.zeros((b, k), np.uint64)
    out_s = np.zeros((b, k), np.float32)
    out_c = np.zeros(b, np.uint32)
    for q in range(b):
        cand = []
        for s in range(g):
            for t in range(int(counts[s, q])):
                cand.append((float(scores[s, q, t]), int(ids[s, q, t])))
        cand.sort()
        cand = cand[:k]
        out_c[q] = len(cand)
        for t, (sc, i) in enumerate(cand):
            out_i[q, t] = i
            out_s[q, t] = np.float32(sc)
    return out_i, out_s, out_c


def round_bf16(x: np.ndarray) -> np.ndarray:
    """f32 -> nearest bf16 (ties to even) -> f32: the values a bf16-stored index holds."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    lsb = (u >> np.uint64(16)) & np.uint64(1)
    r = ((u + np.uint64(0x7FFF) + lsb) >> np.uint64(16)) << np.uint64(16)
    return (r & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.float32).reshape(np.shape(x))


def quantize_fp8_rows(x: np.ndarray) -> np.ndarray:
    """The values an fp8-e4m3fn-stored index holds (twin of quantize_fp8_kernel, hvx_dtype.hip): per row
    scale = max|x| / 448, code = RNE(x / scale) to e4m3fn, value = fl32(scale * decode(code))."""
    x = np.ascontiguousarray(x, np.float32)
    amax = np.abs(x).max(axis=1).astype(np.float32)
    scale = np.where(amax > 0, amax / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    y = (x / scale[:, None]).astype(np.float32)
    a = np.abs(y)
    a = np.where(a < np.float32(464.0), a, np.float32(448.0)).astype(np.float32)
    _, ex = np.frexp(a)
    e = ex.astype(np.int32) - 1
    e = np.where((a == 0) | (e < -6), -6, e)
    step = np.ldexp(np.float32(1.0), e - 3).astype(np.float32)
    v = (np.rint(a / step) * step).astype(np.float32)
    v = np.minimum(v, np.float32(448.0))
    v = np.where(y < 0, -v, v).astype(np.float32)
    return (scale[:, None] * v).astype(np.float32)


# ---- adversarial rounding for the matrix-core exact scan (hvx_flat_mfma.h, scan_error_bound) ----
# The one-pass contraction rounds the query to bf16 (and f32 rows too); the exact tail (hvx_flat_tail.hip) and the re-rank
# certificate (hvx_flat_mfma.hip) are exact only if E bounds |approximate - reference-order score|.  Gaussian rows let the
# per-element rounding errors cancel; these rows line every error up with the same sign.

# contraction kinds of scan_error_bound (same order as the C++ enum)
ERR_BF16_ONE_PASS, ERR_BF16_FULL, ERR_F32_SHADOW_ONE_PASS, ERR_F32_REG_ONE_PASS, ERR_F32_FULL, ERR_FP8_ONE_PASS, ERR_FP8_FULL, ERR_MX_FP8 = range(8)


def scan_error_bound(kind: int, l2: bool, dim: int) -> float:
    """numpy twin of hvx::scan_error_bound: relative to (|q|^2 + max|x|^2) / 2 for L2, absolute for cosine."""
    u = 2.0 ** -8
    eps = {ERR_BF16_ONE_PASS: u, ERR_FP8_ONE_PASS: u, ERR_BF16_FULL: 2.0 ** -17, ERR_FP8_FULL: 2.0 ** -17,
           ERR_F32_SHADOW_ONE_PASS: 2 * u + u * u, ERR_F32_REG_ONE_PASS: 2 * u + u * u, ERR_F32_FULL: 2.0 ** -15 + 2.0 ** -23,
           ERR_MX_FP8: u + 2.0 ** -21 * math.sqrt(dim)}[kind]
    return (2.0 * eps if l2 else eps) + 12.0 * dim * 2.0 ** -24 + 2.0 ** -18


def scan_error_bound_before_fix(one_pass: bool, f32_rows: bool, l2: bool, dim: int) -> float:
    """the bound the library used before it was derived per kind (RerankArgs::extra_rel): one rounded operand taken to
    drop <= 2^-9 |q||x|, which under-states bf16's 2^-8 unit roundoff"""
    extra = (2.0 ** -7 if f32_rows else 2.0 ** -8) if one_pass else 0.0
    return 2.0e-5 + 12.0 * dim * 2.0 ** -24 + extra


def _f32(x) -> np.ndarray:
    return np.asarray(x, np.float32)


def _halves(dim: int):
    h = dim // 2
    return np.arange(h), np.arange(h, dim)


def adversarial_query(dim: int) -> np.ndarray:
    """half the elements at 1 + 2^-8 - 2^-20 (bf16 RNE rounds them DOWN by almost 2^-8), half at 1 + 2^-8 + 2^-20 (rounded UP)"""
    A, B = _halves(dim)
    q = np.empty(dim, np.float32)
    q[A] = 1.0 + 2.0 ** -8 - 2.0 ** -20
    q[B] = 1.0 + 2.0 ** -8 + 2.0 ** -20
    return q


FP8_ROW_MAX = 448.0 / 256.0  # 1.75


def adversarial_query_mx(dim: int) -> np.ndarray:
    """the MX build's trap (split_queries_mx_kernel: s = 2^-6 here, max |q| / s in [128, 256)): q / s = 132.25 -+ 2^-10, so hi = 128 and
    lo = RNE(16 (4.25 -+ 2^-10)) = 64 resp. 72 in e4m3 (step 8 at [64, 128)): half the elements rounded DOWN by (0.25 - 2^-10) s, half
    UP by as much -- 2^-9.05 of |q|, the two-piece split's worst case for normal pieces"""
    A, B = _halves(dim)
    q = np.empty(dim, np.float32)
    q[A] = (132.25 - 2.0 ** -10) * 2.0 ** -6
    q[B] = (132.25 + 2.0 ** -10) * 2.0 ** -6
    return q


def e4m3_rne(y) -> np.ndarray:
    """f64 -> the nearest e4m3fn value (ties to even, saturating at 448): fp8_e4m3_encode / decode of hvx_device.h"""
    y = np.asarray(y, np.float64)
    a = np.minimum(np.abs(y), 448.0)
    e = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    e = np.where((a == 0) | (e < -6), -6.0, e)
    step = np.exp2(e - 3)
    v = np.minimum(np.rint(a / step) * step, 448.0)
    return np.where(y < 0, -v, v)


def mx_query(q: np.ndarray) -> np.ndarray:
    """f64 model of split_queries_mx_kernel: the value the MX build multiplies, s hi + (s / 16) lo"""
    q = _f32(q)
    mx = float(np.abs(q).max())
    e = (math.frexp(mx)[1] - 8) if mx > 0 else 0
    s = 2.0 ** e
    hi = e4m3_rne(q.astype(np.float64) / s)
    res = q.astype(np.float64) - hi * s
    lo = e4m3_rne(res / s * 16.0)
    return s * hi + s / 16.0 * lo


def adversarial_pair(dim: int, rows: str, nudge: float = 1.0 / 16.0):
    """(r, t) for adversarial_query: r's one-pass score is pushed UP by the rounding, its mirror t's DOWN, by as much as the
    rounding can; one element of r is nudged toward the query so that r is the exact nearest (L2 and cosine).  rows: "bf16"
    (values exact in bf16: only the query rounds) or "f32" (the rows round too, in the same direction)."""
    A, B = _halves(dim)
    q = adversarial_query(dim)
    r = np.empty(dim, np.float32)
    t = np.empty(dim, np.float32)
    if rows == "bf16":
        r[A], r[B] = 2.0, -2.0
        t[A], t[B] = -2.0, 2.0
    elif rows == "fp8":  # +-448 x 2^-8: the row scale max|x| / 448 is 2^-8, every value an e4m3 code point; the nudge is one code step
        r[A], r[B] = FP8_ROW_MAX, -FP8_ROW_MAX
        t[A], t[B] = -FP8_ROW_MAX, FP8_ROW_MAX
        r[B[0]] = -416.0 / 256.0
        return _f32(r), _f32(t)
    else:  # |x| = 2 q: x rounds in the direction its query element does
        r[A], r[B] = 2.0 * q[A], -2.0 * q[B]
        t[A], t[B] = -2.0 * q[A], 2.0 * q[B]
    r[B[0]] += np.float32(nudge)
    return _f32(r), _f32(t)


def far_rows(n: int, dim: int, rng, rows: str) -> np.ndarray:
    """rows far from the adversarial queries (every element in -[1.5, 1.99], fp8: -[1.3, 1.74] quantised) whose norms stay below the
    fixture's: max |x|^2 -- and with it E -- is the adversarial rows' own"""
    if rows == "fp8":
        return quantize_fp8_rows((-rng.uniform(1.3, 1.74, (n, dim))).astype(np.float32))
    x = (-rng.uniform(1.5, 1.99, (n, dim))).astype(np.float32)
    return round_bf16(x) if rows == "bf16" else x


def one_pass_scores(metric: int, data: np.ndarray, q: np.ndarray, rows: str, full: bool = False, mx: bool = False) -> np.ndarray:
    """f64 model of the matrix-core scores of every row: the dot product of the bf16-RNE query (+ its lo part when full) with the
    rows as the contraction sees them (bf16 rows as stored; f32 rows bf16-RNE, + their lo parts when full), turned into the
    metric's score with the exact norms the kernels use (|q|^2, |x|^2 in f64 rounded to f32; cosine: (1 - c) / 2).  fp8 rows: the stored
    values (codes widened exactly, the row scale applied after); mx: the query as the MX build's two e4m3 pieces (mx_query)."""
    q = _f32(q)
    x = _f32(data).astype(np.float64)
    qh = mx_query(q) if mx else round_bf16(q).astype(np.float64)
    ql = 0.0 if mx else round_bf16(_f32(q - round_bf16(q))).astype(np.float64)
    if rows == "f32":
        xh = round_bf16(_f32(data)).astype(np.float64)
        xl = round_bf16(_f32(_f32(data) - round_bf16(_f32(data)))).astype(np.float64)
        dot = xh @ qh + ((xh @ ql + xl @ qh) if full else 0.0)
    else:
        dot = x @ (qh + (ql if full else 0.0))
    qn2 = float(np.float32((q.astype(np.float64) ** 2).sum()))
    xn2 = (x ** 2).sum(axis=1).astype(np.float32).astype(np.float64)
    if metric == 1:
        return np.maximum(qn2 + xn2 - 2.0 * dot, 0.0)
    c = np.clip(dot / (math.sqrt(qn2) * np.sqrt(xn2)), -1.0, 1.0)
    return (1.0 - c) * 0.5


def exact_scores(metric: int, data: np.ndarray, q: np.ndarray) -> np.ndarray:
    """the scores in f64 on the stored values (the oracle's f32 scores are within its accumulation error of these)"""
    x = _f32(data).astype(np.float64)
    qd = _f32(q).astype(np.float64)
    if metric == 1:
        return ((x - qd) ** 2).sum(axis=1)
    return (1.0 - (x @ qd) / (np.linalg.norm(x, axis=1) * np.linalg.norm(qd))) * 0.5


def error_scale(metric: int, data: np.ndarray, q: np.ndarray) -> float:
    """what the relative L2 bound multiplies: (|q|^2 + max|x|^2) / 2; 1 for cosine's absolute bound"""
    if metric != 1:
        return 1.0
    return 0.5 * (float((_f32(q).astype(np.float64) ** 2).sum()) + float((_f32(data).astype(np.float64) ** 2).sum(axis=1).max()))


def tail_fixture(dim: int, rows: str, k: int, n_far: int, seed: int):
    """the exact tail's trap: r (the exact nearest, at a random position) and k copies of its mirror t among n_far far rows.  With an
    E below the rounding, the tail publishes t's approximate score + E as the k-th bound and never re-scores r.
    Returns (stored rows, query, r's position, t positions)."""
    rng = np.random.default_rng(seed)
    r, t = adversarial_pair(dim, rows)
    n = n_far + 1 + k
    data = far_rows(n, dim, rng, rows)
    # the t's at consecutive positions from a multiple of 64: distinct lanes of ONE wavefront of the tail, whose k-th smallest lane
    # minimum is then t's score (scattered copies leave a far row's score there, and the bound never gets tight)
    t0 = 64 * int(rng.integers(0, (n - k) // 64))
    tp = list(range(t0, t0 + k))
    rp = int(rng.choice(np.setdiff1d(np.arange(n), tp)))
    data[tp] = t
    data[rp] = r
    return data, adversarial_query(dim), rp, tp


def fp8_filler_row(dim: int, q: np.ndarray, target: float) -> np.ndarray:
    """filler_row for fp8 rows: values on the e4m3 code points of the row scale 2^-8 (one pair at -1.75 sets that scale), equal within
    each pair (one element per query half: the query's rounding errors cancel), chosen pair by pair to bring the score to the target"""
    A, B = _halves(dim)
    qd = _f32(q).astype(np.float64)
    codes = np.unique(np.abs(e4m3_rne(np.linspace(0.0, 448.0, 20000))))
    grid = -codes * 2.0 ** -8
    x = np.full(dim, -(1.0 / 256.0) * float(e4m3_rne(256.0 * (float(qd.mean()) - math.sqrt(target / dim)))), np.float64)
    x = -np.abs(x)
    x[A[0]] = x[B[0]] = -FP8_ROW_MAX
    for sweep in range(3):  # nearest first, then from above
        for j in range(1, len(A)):
            others = ((qd - x) ** 2).sum() - (qd[A[j]] - x[A[j]]) ** 2 - (qd[B[j]] - x[B[j]]) ** 2
            f = others + (qd[A[j]] - grid) ** 2 + (qd[B[j]] - grid) ** 2
            ok = f >= target if sweep == 2 else np.ones(f.shape, bool)
            v = grid[ok][np.argmin(np.abs(f[ok] - target))] if ok.any() else grid[np.argmax(f)]
            x[A[j]] = x[B[j]] = v
    assert ((qd - x) ** 2).sum() >= target
    return _f32(x)


def filler_row(dim: int, q: np.ndarray, target: float) -> np.ndarray:
    """a row of bf16 values whose one-pass L2 score is EXACT up to accumulation (equal sums over the two query halves: the
    query's rounding errors cancel) and lies in [target, target + a few bf16 steps): -c everywhere, then pairs (one element per
    half) one bf16 step further from the query until the score reaches the target"""
    A, B = _halves(dim)
    qd = _f32(q).astype(np.float64)
    c = 1.0 - math.sqrt(target / dim)  # (q - c)^2 = target / dim with q ~ 1
    x = np.full(dim, round_bf16(_f32([c]))[0], np.float32)
    step = np.float32(2.0 ** -7)  # the bf16 step of values in [1, 2)
    while ((qd - x) ** 2).sum() >= target:  # start below the target
        x = round_bf16(x + step)
    for j in range(len(A) * 4):
        if ((qd - x) ** 2).sum() >= target:
            break
        x[A[j % len(A)]] -= step
        x[B[j % len(A)]] -= step
    assert ((qd - x) ** 2).sum() >= target
    return round_bf16(x)


def certificate_fixture(dim: int, rows: str, k: int, m: int, n_far: int, seed: int, mx: bool = False, min_pos: int = 0):
    """the re-rank certificate's trap: k copies of t (approximations pushed down), m + 1 - k fillers with accurate approximations just
    above them, and r (the exact nearest) whose approximation overshoots past the fillers: the m + 1 candidates are the t's and the
    fillers, and r is row m + 2.  The certificate must fail (k-th exact score = t's is not below (m+1)-th approximate - E)
    with an honest E; an E below the rounding certifies the t's -- a wrong answer.
    The fillers sit above t's exact score by more than `e_trap`: the library's bound before scan_error_bound (bf16 / f32 / fp8 rows),
    a quarter of scan_error_bound for the MX build (mx=True: its query, adversarial_query_mx, and rows from position min_pos on, past the
    first chunk that the bf16 query scores).
    Returns (stored rows, query, r's position, t positions, filler positions)."""
    rng = np.random.default_rng(seed)
    r, t = adversarial_pair(dim, rows)
    q = adversarial_query_mx(dim) if mx else adversarial_query(dim)
    pair = np.stack([r, t])
    s_ex = exact_scores(1, pair, q)
    s_ap = one_pass_scores(1, pair, q, rows, mx=mx)
    lo, hi = s_ex[1] + certificate_trap_bound(rows, dim, mx) * error_scale(1, pair, q), s_ap[0]
    target = lo + 0.25 * (hi - lo)
    f = fp8_filler_row(dim, q, target) if rows == "fp8" else filler_row(dim, q, target)
    nf = m + 1 - k
    n = n_far + 1 + k + nf
    data = far_rows(n, dim, rng, rows)
    pos = min_pos + rng.permutation(n - min_pos)
    data[pos[0]] = r
    data[pos[1:k + 1]] = t
    data[pos[k + 1:k + 1 + nf]] = f
    return data, q, int(pos[0]), [int(p) for p in pos[1:k + 1]], [int(p) for p in pos[k + 1:k + 1 + nf]]


def certificate_trap_bound(rows: str, dim: int, mx: bool) -> float:
    """the bound the certificate fixture is built to defeat (relative, L2)"""
    if mx:
        return 0.25 * scan_error_bound(ERR_MX_FP8, True, dim)
    return scan_error_bound_before_fix(True, rows == "f32", True, dim)


# ---- magnitude: the ends of the f32 range (test_magnitude_fixtures.py, test_gpu_magnitude.py) ----
# Cosine has no component limit: the reference answers any finite magnitude through its f64 fallback.  The matrix-core scans form an
# approximate cosine in f32 from |q|^2, the row norm and the dot product, which is worthless once one of them leaves the normal range.
# All scalings are powers of two (np.ldexp): exact in f32, so a scaled cosine case has the ranking of its unit-scale twin.

# (name, sq, sr, outlier scale or None, trap): trap = the unguarded f32 approximation (approx_half_cosine_model) breaks scan_error_bound
COSINE_SCALES = [
    ("unit", 0, 0, None, False),
    ("r70", 0, 70, None, False),
    ("mixed", 0, "mixed", None, False),       # per-row 2^-100 .. 2^100
    ("q40r40", 40, 40, None, False),
    ("q70", 70, 0, None, True),               # |q|^2 = inf
    ("q63", 63, 0, None, True),
    ("q100r-100", 100, -100, None, True),     # max |q| above 2^100: beyond the exponent clamp the MX query split had
    ("q-100r100", -100, 100, None, True),     # ... and below 2^-100; |q|^2 = 0
    ("q-80", -80, 0, None, True),             # |q|^2 = 0
    ("q60r60", 60, 60, None, True),           # |q|^2 = inf, |q||x| = inf
    ("q62r62", 62, 62, None, True),           # the dot product overflows too
    ("q-78r40", -78, 40, None, True),         # |q|^2 a one-bit subnormal, |q||x| normal
    ("q-77r40", -77, 40, None, True),
    ("q-74", -74, 0, None, False),            # |q|^2 subnormal with ~10 bits: within the bound
    ("outliers", 0, 0, 122, True),            # five rows x 2^122, the query's source row among them: |q||x| overflows for those alone
    ("r126", 0, 126, None, True),             # the row norm exceeds FLT_MAX (unit components clipped to +-3.9: every element stays finite)
    ("q-70r-70", -70, -70, None, True),       # every product q_i x_i is below the normal range
]
COSINE_SCALE = {c[0]: c for c in COSINE_SCALES}
# the pairs kept on the large-batch paths
COSINE_SCALES_LARGE = ["unit", "q70", "q-80", "q62r62", "q-78r40", "outliers"]
# on top of those, for the MX-scaled fp8 build alone: queries past 2^+-100 (its query split clamped the block exponent there)
COSINE_SCALES_MX = ["q100r-100", "q-100r100"]
# L2 / L1: (name, kind): "limit" = uniform in +-0.99 component_limit(metric, dim); the others scale Gaussian clusters
L2_SCALES = [("limit", None), ("tiny", -60), ("subnormal", -72)]
N_OUTLIERS = 5
# seed per (dim, rows) of the exact-scan tests: the f64 gap between rank 10 and rank 11 is >= 2^-12 (cosine absolute, L2 relative to the
# 10th score) -- checked by test_magnitude_fixtures.py; the gap does not depend on the scaling
MAGNITUDE_SEEDS = {(100, 3000): 1, (768, 3000): 3, (256, 3000): 9, (256, 17500): 1, (256, 6000): 1, (256, 20000): 3, (256, 66000): 3}


def clustered_rows(dim: int, n: int, seed: int):
    """16 Gaussian centres plus 0.5 sigma noise (the tile tests' corpus); the query is one row plus 5 % noise.
    Returns (rows, query, the query's source row)."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((16, dim)).astype(np.float32)
    data = (centres[rng.integers(0, 16, n)] + 0.5 * rng.standard_normal((n, dim))).astype(np.float32)
    src = int(rng.integers(n // 2, n))
    q = (data[src] + 0.05 * rng.standard_normal(dim)).astype(np.float32)
    return data, q, src


def mixed_row_scales(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed + 977).integers(-100, 101, n).astype(np.int32)


def scaled_case(dim: int, n: int, seed: int, sq, sr, outliers=None, src_min: int = 0, allow_flush: bool = False, clip=None):
    """clustered_rows with the query times 2^sq and the rows times 2^sr (an int, "mixed", or one exponent per row); `outliers`: N_OUTLIERS
    rows -- the query's source row among them -- times 2^outliers on top.  src_min: the source row is moved (swapped) to a position >= it.
    clip: the unit-scale components are clipped to +-clip first (the query is drawn from the clipped row).
    Asserts that the scaling was exact: nothing overflowed and nothing non-zero fell below the normal range (unless allow_flush).
    Returns (rows, query, source row)."""
    data, q, src = clustered_rows(dim, n, seed)
    if clip is not None:
        q = (q - data[src]).astype(np.float32)
        data = np.clip(data, -clip, clip).astype(np.float32)
        q = (q + data[src]).astype(np.float32)
    if src < src_min:
        to = src_min + (src * 7919) % (n - src_min)
        data[[src, to]] = data[[to, src]]
        src = to
    e = mixed_row_scales(n, seed) if isinstance(sr, str) else np.broadcast_to(np.asarray(sr, np.int32), (n,)).copy()
    if outliers is not None:
        rng = np.random.default_rng(seed + 5)
        rows = np.concatenate([[src], rng.choice(np.setdiff1d(np.arange(n), [src]), N_OUTLIERS - 1, replace=False)])
        e[rows] += outliers
    sd = np.ldexp(data, e[:, None]).astype(np.float32)
    sqv = np.ldexp(q, sq).astype(np.float32)
    tiny = np.finfo(np.float32).tiny
    for a, b in ((data, sd), (q, sqv)):
        assert np.isfinite(b).all()
        if not allow_flush:
            assert (np.abs(b[a != 0]) >= tiny).all()
    return sd, sqv, src


def cosine_clip(name: str):
    return 3.9 if name == "r126" else None


def cosine_case(name: str, dim: int, n: int, seed: int, src_min: int = 0, unit: bool = False):
    """the named row of COSINE_SCALES; unit=True: its unit-scale twin (the same rows and query before the powers of two)"""
    _, sq, sr, out, _ = COSINE_SCALE[name]
    if unit:
        return scaled_case(dim, n, seed, 0, 0, src_min=src_min, clip=cosine_clip(name))
    return scaled_case(dim, n, seed, sq, sr, outliers=out, src_min=src_min, clip=cosine_clip(name))


def limit_case(dim: int, n: int, seed: int, limit: float):
    """rows and a query (one row plus 5 % noise, clipped) uniform in +-0.99 limit"""
    rng = np.random.default_rng(seed)
    lim = np.float32(0.99) * np.float32(limit)
    data = (rng.uniform(-1.0, 1.0, (n, dim)).astype(np.float32) * lim).astype(np.float32)
    src = int(rng.integers(n // 2, n))
    q = np.clip(data[src] + (0.05 * rng.standard_normal(dim)).astype(np.float32) * lim, -lim, lim).astype(np.float32)
    return data, q, src


def l2_seed(name: str, dim: int, n: int) -> int:
    """the seed whose rank-10 / rank-11 gap is >= 2^-12 of the 10th score and whose f32 top-10 is the f64 one (test_magnitude_fixtures.py):
    uniform rows are nearly equidistant, so the limit case keeps a seed of its own"""
    return 5 if name == "limit" else MAGNITUDE_SEEDS[(dim, n)]


def l2_case(name: str, dim: int, n: int, seed: int, limit: float):
    if name == "limit":
        return limit_case(dim, n, seed, limit)
    s = dict(L2_SCALES)[name]
    return scaled_case(dim, n, seed, s, s)


def _pow2_normalised(a: np.ndarray, axis=None):
    """a / 2^floor(log2 max|a|) in f64 (exact), per row (axis=1) or whole: magnitudes in [0, 2)"""
    a = np.asarray(a, np.float64)
    m = np.abs(a).max(axis=axis, keepdims=axis is not None)
    _, ex = np.frexp(np.where(m > 0, m, 1.0))
    return np.ldexp(a, -(ex - 1)), ex - 1


def f64_half_cosine(data: np.ndarray, q: np.ndarray) -> np.ndarray:
    """(1 - cos) / 2 in f64, each operand first scaled by its own max-abs power of two: no overflow at any f32 magnitude"""
    x, _ = _pow2_normalised(_f32(data), axis=1)
    qq, _ = _pow2_normalised(_f32(q))
    return (1.0 - (x @ qq) / (np.linalg.norm(x, axis=1) * np.linalg.norm(qq))) * 0.5


def f64_l2sq(data: np.ndarray, q: np.ndarray) -> np.ndarray:
    """|x - q|^2 in f64 with both operands scaled by ONE power of two (the larger max-abs), the scale restored in f64"""
    x = _f32(data).astype(np.float64)
    qq = _f32(q).astype(np.float64)
    m = max(float(np.abs(x).max()), float(np.abs(qq).max()), np.finfo(np.float64).tiny)
    e = math.frexp(m)[1] - 1
    d = np.ldexp(x, -e) - np.ldexp(qq, -e)
    return np.ldexp((d * d).sum(axis=1), 2 * e)


def approx_half_cosine_model(data: np.ndarray, q: np.ndarray, flush: bool = False) -> np.ndarray:
    """numpy twin of the f32 expression the matrix-core scans evaluated WITHOUT a magnitude guard: qn2 = fl32(|q|^2), term = fl32(|x|)
    clamped to FLT_MAX, dot accumulated in f32 from f32 products; den = sqrtf(qn2) * term; c = den > 0 ? dot / den : 0, clamped to
    [-1, 1]; (1 - c) / 2.  flush: a matrix core that flushes subnormal products and sums to zero (the scalar f32 operations keep
    subnormals either way).  It shows which cases are traps; it is never the expected value of a device test."""
    x = _f32(data)
    qv = _f32(q)
    fmax = np.finfo(np.float32).max
    with np.errstate(all="ignore"):
        qn2 = np.float32(min((qv.astype(np.float64) ** 2).sum(), np.inf))
        xs, ex = _pow2_normalised(x, axis=1)
        term = np.minimum(np.ldexp(np.linalg.norm(xs, axis=1), ex[:, 0]), fmax).astype(np.float32)
        prod = (x * qv[None, :]).astype(np.float32)
        if flush:
            prod = np.where(np.abs(prod) < np.finfo(np.float32).tiny, np.float32(0), prod)
        dot = prod.sum(axis=1, dtype=np.float32)
        if flush:
            dot = np.where(np.abs(dot) < np.finfo(np.float32).tiny, np.float32(0), dot)
        den = (np.sqrt(qn2) * term).astype(np.float32)
        c = np.where(den > 0, dot / den, np.float32(0)).astype(np.float32)
        c = np.where(c < -1, np.float32(-1), np.where(c > 1, np.float32(1), c))
        return ((np.float32(1) - c) * np.float32(0.5)).astype(np.float32)


COS_TERM_MIN, COS_TERM_MAX, COS_QUERY_EXP = 2.0 ** -100, 2.0 ** 107, 12  # hvx_flat_mfma.h: kCosTermMin, kCosTermMax, kCosQueryExp


def guarded_half_cosine_model(data: np.ndarray, q: np.ndarray, flush: bool = False):
    """numpy twin of what the scans evaluate since the magnitude precondition (hvx_flat_mfma.h: approx_half_cosine over the scaled query of
    split_queries_kernel): q^ = q 2^-e with max |q^_i| in [2^12, 2^13), qn2 = fl32(|q^|^2), the same f32 products and sums as
    approx_half_cosine_model; rows whose norm header leaves [2^-100, 2^107] and non-finite dot products score 0.
    Returns (scores, mask of the rows that HAVE an approximation)."""
    x = _f32(data)
    qv = _f32(q)
    fmax = np.finfo(np.float32).max
    mx = float(np.abs(qv).max())
    e = math.frexp(mx)[1] - 1 - COS_QUERY_EXP
    qh = np.ldexp(qv, -e).astype(np.float32)
    with np.errstate(all="ignore"):
        qn2 = np.float32((qh.astype(np.float64) ** 2).sum())
        xs, ex = _pow2_normalised(x, axis=1)
        term = np.minimum(np.ldexp(np.linalg.norm(xs, axis=1), ex[:, 0]), fmax).astype(np.float32)
        prod = (x * qh[None, :]).astype(np.float32)
        if flush:
            prod = np.where(np.abs(prod) < np.finfo(np.float32).tiny, np.float32(0), prod)
            prod = np.where(np.abs(x) < np.finfo(np.float32).tiny, np.float32(0), prod)  # subnormal row elements too
        dot = prod.sum(axis=1, dtype=np.float32)
        has = (term >= np.float32(COS_TERM_MIN)) & (term <= np.float32(COS_TERM_MAX)) & np.isfinite(dot)
        c = (dot / (np.sqrt(qn2) * term)).astype(np.float32)
        c = np.where(c < -1, np.float32(-1), np.where(c > 1, np.float32(1), c))
        s = ((np.float32(1) - c) * np.float32(0.5)).astype(np.float32)
    return np.where(has, s, np.float32(0)), has


# ---- tie-heavy corpora for the write path (test_tie_fixtures.py, test_gpu_build_ties.py) ----
# Gaussian rows never give two equal distances, so the (score, id) order of the beam, the strict < of select_diverse and the slack of
# the device's register beam decide nothing on them.  These rows have a handful of distinct distances among thousands of pairs.

def lattice_rows(n: int, dim: int, nz: int, seed: int, support: int = 0) -> np.ndarray:
    """n DISTINCT rows with exactly nz entries of +-1 and zeros elsewhere (support > 0: all of them within the first `support` coordinates
    -- a denser lattice: more rows share a coordinate, so more rows lie strictly closer than the mass of ties).  Every product and partial sum of a distance between two of them
    is a small integer, exact under every metric, summation tree and fused or unfused multiply-add (L2: even integers 2 .. 4 nz, cosine:
    (1 - j / nz) / 2 with one correctly rounded division); round_bf16 is the identity on them."""
    rng = np.random.default_rng(seed)
    seen, out = set(), np.zeros((n, dim), np.float32)
    i = 0
    while i < n:
        pos = np.sort(rng.choice(support or dim, nz, replace=False))
        sign = rng.integers(0, 2, nz) * 2 - 1
        key = (tuple(pos.tolist()), tuple(sign.tolist()))
        if key in seen:
            continue
        seen.add(key)
        out[i, pos] = sign
        i += 1
    return out


def duplicate_groups(groups, copies, filler: int, dim: int, seed: int):
    """Exact copies of `groups` lattice points (nz 2), copies[g] of point g, plus `filler` further distinct lattice rows, shuffled.
    Rows of a group tie at distance 0 with each other and at equal distances with everything else.
    Returns (rows, label per row: the group's number, -1 for a filler row)."""
    copies = [copies] * groups if np.isscalar(copies) else list(copies)
    assert len(copies) == groups
    base = lattice_rows(groups + filler, dim, 2, seed)
    rows = np.concatenate([np.repeat(base[:groups], copies, axis=0), base[groups:]])
    label = np.concatenate([np.repeat(np.arange(groups), copies), np.full(filler, -1)]).astype(np.int64)
    perm = np.random.default_rng(seed + 1).permutation(rows.shape[0])
    return np.ascontiguousarray(rows[perm]), label[perm]


def tie_prone_inserts(orc, oix_factory, data, ids, levels, efc: int, beam: int):
    """The oracle's sequential insertion of the rows into oix_factory()'s index.  Before insert i it counts the inserts that a register
    beam of `beam` entries cannot hold without evicting an equal-score candidate: the oracle's search(data[i], efc, efc) over the rows
    inserted so far is full (efc results) AND more than `beam` of those rows score at or under the worst entry of that W (oix.flat, the
    exact scan in the same arithmetic).  Returns (the oracle index, that count)."""
    oix = oix_factory()
    prone = 0
    for i in range(data.shape[0]):
        if i > beam:
            rc, _, wsc = oix.search(data[i], efc, efc)
            assert rc == orc.OK
            if wsc.size == efc:
                rc, _, fsc = oix.flat(data[i], beam + 1)
                assert rc == orc.OK
                prone += int(fsc.size > beam and fsc[beam] <= wsc[-1])
        assert oix.insert(int(ids[i]), data[i], int(levels[i])) == orc.OK
    return oix, prone


def unreachable_l0(ex) -> int:
    """rows of an oracle export that a walk over layer 0 from the entry point does not reach"""
    ids = ex["node_ids"].tolist()
    if not ids:
        return 0
    pos = {nid: t for t, nid in enumerate(ids)}
    off, nb = ex["l0_offsets"], ex["l0_neighbors"]
    seen = {pos[int(ex["entry_point"])]}
    stack = list(seen)
    while stack:
        t = stack.pop()
        for x in nb[int(off[t]):int(off[t + 1])].tolist():
            u = pos[x]
            if u not in seen:
                seen.add(u)
                stack.append(u)
    return len(ids) - len(seen)


TIE_BEAM = 192  # the register beam of the build searches at max(ef_construction, 2 M) <= 160: 64 * 3 entries
# name -> (corpus, n, dim, nz, metric, m, m0, ef_construction, oracle kernel name, level multiplier, min tie-prone inserts, min full rows)
# corpus "lattice": lattice_rows(n, dim, nz, seed 1), "lattice32": the same with support 32; "dup": duplicate_groups(2, [20, 80], n - 100, dim, seed 5).  metric: 0 cosine,
# 1 squared Euclidean, 2 Manhattan.  Full rows (layer-0 rows with m0 ids): >= 100 where the prune is the point of the case, >= 50 on the
# M 32 / M0 64 cases (<= 400 rows for the oracle's time: ~60 rows reach 64 ids), so that the 65-id prune runs under ties there too.
TIE_CASES = {
    "l2_efc160":   ("lattice", 1200, 128, 2, 1, 16, 32, 160, "avx_fma", 16, 100, 0),
    # non-zeros within 32 coordinates: ~70 rows at distance 2 from each row under ~1 000 at distance 4.  A full W of 4s then admits more
    # than 32 closer rows, which is what makes the DEVICE's 192-entry beam evict a tie (the count above says only that the ties exist)
    "l2_dense":    ("lattice32", 1200, 128, 2, 1, 16, 32, 160, "avx_fma", 16, 100, 0),
    "l2_prune":    ("lattice", 1200, 128, 3, 1, 16, 32, 100, "avx_fma", 16, 100, 100),
    "l2_small":    ("lattice", 380, 128, 2, 1, 16, 32, 160, "avx_fma", 16, 100, 0),
    "cos_small":   ("lattice", 380, 128, 2, 0, 16, 32, 160, "avx_fma", 16, 100, 0),
    "cos_prune":   ("lattice", 1200, 128, 3, 0, 16, 32, 100, "avx_fma", 16, 100, 100),
    "wide":        ("lattice", 380, 128, 2, 1, 32, 64, 160, "avx_fma", 32, 100, 50),
    "scalar_100":  ("lattice", 600, 100, 2, 1, 16, 32, 100, "scalar", 16, 100, 0),
    "l1_prune":    ("lattice", 600, 100, 3, 2, 8, 16, 64, "scalar", 8, 100, 100),
    "l1_wide":     ("lattice", 400, 100, 2, 2, 32, 64, 100, "scalar", 32, 100, 50),
    "dup":         ("dup", 380, 128, 2, 1, 16, 32, 160, "avx_fma", 16, 100, 0),
    "dup_wide":    ("dup", 380, 128, 2, 1, 32, 64, 160, "avx_fma", 32, 100, 50),
}
_TIE_BUILT = {}


def tie_inputs(name: str):
    """(rows, ids, levels, group label per row or None) of a TIE_CASES entry"""
    corpus, n, dim, nz, metric, m, m0, efc, kern, lm, _, _ = TIE_CASES[name]
    if corpus == "dup":
        data, label = duplicate_groups(2, [20, 80], n - 100, dim, 5)
    else:
        data, label = lattice_rows(n, dim, nz, 1, support=32 if corpus == "lattice32" else 0), None
    ids = np.arange(n, dtype=np.uint64) * 2 + 3
    return data, ids, draw_levels(n, lm, seed=n + 1), label


def tie_oracle_factory(orc, name: str):
    _, _, dim, _, metric, m, m0, efc, kern, _, _, _ = TIE_CASES[name]
    k = {"avx_fma": orc.K_AVX_FMA, "scalar": orc.K_SCALAR}[kern]
    return lambda: orc.Index(dim, metric, kernel=k, m=m, m0=m0, ef_construction=efc)


def tie_case(orc, name: str):
    """The oracle's sequential build of a TIE_CASES entry, once per process (nobody changes it): a dict with the oracle index `oix`, its
    export `ex`, the inputs (`data`, `ids`, `levels`, `label`), `prone` (tie_prone_inserts), `full` (layer-0 rows with m0 ids) and
    `unreachable` (unreachable_l0 of the oracle's own graph).  Asserts the counts the case is there for."""
    if name not in _TIE_BUILT:
        _, n, _, _, _, _, m0, efc, _, _, min_prone, min_full = TIE_CASES[name]
        data, ids, lv, label = tie_inputs(name)
        oix, prone = tie_prone_inserts(orc, tie_oracle_factory(orc, name), data, ids, lv, efc, TIE_BEAM)
        ex = oix.export()
        full = int((np.diff(ex["l0_offsets"].astype(np.int64)) == m0).sum())
        unreach = unreachable_l0(ex)
        print(f"oracle {name}: {prone} of {n} inserts tie-prone at a beam of {TIE_BEAM}, {full} layer-0 rows with {m0} ids, {unreach} unreachable nodes")
        assert prone >= min_prone and full >= min_full, (name, prone, full)
        _TIE_BUILT[name] = dict(oix=oix, ex=ex, data=data, ids=ids, levels=lv, label=label, prone=prone, full=full, unreachable=unreach)
    return _TIE_BUILT[name]


# ---- the graph prefilter at sizes where its kernels split their work (tests/test_prefilter_fixtures.py proves on the CPU that
# ---- every case below is what tests/test_gpu_prefilter_scale.py says it is)
BITMAP_BLOCK_IDS = 8192   # bitmap_count / _compact / _select cut the candidate bitmap into blocks of 256 words
UNBOUNDED = 1 << 30       # a max_depth no traversal here reaches


def csr_graph(n: int, seed: int, avg_row: int = 3, hubs=(), rows=None, sinks=(), n_labels: int = 0):
    """A seeded CSR graph in the reference's form (crates/graph-algorithms/src/model.rs:656-666: every outgoing row ascends by
    target); parallel edges and self-loops occur.  Row lengths are uniform in 0 .. 2 * avg_row, targets uniform over the nodes.
    `hubs` = (node, row length) overrides, `rows` = {node: the row's targets} spelled out, `sinks` = (node, k): k different
    ordinary sources trade one of their arcs for one to `node`.  Returns (offsets u64 [n + 1], targets u64, labels u32 or None)."""
    rng = np.random.default_rng(seed)
    rows = {int(u): np.sort(np.asarray(r, np.int64)) for u, r in (rows or {}).items()}
    lens = rng.integers(0, 2 * avg_row + 1, n)
    for u, length in hubs:
        lens[u] = length
    for u, r in rows.items():
        lens[u] = r.size
    off = np.zeros(n + 1, np.int64)
    off[1:] = np.cumsum(lens)
    tgt = rng.integers(0, n, int(off[-1]))
    for u, r in rows.items():
        tgt[off[u]:off[u + 1]] = r
    ordinary = np.ones(n, bool)
    ordinary[[u for u, _ in hubs] + list(rows)] = False
    ordinary &= lens > 0
    for v, k in sinks:
        src = rng.choice(np.nonzero(ordinary)[0], k, replace=False)
        tgt[off[src]] = v
    owner = np.repeat(np.arange(n), lens)
    tgt = tgt[np.lexsort((tgt, owner))]
    lab = rng.integers(0, n_labels, tgt.size).astype(np.uint32) if n_labels else None
    return off.astype(np.uint64), tgt.astype(np.uint64), lab


def chain_graph(length: int):
    """0 -> 1 -> ... -> length: (n, offsets, targets)"""
    n = length + 1
    off = np.minimum(np.arange(n + 1), length).astype(np.uint64)
    return n, off, np.arange(1, n, dtype=np.uint64)


def bitmap_ids(words) -> set:
    """the ids whose bit is set in a candidate bitmap (u64 or u32 words, bit i of word w = id 64 w + i / 32 w + i)"""
    return set(np.nonzero(np.unpackbits(np.ascontiguousarray(words).view(np.uint8), bitorder="little"))[0].tolist())


def bitmap_blocks(ids) -> list:
    """the bitmap blocks (of BITMAP_BLOCK_IDS ids) that hold at least one of `ids`, ascending"""
    return sorted(set(int(i) // BITMAP_BLOCK_IDS for i in ids))


def has_empty_block_between(ids) -> bool:
    blocks = bitmap_blocks(ids)
    return any(b - a > 1 for a, b in zip(blocks, blocks[1:]))


def row_union(off, tgt, seeds, lab=None, allowed=(), direction: int = 0) -> np.ndarray:
    """what one `expand` hop from `seeds` reaches (access/expand.rs:16-80): the union of their rows, ascending (numpy only)"""
    off = np.asarray(off, np.int64)
    tgt = np.asarray(tgt, np.int64)
    keep = np.ones(tgt.size, bool) if lab is None or not len(allowed) else np.isin(lab, np.asarray(allowed))
    owner = np.repeat(np.arange(off.size - 1), np.diff(off))
    is_seed = np.zeros(off.size - 1, bool)
    is_seed[np.asarray(seeds, np.int64)] = True
    parts = []
    if direction in (0, 2):
        parts.append(tgt[keep & is_seed[owner]])
    if direction in (1, 2):
        parts.append(owner[keep & is_seed[tgt]])
    return np.unique(np.concatenate(parts)).astype(np.uint64)


# the 20 011-node graph of the traversal tests (not a multiple of 32: the last bitmap word is partial): two hubs and one node
# with a long INCOMING row, three labels
G20K = dict(n=20011, seed=20011, hubs=((5, 300), (12345, 1000)), sinks=((777, 200),), n_labels=3)
G20K_HUBS, G20K_SINK = (5, 12345), 777
# the 70 001-node graph of the fused-hop tests.  1000 .. 1063 is one wavefront's group of seeds with rows of length 0, 1, 16, 17,
# 65 and 1 000 among ordinary ones; 2000 reaches every id of CONTIGUOUS_IDS; 2001 only ids that hold no vector in either image;
# 2002 is 300 parallel edges to five nodes; 300 .. 303 and the rows of what they reach are an island whose two-hop neighbourhood
# has candidates on both sides of two block boundaries and leaves blocks 4 and 5 empty; 304 / 305 are two populous rows inside
# blocks 0 and 6; 3000 has a long incoming row
G70K_GROUP = ((1003, 0), (1010, 1), (1020, 16), (1021, 17), (1030, 65), (1040, 1000))
THIRD_IDS = np.arange(0, 70001, 3, dtype=np.uint64)           # 23 334 rows behind the binary-search id map
CONTIGUOUS_IDS = np.arange(5000, 30000, dtype=np.uint64)
VECTORLESS = (1, 4, 7, 40003, 60001)
ISLAND_SEEDS = (300, 301, 302, 303)
_ISLAND = {300: [8191, 8192], 301: [24575, 24576], 302: [10, 8000], 303: [49152, 50001, 57343],
           8191: [8190, 8192], 8192: [8193], 24575: [24570], 24576: [24580], 10: [11], 8000: [], 49152: [49153], 50001: [57343],
           57343: [57342]}


def _g70k_rows():
    rng = np.random.default_rng(70001)
    rows = dict(_ISLAND)
    rows[304] = rng.choice(np.arange(0, 8192), 200, replace=False)
    rows[305] = rng.choice(np.arange(49152, 57344), 200, replace=False)
    rows[2000] = CONTIGUOUS_IDS
    rows[2001] = VECTORLESS
    rows[2002] = np.repeat([9, 12, 6000, 6003, 6006], 60)
    return rows


_GRAPHS = {}


def prefilter_graph(name: str):
    """(n, offsets, targets, labels) of "g20k" / "g70k", built once per process; nobody changes the arrays"""
    if name not in _GRAPHS:
        if name == "g20k":
            _GRAPHS[name] = (G20K["n"],) + csr_graph(**G20K)
        else:
            _GRAPHS[name] = (70001,) + csr_graph(70001, seed=70001, hubs=G70K_GROUP, rows=_g70k_rows(), sinks=((3000, 200),), n_labels=3)
    return _GRAPHS[name]


def _many_seeds(n: int, distinct: int, repeats: int, seed: int, first=()):
    """`distinct` different nodes and `repeats` second copies of some of them, shuffled, behind the nodes of `first`"""
    rng = np.random.default_rng(seed)
    pick = rng.choice(n, distinct, replace=False)
    s = np.concatenate([pick, rng.choice(pick, repeats)])
    rng.shuffle(s)
    return np.concatenate([np.asarray(first, np.int64), s]).astype(np.uint64)


def prefilter_traversals():
    """name -> (graph, seeds, max_depth, direction, allowed labels, hub degree): the traversals the scale tests run"""
    n = G20K["n"]
    return {
        "out1": ("g20k", np.array([2], np.uint64), UNBOUNDED, 0, (), 0),
        "in1": ("g20k", np.array([2], np.uint64), UNBOUNDED, 1, (), 0),
        "both1": ("g20k", np.array([2], np.uint64), UNBOUNDED, 2, (), 0),
        "many": ("g20k", _many_seeds(n, 4600, 400, 1), 3, 0, (), 0),                      # 5 000 seeds, shuffled, 400 twice
        "twice": ("g20k", np.tile(np.arange(n, dtype=np.uint64), 2), 2, 2, (), 0),        # more seeds than nodes
        "labelled": ("g20k", _many_seeds(n, 1400, 98, 2, first=G20K_HUBS), 3, 2, (1, 2), 0),   # 1 500 seeds, both hubs first
        "hubs": ("g20k", np.array([G20K_HUBS[1], 7], np.uint64), UNBOUNDED, 0, (), 100),  # one hub a seed, the other one met
        "island": ("g70k", np.array(ISLAND_SEEDS, np.uint64), 2, 0, (), 0),
        "dense": ("g70k", np.arange(0, 3000, dtype=np.uint64), 2, 0, (), 0),
    }


_ORACLE_RUNS = {}


def prefilter_oracle(orc, name: str):
    """orc.breadth_first of a prefilter_traversals() entry, once per process: (visits, edges)"""
    if name not in _ORACLE_RUNS:
        graph, seeds, md, direction, allowed, hub = prefilter_traversals()[name]
        n, off, tgt, lab = prefilter_graph(graph)
        _ORACLE_RUNS[name] = orc.breadth_first(n, off.astype(np.int64), tgt, lab, seeds, md, direction, allowed, hub)
    return _ORACLE_RUNS[name]


def hop_cases():
    """name -> (seeds, keyword arguments of prefilter_search_batch) on "g70k": the one-hop cases of the fused call"""
    group = np.arange(1000, 1064, dtype=np.uint64)
    run = lambda c: np.arange(1000, 1000 + c, dtype=np.uint64)
    return {
        "one": (run(1), {}), "group": (group, {}), "65": (run(65), {}), "1024": (run(1024), {}), "1025": (run(1025), {}),
        "5000": (run(5000), {}),                                                   # the seed buffer regrows; bound > both images
        "duplicates": (np.concatenate([group, group, np.full(5, 1040, np.uint64)]), {}),
        "parallel": (np.array([2002], np.uint64), {}),
        "in": (np.concatenate([group, np.array([3000], np.uint64)]), dict(direction=1)),
        "both_labelled": (run(700), dict(direction=2, allowed_labels=[1])),
        "every_row": (np.array([2000, 1040], np.uint64), {}),                      # reaches every row of the contiguous image
        "vectorless": (np.array([2001], np.uint64), {}),
        "sparse": (np.arange(300, 306, dtype=np.uint64), {}),                      # blocks 0 - 3 and 6, boundary ids
    }


# the sampled walk's image: walk_harness.random_graph(.., WALK_ROWS, 32, L2SQ, .., id_gap=True) holds ids 1, 4, .. 16 798, so the graph
# around it has three bitmap blocks (9 000 rows, four blocks, cost 10 s of oracle inserts; 5 600 is the smallest round count whose
# ids reach well into the third block)
WALK_ROWS = 5600
WALK_NODES = 3 * (WALK_ROWS - 1) + 1 + 3


def walk_hop_graph(n_nodes: int, seed: int, sources: int = 1500):
    """One edge per source (config #3's where_() shape) whose targets lie in the first and the last bitmap block only, the ids on
    the block edges among them: (offsets, targets, the sources)"""
    rng = np.random.default_rng(seed)
    last = (n_nodes - 1) // BITMAP_BLOCK_IDS * BITMAP_BLOCK_IDS
    pool = np.concatenate([np.arange(1, BITMAP_BLOCK_IDS), np.arange(last, n_nodes)])
    edge_ids = np.array([BITMAP_BLOCK_IDS - 2, BITMAP_BLOCK_IDS - 1, last, last + 1], np.int64)
    tgt = np.concatenate([edge_ids, rng.choice(pool, sources - edge_ids.size)]).astype(np.uint64)
    off = np.minimum(np.arange(n_nodes + 1), sources).astype(np.uint64)
    return off, tgt, np.arange(sources, dtype=np.uint64)


# ---- the exact scan along the result count and its attempt ladder (test_scan_ladder_fixtures.py proves on the CPU that every corpus
# ---- below is what tests/test_gpu_scan_result_counts.py says it is)
# The matrix-core scan tries three certificates in turn (hvx_flat_mfma.hip, flat_mfma_impl): the one-pass contraction with
# m = max(63, 2 k), the full hi + lo split with the same m, the full split with m = 1023; then the last resort (bf16 rows: the exact tail
# in sub-batches of 128 queries, f32 rows: the VALU scan, fp8 rows: an error).  Gaussian rows certify at the first one.
LADDER_M_WIDE = 1023
SCAN_COUNTS = [10, 511, 1, 128, 31, 257, 64, 32, 127, 65, 256, 255]   # grows and shrinks kc = max(63, 2 k) + 1 across every switch on k
SCAN_BATCHES = [1, 33, 130]
SCAN_SHAPES = {"bf16": (5000, 128), "fp8": (5000, 128), "f32": (17500, 256)}   # f32: past 2^22 row elements (the small-batch stream)
TIE_BLOCKS = [48, 100, 200, 300]
TIE_CASES_K_T = [(10, 48), (32, 48), (64, 100), (128, 200), (255, 300)]
_SCAN_IMAGES = {}


def stored_rows(rows: str, data: np.ndarray) -> np.ndarray:
    """the values an index of this row type holds for `data`"""
    return {"bf16": round_bf16, "fp8": quantize_fp8_rows, "f32": lambda x: np.ascontiguousarray(x, np.float32)}[rows](data)


def certificate_holds(approx: np.ndarray, exact: np.ndarray, k: int, m: int, e: float) -> bool:
    """rerank_bf16_kernel's certificate on modelled scores: the candidates are the m + 1 rows of smallest (approximate score, row), kth
    is the k-th smallest exact score among them and t the (m + 1)-th approximate score; the answer is certified iff kth < t - e (a
    scan of at most m rows re-scores every row and needs no certificate)"""
    if approx.shape[0] <= m:
        return True
    order = np.lexsort((np.arange(approx.shape[0]), approx))
    return bool(np.sort(exact[order[: m + 1]])[k - 1] < approx[order[m]] - e)


def scan_image(rows: str):
    """The image of the result-count tests, built once per process (nobody changes the arrays): a seeded normal corpus of
    SCAN_SHAPES[rows] (fp8: per-row magnitudes in [0.2, 3]) in which two rows are exact copies of two others and, for every T of
    TIE_BLOCKS, T rows at scattered positions are copies of one row.  `pool` holds 129 queries: a stored row, a row near each pair of
    duplicates, a row near each block, and normal draws.  Returns a dict: data (what the index is given), stored (what it holds), dups
    [(row, its copy)], blocks {T: ascending positions}, near {T: 33 queries next to block T}, pool."""
    if rows not in _SCAN_IMAGES:
        n, dim = SCAN_SHAPES[rows]
        rng = np.random.default_rng({"bf16": 501, "fp8": 502, "f32": 503}[rows])
        data = rng.standard_normal((n, dim)).astype(np.float32)
        if rows == "fp8":
            data *= rng.uniform(0.2, 3.0, (n, 1)).astype(np.float32)
        if rows == "bf16":
            data = round_bf16(data)
        pos = rng.permutation(n)
        blocks, at = {}, 4
        for t in TIE_BLOCKS:
            blocks[t] = np.sort(pos[at:at + t])
            data[blocks[t]] = data[blocks[t][0]]
            at += t
        dups = [(int(pos[0]), int(pos[1])), (int(pos[2]), int(pos[3]))]
        for a, b in dups:
            data[b] = data[a]
        stored = stored_rows(rows, data)
        # (5 % of the row's own magnitude: fp8 rows differ in theirs)
        noise = lambda src, cnt: (stored[src][None, :] + 0.05 * np.abs(stored[src]).mean() * rng.standard_normal((cnt, dim))).astype(np.float32)
        near = {t: noise(blocks[t][0], 33) for t in TIE_BLOCKS}
        pool = rng.standard_normal((129, dim)).astype(np.float32)
        pool[0] = stored[int(pos[at])]
        pool[1], pool[2] = noise(dups[0][0], 1)[0], noise(dups[1][0], 1)[0]
        for j, t in enumerate(TIE_BLOCKS):
            pool[3 + j] = near[t][0]
            pool[40 + j] = near[t][1]      # ... and past the first 32 queries
        _SCAN_IMAGES[rows] = dict(data=data, stored=stored, dups=dups, blocks=blocks, near=near, pool=pool)
    return _SCAN_IMAGES[rows]


def rung1_fixture(dim: int = 128, k: int = 10, n: int = 3000, ring: int = 80, seed: int = 11):
    """Rung 1 of the ladder: the one-pass certificate fails and the full split certifies.  Every value -- the hard query's components
    too -- is a multiple of 2^-5 below 4: exact in bf16, and every squared distance, norm and dot product an exact f32 sum whatever its
    order.  So the one-pass scores carry NO rounding error, and what fails the first certificate is its bound alone: k rows at distance^2
    1/4 (one component moved by 1/2), `ring` >= m + 1 rows a gap c^2 further (a second component moved by c), with c^2 the grid's
    nearest to g = sqrt(E_one E_full) scale -- a factor ~8 inside either bound -- and the rest of the rows two hundred times as far.
    Returns a dict: data, hard (the query), near / ring (positions), gap (c^2), g, easy (130 queries, a far row + 5 % noise each)."""
    rng = np.random.default_rng(seed)
    grid = 2.0 ** -5
    q = (rng.integers(-48, 49, dim) * grid).astype(np.float32)
    data = (rng.integers(-64, 65, (n, dim)) * grid).astype(np.float32)
    scale = error_scale(1, data, q)
    g = math.sqrt(scan_error_bound(ERR_BF16_ONE_PASS, True, dim) * scan_error_bound(ERR_BF16_FULL, True, dim)) * scale
    c = max(1.0, float(np.rint(math.sqrt(g) / grid))) * grid
    pos = rng.permutation(n)
    near, rpos = np.sort(pos[:k]), np.sort(pos[k:k + ring])
    for t, p in enumerate(near):
        data[p] = q
        data[p, t] += 0.5 if q[t] <= 0 else -0.5
    for t, p in enumerate(rpos):
        i = t % dim
        j = (i + 1 + t // dim) % dim
        data[p] = q
        data[p, i] += 0.5 if q[i] <= 0 else -0.5
        data[p, j] += c if q[j] <= 0 else -c
    assert error_scale(1, data, q) == scale  # the near rows' norms stay below the corpus's largest
    src = pos[k + ring:k + ring + 130]
    easy = (data[src] + 0.05 * rng.standard_normal((130, dim))).astype(np.float32)
    return dict(data=data, hard=q, near=near, ring=rpos, gap=c * c, g=g, easy=easy)


def block_fixture(rows: str, block: int, n: int, dim: int, seed: int, hard: int = 24, easy: int = 130):
    """Rungs 2 and 3: `block` stored-identical rows at scattered positions are the nearest to every hard query (the row + 5 % noise),
    the other rows (normal draws) at least ten times as far.  A certificate needs a candidate list that reaches past the block: m = 63
    never does, m = 1023 does for 500 rows and does not for 1 500.  The block's row is 1.5 times as long as the others, so the plateau of
    equal scores is nowhere near the top of any other query.  The easy queries are an ordinary row + 5 % noise each, kept only if the
    modelled one-pass certificate for k = 10 holds with twice its bound: they certify at the first attempt whatever the handle did before.
    Returns a dict: data, stored, block (ascending positions), hard [hard, dim], easy [easy, dim]."""
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((n, dim)).astype(np.float32)
    pos = rng.permutation(n)
    bp = np.sort(pos[:block])
    data[bp] = 1.5 * data[bp[0]]
    if rows == "bf16":
        data = round_bf16(data)
    stored = stored_rows(rows, data)
    hq = (stored[bp[0]][None, :] + 0.05 * rng.standard_normal((hard, dim))).astype(np.float32)
    kind = {"bf16": ERR_BF16_ONE_PASS, "fp8": ERR_FP8_ONE_PASS, "f32": ERR_F32_REG_ONE_PASS}[rows]
    cand = (stored[pos[block:block + 2 * easy]] + 0.05 * rng.standard_normal((2 * easy, dim))).astype(np.float32)
    ex, ap, _ = l2_model_scores(stored, cand, rows)
    e = 2.0 * scan_error_bound(kind, True, dim) * l2_error_scales(stored, cand)
    keep = [i for i in range(cand.shape[0]) if certificate_holds(ap[i], ex[i], 10, 63, e[i])][:easy]
    assert len(keep) == easy
    return dict(data=data, stored=stored, block=bp, hard=hq, easy=cand[keep])


def l2_model_scores(stored: np.ndarray, qs: np.ndarray, rows: str):
    """exact_scores and one_pass_scores (one pass, full split) of squared Euclidean for MANY queries at once, [queries, rows] each in
    f64: the same model with matrix products for the dot products and |x|^2 + |q|^2 - 2 x.q for the exact score (an f64 rounding of
    ~1e-13 of the norms, far below every bound it is compared with).  Returns (exact, one pass, full split)."""
    x = _f32(stored).astype(np.float64)
    qf = _f32(qs)
    qd = qf.astype(np.float64)
    qh = round_bf16(qf).astype(np.float64)
    ql = round_bf16(_f32(qf - round_bf16(qf))).astype(np.float64)
    if rows == "f32":
        xh = round_bf16(_f32(stored)).astype(np.float64)
        xl = round_bf16(_f32(_f32(stored) - round_bf16(_f32(stored)))).astype(np.float64)
        dot1 = qh @ xh.T
        dot2 = dot1 + ql @ xh.T + qh @ xl.T
    else:
        dot1 = qh @ x.T
        dot2 = (qh + ql) @ x.T
    qn2 = (qd ** 2).sum(axis=1)
    xn2 = (x ** 2).sum(axis=1)
    qn2f = qn2.astype(np.float32).astype(np.float64)[:, None]
    xn2f = xn2.astype(np.float32).astype(np.float64)[None, :]
    exact = np.maximum(qn2[:, None] + xn2[None, :] - 2.0 * (qd @ x.T), 0.0)
    return exact, np.maximum(qn2f + xn2f - 2.0 * dot1, 0.0), np.maximum(qn2f + xn2f - 2.0 * dot2, 0.0)


def l2_error_scales(stored: np.ndarray, qs: np.ndarray) -> np.ndarray:
    """error_scale of squared Euclidean for every query: (|q|^2 + max |x|^2) / 2"""
    return 0.5 * ((_f32(qs).astype(np.float64) ** 2).sum(axis=1) + float((_f32(stored).astype(np.float64) ** 2).sum(axis=1).max()))


OVERFLOW_FIRST_CHUNK, OVERFLOW_PAIR_CAP = 1024, 1024


def overflow_fixture(dim: int = 128, near: int = 4000, b: int = 130, seed: int = 17):
    """The filtered epilogue's pair buffer: rows 0 .. 1 023 (the first chunk under OPT_FLAT_FIRST_CHUNK = 1024) lie beyond ten times the
    squared distance of the `near` rows behind them, so the thresholds they give let the whole first filtered slice (3 072 rows) through:
    more than the 1 024 pairs a query's buffer holds.  bf16 values.  Returns (rows, queries)."""
    rng = np.random.default_rng(seed)
    data = rng.standard_normal((OVERFLOW_FIRST_CHUNK + near, dim)).astype(np.float32)
    data[:OVERFLOW_FIRST_CHUNK] += (8.0 * (rng.integers(0, 2, (OVERFLOW_FIRST_CHUNK, dim)) * 2 - 1)).astype(np.float32)
    q = rng.standard_normal((b, dim)).astype(np.float32)
    return round_bf16(data), q


_LADDER_BLOCKS = {}


def ladder_block(rung: int, rows: str):
    """block_fixture of rung 2 (500 identical rows of 3 000, dim 128) or rung 3 (1 500 of 4 000; f32 rows: of 17 500 at dim 256, the
    smallest f32 image a small batch scans on the matrix cores), once per process: nobody changes the arrays"""
    if (rung, rows) not in _LADDER_BLOCKS:
        block, n = (500, 3000) if rung == 2 else (1500, 4000)
        n, dim = (17500, 256) if rows == "f32" else (n, 128)
        _LADDER_BLOCKS[(rung, rows)] = block_fixture(rows, block, n, dim, seed=100 * rung + ["bf16", "fp8", "f32"].index(rows))
    return _LADDER_BLOCKS[(rung, rows)]
