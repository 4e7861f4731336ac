"""The one table of GPU cases of tests/test_gpu_hnsw_cover.py: plain data, no torch, no library.

tests/test_hnsw_cover_ledger.py resolves every case through tests/native/hnsw_cover_probe.cpp (the plan header alone) and holds the
instantiations they launch to the set the plan can pick; tests/hnsw_cover_table.txt records what each case runs.

A GROUP is one index shape: every case of a group runs on the same oracle graphs.
A CASE is one search launch: the handle settings it runs under and the corpus it searches."""
from collections import namedtuple

COSINE, L2, L1 = 0, 1, 2          # hvx_metric
F32, BF16 = 0, 1                  # hvx_dtype
TREE_AVX, TREE_AVX_FMA = 2, 3     # hvx_float_kernel: the summation tree of the distances

Group = namedtuple("Group", "name dim metric dtype tree m m0")
# arm: "strict" | "non-strict"; stats: non-strict only, with the per-query SearchStats of the filter / sampling stages;
# pair: HVX_OPT_HNSW_PAIR (1 never, 2 always, 3 always with one gatherer); log2cap: HVX_OPT_WAVE_LOG2CAP (0 = the plan's table size);
# prune_off: HVX_OPT_HNSW_SHADOW_PRUNE (0 = the bf16-shadow pre-pass where the build has one, 1 = off);
# corpus: "clustered" | "ties" (masses of exactly equal scores over the same graph: the first launch overflows its beam's slack and the
# re-run launch has queries to search)
Case = namedtuple("Case", "group arm stats ef k occupancy pair log2cap prune_off corpus")

_METRIC_NAME = {COSINE: "cos", L2: "l2", L1: "l1"}
UNROLLED_DIMS = (128, 256, 384, 512, 768, 1024, 1536)
# 64-id rows (M 32 / M0 64) under the wider rungs: one f32 and one bf16 group
_WIDE_ROWS = {("f32", L2, 384), ("bf16", COSINE, 256)}

UNROLLED_GROUPS = tuple(
    Group(f"{dt}-{_METRIC_NAME[me]}-{dim}", dim, me, BF16 if dt == "bf16" else F32, TREE_AVX_FMA,
          32 if (dt, me, dim) in _WIDE_ROWS else 16, 64 if (dt, me, dim) in _WIDE_ROWS else 32)
    for dt in ("f32", "bf16") for me in (L2, COSINE) for dim in UNROLLED_DIMS)
GENERIC_GROUPS = (
    Group("gen-l2-100", 100, L2, F32, TREE_AVX_FMA, 16, 32),
    Group("gen-cos-100", 100, COSINE, F32, TREE_AVX_FMA, 16, 32),
    Group("gen-l1-100", 100, L1, F32, TREE_AVX_FMA, 16, 32),
    Group("gen-avx-l2-768", 768, L2, F32, TREE_AVX, 16, 32),   # an unrolled dimension under the AVX tree: the GENERIC build
)
GROUPS = UNROLLED_GROUPS + GENERIC_GROUPS


def _k(ef):
    return 10 if ef < 400 else 50 if ef < 800 else 100


def _unrolled_cases(g):
    out = []
    shadow = g.dtype == F32 and g.metric == L2   # the strict L2 beam over f32 rows has the bf16-shadow pre-pass in its two-per-SIMD builds
    # strict wave: one ef per rung of the beam ladders (192 / 384 / 448 / 832 entries), at the rung's largest ef on one-per-SIMD handles
    for ef in (160, 352, 416, 800):
        out.append(Case(g.name, "strict", False, ef, _k(ef), 1, 1, 0, 0, "clustered"))
    for ef in (48, 200, 400, 640):
        for prune_off in (0, 1) if shadow else (0,):
            out.append(Case(g.name, "strict", False, ef, _k(ef), 2, 1, 0, prune_off, "clustered"))
    # strict pair: owner + three gatherers where built (else one), and one gatherer on request
    for ef in (160, 300):
        for pair in (2, 3):
            out.append(Case(g.name, "strict", False, ef, 10, 1, pair, 0, 0, "clustered"))
    # non-strict (SearchParams.new(k).with_ef(ef), the default SimHash config): both rungs, both occupancies, with and without stats
    for occ, efs in ((1, (160, 352)), (2, (64, 200))):
        for ef in efs:
            for stats in (True, False):
                out.append(Case(g.name, "non-strict", stats, ef, 10, occ, 1, 0, 0, "clustered"))
    # visited-table spill: a 256-slot table
    out.append(Case(g.name, "strict", False, 128, 10, 2, 1, 8, 0, "clustered"))
    out.append(Case(g.name, "non-strict", True, 128, 10, 1, 1, 8, 0, "clustered"))
    # re-run with a wider beam: 192 -> 384 entries (strict at both occupancies, non-strict), 384 -> 832 (strict)
    for occ in (1, 2):
        out.append(Case(g.name, "strict", False, 128, 10, occ, 1, 0, 0, "ties"))
    for stats in (True, False):
        out.append(Case(g.name, "non-strict", stats, 128, 10, 1, 1, 0, 0, "ties"))
    for occ in (1, 2):
        out.append(Case(g.name, "strict", False, 256, 10, occ, 1, 0, 0, "ties"))
    return out


def _generic_cases(g):
    out = []
    # non-strict, one ef per rung of the GENERIC ladder (192 / 448 / 832 entries)
    for ef in (160, 416, 800):
        for stats in (True, False):
            out.append(Case(g.name, "non-strict", stats, ef, _k(ef), 1, 1, 0, 0, "clustered"))
    # re-run with a wider beam: 192 -> 448 and 448 -> 832 entries
    for ef in (128, 416):
        for stats in (True, False):
            out.append(Case(g.name, "non-strict", stats, ef, 10, 1, 1, 0, 0, "ties"))
    return out


CASES = tuple(c for g in UNROLLED_GROUPS for c in _unrolled_cases(g)) + tuple(c for g in GENERIC_GROUPS for c in _generic_cases(g))


def group_named(name):
    return next(g for g in GROUPS if g.name == name)


def cases_of(group_name):
    return [c for c in CASES if c.group == group_name]


def case_name(c):
    arm = c.arm + ("+stats" if c.stats else "")
    return f"{c.group}/{c.corpus}/{arm}/ef{c.ef}/k{c.k}/occ{c.occupancy}/pair{c.pair}/log2cap{c.log2cap}/prune_off{c.prune_off}"


def probe_line(c):
    """the case as an input line of `hnsw_cover_probe resolve`"""
    g = group_named(c.group)
    arm = 0 if c.arm == "strict" else 2 if c.stats else 1
    return f"{case_name(c)} {g.dtype} {g.metric} {g.tree} {g.dim} {g.m0} {arm} {c.occupancy} {c.pair} {c.log2cap} {c.ef}"
