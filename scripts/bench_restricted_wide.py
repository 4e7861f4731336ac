#!/usr/bin/env python3
"""Restricted exact scans at result counts above 64 on config #3's shape (rows x 1536 f32, Euclidean, clustered stand-in): the calls the
wide builds of the one-launch scan (csrc/hvx_restricted_wide4.hip / _wide13.hip) are measured with, next to a library that lacks them
(HVX_LIB_PATH selects the library; run the two alternately, one process each, and compare the medians against the older library's
run-to-run spread).
  a:  256 queries x their own 1 000-id lists, k 100 (hvx_search_restricted_batch_params with offsets)
  c:  the same call at k 10 -- the narrow build on both sides
  b:  one query x 10 000 ids, k 100 and k 800
Prints one JSON line: per call the median / minimum end-to-end milliseconds (host clock around a call that ends synchronised) and the
scan path the library reported.
With the label `sweep` it prints instead the records the routing rule (restricted_direct_pays, csrc/hvx_restricted_exact.hip) is drawn
from, one JSON line each: the one-launch scan forced (HVX_OPT_RESTRICTED_DIRECT = 2, `direct_ms`) against the older pipeline (= 1,
`older_ms`) in this one process, for `lists` per call x `ids` per list at k, and for one `shared` set of `ids` for b queries.
usage: bench_restricted_wide.py [label | sweep] [rows=50000] [dim=1536]"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "helix-db_amd"))
import numpy as np
import pyhvx as hv

label = sys.argv[1] if len(sys.argv) > 1 else "run"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 50_000
dim = int(sys.argv[3]) if len(sys.argv) > 3 else 1536
rng = np.random.default_rng(20261018)
centres = rng.standard_normal((256, dim), dtype=np.float32)
x = centres[rng.integers(0, 256, n)] + np.float32(0.15) * rng.standard_normal((n, dim), dtype=np.float32)
ids_all = np.arange(n, dtype=np.uint64)
ix = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids_all, vectors=x, l0_offsets=np.zeros(n + 1, np.uint64),
                                         l0_neighbors=np.zeros(0, np.uint64), entry_point=0, device=0, max_batch=256)
q = x[rng.integers(0, n, 256)] + np.float32(0.05) * rng.standard_normal((256, dim), dtype=np.float32)


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(t)), 4), "min_ms": round(float(np.min(t)), 4), "path": ix.last_scan_path()}


def lists_call(b, m, k):
    lists = [rng.choice(ids_all, m, replace=False) for _ in range(b)]
    off = np.arange(b + 1, dtype=np.uint64) * np.uint64(m)
    flat = np.concatenate(lists).astype(np.uint64)
    rp = hv.RestrictedParams.auto(k, max(k, 100))
    return lambda: ix.search_restricted_batch_params(q[:b], rp, flat, offsets=off)


def single_call(m, k):
    allowed = rng.choice(ids_all, m, replace=False).astype(np.uint64)
    rp = hv.RestrictedParams.auto(k, max(k, 100))
    return lambda: ix.search_restricted_batch_params(q[:1], rp, allowed)


def sweep():
    def exact(k):
        return hv.RestrictedParams.new(k, max(k, 100), strategy=hv.RESTRICTED_EXACT)

    def lists(b, m, k):
        off = np.arange(b + 1, dtype=np.uint64) * np.uint64(m)
        flat = np.concatenate([rng.choice(ids_all, m, replace=False) for _ in range(b)]).astype(np.uint64)
        rp = exact(k)
        return lambda: ix.search_restricted_batch_params(q[:b], rp, flat, offsets=off)

    def shared(b, m, k):
        allowed = rng.choice(ids_all, m, replace=False).astype(np.uint64)
        rp = exact(k)
        return lambda: ix.search_restricted_batch_params(q[:b], rp, allowed)

    cases = [("lists", b, m, 800) for m in (1000, 10000) for b in (1, 2, 4, 8, 16, 64)]
    cases += [("lists", 1, m, k) for k in (128, 256, 300, 400, 512) for m in (1000, 10000)]
    cases += [("shared", b, 10000, k) for k in (100, 256, 800) for b in (4, 32)]
    for kind, b, m, k in cases:
        fn = lists(b, m, k) if kind == "lists" else shared(b, m, k)
        row = {"kind": kind, "b": b, "ids": m, "k": k}
        for name, opt in (("direct", 2), ("older", 1)):
            ix.set_option(hv.OPT_RESTRICTED_DIRECT, opt)
            r = timed(fn, 3, 30 if b * (1 if name == "direct" else 8) <= 64 else 8)
            row[name + "_ms"], row[name + "_path"] = r["median_ms"], r["path"]
        print(json.dumps(row), flush=True)


if label == "sweep":
    sweep()
    ix.close()
    sys.exit(0)
rec = {"label": label, "rows": n, "dim": dim}
rec["a_256x1000_k100"] = timed(lists_call(256, 1000, 100), 3, 15)
rec["c_256x1000_k10"] = timed(lists_call(256, 1000, 10), 20, 300)
rec["b_1x10000_k100"] = timed(single_call(10000, 100), 10, 100)
rec["b_1x10000_k800"] = timed(single_call(10000, 800), 10, 100)
print(json.dumps(rec), flush=True)
ix.close()
