#!/usr/bin/env python3
"""A batch of requests g().n(user).repeat(out()).times(n).emit().vector_search(..) that share the loop and bring their OWN start node,
three ways:
  (a) lists   ONE hvx_prefilter_repeat_search_lists_params call: one repeat kernel for the batch + the one-launch scan over per-query slots;
  (b) loop    b hvx_prefilter_search_batch_params calls in HVX_PREFILTER_TRAVERSE mode (max_depth = times, include_seeds = 1), one request
              each: the only device route to the emitted set of emit ALL without the batched call;
  (c) host    the traversal on the CPU (numpy over the host CSR) + hvx_search_restricted_batch_params with per-query host id lists.
Corpus: --rows x --dim f32 (50 000 x 1536, the corpus of scripts/bench_prefilter_own_seeds.py), k 10, emit ALL.  Graphs: every node has
`fanout` random out-arcs, so `times` iterations from one node reach ~1 + fanout + .. + fanout^times nodes.  A cell whose reach set cannot
fit the largest slot (16 384 nodes) is not run and says so: such requests go through the traversal call one at a time.
The legs of a shape alternate inside one timed loop (warm-up first, medians of end-to-end host time: every leg ends in its own host wait).
Prints one JSON line per shape; --log also appends them to a file.  Measured: profiles/prefilter_repeat.log, DESIGN 4.4d."""
import argparse, json, os, sys, time

import numpy as np


def fan_graph(n, fanout, seed):
    rng = np.random.default_rng(seed)
    tgt = np.sort(rng.integers(0, n, (n, fanout)), axis=1).reshape(-1).astype(np.uint64)   # rows ascend by target (model.rs:656-666)
    return np.arange(n + 1, dtype=np.uint64) * np.uint64(fanout), tgt


def host_repeat_all(tgt, fanout, seed, times):
    """emit ALL from one seed: the seed and everything within `times` hops, breadth-first with exclusion"""
    rows = tgt.reshape(-1, fanout)
    seen = np.array([seed], np.int64)
    level = seen
    for _ in range(times):
        level = np.setdiff1d(np.unique(rows[level].reshape(-1)).astype(np.int64), seen, assume_unique=True)
        if level.size == 0:
            break
        seen = np.union1d(seen, level)
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--batches", default="32,256,1024")
    ap.add_argument("--fanouts", default="10,32,100")
    ap.add_argument("--times", default="2,3")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-cap", type=int, default=256, help="leg (b) runs at most this many of the batch's requests and is scaled to b")
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "helix-db_amd"))
    import torch
    import pyhvx as hv
    from pyhvx import synth
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    n, dim, k = args.rows, args.dim, 10
    dev = torch.device("cuda", 0)
    x, _ = synth.embedding_like(n, dim, 1, 20261019, dev, latent=24, clusters=256)
    bmax = max(int(b) for b in args.batches.split(","))
    ix = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=hv.EUCLIDEAN, node_ids=np.arange(n, dtype=np.uint64), vectors=x,
                                             l0_offsets=np.zeros(n + 1, np.uint64), l0_neighbors=np.zeros(0, np.uint64), max_batch=bmax)
    rng = np.random.default_rng(7)
    qall = x[rng.integers(0, n, bmax)].cpu().numpy().copy()
    p = hv.SearchParams(k)
    rp = hv.RestrictedParams(k=k, ef=k, strategy=hv.RESTRICTED_EXACT)
    out = open(args.log, "a") if args.log else None

    def emit_line(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for fanout in [int(f) for f in args.fanouts.split(",")]:
        off, tgt = fan_graph(n, fanout, fanout)
        g = hv.Graph(n, off, tgt)
        for times in [int(t) for t in args.times.split(",")]:
            bound = sum(fanout ** i for i in range(times + 1))       # the reach set's bound from one seed
            mf = 1 << int(np.ceil(np.log2(bound)))                   # the slot: the bound rounded up to a power of two
            for b in [int(s) for s in args.batches.split(",")]:
                if mf > 16384:
                    emit_line({"b": b, "fanout": fanout, "times": times, "not_run": f"a reach set of up to {min(bound, n)} nodes does not fit the largest slot"})
                    continue
                q = qall[:b]
                starts = rng.integers(0, n, b)
                seeds = [[int(s)] for s in starts]
                nb = min(b, args.loop_cap)

                def lists():
                    return ix.prefilter_repeat_search_lists(g, q, p, seeds, times, hv.REPEAT_EMIT_ALL, max_frontier=mf)

                def loop():
                    return [ix.prefilter_search_batch_params(g, q[i:i + 1], rp, seeds[i], traverse=True, max_depth=times, include_seeds=True)
                            for i in range(nb)]

                def host():
                    sets = [host_repeat_all(tgt, fanout, int(s), times) for s in starts]
                    offs = np.zeros(b + 1, np.uint64)
                    offs[1:] = np.cumsum([s.size for s in sets])
                    return ix.search_restricted_batch_params(q, rp, np.concatenate(sets).astype(np.uint64), offs)

                legs = {"lists": lists, "loop": loop, "host": host}
                timed = {name: [] for name in legs}
                last = {}
                for r in range(args.warmup + args.iters):
                    for name, fn in legs.items():
                        t = time.perf_counter()
                        last[name] = fn()
                        if r >= args.warmup:
                            timed[name].append(time.perf_counter() - t)
                ids, sc, cnt, st, ncand, stats = last["lists"]
                assert st.tolist() == [hv.OK] * b
                hid, hsc, hcnt, hst, _ = last["host"]                  # the same answers, to the bit
                assert hcnt.tolist() == cnt.tolist() and hid.tolist() == ids.tolist() and hsc.view(np.uint32).tolist() == sc.view(np.uint32).tolist()
                for i, one in enumerate(last["loop"]):
                    assert one[0][0, :one[2][0]].tolist() == ids[i, :cnt[i]].tolist() and one[3] == ncand[i]
                emit_line({"b": b, "fanout": fanout, "times": times, "max_frontier": mf, "candidates_median": int(np.median(ncand)), "iters": args.iters,
                           "lists_ms": round(float(np.median(timed["lists"])) * 1e3, 3),
                           "loop_ms": round(float(np.median(timed["loop"])) * 1e3 * b / nb, 3), "loop_requests_timed": nb,
                           "host_ms": round(float(np.median(timed["host"])) * 1e3, 3),
                           "lists_scan_kernel_ms": round(stats["device_ms"], 3), "repeat_workgroups": b})
        g.close()


if __name__ == "__main__":
    main()
