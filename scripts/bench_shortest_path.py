#!/usr/bin/env python3
"""A batch of shortest_path requests that share direction Out, every label and max_depth, three ways:
  (a) batch    ONE hvx_shortest_path_batch call: one workgroup per request, one host wait;
  (b) ordered  one hvx_traverse_ordered call per request (the whole breadth-first search to max_depth, no stop at the target) and the host
               chasing out_parents from the target back: one call and one host wait per request;
  (c) host     hvx_traverse_host (strategy 0) over the host's arrays and the same chase.
(b) and (c) exist without the batched call and are not code under test.  Legs (b) and (c) run --loop-cap / --host-cap of the batch's
requests and are scaled to b (their cost per request does not depend on b).
Graphs: every node has `fanout` random out-arcs (the 50 000-node graphs of scripts/bench_prefilter_repeat.py with 10 and 32), and a 1M-node
graph with 16 and one hub (4 096 arcs out of node 0, 4 096 into it).  Endpoint pairs: `random` (both uniform; on these expanders the backward
reach set of max_depth levels must stay inside 16 384 nodes, which is fewer levels than a random pair is apart: most such requests find
no path within max_depth) and `walk` (the target is where a random walk of max_depth arcs from the source ends: what a host asks about
nodes it knows to be near; nearly all of them find a path).  max_depth per graph is the largest whose backward reach set fits the slot.
All three legs must return the same path for every request that does not overflow; the share that overflowed is reported in every cell.
The legs alternate inside one timed loop (warm-up first, medians of end-to-end host time).  Prints one JSON line per cell; --log appends them
to a file.  Measured: profiles/shortest_path.log, DESIGN 4.4f."""
import argparse, ctypes as C, json, os, sys, time

import numpy as np


def fan_graph(n, fanout, seed, hub=0):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n, (n, fanout))
    if hub:
        rows[rng.choice(np.arange(1, n), hub, replace=False), 0] = 0          # arcs into the hub
    rows = np.sort(rows, axis=1)                                               # rows ascend by target (model.rs:656-666)
    off = np.arange(n + 1, dtype=np.int64) * fanout
    tgt = rows.reshape(-1)
    if hub:                                                                    # node 0's row becomes `hub` arcs long
        row0 = np.sort(rng.integers(0, n, hub))
        tgt = np.concatenate([row0, tgt[fanout:]])
        off[1:] += hub - fanout
    return off.astype(np.uint64), tgt.astype(np.uint64)


def walk_targets(off, tgt, sources, steps, rng):
    cur = sources.astype(np.int64)
    o = off.astype(np.int64)
    for _ in range(steps):
        deg = o[cur + 1] - o[cur]
        cur = tgt[o[cur] + rng.integers(0, 1 << 30, cur.size) % deg].astype(np.int64)
    return cur.astype(np.uint64)


class Chaser:
    """the comparators' side: one traversal's visits in preallocated arrays, the predecessor chain of `target` read out of them"""

    def __init__(self, n):
        self.nodes, self.parents = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self.par = np.zeros(n, np.int64)
        self.cnt = C.c_uint64(0)
        self.seed = np.zeros(1, np.uint64)

    def path(self, source, target):
        c = self.cnt.value
        nodes = self.nodes[:c].astype(np.int64)
        if not (nodes == target).any():
            return []
        self.par[nodes] = self.parents[:c].view(np.int64)
        out, cur = [int(target)], int(target)
        while cur != source:
            cur = int(self.par[cur])
            out.append(cur)
        return out[::-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="50000:10:4,50000:32:2,1000000:16:3", help="nodes:fanout:max_depth")
    ap.add_argument("--batches", default="32,256,1024")
    ap.add_argument("--pairs", default="random,walk")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop-cap", type=int, default=32)
    ap.add_argument("--host-cap", type=int, default=8)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "helix-db_amd"))
    import torch
    import pyhvx as hv
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    L = hv.lib()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    out = open(args.log, "a") if args.log else None

    def emit_line(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    for spec in args.graphs.split(","):
        n, fanout, max_depth = (int(x) for x in spec.split(":"))
        hub = 4096 if n >= 1_000_000 else 0
        off, tgt = fan_graph(n, fanout, fanout, hub)
        g = hv.Graph(n, off, tgt)
        ch = Chaser(n)
        big = n >= 1_000_000
        iters = args.iters
        rng = np.random.default_rng(7)
        for pairs in args.pairs.split(","):
            for b in [int(s) for s in args.batches.split(",")]:
                src = rng.integers(0, n, b).astype(np.uint64)
                dst = rng.integers(0, n, b).astype(np.uint64) if pairs == "random" else walk_targets(off, tgt, src, max_depth, rng)
                nl, nh = min(b, args.loop_cap), min(b, args.host_cap if not big else max(2, args.host_cap // 4))   # (the host leg rebuilds a 16M-arc incoming adjacency per request)

                def batch():
                    return g.shortest_paths(src, dst, max_depth, hv.DIR_OUT)

                def ordered():
                    res = []
                    for i in range(nl):
                        ch.seed[0] = src[i]
                        rc = L.hvx_traverse_ordered(g._h, p(ch.seed), 1, max_depth, hv.DIR_OUT, None, 0, 0, n, p(ch.nodes), None, p(ch.parents), None, None,
                                                    C.byref(ch.cnt))
                        assert rc == hv.OK
                        res.append(ch.path(int(src[i]), int(dst[i])))
                    return res

                def host():
                    res = []
                    for i in range(nh):
                        ch.seed[0] = src[i]
                        rc = L.hvx_traverse_host(n, tgt.size, p(off), p(tgt), None, 0, p(ch.seed), 1, max_depth, hv.DIR_OUT, None, 0, 0, n, p(ch.nodes), None,
                                                 p(ch.parents), None, None, C.byref(ch.cnt))
                        assert rc == hv.OK
                        res.append(ch.path(int(src[i]), int(dst[i])))
                    return res

                legs = {"batch": batch, "ordered": ordered, "host": host}
                timed = {name: [] for name in legs}
                last = {}
                for r in range(args.warmup + iters):
                    for name, fn in legs.items():
                        t = time.perf_counter()
                        last[name] = fn()
                        if r >= args.warmup:
                            timed[name].append(time.perf_counter() - t)
                paths, st, sizes = last["batch"]
                over = st == hv.ERR_CANDIDATE_LIMIT
                assert ((st == hv.OK) | over).all()
                for name, cap in (("ordered", nl), ("host", nh)):              # the same paths wherever the batched call answered
                    for i in range(cap):
                        assert over[i] or last[name][i] == paths[i].tolist(), (name, i)
                ok = ~over
                emit_line({"nodes": n, "fanout": fanout, "max_depth": max_depth, "pairs": pairs, "b": b, "iters": iters,
                           "overflow_share": round(float(over.mean()), 3), "found_share": round(float(np.mean([len(x) > 0 for x in paths])), 3),
                           "reach_median": int(np.median(sizes[ok].max(axis=1))) if ok.any() else None,
                           "batch_ms": round(float(np.median(timed["batch"])) * 1e3, 3),
                           "ordered_ms": round(float(np.median(timed["ordered"])) * 1e3 * b / nl, 3), "ordered_requests_timed": nl,
                           "host_ms": round(float(np.median(timed["host"])) * 1e3 * b / nh, 3), "host_requests_timed": nh})
        g.close()


if __name__ == "__main__":
    main()
