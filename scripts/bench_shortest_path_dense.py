#!/usr/bin/env python3
"""hvx_shortest_path_batch_dense (64 requests share one bit-parallel sweep, no reach limit) on scripts/bench_shortest_path.py's three graphs
and pair kinds, direction Out, every label:
  deep cells     max_depth one above the sibling's (5 / 3 / 4), where hvx_shortest_path_batch refuses most requests.  (a) dense: ONE
                 hvx_shortest_path_batch_dense call; (b) ordered: what the contract prescribed for refused requests before -- one
                 hvx_traverse_ordered call per request and the host chasing out_parents, timed on --loop-cap requests and scaled to b (its
                 cost per request does not depend on b; it exists without this call and is not code under test).  The paths of both legs
                 must be identical.  The sibling runs once, untimed, for its refused share.
  shallow cells  the sibling's max_depth (4 / 2 / 3), where it answers: both batch calls timed side by side, same paths wherever the sibling
                 answered.  This table tells a host which call to pick.
The legs alternate inside one timed loop (warm-up first, medians of end-to-end host time).  For the largest batch of every graph and pair
kind the sweep itself is replayed in numpy for the LARGEST round: nodes with a frontier word, arcs walked, fetch-ors issued per level, and
the bytes those touch when every word and level-line access is its own 64-byte line (an upper bound, no bandwidth fraction is claimed),
next to hvx_device_stream_read_gbs of the same run.  Prints one JSON line per cell; --log appends them to a file.
Measured: profiles/shortest_path_dense.log, DESIGN 4.4g."""
import argparse, ctypes as C, json, os, sys, time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_shortest_path import Chaser, fan_graph, walk_targets

GROUP, NODE_GROUP_BYTES = 64, 88


def sweep_stats(n, off, tgt, src, dst, max_depth, groups_per_round):
    """the push / commit sweep of the first (a largest) round replayed with numpy words: per level (frontier nodes, arcs walked,
    fetch-ors, bits committed, nodes reached), summed over the round's groups"""
    order = np.argsort(tgt, kind="stable")                      # the incoming adjacency: direction Out pushes over it
    in_tgt = np.repeat(np.arange(n, dtype=np.int64), np.diff(off.astype(np.int64)))[order]
    in_off = np.zeros(n + 1, np.int64)
    in_off[1:] = np.cumsum(np.bincount(tgt.astype(np.int64), minlength=n))
    levels = [[0, 0, 0, 0, 0] for _ in range(max_depth)]
    b = min(src.size, groups_per_round * GROUP)
    for g0 in range(0, b, GROUP):
        s, d = src[g0:g0 + GROUP].astype(np.int64), dst[g0:g0 + GROUP].astype(np.int64)
        seen, cur = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        active = np.uint64(0)
        for q in range(s.size):
            if s[q] != d[q]:
                seen[d[q]] |= np.uint64(1) << np.uint64(q)
                active |= np.uint64(1) << np.uint64(q)
        cur[:] = seen
        for level in range(max_depth):
            if not active:
                break
            front = np.flatnonzero(cur & active)
            lens = in_off[front + 1] - in_off[front]
            total = int(lens.sum())
            at = np.repeat(in_off[front] - (np.cumsum(lens) - lens), lens) + np.arange(total)
            v = in_tgt[at]
            add = np.repeat(cur[front] & active, lens) & ~seen[v]
            nxt = np.zeros(n, np.uint64)
            np.bitwise_or.at(nxt, v[add != 0], add[add != 0])
            w = nxt & ~seen & active
            seen |= w
            cur = w
            grew = np.bitwise_or.reduce(w) if w.size else np.uint64(0)
            bits = int(np.unpackbits(w[w != 0].view(np.uint8)).sum())
            for k, x in enumerate((front.size, total, int((add != 0).sum()), bits, int((w != 0).sum()))):
                levels[level][k] += x
            found = np.uint64(0)
            for q in range(s.size):
                if (cur[s[q]] >> np.uint64(q)) & np.uint64(1):
                    found |= np.uint64(1) << np.uint64(q)
            active &= ~(found | ~grew)
    return levels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", default="50000:10:5:4,50000:32:3:2,1000000:16:4:3", help="nodes:fanout:deep max_depth:shallow max_depth")
    ap.add_argument("--batches", default="64,256,1024")
    ap.add_argument("--pairs", default="random,walk")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--loop-cap", type=int, default=32)
    ap.add_argument("--no-sweep-stats", action="store_true")
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

    best_gbs, _ = hv.device_stream_read_gbs(0)
    slower = []   # deep cells in which the one call did not beat the loop: there must be none
    batches = [int(s) for s in args.batches.split(",")]

    def timed_legs(legs):
        timed, last = {name: [] for name in legs}, {}
        for r in range(args.warmup + args.iters):
            for name, fn in legs.items():
                t = time.perf_counter()
                last[name] = fn()
                if r >= args.warmup:
                    timed[name].append(time.perf_counter() - t)
        return {name: float(np.median(ts)) * 1e3 for name, ts in timed.items()}, last

    for spec in args.graphs.split(","):
        n, fanout, deep, shallow = (int(x) for x in spec.split(":"))
        off, tgt = fan_graph(n, fanout, fanout, 4096 if n >= 1_000_000 else 0)
        g = hv.Graph(n, off, tgt)
        ch = Chaser(n)
        rng = np.random.default_rng(7)
        for kind, max_depth in (("deep", deep), ("shallow", shallow)):
            for pairs in args.pairs.split(","):
                for b in batches:
                    src = rng.integers(0, n, b).astype(np.uint64)
                    dst = rng.integers(0, n, b).astype(np.uint64) if pairs == "random" else walk_targets(off, tgt, src, max_depth, rng)
                    nl = min(b, args.loop_cap)

                    def dense():
                        return g.shortest_paths_dense(src, dst, max_depth, hv.DIR_OUT)

                    def sibling():
                        return g.shortest_paths(src, dst, max_depth, hv.DIR_OUT)

                    def ordered():
                        res = []
                        for i in range(nl):
                            ch.seed[0] = src[i]
                            rc = L.hvx_traverse_ordered(g._h, p(ch.seed), 1, max_depth, hv.DIR_OUT, None, 0, 0, n, p(ch.nodes), None, p(ch.parents), None,
                                                        None, C.byref(ch.cnt))
                            assert rc == hv.OK
                            res.append(ch.path(int(src[i]), int(dst[i])))
                        return res

                    ms, last = timed_legs({"dense": dense, "ordered": ordered} if kind == "deep" else {"dense": dense, "sibling": sibling})
                    paths, st, sizes = last["dense"]
                    assert (st == hv.OK).all()
                    spaths, sst, _ = last["sibling"] if kind == "shallow" else sibling()
                    over = sst == hv.ERR_CANDIDATE_LIMIT
                    for i in range(b):                                          # identical paths on every leg
                        assert over[i] or spaths[i].tolist() == paths[i].tolist(), ("sibling", i)
                    rec = {"cell": kind, "nodes": n, "fanout": fanout, "max_depth": max_depth, "pairs": pairs, "b": b, "iters": args.iters,
                           "sibling_refused_share": round(float(over.mean()), 3), "found_share": round(float(np.mean([len(x) > 0 for x in paths])), 3),
                           "reach_median": int(np.median(sizes.max(axis=1))), "reach_max": int(sizes.max()), "dense_ms": round(ms["dense"], 3)}
                    if kind == "deep":
                        for i in range(nl):
                            assert last["ordered"][i] == paths[i].tolist(), ("ordered", i)
                        rec.update(ordered_ms=round(ms["ordered"] * b / nl, 3), ordered_requests_timed=nl,
                                   speedup=round(ms["ordered"] * b / nl / ms["dense"], 2), dense_faster=bool(ms["dense"] < ms["ordered"] * b / nl))
                    else:
                        rec.update(sibling_ms=round(ms["sibling"], 3), dense_over_sibling=round(ms["dense"] / ms["sibling"], 2))
                    if b == max(batches) and not args.no_sweep_stats:
                        per_round = max(1, min((1 << 30) // (n * NODE_GROUP_BYTES), (b + GROUP - 1) // GROUP))
                        levels = sweep_stats(n, off, tgt, src, dst, max_depth, per_round)
                        ran = [lv for lv in levels if lv[0]]
                        # push: a cur word per node and group, per arc its target (4 B) and a seen line, per fetch-or a next line;
                        # commit: a next word per node and group and a cur word written, per node reached its seen line twice and a level line
                        groups = min(per_round, (b + GROUP - 1) // GROUP)
                        line_bytes = sum(groups * n * 24 + arcs * (4 + 64) + ors * 64 + reached * 3 * 64 for _, arcs, ors, _, reached in ran)
                        rec.update(round_groups=groups, levels_run=len(ran), frontier_nodes=[lv[0] for lv in ran], arcs_per_sweep=[lv[1] for lv in ran],
                                   fetch_ors=[lv[2] for lv in ran], bits_committed=[lv[3] for lv in ran], nodes_reached=[lv[4] for lv in ran],
                                   line_bytes_upper_bound=int(line_bytes), stream_read_gbs=round(best_gbs, 1))
                    emit_line(rec)
                    if kind == "deep" and not rec["dense_faster"]:
                        slower.append((n, fanout, pairs, b))
        g.close()
    if slower:
        raise SystemExit(f"hvx_shortest_path_batch_dense was not faster than the per-request loop in {slower}")


if __name__ == "__main__":
    main()
