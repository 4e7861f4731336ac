#!/usr/bin/env python3
"""A batch of requests that share a two-hop plan and bring their OWN start node, three ways:
  (a) lists   ONE hvx_prefilter_path_search_lists_params call: one chain kernel for the batch + the one-launch scan over per-query slots;
  (b) loop    b hvx_prefilter_path_search_batch_params calls, one request each (the only device route before the batched call);
  (c) host    the traversal on the CPU (numpy over the host CSR) + hvx_search_restricted_batch_params with per-query host id lists.
Corpus: --rows x --dim f32 (50 000 x 1536: what profiles/restricted_wide_ab.log used), k 10.  Graphs: every node has `fanout` random
out-arcs, so two hops from one node reach ~fanout^2 nodes: fanout 10 / 32 / 100 -> ~100 / 1 000 / 9 000 candidates per request.
The legs of a shape alternate inside one timed loop (warm-up first, medians of end-to-end host time: every leg ends in its own host wait).
Known costs of (a), reported per shape: the scan's grid is sized for max_frontier because the host never learns a list's length
(`scan_empty_workgroup_share` = 1 - workgroups whose slice holds ids / workgroups launched), and one workgroup per request leaves
compute units idle at small b.  Prints one JSON line per shape; --log also appends them to a file.

Routing advice as measured (profiles/prefilter_own_seeds.log): (a) won at every shape above, from b = 32 on -- 8.6 - 140 x over
(b), 2.6 - 10 x over (c).  Not measured: b < 32, slots far larger than the sets they hold (the scan's empty-workgroup share grows with
max_frontier / candidates), labelled or hub-heavy graphs."""
import argparse, json, os, sys, time

import numpy as np


def fan_graph(n, fanout, seed):
    rng = np.random.default_rng(seed)
    tgt = np.sort(rng.integers(0, n, (n, fanout)), axis=1).reshape(-1).astype(np.uint64)   # rows ascend by target (model.rs:656-666)
    return np.arange(n + 1, dtype=np.uint64) * np.uint64(fanout), tgt


def host_two_hops(off, tgt, fanout, seed):
    one = tgt[seed * fanout:(seed + 1) * fanout].astype(np.int64)
    two = tgt.reshape(-1, fanout)[np.unique(one)].reshape(-1)
    return np.unique(two)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=50_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--batches", default="32,256,1024")
    ap.add_argument("--fanouts", default="10,32,100")
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
    hops = [hv.DIR_OUT, hv.DIR_OUT]
    out = open(args.log, "a") if args.log else None
    for fanout in [int(f) for f in args.fanouts.split(",")]:
        off, tgt = fan_graph(n, fanout, fanout)
        g = hv.Graph(n, off, tgt)
        mf = 1 << int(np.ceil(np.log2(fanout * fanout)))          # the slot: the chain's bound, rounded up to a power of two
        for b in [int(s) for s in args.batches.split(",")]:
            q = qall[:b]
            starts = rng.integers(0, n, b)
            seeds = [[int(s)] for s in starts]
            nb = min(b, args.loop_cap)

            def lists():
                return ix.prefilter_path_search_lists(g, q, p, seeds, hops, max_frontier=mf)

            def loop():
                return [ix.prefilter_path_search_batch(g, q[i:i + 1], p, seeds[i], hops) for i in range(nb)]

            def host():
                sets = [host_two_hops(off, tgt, fanout, int(s)) for s in starts]
                offs = np.zeros(b + 1, np.uint64)
                offs[1:] = np.cumsum([s.size for s in sets])
                return ix.search_restricted_batch_params(q, rp, np.concatenate(sets).astype(np.uint64), offs)

            legs = {"lists": lists, "loop": loop, "host": host}
            times = {name: [] for name in legs}
            last = {}
            for r in range(args.warmup + args.iters):
                for name, fn in legs.items():
                    t = time.perf_counter()
                    last[name] = fn()
                    if r >= args.warmup:
                        times[name].append(time.perf_counter() - t)
            ids, sc, cnt, st, ncand, stats = last["lists"]
            assert st.tolist() == [hv.OK] * b
            hid, hsc, hcnt, hst, _ = last["host"]                  # the same answers, to the bit
            assert hcnt.tolist() == cnt.tolist() and hid.tolist() == ids.tolist() and hsc.view(np.uint32).tolist() == sc.view(np.uint32).tolist()
            for i, one in enumerate(last["loop"]):
                assert one[0][0, :one[2][0]].tolist() == ids[i, :cnt[i]].tolist() and one[3] == ncand[i]
            # the scan's grid: slices x b workgroups sized for mf ids per query; a workgroup whose slice starts past its list is empty
            passes = max(1, (mf + 63) // 64)
            want = max(1, min(1024, (1024 + b - 1) // b))
            chunk = ((passes + want - 1) // want) * 64
            slices = max(1, (mf + chunk - 1) // chunk)
            busy = sum(min(slices, (int(c) + chunk - 1) // chunk) for c in ncand)
            rec = {"b": b, "fanout": fanout, "max_frontier": mf, "candidates_median": int(np.median(ncand)), "iters": args.iters,
                   "lists_ms": round(float(np.median(times["lists"])) * 1e3, 3),
                   "loop_ms": round(float(np.median(times["loop"])) * 1e3 * b / nb, 3), "loop_requests_timed": nb,
                   "host_ms": round(float(np.median(times["host"])) * 1e3, 3),
                   "lists_scan_kernel_ms": round(stats["device_ms"], 3),
                   "scan_empty_workgroup_share": round(1.0 - busy / (slices * b), 3), "chain_workgroups": b}
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        g.close()


if __name__ == "__main__":
    main()
