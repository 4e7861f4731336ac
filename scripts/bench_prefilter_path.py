#!/usr/bin/env python3
"""A two-hop chain + restricted kNN in one call (hvx_prefilter_path_search_batch_params) against the two-call composition it replaces
(hvx_expand_filter, a host bitmap -> ids conversion, hvx_prefilter_search_batch in expand mode).

Topology: bench.py's config #3 graph -- 1M nodes, edge i -> i + N/2 (label 0) -- plus a second family of the same kind, i -> i + N/3
(label 1), so `src -[0]-> x -[1]-> doc` from a where_() equality group of 10 000 / 100 000 sources reaches that many distinct docs.
Image: --rows x --dim f32, ONE query, k 10.  The legs of a size alternate inside one timed loop (warm-up first, medians reported).

  --mode both     path call and composition, alternating (needs the path entry points)
  --mode compose  the composition only: every entry point it uses exists before the path call did (--tree = that checkout)
  --mode path     the path call only: the run to put under `rocprofv3 --kernel-trace --stats` (kernel totals / iters = kernel time per call)
Prints one JSON line per size."""
import argparse, json, os, sys, time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=1536)
    ap.add_argument("--sizes", default="10000,100000")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--mode", choices=("both", "compose", "path"), default="both")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="the checkout whose helix-db_amd (binding + built library) is measured")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(args.tree, "helix-db_amd"))
    import torch
    import pyhvx as hv
    from pyhvx import synth
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: this script measures, it does not fall back")
    n, dim, k = args.rows, args.dim, 10
    dev = torch.device("cuda", 0)
    x, _ = synth.embedding_like(n, dim, 1, 20260923, dev, latent=24, clusters=1024)
    ix = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=hv.EUCLIDEAN, node_ids=np.arange(n, dtype=np.uint64), vectors=x,
                                             l0_offsets=np.zeros(n + 1, np.uint64), l0_neighbors=np.zeros(0, np.uint64), max_batch=32)
    idx = np.arange(n, dtype=np.uint64)
    t0, t1 = (idx + np.uint64(n // 2)) % np.uint64(n), (idx + np.uint64(n // 3)) % np.uint64(n)
    swap = t1 < t0                                      # rows ascend by target (model.rs:656-666); the labels follow their arcs
    tgt = np.stack([np.where(swap, t1, t0), np.where(swap, t0, t1)], 1).reshape(-1)
    lab = np.stack([np.where(swap, 1, 0), np.where(swap, 0, 1)], 1).reshape(-1).astype(np.uint32)
    g = hv.Graph(n, 2 * np.arange(n + 1, dtype=np.uint64), tgt, lab)
    q = x[[int(n * 0.8)]].cpu().numpy().copy()
    p = hv.SearchParams(k)
    hops = [(hv.DIR_OUT, (0,)), (hv.DIR_OUT, (1,))]
    starts = {10000: 1100, 100000: 11100}

    def compose(src):
        words = g.expand(src, hv.DIR_OUT, (0,))
        mid = np.nonzero(np.unpackbits(words.view(np.uint8), bitorder="little"))[0].astype(np.uint64)
        return ix.prefilter_search_batch(g, q, p, mid, direction=hv.DIR_OUT, allowed_labels=(1,))

    def path(src, option=0):
        ix.set_option(hv.OPT_RESTRICTED_DIRECT, option)
        try:
            out = ix.prefilter_path_search_batch(g, q, p, src, hops, want_sizes=True)
            return out, ix.last_scan_path()
        finally:
            ix.set_option(hv.OPT_RESTRICTED_DIRECT, 0)

    for size in [int(s) for s in args.sizes.split(",")]:
        src = np.arange(starts.get(size, 0), starts.get(size, 0) + size, dtype=np.uint64)
        legs = {}
        if args.mode != "path":
            legs["compose"] = lambda: compose(src)
        if args.mode != "compose":
            legs["path"] = lambda: path(src)
            legs["path_forced_lean"] = lambda: path(src, 2)
        times = {name: [] for name in legs}
        last = {}
        for r in range(args.warmup + args.iters):
            for name, fn in legs.items():
                t = time.perf_counter()
                last[name] = fn()                       # (every leg ends in the call's own host wait: the results are on the host)
                if r >= args.warmup:
                    times[name].append(time.perf_counter() - t)
        rec = {"sources": size, "iters": args.iters, "mode": args.mode}
        for name, t in times.items():
            rec[name + "_ms_median"] = round(float(np.median(t)) * 1e3, 4)
            rec[name + "_ms_min"] = round(float(np.min(t)) * 1e3, 4)
        if "path" in last:
            (fid, fsc, fcnt, ncand, fst, sizes), route = last["path"]
            rec.update(candidates=ncand, hop_sizes=sizes, path_route="lean" if route == hv.PATH_DIRECT else "bitmap",
                       path_scan_kernels_ms=round(fst["device_ms"], 4))
            (lid, lsc, lcnt, lcand, _, _), lroute = last["path_forced_lean"]
            assert lroute == hv.PATH_DIRECT and lcand == ncand and lid.tolist() == fid.tolist()
            assert lsc.view(np.uint32).tolist() == fsc.view(np.uint32).tolist()
            if "compose" in last:                       # the same answer, to the bit
                cid, csc, ccnt, ccand, _ = last["compose"]
                assert ccand == ncand and ccnt.tolist() == fcnt.tolist() and cid.tolist() == fid.tolist()
                assert csc.view(np.uint32).tolist() == fsc.view(np.uint32).tolist()
        else:
            rec.update(candidates=last["compose"][3])
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
