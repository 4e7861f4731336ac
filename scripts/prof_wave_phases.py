#!/usr/bin/env python3
"""Phase cycles of the strict wave kernel on the benchmark corpus: builds bench.py's headline graph (same corpus, seed, level seed and
build parameters), then searches ONE lone 1 024-query batch.  With the tuning library (make TUNING=1, loaded through HVX_LIB_PATH) and
HVX_WAVE_PROF=1 in the environment the library launches its phase-timing build and prints the `[hvx prof]` line to stderr: cycles per
query by phase, and the full-beam rows the bf16 shadow rejected / scored in f32.  The script itself prints the batch's counters, which
must not move between two libraries.
The device build is not bit-reproducible from process to process.  To compare two libraries on ONE graph give a graph file: the
first process builds the graph and saves its export there, every later one imports it.
usage: HVX_LIB_PATH=.../libhelix_vec_gfx950_tuning.so HVX_WAVE_PROF=1 python scripts/prof_wave_phases.py [rows] [dim] [repeats] [graph.npz]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "helix-db_amd"))

import numpy as np
import torch


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    dim = int(sys.argv[2]) if len(sys.argv) > 2 else 768
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    graph_file = sys.argv[4] if len(sys.argv) > 4 else ""
    b, k, ef, m, seed, steps = 1024, 10, 128, 16, 20260921, 25  # bench.py's defaults (steps + warmup query batches are drawn)
    import pyhvx as hv
    from pyhvx import synth
    hv.lib()
    dev = torch.device("cuda", 0)
    x, q_all = synth.corpus("embedding", rows, dim, b * steps, seed, dev)
    torch.cuda.synchronize()
    ids = np.arange(rows, dtype=np.uint64)
    lv = synth.draw_levels(rows, m, 7)
    keys = ("l0_offsets", "l0_neighbors", "level", "up_offsets", "up_neighbors")
    if graph_file and os.path.exists(graph_file):
        z = np.load(graph_file)
        ix = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids, vectors=x, **{kk: z[kk] for kk in keys},
                                                 entry_point=int(z["entry_point"]), max_layer=int(z["max_layer"]), m=m, m0=2 * m,
                                                 device=0, max_batch=b)
    else:
        ix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids, vectors=x, levels=lv, m=m, m0=2 * m,
                                                  ef_construction=200, max_batch=2048, batch_divisor=32, device=0, search_max_batch=b)
        ix.sync()
        if graph_file:
            g = ix.export_graph()
            np.savez(graph_file, entry_point=np.uint64(g["entry_point"]), max_layer=np.uint32(g["max_layer"]), **{kk: g[kk] for kk in keys})
    q = q_all[:b].cpu().numpy()
    p = hv.SearchParams(k).with_ef(ef)
    for _ in range(repeats):  # the first launch loads the code object and builds the shadow; the last line is the one to read
        out_ids, sc, cnt, st, per_query, tot = ix.search_batch_with_stats(q, p)
    print(json.dumps({"lib": os.path.basename(hv.LIB_PATH), "rows": rows, "dim": dim, "batch": b, "ef": ef,
                      "totals": {kk: int(tot[kk]) for kk in ("expansion_steps", "neighbors_examined", "vectors_loaded", "distance_computations")},
                      "ids_sum": int(out_ids.astype(np.uint64).sum() % (1 << 61)), "score_bits_sum": int(sc.view(np.uint32).astype(np.uint64).sum())}))


if __name__ == "__main__":
    main()
