#!/usr/bin/env python3
"""Device HNSW build (hvx_index_build) at benchmark scale: build time, then recall@10 / work per query at ef=128 against the
exact scan.  usage: bench_build.py [rows=1000000] [max_batch=2048] [divisor=32] [dataset=embedding] [link_mode=0] [m=16] [m0=32] [dtype=f32]
dtype = the route to the index: f32 (build over f32 rows), bf16 (build the image in bf16), f32-then-bf16 (build over f32 rows, export the
graph, import it again with dtype bf16: the route to a bf16 index before the bf16 build).  build_seconds is the whole route, wall clock."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "helix-db_amd"))
import numpy as np
import torch


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 1_000_000
    bmax = int(sys.argv[2]) if len(sys.argv) > 2 else 2048
    div = int(sys.argv[3]) if len(sys.argv) > 3 else 32
    dataset = sys.argv[4] if len(sys.argv) > 4 else "embedding"
    link_mode = int(sys.argv[5]) if len(sys.argv) > 5 else 0
    m = int(sys.argv[6]) if len(sys.argv) > 6 else 16
    m0 = int(sys.argv[7]) if len(sys.argv) > 7 else 2 * m
    route = sys.argv[8] if len(sys.argv) > 8 else "f32"
    if route not in ("f32", "bf16", "f32-then-bf16"):
        sys.exit(f"dtype is f32, bf16 or f32-then-bf16, not {route}")
    import pyhvx as hv
    from pyhvx import synth
    dev = torch.device("cuda", 0)
    dim, b, k, ef = 768, 1024, 10, 128
    x, q = synth.corpus(dataset, n, dim, b, 20260921, dev)
    lv = synth.draw_levels(n, m, 7)
    torch.cuda.synchronize()
    t0 = time.time()
    ids = np.arange(n, dtype=np.uint64)
    ix, st = hv.ValidatedVectorReadIndex.build(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids, vectors=x, levels=lv,
                                               m=m, m0=m0, ef_construction=200, max_batch=bmax, batch_divisor=div, search_max_batch=b, link_mode=link_mode,
                                               **({"dtype": hv.BF16} if route == "bf16" else {}))
    ix.sync()
    t_graph = time.time() - t0
    if route == "f32-then-bf16":
        gr = ix.export_graph()
        ix.close()
        ix = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids, vectors=x, l0_offsets=gr["l0_offsets"], l0_neighbors=gr["l0_neighbors"],
                                                 level=gr["level"], up_offsets=gr["up_offsets"], up_neighbors=gr["up_neighbors"], entry_point=gr["entry_point"],
                                                 max_layer=gr["max_layer"], m=m, m0=m0, max_batch=b, dtype=hv.BF16)
        ix.sync()
    t_build = time.time() - t0
    bufs = [torch.zeros(b, k, dtype=torch.int64, device=dev), torch.zeros(b, k, dtype=torch.float32, device=dev),
            torch.zeros(b, dtype=torch.int32, device=dev), torch.zeros(b, dtype=torch.int32, device=dev), torch.zeros(b, 4, dtype=torch.int32, device=dev)]
    s = ix.search_batch_device(q, k, ef, *bufs, want_stats=True)
    s = ix.search_batch_device(q, k, ef, *bufs, want_stats=True)
    f = [torch.zeros(b, k, dtype=torch.int64, device=dev), torch.zeros(b, k, dtype=torch.float32, device=dev),
         torch.zeros(b, dtype=torch.int32, device=dev), torch.zeros(b, dtype=torch.int32, device=dev)]
    ix.flat_search_batch_device(q, k, *f)
    torch.cuda.synchronize()
    g, t = bufs[0].cpu().numpy(), f[0].cpu().numpy()
    rec = sum(len(set(g[i].tolist()) & set(t[i].tolist())) for i in range(b)) / float(b * k)
    gr = ix.export_graph()
    deg = np.diff(gr["l0_offsets"].astype(np.int64))
    print(json.dumps({"rows": n, "dim": dim, "dataset": dataset, "max_batch": bmax, "divisor": div, "link_mode": link_mode, "m": m, "m0": m0, "dtype": route, "build_seconds": round(t_build, 2), "graph_seconds": round(t_graph, 2),
                      "inserts_per_s": round(n / t_build, 1), "batches": st["batches"], "recall_at_10": round(rec, 4),
                      "distance_computations_per_query": round(s["distance_computations"] / b, 1), "kernel_ms": round(s["device_ms"], 4),
                      "degree_mean": round(float(deg.mean()), 2), "degree_full_frac": round(float((deg == m0).mean()), 3), "max_layer": gr["max_layer"]}))


if __name__ == "__main__":
    main()
