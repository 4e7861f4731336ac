#!/usr/bin/env python3
"""hvx_csr_apply_edges against the only other way to change a device graph: hvx_csr_free + hvx_csr_import of the edited arrays.

A 1M-node labelled graph with 16 and with 64 arcs per node (node 7 a hub of 200 000 arcs); batches of 1 / 1 000 / 100 000 edits, half
additions and half removals, with sources uniform over the nodes and with every edit in the hub row.  Per cell, alternating:
  edit      Graph.apply_edges(batch), end to end on the host clock; every second repeat applies the inverse batch (what was added is
            removed, what was removed is added), so the graph keeps its size and every repeat is a batch of the same shape;
  re-import Graph.close() + Graph(...) of the edited arrays (taken from export() once, outside the timing).
Medians of the repeats.  `copy GB/s`: the bytes the two copy kernels move for this graph (targets and labels of both adjacencies and
the stored-edge map, read and written: 40 bytes per arc) over the WHOLE call's time for the one-edit batch -- a lower bound of their
rate: the call also plans, uploads, runs the offset, row and fix-up kernels and waits -- next to hvx_device_stream_read_gbs of the same
run.  (Every second repeat edits a freshly imported handle, which allocates its spare set first: the median is the steady state.)

usage: bench_graph_edit.py [--out profiles/graph_edit.log] [--repeats 5]      (the driver: one child process per degree, each under
       its own time limit)
       bench_graph_edit.py --degree 16                                        (one child)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "helix-db_amd"),):
    if p not in sys.path:
        sys.path.insert(0, p)

N = 1_000_000
HUB, HUB_ARCS = 7, 200_000
BATCHES = (1, 1000, 100_000)


def make_graph(np, degree, seed):
    rng = np.random.default_rng(seed)
    lens = np.full(N, degree, np.int64)
    lens[HUB] = HUB_ARCS
    off = np.zeros(N + 1, np.int64)
    off[1:] = np.cumsum(lens)
    owner = np.repeat(np.arange(N, dtype=np.int64), lens)
    tgt = rng.integers(0, N, int(off[-1]))
    tgt = np.sort(owner * N + tgt) % N  # every row ascends by target
    lab = rng.integers(0, 3, tgt.size).astype(np.uint32)
    return off.astype(np.uint64), tgt.astype(np.uint64), lab, owner


def make_batch(np, rng, off, tgt, lab, owner, size, hub):
    n_add = (size + 1) // 2
    n_del = size - n_add
    o = off.astype(np.int64)
    if hub:
        pos = o[HUB] + rng.choice(HUB_ARCS, n_del, replace=False)
        a_src = np.full(n_add, HUB, np.uint64)
    else:
        pos = rng.choice(tgt.size, n_del, replace=False)
        a_src = rng.integers(0, N, n_add).astype(np.uint64)
    remove = (owner[pos].astype(np.uint64), tgt[pos], lab[pos])
    add = (a_src, rng.integers(0, N, n_add).astype(np.uint64), rng.integers(0, 3, n_add).astype(np.uint32))
    return remove, add


def child(degree, repeats):
    import numpy as np
    import pyhvx as hv
    hv.lib()
    off, tgt, lab, owner = make_graph(np, degree, degree)
    rng = np.random.default_rng(1000 + degree)
    best_gbs, mean_gbs = hv.device_stream_read_gbs(0)
    g = hv.Graph(N, off, tgt, lab)
    g.apply_edges(add=(np.array([1], np.uint64), np.array([2], np.uint64), np.array([0], np.uint32)))  # the spare set exists from here on
    g.apply_edges(remove=(np.array([1], np.uint64), np.array([2], np.uint64), np.array([0], np.uint32)))
    rows = []
    for hub in (False, True):
        for size in BATCHES:
            remove, add = make_batch(np, rng, off, tgt, lab, owner, size, hub)
            g.apply_edges(remove=remove, add=add)  # warm: the plan buffers grow here
            g.apply_edges(remove=add, add=remove)
            edited = None
            t_edit, t_import = [], []
            for r in range(repeats):
                fwd = r % 2 == 0
                t0 = time.perf_counter()
                g.apply_edges(remove=remove if fwd else add, add=add if fwd else remove)
                t_edit.append(time.perf_counter() - t0)
                if edited is None:  # the comparator's input, once: the arrays of the edited graph
                    a = g.export()
                    edited = (a["out_offsets"], a["out_targets"], a["out_labels"])
                    del a
                t0 = time.perf_counter()
                g.close()
                g = hv.Graph(N, *edited)
                t_import.append(time.perf_counter() - t0)
                if not fwd:  # the fresh import holds the EDITED graph; the next repeat applies the batch itself again: undo it first
                    g.apply_edges(remove=add, add=remove)
            if repeats % 2 == 1:
                g.apply_edges(remove=add, add=remove)
            e = int(tgt.size)
            edit_ms, import_ms = statistics.median(t_edit) * 1e3, statistics.median(t_import) * 1e3
            copy_bytes = e * 4 * (2 * 2 + 1) * 2  # ((targets + labels) x (outgoing + incoming) + stored-edge map) x (read + write)
            rows.append(dict(degree=degree, arcs=e, where="hub row" if hub else "uniform", edits=size, edit_ms=round(edit_ms, 3),
                             reimport_ms=round(import_ms, 1), speedup=round(import_ms / edit_ms, 1),
                             copy_gbs_lower_bound=round(copy_bytes / (edit_ms * 1e-3) / 1e9, 1) if size == 1 else None,
                             stream_read_gbs=round(best_gbs, 1), edit_ms_all=[round(t * 1e3, 3) for t in t_edit]))
            print(json.dumps(rows[-1]), flush=True)
    g.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--degree", type=int, default=0)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_edit.log"))
    ap.add_argument("--limit", type=int, default=420, help="seconds one child may take")
    args = ap.parse_args()
    if args.degree:
        child(args.degree, args.repeats)
        return 0
    lines = []
    for degree in (16, 64):
        run = subprocess.run(["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--degree", str(degree), "--repeats",
                              str(args.repeats)], capture_output=True, text=True)
        sys.stderr.write(run.stderr[-2000:])
        if run.returncode != 0:  # nothing more is started on the device after a child that failed or ran out of time
            print(f"degree {degree}: child ended with status {run.returncode}", file=sys.stderr)
            return run.returncode
        lines += [l for l in run.stdout.splitlines() if l.startswith("{")]
    head = "| arcs/node | arcs | edits | where | apply_edges ms | free + import ms | ratio | copy GB/s (lower bound) | stream read GB/s |"
    table = [head, "|" + "---|" * 9]
    for l in lines:
        r = json.loads(l)
        table.append(f"| {r['degree']} | {r['arcs']} | {r['edits']} | {r['where']} | {r['edit_ms']} | {r['reimport_ms']} | {r['speedup']}x | "
                     f"{r['copy_gbs_lower_bound'] if r['copy_gbs_lower_bound'] is not None else ''} | {r['stream_read_gbs']} |")
    text = "\n".join(table) + "\n\n" + "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
