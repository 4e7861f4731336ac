#!/usr/bin/env python3
"""bench.py -- BASELINE.json metric on MI355X: QPS of the HNSW search hot path at recall@10 >= 0.95.

One "step" = one pass of the hot path over one batch of 1024 synthetic queries (config #2:
1M x 768 f32, HNSW M=16/M0=32, ef_search=128, k=10) with index AND queries already resident in HBM.
Contract (driver): `python bench.py --gpus N --steps K --warmup W` prints ONE JSON line on rank 0 -- the LAST line of stdout.  Such a
plain run does only what the headline needs: corpus, graph, lanes, W + K steps, `--dump-outputs`, and a line of the contract keys
(metric / value / unit / ms_per_step / higher_is_better / dtype ...) and the configuration.  `--full` adds every other leg below and
prints a compact record instead (< 4 KB, strict JSON: + roofline / cpu_baseline / parity + one-line summaries of the other legs);
everything else every leg measured goes to `bench_full.json` next to this file (path in the line's `full_record`).

Steps are issued round-robin on `--lanes` execution lanes (hvx_index_fork: same index image, own stream + scratch), so
that consecutive batches overlap on the device -- the way a serving host keeps the device fed: a batch that is still
finishing its slowest queries no longer leaves SIMDs idle.  Nothing synchronises inside the timed region; `ms_per_step` is
the host wall time of the K steps / K.  With `--full`, `roofline.achieved` = algorithmic bytes per launch / (HIP-event span of
the K search kernels / K), and the latency of ONE lone batch is reported next to it (`roofline.lone_batch`).

N > 1 (launched by torch.distributed.run, one rank per GPU): the corpus is sharded by vector-id range, every rank
searches the whole query batch on its shard, per-shard top-k are exchanged with ONE all-gather of a packed payload and
merged on the device by Candidate order.  The headline is weak scaling (`--rows` PER GPU, the corpus grows with N; ideal =
constant QPS); `--full` also measures strong scaling (`--rows` in total, 1/N per GPU; `strong_scaling`).

The CPU oracle (oracle/) is used here ONLY by `--full`, as (a) the `cpu_baseline` leg and (b) a bit-exact checker of the GPU
results; the timed product path is the HIP library through its C ABI.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.join(ROOT, "helix-db_amd"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

# HIP multiplexes a process's streams onto a few hardware queues; lanes that share one run back to back.  main() loads the library
# (hvx_runtime_prepare: at most 2 queues) before the runtime starts; a value the environment exports is kept.

import numpy as np
import torch

HBM_PEAK_GBS = 8000.0    # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.29 TB/s measured float4 copy)
MFMA_BF16_TFLOPS = 2500.0  # dense bf16 MFMA peak; the fp8 scan runs two e4m3 query pieces through the MX-scaled fp8 instruction: quoted against this peak too
SHARED_GPU = bool(os.environ.get("HVX_BENCH_SHARED_GPU"))  # plumbing check of the N > 1 path on a 1-GPU box (gloo, host staging)


def log(*a):
    if int(os.environ.get("RANK", "0")) == 0:
        print("[bench]", *a, file=sys.stderr, flush=True)



HEADLINE_KERNEL = "hnsw_wave_kernel<1u, 3, 24, false, false, false, true, 2, false>"


def measure_traffic_pass(args, timeout_s=150):
    """roofline.traffic of THIS run: a child `rocprofv3 --pmc FETCH_SIZE TCC_EA0_RDREQ_sum --kernel-trace` pass of a plain run (the headline leg
    only) of this command (its own pass, counters + kernel trace only -- MI355X_MICROARCH.md, HBM section), FETCH_SIZE KiB x 1024 x 2 (gfx950 reports
    half of a wide coalesced read), mean over the headline kernel's 3 warm-up + 6 timed launches; cross-check TCC_EA0_RDREQ_sum x 128 B.
    Returns None (and the caller keeps the labelled static figure) when rocprofv3 is absent, the pass fails or times out."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    if os.environ.get("HVX_BENCH_CHILD") or not shutil.which("rocprofv3"):
        return None
    out_dir = tempfile.mkdtemp(prefix="hvx_pmc_", dir="/tmp")
    cmd = ["rocprofv3", "--pmc", "FETCH_SIZE", "TCC_EA0_RDREQ_sum", "--kernel-trace", "--output-format", "csv", "-d", out_dir, "-o", "pmc", "--",
           sys.executable, os.path.abspath(__file__), "--steps", "6", "--warmup", "3",
           "--rows", str(args.rows), "--batch", str(args.batch), "--seed", str(args.seed), "--lanes", str(args.lanes), "--occupancy", str(args.occupancy),
           "--m", str(args.m), "--builder", args.builder, "--build-batch", str(args.build_batch)]
    env = dict(os.environ, HVX_BENCH_CHILD="1", TMPDIR="/tmp")
    t0 = time.time()
    try:
        subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=timeout_s, check=False)
        files = glob.glob(os.path.join(out_dir, "**", "*counter_collection.csv"), recursive=True)
        if not files:
            return None
        vals = {"FETCH_SIZE": [], "TCC_EA0_RDREQ_sum": []}
        for r in csv.DictReader(open(files[0])):
            if HEADLINE_KERNEL in r.get("Kernel_Name", "") and r.get("Counter_Name") in vals:
                vals[r["Counter_Name"]].append((int(r["Dispatch_Id"]), float(r["Counter_Value"])))
        fs = [v for _, v in sorted(vals["FETCH_SIZE"])][:9]
        rq = [v for _, v in sorted(vals["TCC_EA0_RDREQ_sum"])][:9]
        if len(fs) < 4:
            return None
        return {"hbm_bytes_per_launch": int(sum(fs) / len(fs) * 2048), "tcc_ea0_rdreq_x128B": int(sum(rq) / len(rq) * 128) if rq else None,
                "dispatches": len(fs), "min": int(min(fs) * 2048), "max": int(max(fs) * 2048), "seconds": round(time.time() - t0, 1)}
    except Exception as e:  # noqa: BLE001 -- the pass is optional; the bench line must not depend on it
        log(f"traffic pass failed: {e}")
        return None
    finally:
        shutil.rmtree(out_dir, ignore_errors=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000, help="rows per GPU shard (weak mode) / in total (strong mode)")
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--ef", type=int, default=128)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--lanes", type=int, default=4, help="execution lanes the steps are issued on round-robin (1 = every step waits for the previous one)")
    ap.add_argument("--occupancy", type=int, default=0, help="queries per SIMD of the HNSW kernel build: 0 = 2 when lanes > 1, else 1")
    ap.add_argument("--mode", default="shard", choices=["shard", "replica"],
                    help="N>1: 'shard' = id-range shards + all-gather top-k merge (north star); 'replica' = every GPU holds "
                         "the whole index and answers its own batch (no collective)")
    ap.add_argument("--exchange", default="capi", choices=["capi", "torch"],
                    help="N>1: 'capi' = hvx_shard_group_* (ncclAllGather inside the library), 'torch' = torch.distributed all-gather + device merge")
    ap.add_argument("--scaling", default="both", choices=["weak", "strong", "both"], help="N>1 shard mode: which corpus sizing to measure")
    ap.add_argument("--dtype", default="f32", choices=["f32", "bf16"], help="row storage on the device (bf16 = config #4)")
    ap.add_argument("--dataset", default="embedding", choices=["embedding", "clustered", "gaussian"])
    ap.add_argument("--seed", type=int, default=20260921)
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="budget of the cpu_baseline leg (0 = skip)")
    ap.add_argument("--deadline", type=float, default=330.0,
                    help="seconds after which the line is printed with whatever legs have finished (the headline is complete long before; 0 = no deadline)")
    ap.add_argument("--cpu-threads", type=int, default=0, help="0 = the cores this process may use (cgroup quota, else all; capped at 64)")
    ap.add_argument("--no-verify", action="store_true", help="skip the oracle bit-exactness check")
    ap.add_argument("--metric", default="l2", choices=["l2", "cosine"])
    ap.add_argument("--deletes", type=int, default=2000, help="nodes the insert leg deletes again (hvx_index_delete_batch), 0 = none")
    ap.add_argument("--skip", default="", help="comma list of extra legs to skip: production,production_lanes,batcher,insert,datasets,iso_recall,latent,config3,config4,config5,"
                                               "graph_equivalence,ef_sweep,peak,vendor_gemm")
    ap.add_argument("--full-record", default=os.path.join(ROOT, "bench_full.json"), help="where the full record of every leg is written")
    ap.add_argument("--c3-corpus", default="clustered", choices=["clustered", "topic_ordered"],
                    help="configs[2] stand-in rows when HELIX_DBPEDIA_1M_FBIN is unset: 'clustered' = SURVEY 8(d) as written (1 024 Gaussian centres, "
                         "sigma 0.15, seed 20260923, id-order build); 'topic_ordered' = round 4's fitted corpus (scattered insertion order)")
    ap.add_argument("--c5-rows", type=int, default=12_500_000, help="config #5 per-GPU shard (100M / 8)")
    ap.add_argument("--c4-rows", type=int, default=1_250_000, help="config #4 per-GPU shard (10M / 8)")
    ap.add_argument("--builder", default="device", choices=["device", "bulk"], help="how the benchmark graph is built")
    ap.add_argument("--build-batch", type=int, default=2048, help="largest insertion batch of the device build")
    ap.add_argument("--leg", default="headline", choices=["headline", "config5"],
                    help="'config5' = ONLY the sharded exact scan of configs[4] (100M x 1536 fp8 over 8 GPUs = --c5-rows per GPU, batch 4096): "
                         "hvx_shard_group_flat_search_batch_device per step (scan -> ncclAllGather -> merge in one C-ABI call)")
    ap.add_argument("--query-batches", type=int, default=0,
                    help="distinct query batches the timed steps cycle through (0 = steps + warmup, at most 64): no two steps in flight "
                         "gather the same rows")
    ap.add_argument("--traffic-file", default=os.path.join(ROOT, "profiles", "traffic_latest.json"))
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the headline's timed steps, write what its last step returned (ids, scores, counts, status) as DIR/<name>.npy")
    ap.add_argument("--full", action="store_true",
                    help="also run every other leg (recall, roofline with the lone batch, traffic and stream-read passes, ef sweep, "
                         "production default, cpu_baseline + oracle parity, batcher, other corpora and configs, strong scaling) and write the "
                         "full record; --skip, --scaling, --cpu-seconds, --no-verify, --deadline and --full-record apply to it")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------------------
# helpers
# ------------------------------------------------------------------------------------------------------------
def import_index(hv, x, g, metric, dtype, b, device):
    """g: graph in hvx_index_import's layout, EXTERNAL node ids throughout"""
    return hv.ValidatedVectorReadIndex.managed(
        dim=x.shape[1], metric=metric, node_ids=g["node_ids"], vectors=x, l0_offsets=g["l0_offsets"],
        l0_neighbors=g["l0_neighbors"], level=g["level"], up_offsets=g["up_offsets"],
        up_neighbors=g["up_neighbors"], entry_point=g["entry_point"],
        max_layer=g["max_layer"], m=g.get("m", 16), m0=2 * g.get("m", 16), device=device, max_batch=b, dtype=dtype)


def build_graph(hv, synth, args, x, metric, id_lo, b, device, level_seed, keep_index=False):
    """The benchmark graph.  'device' (default): hvx_index_build -- the reference's insert_hnsw for batches of nodes on the
    GPU (csrc/hvx_build.hip), M / M0 = 2M / ef_construction 200, levels from the reference's layer rule; 'bulk': the
    round-1 harness builder (pyhvx/synth.py: exact kNN + select_diverse).  Returns (graph dict with external ids, info,
    the built f32 index or None); the graph dict is None when a plain run keeps the built index (it reads nothing back)."""
    n = x.shape[0]
    ids = np.arange(n, dtype=np.uint64) + np.uint64(id_lo)
    t0 = time.time()
    if args.builder == "bulk":
        g = synth.build_hnsw_graph(x, m=args.m, m0=2 * args.m, level_seed=level_seed)
        g["node_ids"] = ids
        for kk in ("l0_neighbors", "up_neighbors"):
            g[kk] = g[kk] + np.uint64(id_lo)
        g["entry_point"] = g["entry_point"] + id_lo
        torch.cuda.synchronize()
        info = {"builder": "pyhvx.synth.build_hnsw_graph (bulk: exact kNN candidates -> select_diverse -> reverse edges)",
                "seconds": round(time.time() - t0, 2)}
        bix = None
    else:
        lv = synth.draw_levels(n, args.m, level_seed)
        bix, st = hv.ValidatedVectorReadIndex.build(dim=x.shape[1], metric=metric, node_ids=ids, vectors=x, levels=lv, m=args.m, m0=2 * args.m,
                                                    ef_construction=200, max_batch=args.build_batch, batch_divisor=32, device=device,
                                                    search_max_batch=b)
        bix.sync()
        secs = time.time() - t0
        info = {"builder": "hvx_index_build: insert_hnsw (mutation.rs:787-895) for batches of nodes on the device, M=%d M0=%d efC=200" % (args.m, 2 * args.m),
                "seconds": round(secs, 2), "inserts_per_s": round(n / secs, 1), "batches": int(st["batches"]), "max_batch": args.build_batch}
        if keep_index and not args.full:  # the host copy of the graph serves --full's legs and checks, and the import of bf16 rows
            return None, info, bix
        g = bix.export_graph()
        g["node_ids"] = ids
        if args.full:
            # every graph a --full run searches is audited where it was built (hvx_index_audit_graph: row invariants of neighbor_set.rs:1-9,
            # symmetry on every layer -- mutation.rs:1498-1583,1890-1908 --, layer-0 reachability from the entry point)
            t1 = time.time()
            info["audit"] = graph_audit(bix, args.m)
            info["audit"]["seconds"] = round(time.time() - t1, 3)
        if not keep_index:
            bix.close()
            bix = None
    g["m"] = args.m
    deg = np.diff(g["l0_offsets"].astype(np.int64))
    info.update({"rows": n, "degree_mean": round(float(deg.mean()), 2), "degree_max": int(deg.max()), "max_layer": int(g["max_layer"])})
    return g, info, bix


def graph_audit(ix, m):
    a = ix.audit_graph()
    a["clean"] = bool(all(a[kk] == 0 for kk in ("asymmetric_edges_l0", "asymmetric_edges_up", "unsorted_entries", "self_loops", "out_of_range_ids",
                                               "holes", "level_violations", "degree_overflow_rows"))
                      and a["max_degree_l0"] <= 2 * m and a["max_degree_up"] <= m)
    return a


def out_buffers(b, k, dev):
    return [torch.zeros(b, k, dtype=torch.int64, device=dev), torch.zeros(b, k, dtype=torch.float32, device=dev),
            torch.zeros(b, dtype=torch.int32, device=dev), torch.zeros(b, dtype=torch.int32, device=dev),
            torch.zeros(b, 4, dtype=torch.int32, device=dev)]


def recall_of(got, truth, b, k):
    g, t = got.cpu().numpy(), truth.cpu().numpy()
    return sum(len(set(g[i].tolist()) & set(t[i].tolist())) for i in range(b)) / float(b * k)


class LaneSet:
    """`lanes` handles on one index image; steps are issued round-robin.  Every lane owns its output buffers (a step in
    flight on one lane must not share them with the next step on another)."""

    def __init__(self, ix, lanes, occ, b, k, dev, sharded_factory=None):
        self.handles = [ix] + [ix.fork() for _ in range(lanes - 1)]
        for h in self.handles:
            h.set_occupancy(occ)
        self.streams = [torch.cuda.ExternalStream(h.stream(), device=dev) for h in self.handles]
        self.bufs = [out_buffers(b, k, dev) for _ in self.handles]
        self.sharded = [sharded_factory(h) for h in self.handles] if sharded_factory else None
        if self.sharded:  # the search writes straight into the lane's payload of the packed exchange buffer
            for l, s in enumerate(self.sharded):
                self.bufs[l][0], self.bufs[l][1], self.bufs[l][2] = s.outputs()
        self.b, self.k, self.dev, self.occ, self.residency = b, k, dev, occ, None
        self.groups = None   # C-ABI shard groups (in-library RCCL exchange), one per lane
        self.merged = None
        self.last_q = [None] * len(self.handles)  # the query batch of every lane's last step (what its buffers hold the answer to)
        self.params = None  # hv.SearchParams: the steps run hvx_search_batch_params_device (the non-strict arms) instead of the strict call

    def use_shard_groups(self, hv, dist, rank, world):
        """ONE RCCL communicator per rank (round 5): lane 0's hvx_shard_group bootstraps it from the 128-byte unique id (broadcast over
        torch.distributed), the other lanes attach to it (hvx_shard_group_attach: own payload buffers, the rank's exchange stream)."""
        t = torch.zeros(128, dtype=torch.uint8, device=self.dev)
        if rank == 0:
            t.copy_(torch.frombuffer(bytearray(hv.ShardGroup.unique_id()), dtype=torch.uint8))
        dist.broadcast(t, 0)
        first = hv.ShardGroup(self.handles[0], bytes(t.cpu().numpy().tobytes()), rank, world, self.b, self.k)
        self.groups = [first] + [first.attach(h) for h in self.handles[1:]]
        self.merged = [out_buffers(self.b, self.k, self.dev) for _ in self.handles]

    def step(self, i, q, ef):
        l = i % len(self.handles)
        self.last_q[l] = q
        if self.groups:  # search -> ncclAllGather -> merge inside the library, one C-ABI call (hvx_shard_group_*)
            m = self.merged[l]
            self.groups[l].search_batch_device(q, self.k, ef, m[0], m[1], m[2])
            return
        ids, sc, cnt, st, qst = self.bufs[l]
        if self.params is not None:
            self.handles[l].search_batch_params_device(q, self.params, ids, sc, cnt, st, qst, None)
            return
        self.handles[l].search_batch_device(q, self.k, ef, ids, sc, cnt, st, qst, want_stats=False)
        if self.sharded:
            with torch.cuda.stream(self.streams[l]):
                self.sharded[l].merge(ids, sc, cnt)

    def sync(self):
        for h in self.handles:
            h.sync()
        torch.cuda.synchronize()

    def close_forks(self):
        if self.groups:
            for g in self.groups:
                g.close()
            self.groups = None
        for h in self.handles[1:]:
            h.close()


def cgroup_throttle():
    """(nr_throttled, throttled_usec) of this container's cgroup (v2), zeros when unreadable"""
    try:
        d = dict(l.split() for l in open("/sys/fs/cgroup/cpu.stat").read().splitlines() if len(l.split()) == 2)
        return int(d.get("nr_throttled", 0)), int(d.get("throttled_usec", 0))
    except Exception:
        return 0, 0


def query_batches(args, b):
    """how many distinct query batches a timed run cycles through"""
    nb = args.query_batches or (args.steps + args.warmup)
    return max(1, min(nb, 64))


def timed_steps(ls, qs, ef, steps, warmup, barrier):
    """W untimed + K timed steps over DISTINCT query batches (qs[j], cycled): steps in flight on different lanes never gather
    the same rows.  Returns (host seconds of the K steps, event span ms of the K steps, per-kernel ms); ls.last_q[l] = the
    batch lane l answered last."""
    L = len(ls.handles)
    nb = len(qs)
    for i in range(warmup):
        ls.step(i, qs[i % nb], ef)
    ls.sync()
    # The GPU boxes of this pool run the process under a CPU quota (cgroup cpu.max = 16 cores per 100 ms period): a burst of host threads
    # right before the timed region (graph export / import, oracle checks) exhausts the period's budget and the kernel then FREEZES every
    # thread of the process for the rest of it -- in the middle of 20 launches that take 14 ms (r05i: 2.7 ms of wall time per step over
    # kernels that took 0.70).  One idle scheduler period lets the budget refill; nothing is timed here.
    time.sleep(0.12)
    barrier()
    for h in ls.handles:
        h.timing_begin((steps + L - 1) // L)
    e0 = torch.cuda.Event(enable_timing=True)
    ends = [torch.cuda.Event(enable_timing=True) for _ in ls.handles]
    thr0 = cgroup_throttle()  # (BEFORE the start event: reading the cgroup file takes tens of milliseconds on this pool)
    e0.record(ls.streams[0])
    for s in ls.streams[1:]:  # every lane starts behind the same instant
        s.wait_event(e0)
    t_start = time.perf_counter()
    for i in range(steps):
        ls.step(i, qs[(warmup + i) % nb], ef)
    t_issued = time.perf_counter()
    for l, s in enumerate(ls.streams):
        ends[l].record(s)
    ls.sync()
    barrier()
    elapsed = time.perf_counter() - t_start
    thr1 = cgroup_throttle()
    # where a host stall sat (the launches or the final wait), and whether the cgroup throttled the process meanwhile
    ls.host_timing = {"issue_ms": round((t_issued - t_start) * 1e3, 3), "wait_ms": round((time.perf_counter() - t_issued) * 1e3, 3),
                      "cgroup_throttled_periods": thr1[0] - thr0[0], "cgroup_throttled_ms": round((thr1[1] - thr0[1]) / 1e3, 2)}
    span = max(e0.elapsed_time(e) for e in ends)
    per = (steps + L - 1) // L
    ls.residency = None
    try:  # wave-slot residency of the timed launches: sum of wavefront lifetimes / (window x wave slots the build is budgeted for)
        wc = np.concatenate([h.wave_clocks(per, ls.b).reshape(-1, 2) for h in ls.handles]).astype(np.int64)
        wc = wc[wc[:, 0] > 0]
        if wc.size:
            window = int(wc[:, 1].max() - wc[:, 0].min())
            slots = torch.cuda.get_device_properties(ls.dev).multi_processor_count * 4 * ls.occ
            ls.residency = {"wave_slot_residency": round(float((wc[:, 1] - wc[:, 0]).sum()) / (window * slots), 4),
                            "wave_slots": slots, "window_ms": round(window / 1e5, 4), "wavefronts": int(wc.shape[0]),
                            "how": "in-kernel constant-rate clock (100 MHz) at the start / end of every query's wavefront over all timed launches"}
    except Exception as e:
        ls.residency = {"error": str(e)}
    kms = np.concatenate([h.timing_collect(per) for h in ls.handles])
    return elapsed, span, kms


DUMP_LIMIT = 64 << 20  # bytes --dump-outputs may write in all


def dump_outputs(ls, steps, out_dir):
    """--dump-outputs: the answer of the LAST timed step, as its caller receives it (the merged lists when the corpus is sharded), from
    the buffers of the lane that ran it -- nothing writes them between the timed steps and this call.  ids as float64 (exact below
    2^53), scores / counts / status as float32, one DIR/<name>.npy each.  A batch too large for DUMP_LIMIT keeps a fixed sample of
    its query rows (seed 0, in order), listed in rows.npy."""
    l = (steps - 1) % len(ls.handles)
    ls.sync()
    if ls.groups:
        ids, sc, cnt = ls.merged[l][:3]
    elif ls.sharded:
        sh = ls.sharded[l]
        ids, sc, cnt = sh.m_ids, sh.m_scores, sh.m_counts
    else:
        ids, sc, cnt = ls.bufs[l][:3]
    out = {"ids": ids.cpu().numpy().astype(np.float64), "scores": sc.cpu().numpy().astype(np.float32),
           "counts": cnt.cpu().numpy().astype(np.float32), "status": ls.bufs[l][3].cpu().numpy().astype(np.float32)}
    b = out["ids"].shape[0]
    per_row = sum(a[:1].nbytes for a in out.values())
    if b * per_row > DUMP_LIMIT:
        keep = np.sort(np.random.default_rng(0).choice(b, size=(DUMP_LIMIT - 8 * b - 4096) // per_row, replace=False))
        out = {name: a[keep] for name, a in out.items()}
        out["rows"] = keep.astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for name, a in out.items():
        np.save(os.path.join(out_dir, f"{name}.npy"), a)
    info = {"dir": out_dir, "step": steps - 1, "lane": l, "arrays": {name: list(a.shape) for name, a in out.items()}}
    log(f"outputs of the last timed step: {info}")
    return info


def hnsw_alg_bytes(qst, dim, elem, b):
    """distance_computations x dim x sizeof(elem) + neighbour-row ids examined x 4 B + the queries."""
    return int(qst[:, 3].sum()) * dim * elem + int(qst[:, 1].sum()) * 4 + b * dim * 4


def pct(a, p):
    return int(np.percentile(a, p))


# ------------------------------------------------------------------------------------------------------------
# one HNSW leg on one GPU: corpus -> graph -> index -> lanes -> QPS, recall, roofline
# ------------------------------------------------------------------------------------------------------------
def hnsw_leg(hv, synth, args, dev, dataset, n, dim, b, k, ef, dtype_name="f32", steps=None, keep=False, seed=None):
    t0 = time.time()
    steps = steps or args.steps
    nbq = max(1, min(args.query_batches or (steps + args.warmup), 64))
    x, q_all = synth.corpus(dataset, n, dim, b * nbq, args.seed if seed is None else seed, dev)
    qs = [q_all[j * b:(j + 1) * b] for j in range(nbq)]
    bf16 = dtype_name == "bf16"
    if bf16:  # the index holds the rounded values; graph, truth and oracle see exactly those
        x = x.to(torch.bfloat16).to(torch.float32)
    torch.cuda.synchronize()  # the library reads x on its own stream: the corpus must be complete before the build starts
    g, ginfo, bix = build_graph(hv, synth, args, x, hv.EUCLIDEAN, 0, b, dev.index, 7, keep_index=not bf16)
    t_build = time.time() - t0
    ix = bix if bix is not None else import_index(hv, x, g, hv.EUCLIDEAN, hv.BF16 if bf16 else hv.F32, b, dev.index)
    lanes = max(1, args.lanes)
    occ = args.occupancy or (2 if lanes > 1 else 1)
    # lanes BEFORE any other handle: HIP maps streams onto the process's hardware queues in creation order, and
    # two lanes that land on one queue run their kernels back to back (measured r03: 0.65 -> 0.44 ms/step on this leg)
    ls = LaneSet(ix, lanes, occ, b, k, dev)
    ix_truth = ix
    if bf16:  # exact-scan ground truth over the same rounded rows through the f32 scan
        ix_truth = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=hv.EUCLIDEAN, node_ids=g["node_ids"], vectors=x,
                                                       l0_offsets=np.zeros(n + 1, np.uint64), l0_neighbors=np.zeros(0, np.uint64),
                                                       device=dev.index, max_batch=b)
    elapsed, span, kms = timed_steps(ls, qs, ef, steps, args.warmup, lambda: None)
    q = ls.last_q[0]  # what lane 0's buffers answer
    f = out_buffers(b, k, dev)
    ix_truth.flat_search_batch_device(q, k, *f[:4])
    torch.cuda.synchronize()
    got = ls.bufs[0]
    recall = recall_of(got[0], f[0], b, k)
    qst = got[4].cpu().numpy().astype(np.int64)
    alg = hnsw_alg_bytes(qst, dim, 2 if bf16 else 4, b)
    per_step = span / steps
    res = {"dataset": dataset, "rows": n, "dim": dim, "dtype": dtype_name, "ef_search": ef, "k": k, "batch": b, "lanes": lanes,
           "distinct_query_batches": nbq,
           "queries_per_simd": occ, "qps": round(b * steps / elapsed, 1), "ms_per_step": round(elapsed * 1e3 / steps, 4),
           "recall_at_10": round(recall, 4), "clears_recall_0.95": bool(recall >= 0.95),
           "distance_computations_per_query": round(float(qst[:, 3].mean()), 1), "expansion_steps_per_query": round(float(qst[:, 0].mean()), 1),
           "roofline": {"bound": "hbm", "achieved": round(alg / (per_step * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(alg / (per_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "algorithmic_bytes_per_launch": alg,
                        "kernel_ms_overlapped": round(per_step, 4), "kernel_ms_each": round(float(kms.mean()), 4)},
           "corpus_and_graph_seconds": round(t_build, 1), "graph": ginfo}
    if keep:
        return res, dict(ix=ix, ix_truth=ix_truth, ls=ls, x=x, q=q, qs=qs, g=g, truth=f, qst=qst)
    ls.close_forks()
    ix.close()
    if ix_truth is not ix:
        ix_truth.close()
    del x, q, q_all, qs
    torch.cuda.empty_cache()
    return res, None


# ------------------------------------------------------------------------------------------------------------
# extra legs (N = 1 only)
# ------------------------------------------------------------------------------------------------------------
C3_FBIN_ENV = "HELIX_DBPEDIA_1M_FBIN"   # the reference's own variable (index_lifecycle_scale.rs:497-534)


def c3_corpus(synth, n, dim, dev, kind="clustered"):
    """The rows of the configs[2] leg: the DBpedia-1M fbin when HELIX_DBPEDIA_1M_FBIN points at one (header <u32 n><u32 dim> LE +
    f32 rows, validated like the reference's loader), else the synthetic stand-in."""
    path = os.environ.get(C3_FBIN_ENV)
    if path:
        rows = synth.load_fbin(path, expect_rows=n, expect_dim=dim)
        x = torch.empty(n, dim, dtype=torch.float32, device=dev)
        step = 1 << 16
        for r0 in range(0, n, step):
            x[r0:r0 + step] = torch.from_numpy(np.ascontiguousarray(rows[r0:r0 + step])).to(dev)
        return x, f"DBpedia-1M fbin {path}"
    if kind == "topic_ordered":  # round 4's fitted corpus, kept for comparison only (no weight as gate evidence)
        x, _ = synth.corpus("topic_ordered", n, dim, 1, 20260923, dev, **C3_STANDIN)
        return x, "synthetic stand-in (fitted, round 4): synth.topic_ordered(%s)" % ", ".join(f"{k_}={v_}" for k_, v_ in C3_STANDIN.items())
    x, _ = synth.corpus("clustered", n, dim, 1, 20260923, dev, centres=1024, sigma=0.15)
    return x, "synthetic stand-in, SURVEY 8(d) as written: clustered (1 024 Gaussian centres, sigma 0.15), seed 20260923"


C3_STANDIN = dict(latent=12, clusters=2048, spread=0.6)


def leg_config3(hv, synth, orc, args, dev, k=10, nq=32, rounds=5):
    """configs[2] stand-in: 1M x 1536 f32 Euclidean, node i -> (i + N/2) mod N, equality groups of
    100 / 1 000 / 10 000 / 100 000 sources (index_lifecycle_scale.rs:592-613,1769-1776), 32 queries, fused hop + restricted kNN,
    HNSW M=16 / M0=32 / efC=200, ef_search 100, filtered beam 150 % (index_lifecycle_scale.rs:1992).  Both strategies:
    `planned` = the reference's execution plan (exact scan <= 256 ids, the filter-aware walk above: what the reference runs,
    gate distance_computations <= 800 per query, :1924-1927) and `exact` = the device's exact gathered scan of every candidate."""
    n, dim, ef = 1_000_000, 1536, 100
    x, corpus_name = c3_corpus(synth, n, dim, dev, args.c3_corpus)
    real_fbin = bool(os.environ.get(C3_FBIN_ENV))
    scatter = (args.c3_corpus == "topic_ordered") and not real_fbin  # 8(d) / the reference: rows are inserted in id order
    torch.cuda.synchronize()
    t0 = time.time()
    lv = synth.draw_levels(n, 16, 11)
    ix, bst = hv.ValidatedVectorReadIndex.build(dim=dim, metric=hv.EUCLIDEAN, node_ids=np.arange(n, dtype=np.uint64), vectors=x, levels=lv,
                                                m=16, m0=32, ef_construction=200, max_batch=args.build_batch, batch_divisor=32,
                                                device=dev.index, search_max_batch=1024, scatter=scatter)
    ix.sync()
    t_build = time.time() - t0
    audit = graph_audit(ix, 16)
    ix.set_simhash()   # SimHash rows + (on first walk) the SimHash directory
    off = np.arange(n + 1, dtype=np.uint64)
    tgt = ((np.arange(n, dtype=np.uint64) + np.uint64(n // 2)) % np.uint64(n)).astype(np.uint64)
    g = hv.Graph(n, off, tgt)
    qrows = [(int(n * 0.8) + j * (n // 10) // nq) % n for j in range(nq)]
    q = x[qrows].cpu().numpy().copy()
    # the oracle over the same rows, graph and SimHash rows: the walk's checker (a sample of queries per group)
    t0 = time.time()
    gg = ix.export_graph()
    oix = orc.Index(dim, orc.L2SQ, kernel=orc.K_AVX_FMA_HW, m=16, m0=32)
    assert oix.seed(np.arange(n, dtype=np.uint64), x.cpu().numpy(), gg["l0_offsets"], gg["l0_neighbors"], gg["level"], gg["up_offsets"],
                    gg["up_neighbors"], entry_point=gg["entry_point"], max_layer=gg["max_layer"]) == orc.OK
    oix.set_simhash(42, node_hashes=ix.get_simhash())
    t_oracle = time.time() - t0
    groups = []
    ok_all = True
    fields = ("termination", "directory_scan_calls", "directory_rows", "directory_hits", "simhash_row_requests", "routing_rows", "bridge_rows",
              "bridge_frontier_pushes", "vector_payload_requests", "vector_bytes", "distance_computations")
    for size, start in ((100, 0), (1000, 100), (10000, 1100), (100000, 11100)):
        src = np.arange(start, start + size, dtype=np.uint64)
        lo = start + n // 2
        allowed = np.arange(lo, lo + size, dtype=np.uint64)
        # ---- exact: every candidate row scanned on the device
        lat, kern = [], []
        for r in range(rounds + 1):
            t1 = time.perf_counter()
            fid, fsc, fcnt, ncand, fst = ix.prefilter_search_batch(g, q, hv.SearchParams(k).with_ef(ef), src, direction=hv.DIR_OUT)
            if r:
                lat.append(time.perf_counter() - t1)
                kern.append(fst["device_ms"])
        assert ncand == size
        rows = x[lo:lo + size].cpu().numpy()
        ok = True
        for qi in range(0, nq, 1 if size <= 10000 else 4):  # the batch against the oracle's exact scan of the candidate rows
            rc, oid, osc = orc.flat_matrix(orc.L2SQ, rows, q[qi], k, kernel=orc.K_AVX_FMA_HW)
            ok &= (fid[qi, :fcnt[qi]] - np.uint64(lo)).tolist() == oid.tolist()
            ok &= fsc[qi, :fcnt[qi]].view(np.uint32).tolist() == osc.view(np.uint32).tolist()
        ms, kms = float(np.median(lat)) * 1e3, float(np.median(kern))
        alg = size * dim * 4 + nq * dim * 4  # every candidate row is needed once per batch (shared candidate set) + the queries
        exact = {"end_to_end_ms_per_batch": round(ms, 3), "us_per_query": round(ms * 1e3 / nq, 1), "scan_kernels_ms": round(kms, 3),
                 "hbm_gbs_scan": round(alg / (kms * 1e-3) / 1e9, 1), "distance_computations_per_query": size,
                 "scan_path_flags": ix.last_scan_path(), "oracle_bit_exact_sample": bool(ok)}
        # ---- device plan (round 6): HVX_RESTRICTED_AUTO, the library's default -- exact while the candidate rows take <= 1 GiB
        rpa = hv.RestrictedParams.auto(k, ef)
        lat, kern = [], []
        for r in range(rounds + 1):
            t1 = time.perf_counter()
            aid, asc, acnt, ncand, ars, ast = ix.prefilter_search_batch_params(g, q, rpa, src, direction=hv.DIR_OUT)
            if r:
                lat.append(time.perf_counter() - t1)
                kern.append(ast["device_ms"])
        ams, akms = float(np.median(lat)) * 1e3, float(np.median(kern))
        arec = sum(len(set(aid[i, :acnt[i]].tolist()) & set(fid[i, :fcnt[i]].tolist())) for i in range(nq)) / float(nq * k)
        device_plan = {"strategy": "exact" if ars[0]["strategy"] == hv.RESTRICTED_EXACT else "filtered_graph", "end_to_end_ms_per_batch": round(ams, 3),
                       "us_per_query": round(ams * 1e3 / nq, 1), "scan_kernels_ms": round(akms, 3), "recall_at_10_vs_exact": round(arec, 4),
                       "ids_equal_exact_leg": bool(aid.tolist() == fid.tolist() and asc.view(np.uint32).tolist() == fsc.view(np.uint32).tolist()),
                       "scan_path_flags": ix.last_scan_path(), "hbm_gbs_scan": round(alg / (akms * 1e-3) / 1e9, 1),
                       "gate_recall_ge_0.92": bool(arec >= 0.92)}
        # ---- reference plan: restricted_execution_plan (exact <= 256 ids / 4 MiB, else the filter-aware walk): what the reference runs
        rp = hv.RestrictedParams.new(k, ef)
        lat, kern = [], []
        for r in range(rounds + 1):
            t1 = time.perf_counter()
            pid, psc, pcnt, ncand, prs, pst = ix.prefilter_search_batch_params(g, q, rp, src, direction=hv.DIR_OUT)
            if r:
                lat.append(time.perf_counter() - t1)
                kern.append(pst["device_ms"])
        pms, pkms = float(np.median(lat)) * 1e3, float(np.median(kern))
        walked = prs[0]["strategy"] == hv.RESTRICTED_FILTERED
        pok = True
        for qi in range(nq):  # EVERY query of the group: ids, score bits, every RestrictedSearchStats counter and the termination vs the oracle's walk
            rc, oid, osc, ost = oix.search_restricted(q[qi], k, ef, allowed)
            pok &= rc == orc.OK and pid[qi, :pcnt[qi]].tolist() == oid.tolist() and psc[qi, :pcnt[qi]].view(np.uint32).tolist() == osc.view(np.uint32).tolist()
            pok &= prs[qi]["strategy"] == ost["strategy"] and all(prs[qi][f] == ost[f] for f in fields)
        rec = sum(len(set(pid[i, :pcnt[i]].tolist()) & set(fid[i, :fcnt[i]].tolist())) for i in range(nq)) / float(nq * k)
        dc = np.array([r_["distance_computations"] for r_ in prs]) if walked else np.full(nq, size)
        terms = {}
        for r_ in prs:
            terms[str(r_["termination"])] = terms.get(str(r_["termination"]), 0) + 1
        # SURVEY 8(d) "filtered graph": vector payloads x dim x 4 + routing rows x degree x 4 (+ the query)
        walk_alg = int(sum(r_["vector_bytes"] + r_["routing_rows"] * 32 * 4 for r_ in prs)) + nq * dim * 4 if walked else alg
        planned = {"strategy": "filtered_graph" if walked else "exact", "end_to_end_ms_per_batch": round(pms, 3), "us_per_query": round(pms * 1e3 / nq, 1),
                   "search_kernel_ms": round(pkms, 3), "recall_at_10_vs_exact": round(rec, 4),
                   "distance_computations_per_query": {"mean": round(float(dc.mean()), 1), "max": int(dc.max())},
                   "reference_gate_distance_computations_le_800": bool(dc.max() <= 800),
                   "directory_rows_max": int(max(r_["directory_rows"] for r_ in prs)), "routing_rows_mean": round(float(np.mean([r_["routing_rows"] for r_ in prs])), 1),
                   "bridge_rows_mean": round(float(np.mean([r_["bridge_rows"] for r_ in prs])), 1),
                   "terminations": terms, "algorithmic_bytes_per_batch": walk_alg, "hbm_gbs": round(walk_alg / (pkms * 1e-3) / 1e9, 1),
                   "oracle_equal_sample": {"queries": nq, "ids_bits_counters_termination_equal": bool(pok)}}
        if size == 100000 and walked:
            # the same walk with the chip filled: 1 024 queries (one workgroup each) over the same candidate set
            qb = x[torch.randint(0, n, (1024,), generator=torch.Generator().manual_seed(5)).to(dev)].cpu().numpy()
            bk = []
            for r in range(3):
                bid, bsc, bcnt, _, brs, bst = ix.prefilter_search_batch_params(g, qb, rp, src, direction=hv.DIR_OUT)
                if r:
                    bk.append(bst["device_ms"])
            bbytes = int(sum(r_["vector_bytes"] + r_["routing_rows"] * 32 * 4 for r_ in brs)) + 1024 * dim * 4
            bms = float(np.mean(bk))
            planned["batch_1024"] = {"search_kernel_ms": round(bms, 3), "queries_per_s_kernel": round(1024 / (bms * 1e-3), 1),
                                     "algorithmic_bytes_per_batch": bbytes, "hbm_gbs": round(bbytes / (bms * 1e-3) / 1e9, 1),
                                     "frac_of_hbm_peak": round(bbytes / (bms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                                     "distance_computations_per_query_max": int(max(r_["distance_computations"] for r_ in brs))}
        # the reference issues ONE query per call (index_lifecycle_scale.rs:1893-1912): per-query end-to-end latency of the fused call
        for name_, fn_ in (("planned", lambda qq: ix.prefilter_search_batch_params(g, qq, rp, src, direction=hv.DIR_OUT)),
                           ("device", lambda qq: ix.prefilter_search_batch_params(g, qq, rpa, src, direction=hv.DIR_OUT)),
                           ("exact", lambda qq: ix.prefilter_search_batch(g, qq, hv.SearchParams(k).with_ef(ef), src, direction=hv.DIR_OUT))):
            one = []
            fn_(q[:1])
            for qi in range(nq):
                t1 = time.perf_counter()
                fn_(q[qi:qi + 1])
                one.append((time.perf_counter() - t1) * 1e3)
            one.sort()
            {"planned": planned, "device": device_plan, "exact": exact}[name_]["single_query_end_to_end_ms"] = {"p50": round(one[(nq - 1) * 50 // 100], 3), "p95": round(one[(nq - 1) * 95 // 100], 3)}
        planned["reference_gates"] = {"recall_at_10_ge_0.92": bool(rec >= 0.92), "distance_computations_le_800": bool(dc.max() <= 800),
                                      "directory_rows_le_65536": bool(planned["directory_rows_max"] <= 65536),
                                      "end_to_end_p95_le_50ms": bool(planned["single_query_end_to_end_ms"]["p95"] <= 50.0)}
        planned["reference_gates"]["passed"] = all(planned["reference_gates"].values())
        ok_all &= bool(ok) and bool(pok)
        groups.append({"candidates": size, "reference_plan": hv.restricted_execution_plan(size, dim, hv.SearchParams.new(k)), "planned": planned,
                       "device_plan": device_plan, "exact": exact})
    # ---- the operator's shape (storage.rs:140-163): every request brings ITS OWN candidate ids -- one launch per batch of requests
    own = []
    rng_o = np.random.default_rng(20260924)
    for m_ids, b_req in ((1000, 256), (1000, 1024), (10000, 256)):
        lists = [np.sort(rng_o.choice(n, m_ids, replace=False)).astype(np.uint64) for _ in range(b_req)]
        offs = (np.arange(b_req + 1, dtype=np.uint64) * np.uint64(m_ids))
        flat_ids = np.concatenate(lists)
        qreq = x[torch.randint(0, n, (b_req,), generator=torch.Generator().manual_seed(9)).to(dev)].cpu().numpy()
        lat, kern = [], []
        for r in range(4):
            t1 = time.perf_counter()
            oid_, osc_, ocnt_, ost_, ors_, ostat_ = ix.search_restricted_batch_params(qreq, rpa, flat_ids, offsets=offs, want_stats=True)
            if r:
                lat.append(time.perf_counter() - t1)
                kern.append(ostat_["device_ms"])
        okq = True
        for qi in range(0, b_req, max(1, b_req // 8)):  # a sample of the requests against the oracle's exact scan of THEIR rows
            rc, wid, wsc = orc.flat_matrix(orc.L2SQ, x[torch.from_numpy(lists[qi].astype(np.int64)).to(dev)].cpu().numpy(), qreq[qi], k, kernel=orc.K_AVX_FMA_HW)
            okq &= lists[qi][wid.astype(np.int64)].tolist() == oid_[qi, :ocnt_[qi]].tolist() and wsc.view(np.uint32).tolist() == osc_[qi, :ocnt_[qi]].view(np.uint32).tolist()
        ms_, kms_ = float(np.median(lat)) * 1e3, float(np.median(kern))
        bytes_ = b_req * m_ids * dim * 4
        own.append({"requests": b_req, "ids_per_request": m_ids, "kernel_ms": round(kms_, 3), "end_to_end_ms": round(ms_, 3), "qps_kernel": round(b_req / (kms_ * 1e-3), 1),
                    "qps_end_to_end": round(b_req / (ms_ * 1e-3), 1), "hbm_gbs": round(bytes_ / (kms_ * 1e-3) / 1e9, 1),
                    "frac_of_hbm_peak": round(bytes_ / (kms_ * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "oracle_bit_exact_sample": bool(okq)})
        ok_all &= bool(okq)
    big = groups[-1]
    out = {"workload": f"configs[2]: {n}x{dim} f32 [{corpus_name}], Euclidean, HNSW M=16/M0=32/efC=200 "
                       f"(device build, {'scattered' if scatter else 'id-order'} insertion, {t_build:.1f} s), benchmark topology i -> i+N/2, one-hop where_() group -> restricted kNN k={k} ef={ef}, "
                       f"{nq} queries per batch, fused hvx_prefilter_search_batch[_params]",
           "corpus": {"rows": corpus_name, "kind": ("dbpedia_fbin" if real_fbin else args.c3_corpus), "fbin_env": C3_FBIN_ENV,
                      "insertion_order": "scattered" if scatter else "id order (as the reference's backfill inserts)",
                      "note": "the DBpedia-1M fbin cannot be fetched here (scripts/prepare-dbpedia-vector-fixture.py:17-19); on a synthetic stand-in the "
                              "reference's recall gate (>= 0.92 per group) is reported as measured, pass or fail -- it says how the ALGORITHM behaves on "
                              "these rows (device == oracle bit for bit), not whether the reference's gate holds on DBpedia"},
           "reference_gates_passed": (bool(all(g_["planned"]["reference_gates"]["passed"] for g_ in groups)) if real_fbin else None),
           "gates_on_this_corpus": [{"candidates": g_["candidates"], **g_["planned"]["reference_gates"]} for g_ in groups],
           "graph_audit": audit,
           "strategies": "device_plan = HVX_RESTRICTED_AUTO, the library's default since round 6: exact gathered scan while the candidate rows take <= 1 GiB "
                         "(recall 1.0 by construction), the filter-aware walk above; planned = the reference's plan (restricted.rs:426-453: exact <= 256 ids, "
                         "filter-aware walk above, 150 % beam: HVX_RESTRICTED_REFERENCE_PLAN, every counter held to the oracle); exact = strategy EXACT forced",
           "groups": groups,
           "per_request_candidate_sets": {"what": "hvx_search_restricted_batch_params with allowed_offsets: every request its own candidate ids, ONE launch per batch "
                                                  "(csrc/hvx_restricted_exact.hip); algorithmic bytes = requests x ids x dim x 4", "rows": own},
           "device_plan_gates": [{"candidates": g_["candidates"], "strategy": g_["device_plan"]["strategy"], "recall_at_10": g_["device_plan"]["recall_at_10_vs_exact"],
                                  "recall_ge_0.92": g_["device_plan"]["gate_recall_ge_0.92"]} for g_ in groups],
           "roofline": {"bound": "hbm", "kernel": "restricted exact scan, 100 000-candidate group", "achieved": big["exact"]["hbm_gbs_scan"],
                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(big["exact"]["hbm_gbs_scan"] / HBM_PEAK_GBS, 4),
                        "note": "algorithmic bytes = candidates x dim x 4 (each row once per batch) / scan-kernel time; "
                                "the small groups are launch-latency bound (a 100-row scan is 0.6 MB)"},
           "walk_roofline": {"bound": "hbm", "kernel": "restricted_walk_kernel, 100 000-candidate group", "achieved": big["planned"]["hbm_gbs"],
                             "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(big["planned"]["hbm_gbs"] / HBM_PEAK_GBS, 4),
                             "note": "a 32-query batch runs 32 workgroups (of 256 CUs): a dependent walk per query, not a streaming kernel; "
                                     "bytes = vector payloads x (4 + dim x 4) + routing rows x 128 B"},
           "reference_gates": {"recall_at_10": 0.92, "distance_computations_per_query_max": 800, "directory_rows_max": 65536,
                               "vector_increment_p95_ms": 15, "end_to_end_p95_ms": 50},
           "oracle_seed_seconds": round(t_oracle, 1), "parity_sample_ok": ok_all}
    del oix
    ix.close()
    del x
    torch.cuda.empty_cache()
    return out


def leg_config5(hv, synth, orc, dev, rows, b=4096, k=10, dim=1536):
    """configs[4] per-GPU shard: exact scan of a 4096-query batch over fp8-e4m3 rows on the matrix cores."""
    out = None
    while rows >= 250_000:
        try:
            t0 = time.time()
            x, q = synth.corpus("embedding", rows, dim, b, 20260924, dev, latent=24, clusters=4096)
            ix = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=hv.EUCLIDEAN, node_ids=np.arange(rows, dtype=np.uint64), vectors=x,
                                                     l0_offsets=np.zeros(rows + 1, np.uint64), l0_neighbors=np.zeros(0, np.uint64),
                                                     device=dev.index, max_batch=b, dtype=hv.FP8_E4M3)
            t_imp = time.time() - t0
            break
        except (hv.HelixDbError, RuntimeError, MemoryError) as e:  # out of HBM: halve the shard, say so
            log(f"config5: {rows} rows did not fit ({type(e).__name__}); halving")
            x = q = None
            torch.cuda.empty_cache()
            rows //= 2
    else:
        return {"error": "no shard size fitted"}
    f = out_buffers(b, k, dev)
    ms = []
    for i in range(3):
        s = ix.flat_search_batch_device(q, k, *f[:4], want_stats=True)
        if i:
            ms.append(s["device_ms"])
    ms = float(np.mean(ms))
    # quantisation loss: recall of the fp8 answer against the exact top-k over the f32 rows (library GEMM, harness only)
    rq = 64
    best_v = best_i = None
    sq = None
    for c0 in range(0, rows, 1 << 20):
        xc = x[c0:c0 + (1 << 20)]
        d2 = (xc * xc).sum(1)[None, :] - 2.0 * (q[:rq] @ xc.t())
        v, i = torch.topk(d2, k, dim=1, largest=False)
        i = i + c0
        if best_v is None:
            best_v, best_i = v, i
        else:
            cv, ci = torch.cat([best_v, v], 1), torch.cat([best_i, i], 1)
            best_v, sel = torch.topk(cv, k, dim=1, largest=False)
            best_i = torch.gather(ci, 1, sel)
    recall = recall_of(f[0][:rq], best_i, rq, k)
    # parity on a sample: the same pipeline restricted to 50 000 candidate rows == the oracle's exact scan over the
    # dequantised values of those rows (numpy twin of the import's quantiser)
    sub = np.arange(0, 50_000, dtype=np.uint64) * np.uint64(max(1, rows // 50_000))
    xs = x[torch.from_numpy(sub.astype(np.int64)).to(dev)].cpu().numpy()
    deq = synth.quantize_fp8_rows(xs)
    qh = q[:8].cpu().numpy()
    rid, rsc, rcnt = ix.search_restricted_batch(qh, hv.SearchParams(k), hv.RestrictedVectorCandidates.from_ids(sub))
    ok = True
    for qi in range(qh.shape[0]):
        rc, oid, osc = orc.flat_matrix(orc.L2SQ, deq, qh[qi], k, kernel=orc.K_AVX_FMA_HW)
        ok &= rid[qi, :rcnt[qi]].tolist() == sub[oid].tolist() and rsc[qi, :rcnt[qi]].view(np.uint32).tolist() == osc.view(np.uint32).tolist()
    # the TIMED full scan itself against the oracle -- the first `fq` queries over ALL stored (dequantised) rows,
    # one 1M-row chunk at a time, per-chunk top-k by the oracle's exact scan, merged by Candidate order (score, id) (model.rs:55-61)
    import concurrent.futures
    fq = 8
    qf = q[:fq].cpu().numpy()
    t_full = time.time()
    # the stored values come from the index itself (hvx_index_read_rows_device: fl32(scale x decode(code)), the expression the
    # import's quantiser stored); the numpy twin of the quantiser must reproduce them on a sample
    probe = torch.empty(4096, dim, dtype=torch.float32, device=dev)
    ix.read_rows_device(0, 4096, probe)
    twin_ok = bool((probe.cpu().numpy() == synth.quantize_fp8_rows(x[:4096].cpu().numpy())).all())
    del probe
    merged = [(np.zeros(0, np.uint32), np.zeros(0, np.uint64)) for _ in range(fq)]
    deq_d = torch.empty(1 << 20, dim, dtype=torch.float32, device=dev)
    with concurrent.futures.ThreadPoolExecutor(max_workers=fq) as pool:
        for c0 in range(0, rows, 1 << 20):
            cn = min(1 << 20, rows - c0)
            ix.read_rows_device(c0, cn, deq_d)
            deq_c = deq_d[:cn].cpu().numpy()
            parts = list(pool.map(lambda qi: orc.flat_matrix(orc.L2SQ, deq_c, qf[qi], k, kernel=orc.K_AVX_FMA_HW), range(fq)))
            for qi, (rc, oid, osc) in enumerate(parts):
                assert rc == orc.OK
                bits = np.concatenate([merged[qi][0], osc.view(np.uint32)])
                ids_ = np.concatenate([merged[qi][1], oid + np.uint64(c0)])
                order = np.lexsort((ids_, bits))[:k]   # non-negative f32 scores order like their bit patterns
                merged[qi] = (bits[order], ids_[order])
            del deq_c
    del deq_d
    got_ids = f[0][:fq].cpu().numpy().astype(np.uint64)
    got_bits = f[1][:fq].cpu().numpy().view(np.uint32)
    full_ok = twin_ok and all(got_ids[qi].tolist() == merged[qi][1].tolist() and got_bits[qi].tolist() == merged[qi][0].tolist() for qi in range(fq))
    t_full = time.time() - t_full
    useful = 2.0 * b * rows * dim
    out = {"workload": f"configs[4] per-GPU shard: exact scan, {rows}x{dim} fp8-e4m3 rows (+ f32 row scale), batch {b}, k={k}, squared-L2; "
                       f"the full config is 100M rows over 8 GPUs = 12.5M per GPU",
           "rows": rows, "ms_per_batch": round(ms, 3), "queries_per_s": round(b / ms * 1e3, 1),
           "roofline": {"bound": "mfma", "achieved": round(useful / ms / 1e9, 1), "peak": MFMA_BF16_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(useful / ms / 1e9 / MFMA_BF16_TFLOPS, 4),
                        "note": "ALGORITHMIC flops 2*b*N*dim / time of the whole scan (contraction + selection + exact re-rank + certificate); "
                                "round 4: the large-tile kernel multiplies the fp8 codes on the MX-scaled fp8 matrix instruction (v_mfma_scale_f32_32x32x64_f8f6f4) "
                                "with the f32 query carried as TWO e4m3 pieces -- two matrix passes per useful flop, so the fraction stays quoted against the "
                                "bf16 dense peak (5 PFLOP/s would be the fp8-MFMA peak: frac_of_fp8_peak below)",
                        "frac_of_fp8_peak": round(useful / ms / 1e9 / 5000.0, 4)},
           "hbm_bytes_per_batch": rows * dim, "hbm_bytes_per_batch_note": "SURVEY 8(d): the fp8 codes stream once per batch (query tiles of a "
           "super-tile share the row tile in L2): 19.2 GB at 12.5M x 1536",
           "recall_at_k_vs_f32_rows": round(recall, 4),
           "exactness": "certificate passed for every query (the call fails otherwise)", "oracle_bit_exact_sample": bool(ok),
           "oracle_bit_exact_full_scan": bool(full_ok),
           "oracle_full_scan_check": {"queries": fq, "rows": rows, "what": "ids and score bits of the TIMED scan's output == the oracle's exact scan over every "
                                      "dequantised row (1M-row chunks merged by (score, id))", "stored_rows_equal_numpy_quantiser_twin_on_sample": twin_ok, "seconds": round(t_full, 1)},
           "corpus_and_import_seconds": round(t_imp, 1)}
    ix.close()
    del x, q
    torch.cuda.empty_cache()
    return out


def leg_incremental_insert(hv, synth, args, dev, n0=500_000, add=100_000, seq=2_000):
    """Round 5 (VERDICT r4 missing #4): writes to a resident image.  A graph built over n0 rows with room to grow takes `add` rows through
    hvx_index_insert_batch in batched mode (one call) and `seq` more in sequential mode (one node per batch = the reference's
    insert_hnsw order: mutation.rs:642-895); the grown graph is audited on the device and searched against its own exact scan."""
    dim, b, k, ef = args.dim, args.batch, args.k, args.ef
    n = n0 + add + seq
    x, q = synth.corpus("embedding", n, dim, b, args.seed + 5, dev)
    torch.cuda.synchronize()
    lv = synth.draw_levels(n, args.m, 13)
    ids = np.arange(n, dtype=np.uint64)
    t0 = time.time()
    ix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids[:n0], vectors=x[:n0], levels=lv[:n0], m=args.m, m0=2 * args.m,
                                              ef_construction=200, max_batch=args.build_batch, batch_divisor=32, device=dev.index, search_max_batch=b,
                                              reserve_rows=add + seq, reserve_upper_rows=int(lv[n0:].sum()) + 8)
    ix.sync()
    t_build = time.time() - t0
    t0 = time.time()
    st = ix.insert_batch(ids[n0:n0 + add], x[n0:n0 + add], lv[n0:n0 + add], ef_construction=200, max_batch=args.build_batch, batch_divisor=32)
    ix.sync()
    t_ins = time.time() - t0
    t0 = time.time()
    st2 = ix.insert_batch(ids[n0 + add:], x[n0 + add:], lv[n0 + add:], ef_construction=200, sequential=True)
    ix.sync()
    t_seq = time.time() - t0
    audit = graph_audit(ix, args.m)
    f = out_buffers(b, k, dev)
    g = out_buffers(b, k, dev)
    ix.flat_search_batch_device(q, k, *f[:4])
    ix.search_batch_device(q, k, ef, *g, want_stats=False)
    torch.cuda.synchronize()
    rec = recall_of(g[0], f[0], b, k)
    newest = int((g[0] >= n0).sum().item())
    out = {"workload": f"{n0}x{dim} f32 built on the device (reserve {add + seq} rows), + {add} rows by ONE hvx_index_insert_batch call (batched), + {seq} rows in "
                       f"sequential mode (one node per batch, the reference's order), M={args.m}/M0={2 * args.m}/efC=200",
           "build_seconds": round(t_build, 2), "batched": {"rows": add, "seconds": round(t_ins, 3), "inserts_per_s": round(add / t_ins, 1), "batches": int(st["batches"])},
           "sequential": {"rows": seq, "seconds": round(t_seq, 3), "inserts_per_s": round(seq / t_seq, 1), "us_per_insert": round(t_seq / seq * 1e6, 1)},
           "rows_after": ix.rows(), "visible_seq": ix.visible_seq(), "audit": audit,
           "recall_at_10_ef%d" % ef: round(rec, 4), "results_from_appended_rows": newest,
           "note": "recall of the grown graph against its own exact scan (which covers the appended rows: row norms / bf16 shadow extended on that scan)"}
    # ---- deletes (hvx_index_delete_batch == VectorIndex::delete, mutation.rs:1606-2055: unlink, relink the sources, entry repair) ----
    n_del = getattr(args, "deletes", 2000)
    if n_del:
        rng = np.random.default_rng(args.seed + 9)
        victims = np.sort(rng.choice(n, size=n_del, replace=False)).astype(np.uint64)
        rng.shuffle(victims)
        t0 = time.time()
        sd = ix.delete_batch(victims)
        ix.sync()
        t_del = time.time() - t0
        audit_d = graph_audit(ix, args.m)
        ix.flat_search_batch_device(q, k, *f[:4])
        ix.search_batch_device(q, k, ef, *g, want_stats=False)
        torch.cuda.synchronize()
        gone = torch.from_numpy(victims.astype(np.int64)).to(dev)
        leaked = int(torch.isin(g[0].reshape(-1), gone).sum().item()) + int(torch.isin(f[0].reshape(-1), gone).sum().item())
        out["deletes"] = {"workload": f"{n_del} scattered nodes of the {n}-row graph deleted one after the other (sequential semantics = the reference's)",
                          "seconds": round(t_del, 3), "deletes_per_s": round(n_del / t_del, 1), "us_per_delete": round(t_del / n_del * 1e6, 1),
                          "relinked_rows": sd["relinked_rows"], "relinked_rows_per_delete": round(sd["relinked_rows"] / max(1, sd["deleted"]), 1),
                          "entry_moves": sd["entry_moves"], "live_rows_after": ix.live_rows(), "audit": audit_d,
                          "recall_at_10_ef%d" % ef: round(recall_of(g[0], f[0], b, k), 4), "deleted_ids_in_results": leaked}
        # ---- upserts (hvx_index_upsert_batch == VectorInsertContract::Upsert: delete + insert under the same id, into the node's own slot) ----
        n_up = min(200, n_del)
        live = np.setdiff1d(np.arange(n, dtype=np.uint64), victims)
        tgt = np.concatenate([rng.choice(live, size=n_up - n_up // 4, replace=False), victims[: n_up // 4]]).astype(np.uint64)   # live ids and deleted ones
        newv = (x[torch.from_numpy(rng.integers(0, n, n_up)).to(dev)] * 0.5 + x[torch.from_numpy(rng.integers(0, n, n_up)).to(dev)] * 0.5).cpu().numpy()
        t0 = time.time()
        su = ix.upsert_batch(tgt, newv, None, ef_construction=200)
        ix.sync()
        t_up = time.time() - t0
        qn = torch.from_numpy(newv[:64]).to(dev)
        fu = out_buffers(64, k, dev)
        ix.flat_search_batch_device(qn, k, *fu[:4])
        torch.cuda.synchronize()
        own = int((fu[0][:, 0].cpu().numpy().astype(np.uint64) == tgt[:64]).sum())
        out["upserts"] = {"workload": f"{n_up} upserts ({n_up - n_up // 4} live ids, {n_up // 4} ids deleted above): delete + sequential insert under the same id",
                          "seconds": round(t_up, 3), "us_per_upsert": round(t_up / n_up * 1e6, 1), "nodes": int(su["nodes"]), "live_rows_after": ix.live_rows(),
                          "new_vector_is_its_ids_nearest_of_64": own}
    ix.close()
    del x, q
    torch.cuda.empty_cache()
    return out


def leg_vendor_gemm(dev):
    """BASELINE.md section 2 / VERDICT r4 #3(a): what the vendor library gets on THIS box for the dense contraction at the heart of the
    exact scan -- a (queries x dim) x (dim x rows) GEMM of one row chunk -- bf16 (torch.matmul -> hipBLASLt / rocBLAS) and fp8-e4m3
    (torch._scaled_mm -> hipBLASLt).  Harness only: the product's scan kernels are hand-written (csrc/hvx_flat_tile.hip); this is the
    number they are held against.  The scan does more than the GEMM (epilogue with per-row terms, threshold filter, selection, exact
    re-rank, certificate), so the GEMM rate is an upper bound for it."""
    res = {}
    try:
        torch.backends.cuda.preferred_blas_library("hipblaslt")
    except Exception:
        pass

    def time_it(fn, flops, iters=10):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        return {"ms": round(ms, 4), "tflops": round(flops / ms / 1e9, 1)}

    for name, (m, n, kk) in (("c5_shape_4096x32768x1536", (4096, 32768, 1536)), ("c2_shape_1024x65536x768", (1024, 65536, 768))):
        flops = 2.0 * m * n * kk
        a = torch.randn(m, kk, device=dev, dtype=torch.float32)
        bm = torch.randn(n, kk, device=dev, dtype=torch.float32)
        row = {"m_queries": m, "n_rows": n, "k_dim": kk}
        try:
            a16, b16 = a.to(torch.bfloat16), bm.to(torch.bfloat16)
            row["bf16"] = time_it(lambda: torch.matmul(a16, b16.t()), flops)
            row["bf16"]["frac_of_bf16_peak"] = round(row["bf16"]["tflops"] / MFMA_BF16_TFLOPS, 4)
        except Exception as e:
            row["bf16"] = {"error": f"{type(e).__name__}: {e}"[:200]}
        try:
            f8 = torch.float8_e4m3fn
            a8, b8 = (a * 0.25).to(f8), (bm * 0.25).to(f8)
            one = torch.ones((), device=dev, dtype=torch.float32)
            row["fp8"] = time_it(lambda: torch._scaled_mm(a8, b8.t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16), flops)
            row["fp8"]["frac_of_fp8_peak"] = round(row["fp8"]["tflops"] / 5000.0, 4)
        except Exception as e:
            row["fp8"] = {"error": f"{type(e).__name__}: {e}"[:200]}
        res[name] = row
        del a, bm
    c5 = res.get("c5_shape_4096x32768x1536", {})
    c2 = res.get("c2_shape_1024x65536x768", {})
    res["fp8"] = c5.get("fp8") if isinstance(c5.get("fp8"), dict) and "tflops" in c5.get("fp8", {}) else None   # beside config5 in the compact line
    res["bf16"] = c2.get("bf16") if isinstance(c2.get("bf16"), dict) and "tflops" in c2.get("bf16", {}) else None  # beside the f32 exact scan
    res["library"] = "torch.matmul / torch._scaled_mm (hipBLASLt preferred) of torch " + torch.__version__
    torch.cuda.empty_cache()
    return res


def kernel_of_ef(ef):
    need = ef + 32
    if need <= 832:
        beam = 192 if need <= 192 else 384 if need <= 384 else 448 if need <= 448 else 832
        return f"one wavefront per query, {beam}-entry register beam"
    return "general kernel (4 wavefronts per query)"


def ef_sweep_rows(ls, qs, ix_truth, dev, dim, b, k, efs, elem=4, steps=24, stop_at=None):
    """Same graph, same lanes, distinct query batches: one row per beam width (QPS, recall against the exact scan, distance
    evaluations, fraction of the HBM peak from the algorithmic bytes of lane 0's last batch)."""
    rows = []
    for ef in efs:
        elapsed, span, kms = timed_steps(ls, qs, ef, steps, 3, lambda: None)
        if elapsed * 1e3 > 1.3 * span:  # a host stall inside the timed steps (this pool freezes a process that spends its CPU quota):
            elapsed, span, kms = timed_steps(ls, qs, ef, steps, 3, lambda: None)  # the wall clock of one repeat is what the row reports
        q = ls.last_q[0]
        f = out_buffers(b, k, dev)
        ix_truth.flat_search_batch_device(q, k, *f[:4])
        torch.cuda.synchronize()
        got = ls.bufs[0]
        rec = recall_of(got[0], f[0], b, k)
        qst = got[4].cpu().numpy().astype(np.int64)
        alg = hnsw_alg_bytes(qst, dim, elem, b)
        rows.append({"ef_search": ef, "recall_at_10": round(rec, 4), "qps": round(b * steps / elapsed, 1), "ms_per_step": round(elapsed * 1e3 / steps, 4),
                     "distance_computations_per_query": round(float(qst[:, 3].mean()), 1),
                     "expansion_steps_per_query": round(float(qst[:, 0].mean()), 1),
                     "frac_of_hbm_peak": round(alg / (span / steps * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "kernel": kernel_of_ef(ef)})
        if stop_at is not None and rec >= stop_at:
            break
    return rows


def leg_iso_recall(hv, synth, orc, args, dev, dataset, n, dim, b, k, efs=(128, 192, 256, 384, 512, 800), target=0.95):
    """The metric is QPS @ recall@10 >= 0.95: on a corpus where ef = 128 misses the gate, sweep ef (scale_contracts.rs:167-215
    protocol: same graph, same queries, recall against the exact scan) and report the smallest beam that clears it -- its QPS,
    roofline fraction and the CPU oracle at the same ef."""
    res0, st = hnsw_leg(hv, synth, args, dev, dataset, n, dim, b, k, efs[0], steps=32, keep=True)  # (32: eight rounds of the four lanes -- 12 left the first and the last round half alone)
    ls, ix_truth = st["ls"], st["ix_truth"]
    sweep = ef_sweep_rows(ls, st["qs"], ix_truth, dev, dim, b, k, efs, stop_at=target)
    hit = dict(sweep[-1]) if sweep and sweep[-1]["recall_at_10"] >= target else None
    out = {"dataset": dataset, "rows": n, "dim": dim, "batch": b, "k": k, "target_recall_at_10": target, "sweep": sweep, "iso_recall": hit,
           "leg_at_first_ef": res0}
    if hit is not None and not args.no_verify:  # the CPU oracle at the same beam width, same graph and queries
        gg = st["g"]
        oix = orc.Index(dim, orc.L2SQ, kernel=orc.K_AVX_FMA_HW, m=args.m, m0=2 * args.m)
        assert oix.seed(gg["node_ids"], st["x"].cpu().numpy(), gg["l0_offsets"], gg["l0_neighbors"], gg["level"], gg["up_offsets"], gg["up_neighbors"],
                        entry_point=gg["entry_point"], max_layer=gg["max_layer"]) == orc.OK
        threads = host_threads(args)
        qh = ls.last_q[0].cpu().numpy()
        oix.search_batch(qh[:64], k, hit["ef_search"], threads=threads)
        t1 = time.perf_counter()
        rc, o_ids, o_sc, o_cnt, o_st = oix.search_batch(qh, k, hit["ef_search"], threads=threads)
        cpu_s = time.perf_counter() - t1
        g_ids = ls.bufs[0][0].cpu().numpy().astype(np.uint64)
        hit["cpu_oracle"] = {"qps": round(b / cpu_s, 1), "cores": threads, "ids_equal_oracle": bool((g_ids == o_ids).all()),
                             "score_bits_equal_oracle": bool((ls.bufs[0][1].cpu().numpy().view(np.uint32) == o_sc.view(np.uint32)).all())}
        out["iso_recall"] = hit
        del oix
    ls.close_forks()
    st["ix"].close()
    if st["ix_truth"] is not st["ix"]:
        st["ix_truth"].close()
    torch.cuda.empty_cache()
    return out


def run_config5_sharded(hv, synth, shard, args, dev, dist, rank, world):
    """configs[4] as written: every rank holds one id-range shard of fp8-e4m3 rows and scans it exactly for the whole 4096-query
    batch; ONE all-gather of the packed per-shard top-k (+ status) and the merge by Candidate order happen inside the same
    C-ABI call.  Weak sizing: --c5-rows per GPU."""
    rows, b, k, dim = args.c5_rows, 4096, 10, 1536
    x, q = synth.corpus("embedding", rows, dim, b, 20260924, dev, latent=24, clusters=4096)   # every shard draws the same rows: ids differ
    ids = np.arange(rows, dtype=np.uint64) + np.uint64(rank * rows)
    t0 = time.time()
    ix = hv.ValidatedVectorReadIndex.managed(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids, vectors=x, l0_offsets=np.zeros(rows + 1, np.uint64),
                                             l0_neighbors=np.zeros(0, np.uint64), device=dev.index, max_batch=b, dtype=hv.FP8_E4M3)
    del x
    torch.cuda.empty_cache()
    t_imp = time.time() - t0
    out = out_buffers(b, k, dev)
    grp = None
    exchange = "single GPU"
    if world > 1 and not SHARED_GPU:
        t = torch.zeros(128, dtype=torch.uint8, device=dev)
        if rank == 0:
            t.copy_(torch.frombuffer(bytearray(hv.ShardGroup.unique_id()), dtype=torch.uint8))
        dist.broadcast(t, 0)
        grp = hv.ShardGroup(ix, bytes(t.cpu().numpy().tobytes()), rank, world, b, k)
        exchange = "hvx_shard_group_flat_search_batch_device: scan + in-library ncclAllGather (RCCL) + merge, one C-ABI call per step"
    elif world > 1:
        ss = shard.ShardedSearcher(ix, world, b, k, dev, None, stage_through_host=True)
        exchange = "torch.distributed all_gather (gloo, host staged: plumbing run on one GPU) + hvx_merge_topk_packed_device"

    def step():
        if grp is not None:
            grp.flat_search_batch_device(q, k, out[0], out[1], out[2], out[3])
        elif world > 1:
            li, ls, lc = ss.outputs()
            ix.flat_search_batch_device(q, k, li, ls, lc, out[3])
            m = ss.merge(li, ls, lc)
            out[0].copy_(m[0]); out[1].copy_(m[1]); out[2].copy_(m[2])
        else:
            ix.flat_search_batch_device(q, k, out[0], out[1], out[2], out[3])

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    steps, warmup = max(1, min(args.steps, 10)), max(1, min(args.warmup, 2))
    for _ in range(warmup):
        step()
    ix.sync()
    barrier()
    t1 = time.perf_counter()
    for _ in range(steps):
        step()
    ix.sync()
    barrier()
    elapsed = time.perf_counter() - t1
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if SHARED_GPU else dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt[0].item())
    assert int(out[3].abs().sum().item()) == 0, "a query was rejected"
    ms = elapsed * 1e3 / steps
    useful = 2.0 * b * rows * dim   # per GPU
    res = {"metric": "exact-scan queries/s, configs[4] (100M x 1536 fp8 over 8 GPUs, batch 4096): every query answered over ALL shards",
           "value": round(b * steps / elapsed, 1), "unit": "queries/s", "n_gpus": world, "steps": steps, "warmup": warmup,
           "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "fp8-e4m3 rows, f32 re-rank",
           "data": "synthetic",
           "config": {"workload": f"configs[4]: {rows}x{dim} fp8-e4m3 rows per GPU ({rows * world} in all), exact kNN k={k}, batch {b}, squared-L2",
                      "rows_per_gpu": rows, "rows_total": rows * world, "exchange": exchange},
           "roofline": {"bound": "mfma", "achieved": round(useful / ms / 1e9, 1), "peak": MFMA_BF16_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(useful / ms / 1e9 / MFMA_BF16_TFLOPS, 4),
                        "note": "per GPU: ALGORITHMIC flops 2*b*rows_per_gpu*dim over the whole step (scan + exchange + merge)"},
           "import_seconds": round(t_imp, 1)}
    if grp is not None:
        grp.close()
    ix.close()
    return res


def leg_graph_equivalence(hv, synth, args, dev, which="embedding"):
    """The builder behind the benchmark graphs vs the reference's sequential insert_hnsw (oracle restatement), same 100 000 x 768
    rows, queries and levels: tests/golden/graph_equivalence_ref[_clustered].json hold the oracle side.  `clustered` (round 4): SURVEY
    8(d)'s clustered variant -- the ef sweep 128 / 256 / 800 and the connected components of layer 0 side by side say whether the
    recall plateau of that corpus is insert_hnsw's or the device builder's."""
    clustered = which == "clustered"
    ref_path = os.path.join(ROOT, "tests", "golden", "graph_equivalence_ref_clustered.json" if clustered else "graph_equivalence_ref.json")
    if not os.path.exists(ref_path):
        return {"error": f"{ref_path} missing (python tests/golden/make_graph_equivalence_ref.py{' clustered' if clustered else ''})"}
    ref = json.load(open(ref_path))
    n, dim, nq, k, ef = ref["n"], ref["dim"], ref["queries"], ref["k"], ref["ef"]
    if clustered:
        xh, qh = synth.clustered_np(n, dim, nq, 20260926, centres=128, sigma=0.15)
    else:
        xh, qh = synth.embedding_like_np(n, dim, nq, 20260925)
    lv = synth.draw_levels(n, args.m, 11)
    x = torch.from_numpy(xh).to(dev)
    torch.cuda.synchronize()
    t0 = time.time()
    if args.builder == "bulk":
        g = synth.build_hnsw_graph(x, m=args.m, m0=2 * args.m, levels=lv)
        g["m"] = args.m
        ix = import_index(hv, x, g, hv.EUCLIDEAN, hv.F32, nq, dev.index)
        bname = "pyhvx.synth.build_hnsw_graph (exact kNN candidates -> select_diverse -> reverse edges, degree cap)"
    else:
        ix, _ = hv.ValidatedVectorReadIndex.build(dim=dim, metric=hv.EUCLIDEAN, node_ids=np.arange(n, dtype=np.uint64), vectors=x, levels=lv,
                                                  m=args.m, m0=2 * args.m, ef_construction=200, max_batch=args.build_batch, batch_divisor=32,
                                                  device=dev.index, search_max_batch=nq)
        ix.sync()
        g = ix.export_graph()
        bname = f"hvx_index_build (device insert_hnsw, batches <= {args.build_batch}, same levels as the reference side)"
    build_s = time.time() - t0
    tid, _, _, _ = ix.flat_search_batch(qh, k)

    def at(ef_):
        ids, sc, cnt, st = ix.search_batch(qh, hv.SearchParams(k).with_ef(ef_))
        rec = sum(len(set(ids[i].tolist()) & set(tid[i].tolist())) for i in range(nq)) / float(nq * k)
        return rec, st

    rec, st = at(ef)
    deg = np.diff(g["l0_offsets"].astype(np.int64))
    mine = {"builder": bname, "build_seconds": round(build_s, 2),
            "recall_at_10": round(rec, 4), "distance_computations_per_query": round(st["distance_computations"] / nq, 1),
            "expansion_steps_per_query": round(st["expansion_steps"] / nq, 1), "degree_mean": round(float(deg.mean()), 2),
            "degree_histogram": np.bincount(deg, minlength=2 * args.m + 1).tolist()}
    keys = ("recall_at_10", "distance_computations_per_query", "expansion_steps_per_query", "degree_mean")
    ref_keys = ("builder",) + keys + ("degree_histogram", "build_seconds_one_core")
    if "ef_sweep" in ref:  # the beam-width curve and the component structure, both sides
        sweep = []
        for row in ref["ef_sweep"]:
            r_, s_ = at(row["ef"])
            sweep.append({"ef": row["ef"], "recall_at_10": round(r_, 4), "distance_computations_per_query": round(s_["distance_computations"] / nq, 1)})
        mine["ef_sweep"] = sweep
        mine["layer0_components"] = synth.layer0_components(g["l0_offsets"], g["l0_neighbors"], np.arange(n, dtype=np.uint64), g["entry_point"])
        mine["audit"] = graph_audit(ix, args.m)
        ref_keys = ref_keys + ("ef_sweep", "layer0_components")
    ix.close()
    out = {"corpus": ref["corpus"], "n": n, "dim": dim, "queries": nq, "ef": ef, "k": k,
           "reference_insert_hnsw": {kk: ref[kk] for kk in ref_keys},
           "bench_builder": mine,
           "relative_difference": {kk: round((mine[kk] - ref[kk]) / ref[kk], 4) for kk in keys},
           "note": "reference side computed by tests/golden/make_graph_equivalence_ref.py (CPU oracle, committed); bench side live on this GPU"}
    if clustered:
        r800 = [r_["recall_at_10"] for r_ in ref["ef_sweep"] if r_["ef"] == 800][0]
        m800 = [r_["recall_at_10"] for r_ in mine["ef_sweep"] if r_["ef"] == 800][0]
        out["plateau"] = {"reference_recall_ef128_to_ef800": [ref["ef_sweep"][0]["recall_at_10"], r800],
                          "bench_builder_recall_ef128_to_ef800": [mine["ef_sweep"][0]["recall_at_10"], m800],
                          "reading": "recall barely moves from ef 128 to ef 800 on the graph the REFERENCE's insert_hnsw builds over these rows, and the "
                                     "device builder's graph behaves the same: the plateau of the clustered corpus is the algorithm's, not a builder defect"}
    return out


# ------------------------------------------------------------------------------------------------------------
def cpu_quota():
    """CPU cores this process may actually use: the cgroup v2 quota when there is one (the GPU boxes of this pool: cpu.max =
    "1600000 100000" = 16 cores of 256 logical CPUs -- a 64-thread oracle run is throttled to 16 cores' worth and every thread of
    the process is frozen for the rest of the 100 ms period when the quota is spent), else the logical CPU count."""
    n = os.cpu_count() or 1
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = max(1, min(n, int(int(quota) / int(period))))
    except Exception:
        pass
    return n


def host_threads(args):
    return args.cpu_threads or min(cpu_quota(), 64)


def leg_batcher(x_host, q_host, g, m, callers=1024, per_caller=300, lanes=3):
    """SURVEY 8f-4 on the headline corpus and graph: `callers` OS threads each issuing single-query hvx_batcher_search calls in a closed
    loop (the reference's one-search-per-operator-call pattern, access/search/storage.rs:140-163).  The callers are a C++ harness
    (scripts/bench_batcher.cpp, compiled here) in its own process: Python threads would measure the GIL.  The harness reads the
    container's cgroup cpu.stat around its timed run (the pool's 16-core quota decides this number as much as the GPU does)."""
    import shutil, subprocess, tempfile
    root = os.path.dirname(os.path.abspath(__file__))
    d = tempfile.mkdtemp(prefix="hvx_batcher_", dir="/tmp")
    try:
        n, dim = x_host.shape
        np.array([n, dim, m, g["entry_point"], g["max_layer"]], np.uint64).tofile(f"{d}/meta.u64")
        np.asarray(g["node_ids"], np.uint64).tofile(f"{d}/ids.u64")
        np.ascontiguousarray(x_host, np.float32).tofile(f"{d}/vectors.f32")
        np.ascontiguousarray(q_host, np.float32).tofile(f"{d}/queries.f32")
        for name in ("l0_offsets", "l0_neighbors", "up_offsets", "up_neighbors"):
            np.asarray(g[name], np.uint64).tofile(f"{d}/{name}.u64")
        np.asarray(g["level"], np.uint16).tofile(f"{d}/level.u16")
        exe = f"{d}/bench_batcher"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(root, "include"), os.path.join(root, "scripts", "bench_batcher.cpp"), "-o", exe,
                               "-L", os.path.join(root, "helix-db_amd"), "-lhelix_vec_gfx950", f"-Wl,-rpath,{os.path.join(root, 'helix-db_amd')}", "-lpthread"])
        env = dict(os.environ, BATCHER_WAIT="200")

        def one(arm, lanes_, extra_env):
            r = subprocess.run([exe, d, str(callers), str(per_caller), arm, str(lanes_), "nodirect"], capture_output=True, text=True, timeout=240,
                               env=dict(env, **extra_env))
            if r.returncode != 0:
                return {"error": (r.stderr or r.stdout)[-400:]}
            line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
            o = {"qps": line["batcher"]["qps"], "mean_us": line["batcher"]["mean_us"], "p99_us": line["batcher"]["p99_us"], "mean_batch": line["batcher"]["mean_batch"],
                 "lanes": lanes_}
            for l in r.stderr.splitlines():
                if l.startswith("timed run:"):
                    o["host"] = l[len("timed run: "):]
                elif l.startswith("lane time shares"):
                    o["lane_times"] = l
            return o

        res = one("strict", lanes, {})
        if "error" in res:
            return res
        res["workload"] = (f"{n}x{dim} f32 (the headline corpus and graph), strict ef=100 k=10, {callers} caller threads x {per_caller} single-query "
                           f"hvx_batcher_search calls, {lanes} dispatcher lanes, max_wait_us 200")
        # the arm /v2/query actually runs (SearchParams::new(k), access/search/storage.rs:140-141): lanes on the two-per-SIMD build (round 5)
        pd = one("default", 4, {"BATCHER_OCC": "2"})
        res["production_default"] = pd
        res["qps_production_default"] = pd.get("qps")
        # the non-blocking form (round 5): 8 submitter threads x 128 tickets in flight, asleep in poll(2) on the batcher's eventfd
        nb = one("strict", lanes, {"BATCHER_NB": "8x128"})
        nb["how"] = "hvx_batcher_submit / hvx_batcher_poll + eventfd, 8 submitter threads x 128 tickets in flight (1 024 queries in flight, as the blocking run)"
        res["nonblocking"] = nb
        res["qps_nonblocking"] = nb.get("qps")
        # ... and the production-default arm the same way with 2 048 queries in flight (tickets cost no threads)
        nbd = one("default", 4, {"BATCHER_OCC": "2", "BATCHER_NB": "8x256"})
        nbd["how"] = "SearchParams::new(10), hvx_batcher_submit / _poll + eventfd, 8 submitter threads x 256 tickets in flight, 4 lanes, two queries per SIMD"
        res["nonblocking_production_default"] = nbd
        res["qps_nonblocking_production_default"] = nbd.get("qps")
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


# ------------------------------------------------------------------------------------------------------------
# the line the driver parses
# ------------------------------------------------------------------------------------------------------------
def _finite(o):
    """strict JSON: non-finite floats become null (json.dumps(..., allow_nan=False) would raise on them)"""
    if isinstance(o, float):
        return o if o == o and o not in (float("inf"), float("-inf")) else None
    if isinstance(o, dict):
        return {str(k): _finite(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_finite(v) for v in o]
    if isinstance(o, (np.floating,)):
        return _finite(float(o))
    if isinstance(o, (np.integer,)):
        return int(o)
    if isinstance(o, (np.bool_,)):
        return bool(o)
    return o


def _pick(d, *keys):
    """d[k0][k1]... or None"""
    for k in keys:
        if not isinstance(d, dict) or k not in d:
            return None
        d = d[k]
    return d


COMPACT_LIMIT = 4096


def compact_record(out, full_path):
    """The <= 4 KB line: the contract's keys + roofline + cpu_baseline + parity, and one short object per extra leg.  Everything it
    summarises is in the full record under the same top-level key."""
    rf = out.get("roofline") or {}
    c = {k: out.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                                 "dtype", "data")}
    cfg = out.get("config") or {}
    c["config"] = {k: cfg.get(k) for k in ("workload", "dataset", "rows_per_gpu", "rows_total", "dim", "batch", "k", "ef_search", "lanes", "parallelism",
                                           "rccl_ranks", "rccl_version") if cfg.get(k) is not None}
    c["recall_at_10"] = out.get("recall_at_10")
    if out.get("timed_runs", 1) != 1:
        c["timed_runs"] = out.get("timed_runs")
        c["host_stall_in_first_run"] = out.get("host_stall_in_first_run")
    c["roofline"] = {k: rf.get(k) for k in ("bound", "kernel", "achieved", "peak", "peak_measured", "unit", "frac", "frac_of_measured",
                                            "algorithmic_bytes_per_launch", "kernel_ms", "kernel_ms_each", "traffic", "traffic_source")}
    c["roofline"]["frac_definition"] = f"overlapped span, {rf.get('lanes')} lanes x {rf.get('queries_per_simd')} per SIMD; alone: lone_batch_frac"
    if isinstance(c["roofline"].get("traffic_source"), str):   # (the full sentence stays in the full record)
        c["roofline"]["traffic_source"] = c["roofline"]["traffic_source"].split(";")[0].replace(" --kernel-trace pass of the headline leg", " pass")[:100]
    lb = rf.get("lone_batch") or {}
    if lb:
        c["roofline"]["lone_batch_frac"] = lb.get("frac")
    cb = out.get("cpu_baseline")
    if cb:
        c["cpu_baseline"] = {k: cb.get(k) for k in ("value", "unit", "cores", "threads", "nproc", "quota_cores", "kind", "sample")}
        if isinstance(c["cpu_baseline"].get("sample"), str):
            c["cpu_baseline"]["sample"] = c["cpu_baseline"]["sample"].split("; median")[0][:100]
    if out.get("parity"):
        c["parity"] = {k: out["parity"].get(k) for k in ("queries", "ids_equal_oracle", "score_bits_equal_oracle")}
    if out.get("strong_scaling"):
        c["strong_scaling"] = {k: out["strong_scaling"].get(k) for k in ("rows_total", "rows_per_gpu", "qps", "ms_per_step", "recall_at_10")}
    pl = out.get("production_default_lanes")
    if isinstance(pl, dict):
        c["production_default_lanes"] = {m: ({k: v.get(k) for k in ("qps", "ms_per_step", "frac", "recall_at_10", "ids_equal_oracle", "score_bits_equal_oracle")}
                                             if isinstance(v, dict) and "error" not in v else v) for m, v in pl.items() if m in ("l2", "cosine", "error")}
    ds = out.get("datasets")
    if isinstance(ds, dict):
        d2 = {}
        for name in ("clustered", "gaussian", "embedding"):
            r = ds.get(name)
            if isinstance(r, dict):
                d2[name] = ({"error": str(r["error"])[:120]} if "error" in r else
                            {"qps": r.get("qps"), "recall_at_10": r.get("recall_at_10"), "frac": _pick(r, "roofline", "frac"), "clears_0.95": r.get("clears_recall_0.95")})
        iso = ds.get("clustered_iso_recall")
        if isinstance(iso, dict) and "clustered" in d2:
            hit = iso.get("iso_recall")
            d2["clustered"]["iso_recall"] = None if not hit else {"ef_search": hit.get("ef_search"), "qps": hit.get("qps"), "recall_at_10": hit.get("recall_at_10")}
        c["datasets"] = d2
    el = out.get("embedding_latent")
    if isinstance(el, dict):
        rows_ = {"16": {"ef_search": _pick(out, "config", "ef_search"), "qps": out.get("value"), "recall_at_10": out.get("recall_at_10"), "frac": _pick(out, "roofline", "frac")}}
        for L_, r_ in el.items():
            hit = r_.get("iso_recall") if isinstance(r_, dict) else None
            first = (r_.get("sweep") or [{}])[0] if isinstance(r_, dict) else {}
            rows_[L_] = ({"error": str(r_.get("error"))[:80]} if isinstance(r_, dict) and "error" in r_ else
                         {"recall_at_ef128": first.get("recall_at_10"), "iso": None if not hit else
                          {"ef_search": hit.get("ef_search"), "qps": hit.get("qps"), "recall_at_10": hit.get("recall_at_10"), "frac": hit.get("frac_of_hbm_peak")}})
        c.setdefault("datasets", {})["embedding_latent"] = rows_
    c3 = out.get("config3_prefilter")
    if isinstance(c3, dict):
        if "error" in c3:
            c["config3"] = {"error": str(c3["error"])[:160]}
        else:
            # groups: plan / recall / us_per_q / p50_1q_ms = the DEVICE plan (HVX_RESTRICTED_AUTO); ref_* = the reference's plan on the same rows
            c["config3"] = {"corpus": _pick(c3, "corpus", "kind"), "parity_ok": c3.get("parity_sample_ok"),
                            "groups": [{"candidates": g_["candidates"], "plan": _pick(g_, "device_plan", "strategy"),
                                        "recall": _pick(g_, "device_plan", "recall_at_10_vs_exact"),
                                        "us_per_q": _pick(g_, "device_plan", "us_per_query"),
                                        "p50_1q_ms": _pick(g_, "device_plan", "single_query_end_to_end_ms", "p50"),
                                        "ref_plan": _pick(g_, "planned", "strategy"), "ref_recall": _pick(g_, "planned", "recall_at_10_vs_exact"),
                                        "ref_us_per_q": _pick(g_, "planned", "us_per_query"),
                                        "hbm_frac": None if _pick(g_, "exact", "hbm_gbs_scan") is None else round(_pick(g_, "exact", "hbm_gbs_scan") / HBM_PEAK_GBS, 3)}
                                       for g_ in c3.get("groups", [])],
                            "own_sets": [{"req": r_["requests"], "ids": r_["ids_per_request"], "qps": r_["qps_kernel"], "frac": r_["frac_of_hbm_peak"]}
                                         for r_ in (_pick(c3, "per_request_candidate_sets", "rows") or [])]}
    c4 = out.get("config4_bf16")
    if isinstance(c4, dict):
        c["config4"] = {"error": str(c4["error"])[:160]} if "error" in c4 else {
            "qps": c4.get("qps"), "recall_at_10": c4.get("recall_at_10"), "frac": _pick(c4, "roofline", "frac"),
            "ids_equal_oracle": _pick(c4, "parity_sample", "ids_equal_oracle")}
    c5 = out.get("config5_fp8_flat")
    if isinstance(c5, dict):
        c["config5"] = {"error": str(c5["error"])[:160]} if "error" in c5 else {
            "rows": c5.get("rows"), "ms_per_batch": c5.get("ms_per_batch"), "tflops": _pick(c5, "roofline", "achieved"),
            "frac_of_fp8_peak": _pick(c5, "roofline", "frac_of_fp8_peak"), "frac_of_bf16_peak": _pick(c5, "roofline", "frac"),
            "vendor_gemm_tflops": _pick(out, "vendor_gemm", "fp8", "tflops"), "bit_exact_full_scan": c5.get("oracle_bit_exact_full_scan")}
    es = out.get("exact_scan")
    if isinstance(es, dict):
        c["exact_scan"] = {"ms": es.get("ms"), "tflops": _pick(es, "roofline", "achieved"), "frac_of_bf16_peak": _pick(es, "roofline", "frac"),
                           "vendor_gemm_tflops": _pick(out, "vendor_gemm", "bf16", "tflops")}
    ii = out.get("incremental_insert")
    if isinstance(ii, dict):
        c["insert"] = {"error": str(ii["error"])[:160]} if "error" in ii else {
            "batched_inserts_per_s": _pick(ii, "batched", "inserts_per_s"), "sequential_us_per_insert": _pick(ii, "sequential", "us_per_insert"),
            "audit_clean": _pick(ii, "audit", "clean"), "recall_at_10": next((v for k_, v in ii.items() if k_.startswith("recall_at_10")), None),
            "delete_us": _pick(ii, "deletes", "us_per_delete"),
            "recall_after_deletes": next((v for k_, v in (ii.get("deletes") or {}).items() if k_.startswith("recall_at_10")), None),
            "deleted_ids_in_results": _pick(ii, "deletes", "deleted_ids_in_results"), "upsert_us": _pick(ii, "upserts", "us_per_upsert")}
    bt = out.get("batcher")
    if isinstance(bt, dict):
        c["batcher"] = {"error": str(bt["error"])[:160]} if "error" in bt else {k: bt.get(k) for k in ("qps", "mean_us", "p99_us", "mean_batch", "qps_production_default",
                                                                                                       "qps_nonblocking", "qps_nonblocking_production_default")}
    if out.get("deadline"):
        c["deadline"] = {"seconds": out["deadline"].get("seconds")}
    c["full_record"] = full_path
    c = _finite(c)
    line = json.dumps(c, allow_nan=False, separators=(",", ":"))
    # a leg that grew must never cost the line its contract: drop summaries (never the contract keys) until it fits
    for victim in ("insert", "batcher", "exact_scan", "config4", "config5", "config3", "datasets", "production_default_lanes", "strong_scaling"):
        if len(line) < COMPACT_LIMIT:
            break
        if victim in c:
            c[victim] = "see full_record"
            line = json.dumps(c, allow_nan=False, separators=(",", ":"))
    return line


def emit(out, full_path, rank=0):
    """full record -> file (+ stderr), compact line -> the LAST line of stdout"""
    if rank != 0:
        return
    full = _finite(out)
    written = None
    for path in (full_path, os.path.join(ROOT, "gpurun_out", "bench_full.json")):
        try:
            if os.path.isdir(os.path.dirname(path)):
                with open(path, "w") as f:
                    json.dump(full, f, allow_nan=False)
                written = written or path
        except OSError as e:
            log(f"could not write {path}: {e}")
    line = compact_record(out, written)
    sys.stderr.flush()
    print(line, flush=True)


def start_deadline(out, seconds, rank, full_path):
    """The extra legs (other corpora, configs 3-5, graph equivalence, CPU baseline) must never cost the headline: once the
    headline object exists, a daemon thread prints it -- with the legs that have finished by then -- when the deadline passes,
    and ends the process."""
    import threading

    def fire():
        for _ in range(20):
            try:
                snap = dict(out)
                snap["deadline"] = {"seconds": seconds, "note": "printed by the deadline watchdog: legs absent from this record had not finished"}
                emit(snap, full_path, rank)
                break
            except RuntimeError:  # the main thread added a key while we copied
                time.sleep(0.05)
        log(f"deadline of {seconds:.0f}s reached: line printed with the legs finished so far")
        sys.stderr.flush()
        os._exit(0)

    t = threading.Timer(seconds, fire)
    t.daemon = True
    t.start()
    return t


def main():
    if os.environ.get("BENCH_TRACE"):  # where is it? (python stacks of all threads every N seconds, to stderr)
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["BENCH_TRACE"]), repeat=True)
    t_start = time.time()
    args = parse()
    # torch's CPU helpers (tensor copies, numpy conversions) would start one thread per logical CPU: under a cgroup quota that burst
    # alone freezes the process for the rest of the scheduler period -- in the middle of a timed section
    torch.set_num_threads(max(1, min(8, cpu_quota())))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = 0 if SHARED_GPU else int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus and world == 1 and args.gpus > 1:
        raise SystemExit("launch with: python -m torch.distributed.run --nproc-per-node N bench.py --gpus N ...")
    import pyhvx  # hvx_runtime_prepare (pyhvx.lib) must run before the HIP runtime initialises
    pyhvx.lib()
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback exists for the product path)")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if SHARED_GPU:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
    import pyhvx as hv
    from pyhvx import shard, synth
    hv.lib()
    skip = set(s for s in args.skip.split(",") if s)

    if args.leg == "config5" and args.dump_outputs:
        raise SystemExit("--dump-outputs writes the headline leg's answer; --leg config5 has none")
    if args.leg == "config5":
        res = run_config5_sharded(hv, synth, shard, args, dev, dist, rank, world)
        emit(res, args.full_record, rank)
        if world > 1:
            dist.destroy_process_group()
        return

    dim, b, k, ef = args.dim, args.batch, args.k, args.ef
    bf16 = args.dtype == "bf16"
    cosine = args.metric == "cosine"
    hv_metric = hv.COSINE if cosine else hv.EUCLIDEAN
    replica = args.mode == "replica" and world > 1
    lanes = max(1, args.lanes)
    occ = args.occupancy or (2 if lanes > 1 else 1)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def shard_run(n_total, label, dump=False):
        """One sharded (or single-GPU) measurement over a corpus of n_total rows; returns (result dict, state).  dump: write the
        last timed step's answer under --dump-outputs."""
        t0 = time.time()
        n = n_total if replica else n_total // world
        nbq = query_batches(args, b)
        nq_total = (b * world if replica else b) * nbq
        # every rank draws the same global corpus from the same seed and keeps its id-range shard
        xg, q_all = synth.corpus(args.dataset, n_total, dim, nq_total, args.seed, dev)
        if cosine:  # unit rows: the L2-built graph is the cosine graph (same neighbour order)
            xg = torch.nn.functional.normalize(xg, dim=1)
            q_all = torch.nn.functional.normalize(q_all, dim=1)
        id_lo = 0 if replica else rank * n
        if replica:  # every replica answers its own batches
            q_all = q_all.view(nbq, world, b, dim)[:, rank].contiguous().view(nbq * b, dim)
        qs = [q_all[j * b:(j + 1) * b] for j in range(nbq)]
        x = xg[id_lo:id_lo + n].contiguous()
        del xg
        if bf16:
            x = x.to(torch.bfloat16).to(torch.float32)
        torch.cuda.synchronize()
        log(f"[{label}] corpus {n_total}x{dim} generated in {time.time() - t0:.1f}s; shard rows [{id_lo},{id_lo + n})")
        g, ginfo, bix = build_graph(hv, synth, args, x, hv_metric, id_lo, b, local_rank, 7 + rank, keep_index=not bf16)
        log(f"[{label}] graph: {ginfo}")
        t0 = time.time()
        ix = bix if bix is not None else import_index(hv, x, g, hv_metric, hv.BF16 if bf16 else hv.F32, b, local_rank)
        ix_truth = ix
        if bf16:  # (a plain run makes it too: HIP assigns hardware queues in stream creation order, so the lanes get the queues of --full)
            ix_truth = hv.ValidatedVectorReadIndex.managed(
                dim=dim, metric=hv_metric, node_ids=g["node_ids"], vectors=x, l0_offsets=np.zeros(n + 1, np.uint64),
                l0_neighbors=np.zeros(0, np.uint64), device=local_rank, max_batch=b)
        log(f"[{label}] index imported in {time.time() - t0:.1f}s")
        sharded = world > 1 and not replica
        group = None

        def factory(h):
            return shard.ShardedSearcher(h, world, b, k, dev, group, stage_through_host=SHARED_GPU)

        ls = LaneSet(ix, lanes, occ, b, k, dev, factory if sharded else None)
        exchange = "single GPU"
        if sharded:
            exchange = "torch.distributed all_gather_into_tensor + hvx_merge_topk_packed_device"
            if not SHARED_GPU and args.exchange == "capi":
                try:
                    ls.use_shard_groups(hv, dist, rank, world)
                    exchange = "hvx_shard_group_search_batch_device: in-library ncclAllGather (RCCL) + merge, one C-ABI call per step"
                except Exception as e:  # RCCL could not be bootstrapped from inside the library: the torch.distributed exchange still works
                    log(f"[{label}] hvx_shard_group_init failed ({e}); falling back to the torch.distributed exchange")
                    ls.groups = None
            ok = torch.tensor([1 if ls.groups else 0], dtype=torch.int32, device="cpu" if SHARED_GPU else dev)
            dist.all_reduce(ok, op=dist.ReduceOp.MIN)  # every rank must take the same path
            if int(ok.item()) == 0 and ls.groups:
                for gq in ls.groups:
                    gq.close()
                ls.groups = None
                exchange = "torch.distributed all_gather_into_tensor + hvx_merge_topk_packed_device"
        elapsed, span, kms = timed_steps(ls, qs, ef, args.steps, args.warmup, barrier)
        timed_runs, stall = 1, None
        if world == 1 and elapsed * 1e3 > 1.3 * span:
            # the wall clock of the K steps is far above the device span of the same K kernels: the host was frozen inside the timed region
            # (CPU quota, see timed_steps).  The SAME K steps are timed once more; both runs are reported, the line carries the second.
            stall = {"first_run_qps": round(b * args.steps / elapsed, 1), "first_run_ms_per_step": round(elapsed * 1e3 / args.steps, 4), "first_run_kernel_ms": round(span / args.steps, 4),
                     "first_run_host": getattr(ls, "host_timing", None)}
            log(f"[{label}] host stall inside the timed steps ({stall}); timing the same {args.steps} steps again")
            elapsed, span, kms = timed_steps(ls, qs, ef, args.steps, args.warmup, barrier)
            timed_runs = 2
        dumped = dump_outputs(ls, args.steps, args.dump_outputs) if dump and args.dump_outputs and rank == 0 else None
        q = ls.last_q[0]  # lane 0's last batch: recall, counters and the oracle check below refer to it
        if world > 1:
            t = torch.tensor([elapsed, span], dtype=torch.float64, device="cpu" if SHARED_GPU else dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed, span = float(t[0].item()), float(t[1].item())
        qps = b * args.steps / elapsed * (world if replica else 1)
        if not args.full:  # the headline figure is complete: recall, counters and the checks below are --full's
            assert int(ls.bufs[0][3].abs().sum().item()) == 0, "a query was rejected"
            return (dict(timed_runs=timed_runs, host_stall=stall, qps=qps, ms_per_step=elapsed * 1e3 / args.steps, n=n, n_total=n_total,
                         exchange=exchange, nbq=nbq), dict(ix=ix, ix_truth=ix_truth, ls=ls))
        # recall@k against the exact scan (itself bit-exact vs the oracle's flat scan, tests/test_gpu_parity.py)
        f = out_buffers(b, k, dev)
        ix_truth.flat_search_batch_device(q, k, *f[:4])  # first use loads the scan's code objects: not timed
        flat_stats = ix_truth.flat_search_batch_device(q, k, *f[:4], want_stats=True)
        got = ls.bufs[0]
        if sharded and ls.groups:
            ls.sync()
            got_ids = ls.merged[0][0].clone()
            truth_ids = ls.sharded[0].merge(f[0], f[1], f[2])[0].clone()
            # per-shard counters of the last step: one more local search into the lane's own buffers
            ix.search_batch_device(q, k, ef, *got, want_stats=False)
            ix.sync()
        elif sharded:
            ix.sync()
            got_ids = ls.sharded[0].merge(got[0], got[1], got[2])[0].clone()   # the lane's buffers ARE the payload views: merge them first,
            truth_ids = ls.sharded[0].merge(f[0], f[1], f[2])[0].clone()       # then let the exact-scan lists overwrite the payload
        else:
            got_ids, truth_ids = got[0], f[0]
        torch.cuda.synchronize()
        recall = recall_of(got_ids, truth_ids, b, k)
        assert int(got[3].abs().sum().item()) == 0, "a query was rejected"
        qst = got[4].cpu().numpy().astype(np.int64)
        alg = hnsw_alg_bytes(qst, dim, 2 if bf16 else 4, b)
        per_step = span / args.steps
        res = dict(timed_runs=timed_runs, host_stall=stall, host_timing=getattr(ls, "host_timing", None), qps=qps, ms_per_step=elapsed * 1e3 / args.steps, recall=recall, alg=alg, per_step=per_step, kms=kms, qst=qst, n=n,
                   n_total=n_total, flat_ms=flat_stats["device_ms"], graph=ginfo, exchange=exchange, nbq=nbq, dumped=dumped)
        state = dict(ix=ix, ix_truth=ix_truth, ls=ls, x=x, q=q, g=g, truth=f, id_lo=id_lo, qs=qs)
        return res, state

    def headline(res, ls):
        """the contract keys and the configuration of the headline measurement: a plain run's line, and the head of --full's record"""
        n = res["n"]
        return {
            "metric": "QPS @ recall@10>=0.95, 1Mx768 fp32; achieved HBM GB/s vs roofline", "value": round(res["qps"], 1),
            "unit": "queries/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(res["ms_per_step"], 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "f32" if not bf16 else "f32 arithmetic on bf16 rows", "data": "synthetic",
            "config": {"workload": f"configs[1]: {n}x{dim} {args.dtype} per GPU, HNSW M={args.m}/M0={2 * args.m} ef_search={ef} k={k}, "
                                   f"batch={b} queries, {'cosine' if cosine else 'squared-L2'}, strict-exhaustive beam (bit-exact vs reference CPU path), "
                                   f"steps issued round-robin on {lanes} execution lanes",
                       "dataset": args.dataset, "rows_per_gpu": n, "rows_total": res["n_total"], "dim": dim, "batch": b, "k": k,
                       "ef_search": ef, "lanes": lanes, "distinct_query_batches": res["nbq"],
                       "exchange": res["exchange"],
                       "rccl_ranks": (world if (world > 1 and ls.groups) else None), "rccl_version": (hv.rccl_version() if world > 1 else None),
                       "parallelism": ("1 GPU" if world == 1 else f"{world} replicas, one query batch each" if replica
                                       else f"id-range shards x{world} + all-gather top-k merge")}}

    n_weak_total = args.rows if replica else args.rows * world
    res, S = shard_run(n_weak_total, "weak" if world > 1 else "1 GPU", dump=True)
    if not args.full:
        out = headline(res, S["ls"])
        if res["timed_runs"] != 1:
            out.update(timed_runs=res["timed_runs"], host_stall_in_first_run=res["host_stall"])
        if rank == 0:
            sys.stderr.flush()
            print(json.dumps(_finite(out), allow_nan=False, separators=(",", ":")), flush=True)
        S["ls"].close_forks()
        S["ix"].close()
        if S["ix_truth"] is not S["ix"]:
            S["ix_truth"].close()
        if world > 1:
            dist.destroy_process_group()
        return
    ix, ls, q, g, x = S["ix"], S["ls"], S["q"], S["g"], S["x"]
    S_qs = S["qs"]
    headline_alive = True
    n = res["n"]
    qst = res["qst"]

    # ---- latency of ONE lone batch (nothing else on the device): a one-query-per-SIMD handle.  Round 4: such a handle runs the
    #      owner / gatherer kernel (two wavefronts per query, hvx_hnsw_pair.h); the one-wavefront kernel on the same handle is the A/B ----
    def lone_run(pair_opt):
        ix.set_option(hv.OPT_HNSW_PAIR, pair_opt)
        ms = []
        lbuf = out_buffers(b, k, dev)
        for it in range(14):
            st_ = ix.search_batch_device(q, k, ef, *lbuf, want_stats=True)
            if it >= 4:
                ms.append(st_["device_ms"])
        return float(np.mean(ms)), lbuf

    ix.set_occupancy(1)
    lone_ms, lone_buf = lone_run(0)
    pair1_ms, pair1_buf = lone_run(3)
    wave_ms, wave_buf = lone_run(1)
    lone_same = all(bool((lone_buf[0] == o[0]).all().item()) and bool((lone_buf[1].view(torch.int32) == o[1].view(torch.int32)).all().item())
                    and bool((lone_buf[4] == o[4]).all().item()) for o in (pair1_buf, wave_buf))
    ix.set_option(hv.OPT_HNSW_PAIR, 0)
    ix.set_occupancy(occ)

    # ---- the beam-width curve of the HEADLINE corpus and graph (round 4): ef 128 .. 800 on the same lanes; every row one wavefront per
    #      query (448 / 832-entry register beams above ef 352; rounds 1-3 sent those to the 4-wavefront general kernel) ----
    ef_sweep = None
    if world == 1 and "ef_sweep" not in skip:
        try:
            timed_steps(ls, S_qs, ef, 6, 3, lambda: None)  # (the first timed pass after the lone-batch loop carries a one-off ~45 ms: r04a)
            ef_sweep = ef_sweep_rows(ls, [qq for qq in S_qs], S["ix_truth"], dev, dim, b, k, (128, 192, 256, 384, 512, 800), elem=2 if bf16 else 4)
        except Exception as e:
            ef_sweep = {"error": f"{type(e).__name__}: {e}"}
        for l in range(lanes):  # the lanes' buffers answer the headline beam width again (the oracle check below reads them)
            ls.step(l, q if l == 0 else S_qs[l % len(S_qs)], ef)
        ls.sync()

    traffic = None
    if os.path.exists(args.traffic_file):
        try:
            traffic = json.load(open(args.traffic_file))
        except Exception:
            traffic = None
    traffic_source = "rocprofv3 --pmc pass of this command on another box (profiles/traffic_latest.json); not measured in this run"
    # the headline instantiation's name is what the pass filters on: only the configuration the metric is quoted on is measured live
    if ("traffic" not in skip and world == 1 and args.leg == "headline" and args.dataset == "embedding" and args.dim == 768 and args.metric == "l2" and
            args.dtype == "f32" and args.ef == 128 and args.k == 10 and occ == 2):
        live = measure_traffic_pass(args)
        if live:
            traffic = live
            traffic_source = (f"this run: child rocprofv3 --pmc FETCH_SIZE TCC_EA0_RDREQ_sum --kernel-trace pass of the headline leg ({live['dispatches']} launches, "
                              f"{live['seconds']} s); FETCH_SIZE KiB x 1024 x 2 (gfx950), cross-check TCC_EA0_RDREQ_sum x 128 B = {live['tcc_ea0_rdreq_x128B']}")
            log(f"traffic pass: {live}")
    achieved = res["alg"] / (res["per_step"] * 1e-3) / 1e9
    # BASELINE.md section 2 / SURVEY 8(d): the MEASURED streaming-read rate of this box next to the 8 TB/s spec -- a read-only
    # global_load_dwordx4 kernel over a 3 GiB buffer (hvx_device_stream_read_gbs, csrc/hvx_probe.hip), timed here, in this run
    peak_measured = None
    if "peak" not in skip:
        try:
            pk_best, pk_mean = hv.device_stream_read_gbs(local_rank, 3 << 30, 5)
            peak_measured = round(pk_best, 1)
            log(f"stream-read probe: best {pk_best:.0f} GB/s, mean {pk_mean:.0f} GB/s over 3 GiB")
        except Exception as e:
            log(f"stream-read probe failed: {e}")
    roofline = {"bound": "hbm", "kernel": "hnsw_wave_kernel", "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "peak_measured": peak_measured,
                "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                "frac_of_measured": None if not peak_measured else round(achieved / peak_measured, 4),
                "peak_measured_how": "hvx_device_stream_read_gbs: read-only 16-byte-load streaming kernel over 3 GiB of HBM, best of 5 launches, this run",
                "traffic": (traffic or {}).get("hbm_bytes_per_launch"),
                "traffic_source": traffic_source,
                "algorithmic_bytes_per_launch": int(res["alg"]),
                "algorithmic_bytes_of": "the per-query counters of lane 0's last batch (every timed step answers a different batch of the same distribution)",
                "frac_definition": f"overlapped span: {lanes} lanes x {occ} queries per SIMD in flight (algorithmic bytes of one launch / (HIP-event span of the "
                                   f"{args.steps} timed kernels / {args.steps})); one launch ALONE on the device: lone_batch.frac",
                "kernel_ms": round(res["per_step"], 4),
                "kernel_ms_definition": f"HIP-event span of the {args.steps} timed search kernels on their {lanes} lane streams / {args.steps} "
                                        f"(consecutive batches overlap on the device); kernel_ms_each = mean duration of one kernel "
                                        f"(what rocprofv3 --stats reports as AverageNs)",
                "kernel_ms_each": round(float(res["kms"].mean()), 4), "lanes": lanes, "queries_per_simd": occ,
                "residency": ls.residency,
                "lone_batch": {"kernel_ms": round(lone_ms, 4), "frac": round(res["alg"] / (lone_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                               "kernel": "hnsw_pair_kernel (an owner wavefront + three gatherer wavefronts per query)",
                               "one_gatherer": {"kernel_ms": round(pair1_ms, 4), "frac": round(res["alg"] / (pair1_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
                               "one_wavefront_kernel": {"kernel_ms": round(wave_ms, 4), "frac": round(res["alg"] / (wave_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)},
                               "ids_score_bits_counters_equal_between_the_kernels": lone_same,
                               "note": "one batch alone on the device, a one-query-per-SIMD handle (what a host that cannot keep several "
                                       "batches in flight -- or the batcher's small batches -- sees)"},
                "distance_computations_per_query": round(float(qst[:, 3].mean()), 1),
                "expansion_steps_per_query": round(float(qst[:, 0].mean()), 1),
                "per_query_distance_computations": {"p50": pct(qst[:, 3], 50), "p99": pct(qst[:, 3], 99), "max": int(qst[:, 3].max())},
                "per_query_expansion_steps": {"p50": pct(qst[:, 0], 50), "p99": pct(qst[:, 0], 99), "max": int(qst[:, 0].max())}}

    out = {
        **headline(res, ls),
        "recall_at_10": round(res["recall"], 4),
        "timed_runs": res["timed_runs"], "host_stall_in_first_run": res["host_stall"], "host_timing": res["host_timing"],
        "shard_searches_per_s": round(res["qps"] * (1 if replica else world), 1),
        "roofline": roofline,
        "flat_scan_ms": round(res["flat_ms"], 3),
        "exact_scan": {"workload": f"exact scan of the same {b} queries over the same {n}x{dim} f32 rows (the recall ground truth), k={k}",
                       "ms": round(res["flat_ms"], 3),
                       "roofline": {"bound": "mfma", "achieved": round(2.0 * b * n * dim / res["flat_ms"] / 1e9, 1), "peak": MFMA_BF16_TFLOPS,
                                    "unit": "TFLOP/s", "frac": round(2.0 * b * n * dim / res["flat_ms"] / 1e9 / MFMA_BF16_TFLOPS, 4),
                                    "note": "ALGORITHMIC flops 2*b*N*dim / time of the whole scan (bf16 shadow contraction on the matrix cores + "
                                            "filtered epilogue + exact f32 re-rank + certificate); bit-exact vs the oracle's exact scan"}},
        "graph_build": res["graph"],
        "ef_sweep": ef_sweep,
    }

    if args.deadline > 0:
        start_deadline(out, max(5.0, args.deadline - (time.time() - t_start)), rank, args.full_record)

    # ---- N > 1: the north star's own curve -- the SAME 1M corpus split over the GPUs (strong scaling) ----
    if world > 1 and not replica and args.scaling in ("strong", "both"):
        ls.close_forks()
        ix.close()
        if S["ix_truth"] is not ix:
            S["ix_truth"].close()
        S = ix = ls = x = q = None
        headline_alive = False
        torch.cuda.empty_cache()
        res_s, S2 = shard_run(args.rows, "strong")
        out["strong_scaling"] = {
            "rows_total": args.rows, "rows_per_gpu": res_s["n"], "qps": round(res_s["qps"], 1), "ms_per_step": round(res_s["ms_per_step"], 4),
            "recall_at_10": round(res_s["recall"], 4), "ef_search": ef, "mode": "iso-ef (every shard searched at the single-GPU ef; "
            "recall rises with the shard count because every shard contributes its own top-k)",
            "per_shard_roofline_frac": round(res_s["alg"] / (res_s["per_step"] * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
            "distance_computations_per_query_per_shard": round(float(res_s["qst"][:, 3].mean()), 1)}
        S2["ls"].close_forks()
        S2["ix"].close()
        del S2
        torch.cuda.empty_cache()

    if world == 1 and rank == 0:
        import orc
        x_host = None
        # ---- what the reference's query path actually runs: SearchParams::new(k) = ef max(k,100), SimHashMode::Adaptive
        #      (access/search/storage.rs:140-141), next to the strict arm at the same beam width ----
        prod = None
        prod_lanes = {}
        if not bf16 and "production" not in skip:
            prod = {}
            # the headline's forks are done (their buffers and last batches stay for the oracle check below): HIP maps streams onto
            # the process's hardware queues, and the lanes of the legs below should not share one with each other (r05a: the cosine
            # lanes of this leg, created as streams 9-12 of the process, ran 1.7 kernels in flight instead of 2.6)
            ls.sync()
            for h in ls.handles[1:]:
                h.close()
            ls.handles, ls.streams = ls.handles[:1], ls.streams[:1]
            x_host = x.cpu().numpy()
            q_host = q.cpu().numpy()
            threads = host_threads(args)
            for mname in ("l2", "cosine"):
                pm = hv.COSINE if mname == "cosine" else hv.EUCLIDEAN
                if (mname == "cosine") == cosine:
                    pix = ix
                else:  # the rows are unit-norm: the same graph serves both metrics
                    pix = import_index(hv, x, g, pm, hv.F32, b, local_rank)
                t0 = time.time()
                pix.set_simhash()  # per-node SimHash rows, computed on the device with SimHasher(dim, seed 42)
                log(f"[production default, {mname}] SimHash rows attached in {time.time() - t0:.1f}s")
                pp = hv.SearchParams.new(k)
                pb = out_buffers(b, k, dev)
                p_ast = torch.zeros(b, C.sizeof(hv.AdaptiveStats), dtype=torch.uint8, device=dev)

                def run(params, bufs, ast_t):
                    # timed without the SearchStats of the non-strict stages (the reference's COLLECT_DIAGNOSTICS=false build is
                    # what its query path runs); one more launch with them afterwards
                    ms = []
                    for it in range(3 + 10):
                        st = pix.search_batch_params_device(q, params, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], None, want_stats=True)
                        if it >= 3:
                            ms.append(st["device_ms"])
                    if ast_t is not None:
                        pix.search_batch_params_device(q, params, bufs[0], bufs[1], bufs[2], bufs[3], bufs[4], ast_t)
                    torch.cuda.synchronize()
                    return float(np.mean(ms)), recall_of(bufs[0], S["truth"][0], b, k), bufs[4].cpu().numpy().astype(np.int64)

                # ---- the same parameters the way a serving host runs them (round 5): `lanes` execution lanes, two queries per SIMD, the
                #      driver's K steps over distinct query batches; every lane's last batch is checked against the oracle below ----
                pl = None
                if "production_lanes" not in skip:
                    pls = LaneSet(pix, lanes, 2 if lanes > 1 else 1, b, k, dev)  # forks made AFTER the SimHash rows were attached
                    pls.params = pp
                    p_el, p_span, p_kms = timed_steps(pls, S_qs, pp.ef, args.steps, args.warmup, lambda: None)
                    if p_el * 1e3 > 1.3 * p_span:  # a host stall inside the timed steps (CPU-quota freeze): one repeat
                        p_el, p_span, p_kms = timed_steps(pls, S_qs, pp.ef, args.steps, args.warmup, lambda: None)
                    pf = out_buffers(b, k, dev)
                    S["ix_truth"].flat_search_batch_device(pls.last_q[0], k, *pf[:4])
                    torch.cuda.synchronize()
                    p_qst = pls.bufs[0][4].cpu().numpy().astype(np.int64)
                    p_alg = hnsw_alg_bytes(p_qst, dim, 4, b)
                    p_step = p_span / args.steps
                    pl = {"params": f"SearchParams::new({k}) on {lanes} lanes, {2 if lanes > 1 else 1} queries per SIMD", "steps": args.steps, "warmup": args.warmup,
                          "qps": round(b * args.steps / p_el, 1), "ms_per_step": round(p_el * 1e3 / args.steps, 4),
                          "kernel_ms_overlapped": round(p_step, 4), "kernel_ms_each": round(float(p_kms.mean()), 4),
                          "recall_at_10": round(recall_of(pls.bufs[0][0], pf[0], b, k), 4),
                          "distance_computations_per_query": round(float(p_qst[:, 3].mean()), 1),
                          "algorithmic_bytes_per_launch": p_alg, "achieved_gbs": round(p_alg / (p_step * 1e-3) / 1e9, 1),
                          "frac": round(p_alg / (p_step * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                          "bytes_note": "SURVEY 8(d) formula (rows scored x dim x 4 + neighbour ids x 4 + queries); the 8-byte SimHash rows the cosine filter reads are not counted"}
                if pl is not None:
                    pls.sync()
                pix.set_occupancy(1)  # the lone-batch numbers below: one query per SIMD, as in rounds 1-4
                sb = out_buffers(b, k, dev)
                strict_ms, strict_rec, strict_qs = run(hv.SearchParams(k).with_ef(pp.ef), sb, None)
                prod_ms, prod_rec, prod_qs = run(pp, pb, p_ast)
                ast = np.frombuffer(p_ast.cpu().numpy().tobytes(), dtype=np.dtype(hv.AdaptiveStats))
                d = {"params": f"SearchParams::new({k}): ef={pp.ef}, SimHashMode::Adaptive, index config threshold 43 / sampling 0.8 / adaptive",
                     "kernel_ms": round(prod_ms, 4), "qps_kernel": round(b / (prod_ms * 1e-3), 1), "recall_at_10": round(prod_rec, 4),
                     "distance_computations_per_query": round(float(prod_qs[:, 3].mean()), 1),
                     "simhash_examined_per_query": round(float(ast["simhash_examined"].mean()), 1),
                     "simhash_filtered_per_query": round(float(ast["simhash_filtered"].mean()), 1),
                     "pre_sample_dropped_per_query": round(float(ast["pre_simhash_sample_dropped"].mean()), 1),
                     "bypass_expansions_per_query": round(float(ast["simhash_bypass_expansions"].mean()), 2),
                     "rng_words_per_query": round(float(ast["rng_words"].mean()), 1),
                     "strict_same_ef": {"kernel_ms": round(strict_ms, 4), "qps_kernel": round(b / (strict_ms * 1e-3), 1),
                                        "recall_at_10": round(strict_rec, 4),
                                        "distance_computations_per_query": round(float(strict_qs[:, 3].mean()), 1)}}
                if not args.no_verify:  # the non-strict arms against the oracle's restatement
                    oix = orc.Index(dim, orc.COSINE if mname == "cosine" else orc.L2SQ, kernel=orc.K_AVX_FMA_HW, m=args.m, m0=2 * args.m)
                    rc = oix.seed(g["node_ids"], x_host, g["l0_offsets"], g["l0_neighbors"], g["level"], g["up_offsets"], g["up_neighbors"],
                                  entry_point=g["entry_point"], max_layer=g["max_layer"])
                    assert rc == orc.OK
                    # SimHash rows: the device's, after an independent check of a 16 384-row sample against the oracle's hasher
                    dev_hashes = pix.get_simhash()
                    hasher = orc.SimHasher(dim, 42)
                    sample = np.linspace(0, n - 1, 16384).astype(np.int64)
                    sh_ok = all(int(hasher.hash(x_host[i])) == int(dev_hashes[i]) for i in sample)
                    oix.set_simhash(42, node_hashes=dev_hashes)
                    t1 = time.perf_counter()
                    rc, a_ids, a_sc, a_cnt, a_st = oix.search_params_batch(q_host, orc.SearchParams.new(k), threads=threads)
                    cpu_s = time.perf_counter() - t1
                    assert rc == orc.OK
                    pa = bool((pb[0].cpu().numpy().astype(np.uint64) == a_ids).all())
                    pbits = bool((pb[1].cpu().numpy().view(np.uint32) == a_sc.view(np.uint32)).all())
                    pc = bool(sum(s_["rng_words"] for s_ in a_st) == int(ast["rng_words"].sum()))
                    d["parity"] = {"queries": b, "ids_equal_oracle": pa, "score_bits_equal_oracle": pbits, "rng_words_equal": pc,
                                   "simhash_rows_equal_oracle_on_sample": {"rows": int(sample.size), "equal": bool(sh_ok)}}
                    d["cpu_oracle_qps"] = round(b / cpu_s, 1)
                    assert pa and pbits and pc and sh_ok, f"GPU non-strict search ({mname}) differs from the CPU oracle"
                    if pl is not None:  # every lane's last batch of the lanes leg
                        same_i = same_b = True
                        for l in range(lanes):
                            if pls.last_q[l] is None:
                                continue
                            rc, l_ids, l_sc, _, _ = oix.search_params_batch(pls.last_q[l].cpu().numpy(), orc.SearchParams.new(k), threads=threads)
                            assert rc == orc.OK
                            same_i &= bool((pls.bufs[l][0].cpu().numpy().astype(np.uint64) == l_ids).all())
                            same_b &= bool((pls.bufs[l][1].cpu().numpy().view(np.uint32) == l_sc.view(np.uint32)).all())
                        pl.update({"lanes_checked": lanes, "queries_checked": b * lanes, "ids_equal_oracle": same_i, "score_bits_equal_oracle": same_b})
                        assert same_i and same_b, f"GPU non-strict search on lanes ({mname}) differs from the CPU oracle"
                    del oix
                prod[mname] = d
                if pix is ix:
                    ix.set_occupancy(occ)
                if pl is not None:
                    prod_lanes[mname] = pl
                    for h in pls.handles[1:]:
                        h.close()
                if pix is not ix:
                    pix.close()
        out["production_default"] = prod
        out["production_default_lanes"] = prod_lanes or None

        # ---- CPU baseline + bit-exact verification of the headline ----
        if args.cpu_seconds > 0 or not args.no_verify:
            threads = host_threads(args)
            t0 = time.time()
            if x_host is None:
                x_host = x.cpu().numpy()
            oix = orc.Index(dim, orc.COSINE if cosine else orc.L2SQ, kernel=orc.K_AVX_FMA_HW, m=args.m, m0=2 * args.m)
            rc = oix.seed(g["node_ids"], x_host, g["l0_offsets"], g["l0_neighbors"], g["level"], g["up_offsets"], g["up_neighbors"],
                          entry_point=g["entry_point"], max_layer=g["max_layer"])
            assert rc == orc.OK, f"oracle seed failed: {rc}"
            q_host = q.cpu().numpy()
            log(f"oracle seeded in {time.time() - t0:.1f}s; timing {threads} threads")
            rounds = []
            t_budget = time.time()
            rc, o_ids, o_sc, o_cnt, o_st = oix.search_batch(q_host, k, ef, threads=threads)  # warm-up pass
            assert rc == orc.OK
            while len(rounds) < 7 and (time.time() - t_budget) < args.cpu_seconds:
                t1 = time.perf_counter()
                rc, o_ids, o_sc, o_cnt, o_st = oix.search_batch(q_host, k, ef, threads=threads)
                rounds.append(time.perf_counter() - t1)
            med = float(np.median(rounds)) if rounds else float("nan")
            t1 = time.perf_counter()
            oix.search_batch(q_host[:64], k, ef, threads=1)
            single = (time.perf_counter() - t1) / 64
            out["cpu_baseline"] = {
                "value": round(b / med, 1) if rounds else None, "unit": "queries/s", "cores": threads, "threads": threads,
                "nproc": os.cpu_count(), "quota_cores": cpu_quota(), "kind": "port",
                "sample": f"all {b} queries of the same batch, same graph, k={k} ef={ef}; median of {len(rounds)} rounds after a warm-up pass; "
                          f"oracle = C restatement with real AVX2+FMA kernels, data resident in RAM (no storage-engine cost)",
                "single_thread_us_per_query": round(single * 1e6, 1),
                "host": f"{os.cpu_count()} logical CPUs, cgroup CPU quota {cpu_quota()} cores (threads = the quota: more would only be throttled)"}
            if not args.no_verify:
                same = True
                o_dc = sum(s["distance_computations"] for s in o_st)
                for l in range(lanes):  # every lane's last batch -- each lane answered a different one
                    if l == 0 or ls.last_q[l] is None:
                        l_ids, l_sc = o_ids, o_sc
                    else:
                        rc, l_ids, l_sc, _, _ = oix.search_batch(ls.last_q[l].cpu().numpy(), k, ef, threads=threads)
                        assert rc == orc.OK
                    g_ids_h, g_sc_h = ls.bufs[l][0].cpu().numpy().astype(np.uint64), ls.bufs[l][1].cpu().numpy()
                    same &= bool((g_ids_h == l_ids).all()) and bool((g_sc_h.view(np.uint32) == l_sc.view(np.uint32)).all())
                out["parity"] = {"queries": b * lanes, "lanes_checked": lanes, "distinct_batches_checked": lanes, "ids_equal_oracle": same, "score_bits_equal_oracle": same,
                                 "distance_computations_equal": bool(o_dc == int(qst[:, 3].sum()))}
                assert same, "GPU HNSW results differ from the CPU oracle"
            del oix
        if "batcher" not in skip and not bf16 and headline_alive:
            t0 = time.time()
            try:
                if x_host is None:
                    x_host = x.cpu().numpy()
                out["batcher"] = leg_batcher(x_host, q.cpu().numpy(), g, args.m)
            except Exception as e:
                out["batcher"] = {"error": f"{type(e).__name__}: {e}"}
            log(f"[batcher] {time.time() - t0:.1f}s")
        del x_host

    # the headline index is no longer needed
    if headline_alive:
        ls.close_forks()
        ix.close()
        if S["ix_truth"] is not ix:
            S["ix_truth"].close()
        S = ix = ls = x = q = None
        torch.cuda.empty_cache()

    if world == 1 and rank == 0:
        import orc

        def guarded(name, fn):
            t0 = time.time()
            try:
                r = fn()
            except Exception as e:  # an extra leg must not take the headline line with it; parity failures inside a leg are reported
                r = {"error": f"{type(e).__name__}: {e}"}
            log(f"[{name}] {time.time() - t0:.1f}s")
            return r

        if "vendor_gemm" not in skip:
            out["vendor_gemm"] = guarded("vendor_gemm", lambda: leg_vendor_gemm(dev))
        if "insert" not in skip:
            out["incremental_insert"] = guarded("incremental_insert", lambda: leg_incremental_insert(hv, synth, args, dev))
        if "config3" not in skip:
            out["config3_prefilter"] = guarded("config3", lambda: leg_config3(hv, synth, orc, args, dev))
        if "config4" not in skip:
            def c4():
                r, st = hnsw_leg(hv, synth, args, dev, "embedding", args.c4_rows, dim, b, k, ef, dtype_name="bf16", steps=int(os.environ.get("C4_STEPS", 32)), keep=True)
                # parity on a sample: the oracle over the same rounded rows and graph
                xh = st["x"].cpu().numpy()
                gg = st["g"]
                oix = orc.Index(dim, orc.L2SQ, kernel=orc.K_AVX_FMA_HW, m=args.m, m0=2 * args.m)
                assert oix.seed(gg["node_ids"], xh, gg["l0_offsets"], gg["l0_neighbors"], gg["level"], gg["up_offsets"], gg["up_neighbors"],
                                entry_point=gg["entry_point"], max_layer=gg["max_layer"]) == orc.OK
                qh = st["q"][:128].cpu().numpy()
                rc, o_ids, o_sc, o_cnt, o_st = oix.search_batch(qh, k, ef, threads=host_threads(args))
                gi = st["ls"].bufs[0][0][:128].cpu().numpy().astype(np.uint64)
                gs = st["ls"].bufs[0][1][:128].cpu().numpy()
                r["parity_sample"] = {"queries": 128, "ids_equal_oracle": bool((gi == o_ids).all()),
                                      "score_bits_equal_oracle": bool((gs.view(np.uint32) == o_sc.view(np.uint32)).all())}
                r["workload"] = (f"configs[3] per-GPU shard: {args.c4_rows}x{dim} bf16 rows (10M / 8), HNSW ef={ef} k={k}, batch {b}; f32 arithmetic "
                                 f"in the reference's summation order on the stored (rounded) values")
                st["ls"].close_forks()
                st["ix"].close()
                st["ix_truth"].close()
                return r
            out["config4_bf16"] = guarded("config4", c4)
            torch.cuda.empty_cache()
        if "config5" not in skip:
            out["config5_fp8_flat"] = guarded("config5", lambda: leg_config5(hv, synth, orc, dev, args.c5_rows))
        if "graph_equivalence" not in skip:
            out["graph_equivalence"] = guarded("graph_equivalence", lambda: leg_graph_equivalence(hv, synth, args, dev))
            out["graph_equivalence_clustered"] = guarded("graph_equivalence_clustered", lambda: leg_graph_equivalence(hv, synth, args, dev, "clustered"))
        # ---- the other corpora of config #2 at the same settings ----
        if "datasets" not in skip:
            ds = {}
            for name in ("clustered", "gaussian"):
                if name == args.dataset:
                    continue
                if name == "clustered" and "iso_recall" not in skip:  # the same leg + the ef sweep to the recall gate on the same graph
                    iso = guarded("dataset clustered + iso_recall", lambda: leg_iso_recall(hv, synth, orc, args, dev, "clustered", args.rows, dim, b, k,
                                                                                          efs=(ef, 192, 256, 384, 512, 800)))
                    ds[name] = iso.pop("leg_at_first_ef", iso)
                    ds["clustered_iso_recall"] = iso
                    continue
                ds[name] = guarded(f"dataset {name}", lambda: hnsw_leg(hv, synth, args, dev, name, args.rows, dim, b, k, ef, steps=32)[0])
            ds["note"] = ("headline = 'embedding' (low intrinsic dimension, recall >= 0.95); 'clustered' = SURVEY 8(d)'s stated variant "
                          "(1 024 Gaussian centres, sigma 0.15, native 768-d: inside a cluster the rows are i.i.d. Gaussian again); 'gaussian' = "
                          "8(d) as literally written, a stated worst case: distance concentration at 768-d leaves no neighbour structure, so "
                          "recall@10 misses 0.95 at ef=128 for every HNSW, the reference's included -- QPS there is not a headline")
            out["datasets"] = ds
        # ---- one sensitivity table (no tuning): the headline family at latent dimension 16 (the headline itself) / 32 /
        #      64 -- the smallest ef of the sweep that reaches recall@10 >= 0.95 on each, and QPS / roofline fraction THERE ----
        if "latent" not in skip:
            lat = {}
            for L in (32, 64):
                iso = guarded(f"embedding latent {L}", lambda: leg_iso_recall(hv, synth, orc, args, dev, f"embedding{L}", args.rows, dim, b, k,
                                                                             efs=(ef, 192, 256, 384, 512, 800)))
                if isinstance(iso, dict):
                    iso.pop("leg_at_first_ef", None)
                lat[str(L)] = iso
            out["embedding_latent"] = lat

    emit(out, args.full_record, rank)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
