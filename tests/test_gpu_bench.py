"""bench.py without --full, end to end on the device: the run times its steps, writes the last step's answer under --dump-outputs and
prints one line of the contract keys -- no recall, roofline, oracle check or full record.  Run with `-m gpu` on an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_bench_run_prints_the_headline_line_and_nothing_else(tmp_path):
    b, k, steps = 256, 10, 4
    full = tmp_path / "full.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--rows", "20000", "--batch", str(b), "--k", str(k), "--steps", str(steps),
                        "--warmup", "2", "--dump-outputs", str(tmp_path / "dump"), "--full-record", str(full)],
                       cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    rec = json.loads(lines[0], parse_constant=lambda c: (_ for _ in ()).throw(ValueError(c)))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config"):
        assert key in rec, key
    assert rec["metric"].startswith("QPS @ recall@10>=0.95") and rec["unit"] == "queries/s" and rec["higher_is_better"] is True
    assert rec["dtype"] == "f32" and (rec["steps"], rec["warmup"]) == (steps, 2)
    assert rec["value"] > 0 and abs(rec["value"] * rec["ms_per_step"] / 1e3 / b - 1) < 1e-2   # value = queries per second of the same steps
    assert not {"recall_at_10", "roofline", "cpu_baseline", "parity", "full_record"} & set(rec)
    assert not full.exists() and os.listdir(tmp_path) == ["dump"]
    got = {n: np.load(tmp_path / "dump" / f"{n}.npy") for n in ("ids", "scores", "counts", "status")}
    assert got["ids"].shape == got["scores"].shape == (b, k) and (got["counts"] == k).all() and (got["status"] == 0).all()
