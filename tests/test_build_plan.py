"""What a device write (build, batched insert, upsert, hvx_index_link_rows) runs -- the degree limits and their refusals, the link
workgroups' geometry, the batch sizes, the scratch layout and, per batch, the select and link kernels with their grids and LDS -- is
decided by helix-db_amd/csrc/hvx_build_plan.h.  This pins those decisions without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plan_table():
    """The recorded lines, keyed by their input (the text before ` -> `): GPU tests look their expected path bits up here."""
    table = {}
    for line in open(os.path.join(ROOT, "tests", "build_plan_table.txt")).read().splitlines():
        key, value = line.split(" -> ")
        table[key] = value
    return table


def test_build_plan_equals_the_recorded_write_decisions(tmp_path):
    """tests/native/build_plan_probe.cpp includes only the plan header and prints, for 519 inputs, what a write call decides: the plan of a
    batch (W: select and link step, grids, workgroup sizes, LDS bytes, g0 / gu, serial, the build search's occupancy, the HVX_WRITE_*
    bits, or the refusal), the degree limits with the first refusal (D), the link workgroups' geometry (G), batch sizes (B) and the
    scratch layout (S); the output must equal tests/build_plan_table.txt line for line.

    The table was NOT produced by the plan header.  It was recorded from the tree BEFORE the plan existed, where these decisions were
    expressions spread over insert_range, hvx_index_insert_batch and hvx_index_link_rows (hvx_build.hip) and wide_link_geom
    (hvx_build_wide.hip): those expressions were lifted verbatim into a recorder with this probe's driver and output format, and both
    were driven over the full grid (the probe's `full` argument) dtype {f32, bf16} x metric {L2, cosine, L1} x summation tree {AVX+FMA,
    AVX, SSE} x dim {32, 100, 128, 192, 768} x ld {dim, dim + 4} x (m, m0) {(8,16), (16,32), (17,33), (24,48), (32,64)} x rows {m0 / m,
    64, 65 ids} x link_mode {0, 1} x mode {auto, batched, one node} x bsz {1, 2, 1 023, 1 024, 1 025, 2 048} x promotes {0, 1} x layers
    {1, 3, 6}, with ef_construction {default, 64, 800, 801}, and on one image per (m, m0, rows) batch sizes and scratch layouts over
    max_batch x divisor x position: 637 165 lines, byte-identical between the recorder and this probe.  The table is the subset of
    those lines the probe walks without `full`: every select and link step, both sides of the 1 024-node threshold and of 33 / 65
    candidate rows, bf16 rows with dim % 64 != 0, Manhattan / the 128-bit tree / padded and short rows (no link workgroups), and every
    refusal.  A change that alters a decision on purpose replaces the affected lines by hand, with the reason."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path / "build_plan_probe"
    out = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "build_plan_probe.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    want = open(os.path.join(ROOT, "tests", "build_plan_table.txt")).read().splitlines()
    got = run.stdout.splitlines()
    assert len(want) == 519
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
