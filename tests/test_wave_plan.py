"""Which build of the one-wavefront-per-query HNSW kernel (and of its owner / gatherer sibling) a launch runs, and with what
geometry, is decided by plan_wave() in helix-db_amd/csrc/hvx_hnsw_plan.h.  This pins those decisions without a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wave_plan_equals_the_recorded_launch_decisions(tmp_path):
    """tests/native/wave_plan_probe.cpp includes only the plan header and prints, for 449 launch arguments, the kernel
    instantiation(s) launch_hnsw_wave would run (search launch and, where one follows, the re-run) with threads, visited-table
    slots and LDS bytes; the output must equal tests/wave_plan_table.txt line for line.

    The table was NOT produced by the plan header.  It was recorded from the tree BEFORE the plan existed (the dispatcher that was
    spread over hvx_hnsw.hip, the launcher templates of hvx_hnsw_wave.h / hvx_hnsw_pair.h and the 30 small translation units): every
    hvx_hnsw*.hip was compiled for the host only, the bodies of launch_wave_kernel / launch_pair_kernel were replaced by a recorder
    that resolves the kernel pointer it is handed (dladdr + __cxa_demangle) and prints it with the launch geometry, and
    launch_hnsw_wave was driven over the full cartesian grid dtype {f32, bf16, fp8} x metric {L2, cosine, L1} x summation tree
    {AVX+FMA, AVX} x dim {128, 384, 768, 1536, 100, 776} x row stride {32, 64, 65} x {strict, non-strict, non-strict with stats} x
    occupancy {1, 2} x pair {0, 1} x pair_gatherers {0, 1} x ef {1, 160, 161, 352, 353, 416, 417, 800, 801} x log2cap {0, 7, 15} x
    prof {null, set} x tie_flags / rerun_ctl {null, set}, plus the build searches (build_ef_upper {64, 200, 400} x ef {100, 200, 353,
    800} x occupancy x log2cap x queries {null, set}): 886 464 lines, byte-identical between that tree and the first tree with the
    plan.  The table is the subset of those lines whose inputs the probe walks: every translation-unit family, every rung of every
    beam ladder on both sides of 160/161, 352/353, 416/417 and 800/801 with and without the re-run, the bf16 / dim-1536 / wide launch
    that stays at one query per SIMD, forced table sizes, the phase-timing build, and inputs nothing serves (`none`; `ERROR` = the
    predicate says yes and no build exists: a phase-timing launch outside L2 / dim 768).  A search launch is only attempted where
    hnsw_wave_supported / hnsw_wave_adaptive_supported hold, a build search where the callers' probe holds, as in the library.
    (The two-per-SIMD fallback `room < 512` cannot be reached: two per SIMD exists for the unrolled shapes only, dim <= 1536, where
    at least 3 200 slots fit.)  A change that alters a decision on purpose replaces the affected lines by hand, with the reason."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path / "wave_plan_probe"
    out = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "wave_plan_probe.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    want = open(os.path.join(ROOT, "tests", "wave_plan_table.txt")).read().splitlines()
    got = run.stdout.splitlines()
    assert len(want) == 449
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
