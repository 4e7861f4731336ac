"""The coverage ledger of the HNSW search kernels: every instantiation of hnsw_wave_kernel / hnsw_pair_kernel that plan_wave()
(helix-db_amd/csrc/hvx_hnsw_plan.h) can pick for a search launch through the public API is run by a case of
tests/test_gpu_hnsw_cover.py.  No GPU: tests/native/hnsw_cover_probe.cpp includes the plan header alone."""
import os
import shutil
import subprocess

import pytest

import hnsw_cover_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "hnsw_cover_table.txt")


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("hnsw_cover") / "hnsw_cover_probe"
    out = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "hnsw_cover_probe.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def enumerate_plan(probe):
    run = subprocess.run([probe, "enumerate"], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    return {l[2:] for l in lines if l.startswith("S ")}, {l[2:] for l in lines if l.startswith("R ")}


def resolve_cases(probe, cases):
    text = "".join(cc.probe_line(c) + "\n" for c in cases)
    run = subprocess.run([probe, "resolve"], input=text, capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == len(cases)
    return lines


def launches_of(line):
    """(case name, search kernel, re-run kernel or None) of a line of the table"""
    parts = line.split(" | ")
    assert len(parts) in (2, 3) and parts[1].startswith("S "), f"the case launches no build of the wave / pair kernels: {line}"
    assert len(parts) == 2 or parts[2].startswith("R "), line
    return parts[0], parts[1][2:], parts[2][2:] if len(parts) == 3 else None


def test_every_search_instantiation_the_plan_can_pick_is_run_by_a_gpu_case(probe):
    """The plan can pick 566 distinct instantiations for a search launch -- 462 of hnsw_wave_kernel, 104 of hnsw_pair_kernel -- and 124
    of them also run as the re-run launch with the wider beam (`hnsw_cover_probe enumerate`: dtype {f32, bf16} x metric {L2, cosine,
    Manhattan} x all five summation trees x dim {128, 256, 384, 512, 768, 1024, 1536, 100, 20} x row width {32, 64} x {strict,
    non-strict, non-strict with stats} x occupancy {1, 2} x HVX_OPT_HNSW_PAIR {0..3} x HVX_OPT_WAVE_LOG2CAP {0, 8} x ef on both sides
    of every beam threshold up to 800; phase-timing launches and build searches are not search launches of the public API).

    (a) resolving the case table reproduces tests/hnsw_cover_table.txt line for line: the committed table says what each case runs;
    (b) the search launches of the cases are exactly the enumerated set: an instantiation no case runs fails the test by name;
    (c) the re-run launches of the cases on the tie-heavy corpus -- the only ones whose re-run has work -- are exactly the
        enumerated re-run set.
    There is no exemption list.  Taking a case out of the table fails (b) or (c) with the instantiation nobody runs any more; where
    another case still runs it (the pre-pass on / off, the spill launches, bf16 rows at dim 1536 under the widest beams, which stay
    one per SIMD under either setting), it fails (a) with the case's name."""
    want_search, want_rerun = enumerate_plan(probe)
    assert len(want_search) == 566 and len(want_rerun) == 124
    assert sum("hnsw_pair_kernel" in s for s in want_search) == 104
    assert want_rerun <= want_search

    got = resolve_cases(probe, cc.CASES)
    names = [cc.case_name(c) for c in cc.CASES]
    assert len(set(names)) == len(names), "two cases with one name"
    search, rerun = set(), set()
    for c, line in zip(cc.CASES, got):
        _, s, r = launches_of(line)
        search.add(s)
        if c.corpus == "ties":
            assert r is not None, f"a case on the tie-heavy corpus without a re-run launch: {line}"
            rerun.add(r)
    missing = sorted(want_search - search)
    assert not missing, f"{len(missing)} search instantiations the plan can pick and no GPU case runs:\n" + "\n".join(missing)
    extra = sorted(search - want_search)
    assert not extra, "GPU cases launch instantiations outside the enumerated domain:\n" + "\n".join(extra)
    missing = sorted(want_rerun - rerun)
    assert not missing, f"{len(missing)} re-run instantiations no case on the tie-heavy corpus runs:\n" + "\n".join(missing)
    extra = sorted(rerun - want_rerun)
    assert not extra, "tie-heavy cases re-run on instantiations outside the enumerated domain:\n" + "\n".join(extra)

    recorded = open(TABLE).read().splitlines()
    rec_by_name = {l.split(" | ")[0]: l for l in recorded}
    got_by_name = {l.split(" | ")[0]: l for l in got}
    for name, line in rec_by_name.items():
        assert name in got_by_name, f"hnsw_cover_table.txt records a case the case table no longer has: {line}"
    for name, line in got_by_name.items():
        assert name in rec_by_name, f"a case hnsw_cover_table.txt does not record: {line}"
    for g, w in zip(got, recorded):
        assert g == w
    assert len(got) == len(recorded)


def test_every_group_has_cases_and_every_case_a_group():
    names = [g.name for g in cc.GROUPS]
    assert len(set(names)) == len(names) == 32
    assert {c.group for c in cc.CASES} == set(names)
    for c in cc.CASES:
        assert c.arm in ("strict", "non-strict") and c.corpus in ("clustered", "ties") and c.k <= c.ef
        assert c.stats is False or c.arm == "non-strict"
