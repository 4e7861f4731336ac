"""The wide builds of the one-launch restricted exact scan (csrc/hvx_restricted_wide4.hip / _wide13.hip) in the built library: they are
there, and the unrolled ones (768 and 1536: NK 24 and 48) keep their 8 / 26 list registers per lane beside the gather without scratch
and without spilled vector registers -- a spilled list register would turn every insertion into memory traffic (docs/next_kernel.md,
round-5 note 2).  Reads the register metadata of the code objects only (scripts/kernel_meta.py); needs `c++filt` (binutils) on PATH, as
that script does."""
import importlib.util
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "helix-db_amd", "libhelix_vec_gfx950.so")


@pytest.fixture(scope="module")
def wide():
    """{(metric, nk, bf16, ext, fused, registers): resources} of every restricted_direct_kernel instantiation whose result list is wider
    than one register pair per lane (the last template argument; such builds serve one query per tile)"""
    spec = importlib.util.spec_from_file_location("kernel_meta", os.path.join(ROOT, "scripts", "kernel_meta.py"))
    km = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(km)
    names = {n: v for n, v in km.kernels_of(LIB).items() if "restricted_direct_kernel" in n}
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    out = {}
    for mangled, text in zip(names, dem):
        m = re.search(r"restricted_direct_kernel<(\d+)u, (\d+), (true|false), 1, (true|false), (true|false), (\d+)>", text)
        if m and int(m.group(6)) > 1:
            out[(int(m.group(1)), int(m.group(2)), m.group(3) == "true", m.group(4) == "true", m.group(5) == "true", int(m.group(6)))] = names[mangled]
    return out


def test_wide_builds_are_present(wide):
    """both list widths; per width the any-shape build of every metric (f32 rows with and without FMA, bf16 rows for cosine and L2) and
    the unrolled builds of 768 / 1536 for cosine and L2 over f32 and bf16 rows; each for shared and for per-query candidate sets"""
    assert wide, "no wide instantiation of restricted_direct_kernel in the library"
    assert {key[5] for key in wide} == {4, 13}
    for r in (4, 13):
        for ext in (False, True):
            for metric in (0, 1, 2):
                assert (metric, 0, False, ext, True, r) in wide and (metric, 0, False, ext, False, r) in wide
            for metric in (0, 1):
                assert (metric, 0, True, ext, True, r) in wide
                for nk in (24, 48):
                    for bf in (False, True):
                        assert (metric, nk, bf, ext, True, r) in wide


def test_unrolled_wide_builds_carry_no_scratch(wide):
    unrolled = {key: v for key, v in wide.items() if key[1] != 0}
    assert len(unrolled) == 32
    for key, v in sorted(unrolled.items()):
        assert v["scratch"] == 0 and v["vgpr_spill"] == 0, (key, v)
