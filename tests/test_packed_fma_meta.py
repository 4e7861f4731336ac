"""Register and scratch figures of the headline HNSW kernel build, compiled here for gfx950 (device only, to assembly; no GPU), against
the committed table profiles/packed_fma_kernel_meta.json (scripts/kernel_meta.py on the built library).  The packed FMAs of the f32
distance passes (hvx_hnsw_wave.h: fma_chunk on register pairs) need even-aligned register pairs, and the two-per-SIMD builds sit at
their 256-register budget: a header or toolchain change that costs the headline build registers or puts it into scratch shows here
by name, before anybody measures it.

The translation unit is the library's own, hvx_hnsw_wave_occ2.hip, with the Makefile's flags: half a minute of one core for its 28
kernels.  (One explicit instantiation of the template compiles in two seconds, but not to the library's code: the bf16 build came
out with 169 registers that way against 138 in the library.)  Read from the assembly: `.amdhsa_next_free_vgpr`,
`.amdhsa_private_segment_fixed_size` and the spill counts of the kernel's metadata -- register and scratch figures only."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "helix-db_amd", "csrc")

# the headline (1M x 768 f32, squared-Euclidean, ef 128, two queries per SIMD) and the 384-entry beam its flagged queries re-run on
HEADLINE = "_ZN3hvx16hnsw_wave_kernelILj1ELi3ELi24ELb0ELb0ELb0ELb1ELi2ELb0EEEvNS_8HnswArgsEj"
RERUN = "_ZN3hvx16hnsw_wave_kernelILj1ELi6ELi24ELb0ELb0ELb0ELb1ELi2ELb0EEEvNS_8HnswArgsEj"


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH\s+\?= (\S+)$", text, re.M).group(1)
    return re.search(r"^CXXFLAGS \?= (.*)$", text, re.M).group(1).replace("$(ARCH)", arch).split()


@pytest.fixture(scope="module")
def assembly(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    asm = tmp_path_factory.mktemp("packed_fma") / "hvx_hnsw_wave_occ2.s"
    out = subprocess.run([hipcc] + makefile_flags() + ["-S", "--cuda-device-only", "-o", str(asm), os.path.join(CSRC, "hvx_hnsw_wave_occ2.hip")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return asm.read_text()


def figures(text, name):
    """the kernel descriptor block and the metadata entry of one kernel"""
    desc = re.search(r"^\s*\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S).group(1)
    note = re.search(r"^\s*\.name:\s+" + re.escape(name) + r"\n(.*?)^\s*\.wavefront_size:", text, re.M | re.S).group(1)
    one = lambda pat, s: int(re.search(pat, s, re.M).group(1))
    return dict(vgpr=one(r"^\s*\.amdhsa_next_free_vgpr (\d+)", desc), scratch=one(r"^\s*\.amdhsa_private_segment_fixed_size (\d+)", desc),
                vgpr_spill=one(r"^\s*\.vgpr_spill_count:\s+(\d+)", note), sgpr_spill=one(r"^\s*\.sgpr_spill_count:\s+(\d+)", note))


@pytest.mark.parametrize("name", [HEADLINE, RERUN], ids=["headline", "rerun-beam"])
def test_headline_build_keeps_its_registers_and_stays_out_of_scratch(assembly, name):
    meta = json.load(open(os.path.join(ROOT, "profiles", "packed_fma_kernel_meta.json")))
    assert meta["headline"] == HEADLINE
    want = meta["kernels"][name]["after"]
    got = figures(assembly, name)
    print(name, got, "committed:", want)
    assert want["agpr"] == 0  # (two per SIMD: 256 registers, no accumulation half; `vgpr` is then the directive's figure)
    assert got["vgpr"] == want["vgpr"], f"{got['vgpr']} registers, the committed table has {want['vgpr']}"
    assert got["scratch"] == want["scratch"]
    assert got["vgpr_spill"] == want["vgpr_spill"] and got["sgpr_spill"] == want["sgpr_spill"]
    assert got["scratch"] == 0 and got["vgpr_spill"] == 0, "the build went into scratch"
