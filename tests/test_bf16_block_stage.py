"""How build_link_wg_kernel stages bf16 rows (csrc/hvx_device.h: bf16_block_piece / bf16_piece_widen -- the index arithmetic the kernel
itself calls), checked on the host against the plain-order rounded row: no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("bf16_stage") / "bf16_block_stage_probe"
    out = subprocess.run([hipcc, "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unused-function", "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "bf16_block_stage_probe.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


@pytest.mark.parametrize("dim", [128, 384, 768, 1536])
@pytest.mark.parametrize("ck", [4, 8])
def test_staged_bf16_column_blocks_equal_the_plain_order_row(probe, dim, ck):
    """A row of distinct values packed with bf16_slot_of, every column block of ck chunks staged piece by piece (the partial last block
    of dim 384 at ck 8 and of dim 128 at ck 8 included): every float of the row arrives once, at its plain-order place, exactly; nothing
    else is written; and the eight decoded float4 pairs of a ds_write_b128 lane group cover 32 banks at the row stride ck * 32 + 32."""
    run = subprocess.run([probe, str(dim), str(ck)], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout.split() == ["ok", str(5 * dim)]
