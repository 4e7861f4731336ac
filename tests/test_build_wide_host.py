"""CPU-side checks of the device build for degree limits above 32 (M 32 / M0 64, csrc/hvx_build_wide.hip): the wide link workgroup
kernel compiles for gfx950 without scratch and without cache maintenance around its row locks, and limits above 64 are refused
before the first HIP call."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wide_link_workgroup_kernel_takes_its_row_locks_without_cache_maintenance_and_without_scratch(tmp_path):
    """The wide twin of build_link_wg_kernel (66 rows, 2 145 pairs, 128-bit masks) keeps what makes the narrow one work: its row locks
    are relaxed atomics + s_waitcnt (no `buffer_wbl2` / `buffer_inv`: an L2 write-back / invalidate of the whole XCD per lock operation),
    and nothing spills: `.amdhsa_private_segment_fixed_size` is 0.  The one-wavefront kernels of the same translation unit lock rows the
    same way and are held to the same."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    src = os.path.join(ROOT, "helix-db_amd", "csrc", "hvx_build_wide.hip")
    assert os.path.exists(src), "the wide build kernels live in their own translation unit"
    asm = tmp_path / "hvx_build_wide.s"
    out = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only",
                          "-o", str(asm), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    text = asm.read_text()
    kernels = re.findall(r"^(_ZN3hvx\d+build_\w+):[^\n]*\n(.*?)\.end_amdhsa_kernel", text, flags=re.S | re.M)
    wg = [(k, b) for k, b in kernels if "build_link_wide_wg_kernel" in k]
    assert len(wg) == 4, [k for k, _ in kernels]              # L2 / cosine x fused / unfused summation tree
    assert not [k for k, _ in kernels if re.match(r"_ZN3hvx20build_link_wg_kernel", k)]   # the narrow kernel's four stay where they are
    for name, body in kernels:
        assert "buffer_wbl2" not in body and "buffer_inv" not in body, name
        seg = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert seg and int(seg.group(1)) == 0, (name, seg.group(0) if seg else None)
        if "link" in name:
            assert "global_atomic_swap" in body, name           # the lock itself


def test_build_refuses_degree_limits_above_64_without_touching_a_gpu():
    """hvx_index_build serves m0 <= 64 (m <= 32): above that ERR_UNSUPPORTED, and the argument checks run before the first HIP call."""
    import pyhvx as hv
    n, dim = 8, 32
    data = np.ones((n, dim), np.float32)
    ids = np.arange(n, dtype=np.uint64)
    for m, m0 in ((32, 96), (40, 64), (40, 80)):
        with pytest.raises(hv.HelixDbError) as e:
            hv.ValidatedVectorReadIndex.build(dim=dim, metric=hv.EUCLIDEAN, node_ids=ids, vectors=data, levels=None, m=m, m0=m0, ef_construction=64)
        assert e.value.status == hv.ERR_UNSUPPORTED, (m, m0, e.value.status)
