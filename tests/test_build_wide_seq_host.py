"""CPU-side checks of the many-workgroup one-node steps for degree limits above 32 (csrc/hvx_build_wide_seq.hip): the kernels compile for
gfx950 without scratch and without cache maintenance, the geometry function lays the matrices out without overlap inside the scratch it
sizes, the `alive` replay keeps what the oracle keeps at the wide widths, and the public interface names the write paths."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from test_walk_twin import _eager_prune_twin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hipcc():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    return hipcc


def test_wide_one_node_steps_compile_without_scratch_and_without_cache_maintenance(tmp_path):
    """Eight instantiations of each kernel -- L2 / cosine / Manhattan x fused / unfused tree over f32 rows, L2 / cosine with the fused
    tree over bf16 rows --, none with scratch (`.amdhsa_private_segment_fixed_size` 0: a 1 024-thread workgroup leaves 128 VGPRs per
    lane) and none with `buffer_wbl2` / `buffer_inv` (an L2 write-back / invalidate of the whole XCD)."""
    src = os.path.join(ROOT, "helix-db_amd", "csrc", "hvx_build_wide_seq.hip")
    assert os.path.exists(src), "the wide one-node steps live in their own translation unit"
    asm = tmp_path / "hvx_build_wide_seq.s"
    out = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-S", "--cuda-device-only",
                          "-o", str(asm), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    kernels = re.findall(r"^(_ZN3hvx\d+build_\w+):[^\n]*\n(.*?)\.end_amdhsa_kernel", asm.read_text(), flags=re.S | re.M)
    names = [k for k, _ in kernels]
    assert sum("build_select_wide_seq_kernel" in k for k in names) == 8, names
    assert sum("build_link_wide_seq_kernel" in k for k in names) == 8, names
    assert len(names) == 16, names
    for name, body in kernels:
        assert "buffer_wbl2" not in body and "buffer_inv" not in body, name
        seg = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert seg and int(seg.group(1)) == 0, (name, seg.group(0) if seg else None)


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    exe = tmp_path_factory.mktemp("wide_seq") / "wide_seq_geom_probe"
    out = subprocess.run([_hipcc(), "--cuda-host-only", "-x", "hip", "-std=c++17", "-O1", "-Wall", "-Wno-unused-function", "-o", str(exe),
                          os.path.join(ROOT, "tests", "native", "wide_seq_geom_probe.cpp")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    return str(exe)


def _fields(line):
    return {k: v for k, v in (t.split("=") for t in line.split()[1:])}


def test_wide_seq_geometry_regions_fit_the_scratch_and_do_not_overlap(probe):
    """wide_seq_geom for (m, m0) in {(32, 64), (24, 48), (17, 33)} x 1..6 layers: every layer holds a select matrix of 2 Mmax + 1 rows and
    Mmax link matrices of 66 rows x 96 floats, no two regions overlap, all lie inside total_floats() (what insert_range allocates), the
    link step's LDS is at most 160 KB; narrow limits (16, 32) and limits above 64 do not fit (the other kernels serve them)."""
    run = subprocess.run([probe], capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    geos, regions = {}, {}
    for line in run.stdout.splitlines():
        f = _fields(line)
        key = (int(f["m"]), int(f["m0"]), int(f["layers"]))
        if line.startswith("G "):
            geos[key] = f
        else:
            regions.setdefault(key, []).append(f)
    for m, m0 in ((32, 64), (24, 48), (17, 33)):
        for layers in range(1, 7):
            g = geos[(m, m0, layers)]
            assert g["ok"] == "1", g
            assert int(g["link_lds"]) <= 160 * 1024
            assert int(g["link_rs"]) % 32 == 0 and int(g["link_rs"]) >= int(g["list"]) == 65
            # rows of at most 64 ids pruned to their limit: <= Mmax links, each dropping <= 65 - Mmax ids
            assert int(g["log"]) >= max(x * (65 - x) for x in range(1, 65))
            total = int(g["total"])
            rs = regions[(m, m0, layers)]
            for L in range(layers):
                maxn = m0 if L == 0 else m
                mine = [r for r in rs if int(r["layer"]) == L]
                sel = [r for r in mine if r["kind"] == "select"]
                assert len(sel) == 1 and len(mine) == 1 + maxn
                hyd = min(2 * maxn, 128)
                assert int(sel[0]["rows"]) >= hyd + 1 and int(sel[0]["rw"]) >= hyd and int(sel[0]["rw"]) % 32 == 0
                assert int(sel[0]["floats"]) == int(sel[0]["rows"]) * int(sel[0]["rw"])
                for r in mine:
                    if r["kind"] != "select":
                        assert int(r["rows"]) >= 66 and int(r["floats"]) == int(r["rows"]) * int(r["rw"])
            spans = sorted((int(r["off"]), int(r["off"]) + int(r["floats"])) for r in rs)
            assert spans[0][0] == 0 and spans[-1][1] <= total
            for (a0, a1), (b0, b1) in zip(spans[:-1], spans[1:]):
                assert a1 <= b0, (m, m0, layers, a0, a1, b0, b1)
    assert all(geos[(16, 32, layers)]["ok"] == "0" and geos[(40, 80, layers)]["ok"] == "0" for layers in range(1, 7))


def test_wide_seq_pair_prefix_covers_exactly_the_lists_above_their_limit(probe):
    """A link whose list holds deg ids takes (deg + 1) deg / 2 pair numbers when deg > Mmax (all pairs among the ids and the owner), none
    otherwise; the prefix is their running sum in selection order."""
    rng = np.random.default_rng(65)
    for maxn in (64, 32, 48, 24, 33, 17):
        for _ in range(6):
            ns = int(rng.integers(1, maxn + 1))
            degs = rng.integers(1, 66, ns).tolist()
            degs[int(rng.integers(0, ns))] = 65
            degs[int(rng.integers(0, ns))] = maxn
            run = subprocess.run([probe, "prefix", str(maxn)] + [str(d) for d in degs], capture_output=True, text=True)
            assert run.returncode == 0, run.stderr
            base = [int(x) for x in run.stdout.split()]
            assert len(base) == ns + 1 and base[0] == 0
            for t, d in enumerate(degs):
                assert base[t + 1] - base[t] == ((d + 1) * d // 2 if d > maxn else 0), (maxn, t, d)
            assert base[-1] == sum((d + 1) * d // 2 for d in degs if d > maxn)


def _alive_replay_twin(orc, metric, kernel, rows, ids, owner, cand, alive, maxn):
    """replay_rows2 with an `alive` mask (csrc/hvx_graph_dev.h): the matrix is the one of the SUPERSET list `cand` (evaluated before some
    ids left); an id that has left ranks behind every live id, rejects nobody and is neither selected nor backfilled.
    -> (kept ids sorted, dropped list positions)"""
    nc = len(cand)
    vec = [rows[c] for c in cand] + [rows[owner]]
    D = np.zeros((nc + 1, nc + 1), np.float32)
    for b in range(1, nc + 1):
        for a in range(b):
            D[a, b] = D[b, a] = orc.distance(metric, vec[a], vec[b], kernel=kernel)
    key = [(0, float(D[nc, c]), int(ids[cand[c]])) if alive[c] else (1, 0.0, c) for c in range(nc)]
    order = sorted(range(nc), key=lambda c: key[c])
    nlive = sum(alive)
    conf = [sum(1 << t for t in range(nc) if t != c and alive[t] and D[c, t] < D[nc, c]) for c in range(nc)]
    sel_pos, sel_rank, ns = 0, [], 0
    for r in range(nlive):
        if ns >= maxn:
            break
        c = order[r]
        if conf[c] & sel_pos:
            continue
        sel_pos |= 1 << c
        sel_rank.append(r)
        ns += 1
    stays = set(sel_rank)
    for r in range(nlive):       # the backfill: the others, closest first
        if len(stays) >= maxn:
            break
        stays.add(r)
    kept = sorted(int(ids[cand[order[r]]]) for r in stays)
    dropped = sorted(order[r] for r in range(nlive) if r not in stays)
    return kept, dropped


@pytest.mark.parametrize("metric,dim,kernel_name,maxn", [(1, 64, "K_AVX_FMA", 64), (0, 96, "K_AVX_FMA", 64), (2, 40, "K_AVX_FMA", 32), (1, 36, "K_AVX", 32)])
def test_alive_replay_over_a_superset_list_keeps_what_the_oracle_keeps(orc, metric, dim, kernel_name, maxn):
    """The exactness argument of the eager link step at the wide widths: lists of 40-65 ids, a matrix evaluated over the list as found,
    some positions gone since -- the masked replay keeps exactly what the oracle's select_diverse + backfill keeps over the SURVIVING
    ids (duplicate rows included: equal scores are decided by id), and with nothing gone it is _eager_prune_twin."""
    kernel = getattr(orc, kernel_name)
    rng = np.random.default_rng(6500 + dim + maxn)
    n = 500
    centres = rng.standard_normal((6, dim)).astype(np.float32)
    rows = (centres[rng.integers(0, 6, n)] + 0.3 * rng.standard_normal((n, dim))).astype(np.float32)
    rows[50:58] = rows[40:48]                       # exact duplicates: equal scores, decided by id
    rows[70] = rows[71]
    ids = np.arange(n, dtype=np.uint64) * 5 + 3
    oix = orc.Index(dim, metric, kernel=kernel, m=32, m0=64, ef_construction=40)
    assert oix.seed(ids, rows, np.zeros(n + 1, np.uint64), np.zeros(0, np.uint64), entry_point=int(ids[0])) == orc.OK
    replays = 0
    for trial in range(60):
        nc = int(rng.integers(40, 66))
        owner = int(rng.integers(0, n))
        pool = np.array([i for i in range(n) if i != owner])
        near = pool[np.argsort(((rows[pool] - rows[owner]) ** 2).sum(1))[: 3 * nc]]   # neighbours of the owner: rejections do happen
        cand = rng.choice(near, nc, replace=False).tolist()
        if trial % 5 == 0 and owner not in range(40, 58):
            cand[:4] = [40, 50, 41, 51]             # duplicate rows among the candidates
            cand = list(dict.fromkeys(cand))
            nc = len(cand)
        alive = [True] * nc
        if trial % 4:
            for c in rng.choice(nc, int(rng.integers(1, 6)), replace=False).tolist():
                alive[c] = False
        live = [cand[c] for c in range(nc) if alive[c]]
        limit = min(maxn, len(live) - 1) if trial % 3 else maxn
        rc, keep = oix.prune_candidates(int(ids[owner]), ids[live], limit)
        assert rc == orc.OK
        kept, dropped = _alive_replay_twin(orc, metric, kernel, rows, ids, owner, cand, alive, limit)
        assert kept == sorted(keep.tolist()), (trial, nc, limit)
        assert sorted(int(ids[cand[c]]) for c in dropped) == sorted(set(int(x) for x in ids[live]) - set(keep.tolist()))
        if all(alive):
            assert kept == _eager_prune_twin(orc, metric, kernel, rows, ids, owner, cand, limit)
        replays += len(live) > limit
    assert replays >= 30


def test_header_and_python_name_the_write_paths():
    """include/helix_vec.h declares enum hvx_write_path and hvx_index_last_write_path; pyhvx exposes the four flags with the header's
    values and the accessor."""
    import pyhvx as hv
    text = open(os.path.join(ROOT, "include", "helix_vec.h")).read()
    assert re.search(r"uint32_t\s+hvx_index_last_write_path\s*\(\s*const\s+hvx_index\s*\*\s*\)\s*;", text)
    body = re.search(r"enum\s+hvx_write_path\s*\{(.*?)\}\s*;", text, flags=re.S)
    assert body, "enum hvx_write_path"
    vals = {k: int(v) for k, v in re.findall(r"(HVX_WRITE_\w+)\s*=\s*(\d+)", body.group(1))}
    assert vals == {"HVX_WRITE_EAGER_STEPS": 1, "HVX_WRITE_ONE_WAVE": 2, "HVX_WRITE_LINK_WG": 4, "HVX_WRITE_WIDE": 8}
    for name, v in vals.items():
        assert getattr(hv, name[len("HVX_"):]) == v, name
    assert callable(hv.ValidatedVectorReadIndex.last_write_path)
