#!/bin/bash
# Evidence for the device build at M 32 / M0 64 (csrc/hvx_build_wide.hip).  Run from the repository root on the GPU box:
#   scripts/collect_profiles_wide_build.sh <out_dir> [parent_tree]
#  a. narrow builds must not get slower: scripts/bench_build.py at the headline shape (1M x 768, M 16 / M0 32) on this tree and on a
#     built checkout of the parent commit (parent_tree), alternating, three runs each            -> narrow_build_ab.jsonl
#  b. the wide batched build of the same rows (M 32 / M0 64), plain and under the kernel trace   -> wide_build.json, wide_build_kernel_stats.csv
#  c. one-node inserts / upserts on a 200 000 x 768 M 32 / M0 64 image                          -> wide_seq_insert.json, wide_seq_insert_kernel_stats.csv
#  d. registers / LDS / scratch of the wide kernels                                             -> wide_kernel_meta.json
# Every GPU step runs under its own time limit; the script stops at the first step that fails.
set -u
out=${1:?out_dir}
parent=${2:-}
mkdir -p "$out"
tmp=$(mktemp -d)
run() { echo "[$(date +%H:%M:%S)] $*" >&2; "$@"; }
if [ -n "$parent" ]; then
    : > "$out/narrow_build_ab.jsonl"
    for i in 1 2 3; do
        run timeout -k 10 240 python "$parent/scripts/bench_build.py" 1000000 > "$tmp/p.log" 2>&1 || { tail -5 "$tmp/p.log"; exit 1; }
        grep '^{' "$tmp/p.log" | tail -1 | sed 's/^{/{"tree": "parent", /' >> "$out/narrow_build_ab.jsonl"
        run timeout -k 10 240 python scripts/bench_build.py 1000000 > "$tmp/t.log" 2>&1 || { tail -5 "$tmp/t.log"; exit 1; }
        grep '^{' "$tmp/t.log" | tail -1 | sed 's/^{/{"tree": "this", /' >> "$out/narrow_build_ab.jsonl"
    done
fi
run timeout -k 10 300 python scripts/bench_build.py 1000000 2048 32 embedding 0 32 64 > "$tmp/w.log" 2>&1 || { tail -5 "$tmp/w.log"; exit 1; }
grep '^{' "$tmp/w.log" | tail -1 > "$out/wide_build.json"
run timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$tmp/wb" -o wb -- python scripts/bench_build.py 1000000 2048 32 embedding 0 32 64 > "$tmp/wp.log" 2>&1 || { tail -5 "$tmp/wp.log"; exit 1; }
st=$(find "$tmp/wb" -name '*kernel_stats.csv' | head -1)
[ -n "$st" ] && (head -1 "$st"; grep -E "build_|hnsw_wave_kernel|iota_kernel" "$st") > "$out/wide_build_kernel_stats.csv"
run timeout -k 10 400 python scripts/seq_insert_bench.py 200000 768 208 32 64 > "$tmp/s.log" 2>&1 || { tail -5 "$tmp/s.log"; exit 1; }
grep '^{' "$tmp/s.log" | tail -1 > "$out/wide_seq_insert.json"
run timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$tmp/si" -o si -- python scripts/seq_insert_bench.py 200000 768 208 32 64 > "$tmp/sp.log" 2>&1 || { tail -5 "$tmp/sp.log"; exit 1; }
st=$(find "$tmp/si" -name '*kernel_stats.csv' | head -1)
[ -n "$st" ] && (head -1 "$st"; grep -E "build_|delete_|hnsw_wave_kernel" "$st") > "$out/wide_seq_insert_kernel_stats.csv"
python scripts/kernel_meta.py helix-db_amd/libhelix_vec_gfx950.so "$tmp/meta.json" > /dev/null &&
    python - "$tmp/meta.json" "$out/wide_kernel_meta.json" <<'PY'
import json, sys
m = json.load(open(sys.argv[1]))
k = m.get("kernels", m)
json.dump({n: v for n, v in k.items() if "_wide_" in n}, open(sys.argv[2], "w"), indent=1, sort_keys=True)
PY
rm -rf "$tmp"
