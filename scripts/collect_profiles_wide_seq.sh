#!/bin/bash
# Evidence for the many-workgroup one-node steps at M 32 / M0 64 (csrc/hvx_build_wide_seq.hip).  Run from the repository root on the GPU box:
#   scripts/collect_profiles_wide_seq.sh <out_dir> <parent_tree> [wide|narrow|trace ...]
#  wide    one-node inserts / upserts on a 200 000 x 768 M 32 / M0 64 image: scripts/seq_insert_bench.py on this tree and on a built checkout
#          of the parent commit (parent_tree), alternating, three runs each                      -> wide_seq_steps_ab.jsonl
#  narrow  narrow builds must not get slower (insert_range and its scratch sizing are shared): scripts/bench_build.py at the headline
#          shape (1M x 768, M 16 / M0 32), the same alternation                                  -> wide_seq_narrow_build_ab.jsonl
#  trace   one kernel-trace run of this tree's one-node inserts / upserts, in a run of its own   -> wide_seq_steps_kernel_stats.csv
# Default: all three.  Every GPU step runs under its own time limit; the script stops at the first step that fails.
set -u
out=${1:?out_dir}
parent=${2:?parent_tree}
shift 2
legs=${*:-wide narrow trace}
mkdir -p "$out"
tmp=$(mktemp -d)
run() { echo "[$(date +%H:%M:%S)] $*" >&2; "$@"; }
ms() { python -c 'import json, sys
r = json.loads(sys.argv[2])
print(json.dumps({"tree": sys.argv[1], "rows": r["rows"], "dim": r["dim"], "m": r["m"], "m0": r["m0"], "ms_per_insert": round(r["us_per_insert"] / 1e3, 3), "ms_per_upsert": round(r["us_per_upsert"] / 1e3, 3)}))' "$1" "$2"; }
for leg in $legs; do
    case $leg in
    wide)
        : > "$out/wide_seq_steps_ab.jsonl"
        for i in 1 2 3; do
            run timeout -k 10 300 python "$parent/scripts/seq_insert_bench.py" 200000 768 208 32 64 > "$tmp/p.log" 2>&1 || { tail -5 "$tmp/p.log"; exit 1; }
            ms parent "$(grep '^{' "$tmp/p.log" | tail -1)" >> "$out/wide_seq_steps_ab.jsonl" || exit 1
            run timeout -k 10 300 python scripts/seq_insert_bench.py 200000 768 208 32 64 > "$tmp/t.log" 2>&1 || { tail -5 "$tmp/t.log"; exit 1; }
            ms this "$(grep '^{' "$tmp/t.log" | tail -1)" >> "$out/wide_seq_steps_ab.jsonl" || exit 1
        done ;;
    narrow)
        : > "$out/wide_seq_narrow_build_ab.jsonl"
        for i in 1 2 3; do
            run timeout -k 10 240 python "$parent/scripts/bench_build.py" 1000000 > "$tmp/p.log" 2>&1 || { tail -5 "$tmp/p.log"; exit 1; }
            grep '^{' "$tmp/p.log" | tail -1 | sed 's/^{/{"tree": "parent", /' >> "$out/wide_seq_narrow_build_ab.jsonl"
            run timeout -k 10 240 python scripts/bench_build.py 1000000 > "$tmp/t.log" 2>&1 || { tail -5 "$tmp/t.log"; exit 1; }
            grep '^{' "$tmp/t.log" | tail -1 | sed 's/^{/{"tree": "this", /' >> "$out/wide_seq_narrow_build_ab.jsonl"
        done ;;
    trace)
        run timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$tmp/si" -o si -- python scripts/seq_insert_bench.py 200000 768 208 32 64 > "$tmp/sp.log" 2>&1 || { tail -5 "$tmp/sp.log"; exit 1; }
        st=$(find "$tmp/si" -name '*kernel_stats.csv' | head -1)
        [ -n "$st" ] || { echo "no kernel statistics were written" >&2; exit 1; }
        (head -1 "$st"; grep -E "build_|delete_|hnsw_wave_kernel" "$st") > "$out/wide_seq_steps_kernel_stats.csv" ;;
    *) echo "unknown leg $leg" >&2; exit 2 ;;
    esac
done
rm -rf "$tmp"
