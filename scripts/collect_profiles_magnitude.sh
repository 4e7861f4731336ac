#!/bin/bash
# Evidence for the magnitude tests (tests/test_gpu_magnitude.py).  Run from the repository root on the GPU box, one step per visit:
#   scripts/collect_profiles_magnitude.sh <out_dir> parent <parent_lib>   the new file against the PARENT commit's library (a built
#                                                                         libhelix_vec_gfx950.so of it): which cases fail there
#                                                                                                  -> magnitude_gpu_tests_parent.log
#   scripts/collect_profiles_magnitude.sh <out_dir> fixed                 the new file against this tree's library
#                                                                                                  -> magnitude_gpu_tests.log
#   scripts/collect_profiles_magnitude.sh <out_dir> suite                 the rest of the -m gpu suite on this tree's library
#                                                                                                  -> magnitude_gpu_tests_rest.log
#   scripts/collect_profiles_magnitude.sh <out_dir> bench <parent_lib>    plain bench.py, the parent's library and this tree's,
#                                                                         alternating, three runs each -> magnitude_bench_ab.jsonl
# The binding loads the library HVX_LIB_PATH names (pyhvx/__init__.py); tests, oracle and bench.py are this tree's in every step.
# Every GPU step runs under its own time limit; the script stops at the first step that fails to run (a failing TEST is a result).
set -u -o pipefail
out=${1:?out_dir}
step=${2:?parent|fixed|suite|bench}
parent_lib=${3:-}
mkdir -p "$out"
case "$step" in
parent)
    [ -f "$parent_lib" ] || { echo "parent: the parent commit's library is needed" >&2; exit 2; }
    HVX_LIB_PATH=$(realpath "$parent_lib") timeout -k 10 1100 python -m pytest tests/test_gpu_magnitude.py -q -m gpu -p no:cacheprovider -rf --tb=line 2>&1 |
        tee "$out/magnitude_gpu_tests_parent.log" | tail -150
    ;;
fixed)
    timeout -k 10 1100 python -m pytest tests/test_gpu_magnitude.py -q -m gpu -p no:cacheprovider -rf --tb=line 2>&1 |
        tee "$out/magnitude_gpu_tests.log" | tail -150
    ;;
suite)
    timeout -k 10 1100 python -m pytest tests -q -m gpu -p no:cacheprovider -rf --tb=short --deselect tests/test_gpu_magnitude.py 2>&1 |
        tee "$out/magnitude_gpu_tests_rest.log" | tail -60
    ;;
bench)
    [ -f "$parent_lib" ] || { echo "bench: the parent commit's library is needed" >&2; exit 2; }
    tmp=$(mktemp -d)
    : > "$out/magnitude_bench_ab.jsonl"
    for i in 1 2 3; do
        for w in parent this; do
            lib=helix-db_amd/libhelix_vec_gfx950.so
            [ $w = parent ] && lib=$parent_lib
            echo "[$(date +%H:%M:%S)] bench.py, library of: $w, run $i" >&2
            HVX_LIB_PATH=$(realpath "$lib") timeout -k 10 300 python bench.py > "$tmp/b.log" 2> "$tmp/b.err" || { tail -5 "$tmp/b.err"; exit 1; }
            grep '^{' "$tmp/b.log" | tail -1 | sed "s/^{/{\"library\": \"$w\", \"run\": $i, /" >> "$out/magnitude_bench_ab.jsonl"
        done
    done
    rm -rf "$tmp"
    cut -c1-400 "$out/magnitude_bench_ab.jsonl"
    ;;
*)
    echo "unknown step $step" >&2; exit 2
    ;;
esac
