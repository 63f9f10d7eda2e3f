#!/bin/bash
# All BASELINE configs on one MI355X:  [OUT=dir] bash tools/gpu_configs.sh <tag>
# GPU tests, then bench.py --full per workload -> $OUT/bench_<tag>_<workload>.json (OUT: bench_out)
set -o pipefail
TAG=${1:-cfg}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > "$OUT/gpu_tests_$TAG.log" 2>&1 || { echo "TESTS FAILED"; tail -30 "$OUT/gpu_tests_$TAG.log"; exit 3; }
tail -2 "$OUT/gpu_tests_$TAG.log"
timeout -k 10 200 python bench.py --full >"$OUT/bench_${TAG}_dsec.json" 2> "$OUT/bench_${TAG}_dsec.err" || { echo "BENCH dsec FAILED"; tail "$OUT/bench_${TAG}_dsec.err"; exit 5; }
timeout -k 10 200 python bench.py --full --workload train --steps 20 > "$OUT/bench_${TAG}_train.json" 2> "$OUT/bench_${TAG}_train.err" || { echo "BENCH train FAILED"; tail "$OUT/bench_${TAG}_train.err"; exit 5; }
timeout -k 10 200 python bench.py --full --workload mvsec --steps 20 --cpu-seconds 10 > "$OUT/bench_${TAG}_mvsec.json" 2> "$OUT/bench_${TAG}_mvsec.err" || { echo "BENCH mvsec FAILED"; tail "$OUT/bench_${TAG}_mvsec.err"; exit 5; }
timeout -k 10 200 python bench.py --full --workload hires1280 --sharded --steps 10 --no-cpu-baseline > "$OUT/bench_${TAG}_hires1280.json" 2> "$OUT/bench_${TAG}_hires1280.err" || { echo "BENCH hires FAILED"; tail "$OUT/bench_${TAG}_hires1280.err"; exit 5; }
for w in dsec train mvsec hires1280; do echo "== $w"; cat "$OUT/bench_${TAG}_$w.json"; done
