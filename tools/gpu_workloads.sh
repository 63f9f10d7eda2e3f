#!/bin/bash
# Every bench workload on one MI355X, with rooflines (--full) and no CPU baselines:
#   [OUT=dir] bash tools/gpu_workloads.sh <tag>   -> $OUT/bench_<tag>_<workload>.json (OUT: bench_out)
set -o pipefail
TAG=${1:-wl}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
for w in dsec mvsec mvsec_crop hires1280 hires1920; do
  timeout -k 10 200 python bench.py --full --workload $w --steps 20 --warmup 5 --no-cpu-baseline > "$OUT/bench_${TAG}_$w.json" 2> "$OUT/bench_${TAG}_$w.err" || { echo "BENCH $w FAILED"; tail "$OUT/bench_${TAG}_$w.err"; exit 5; }
done
timeout -k 10 200 python bench.py --full --workload train --steps 20 --warmup 5 --no-cpu-baseline > "$OUT/bench_${TAG}_train.json" 2> "$OUT/bench_${TAG}_train.err" || { echo "BENCH train FAILED"; exit 5; }
timeout -k 10 100 tools/_build/kbench_build 5 mvsec-pad > "$OUT/kb_${TAG}_mvsec.txt" 2>&1 || exit 6
timeout -k 10 200 tools/_build/kbench_build 3 1920x1280 > "$OUT/kb_${TAG}_1920.txt" 2>&1 || exit 6
python3 - "$TAG" "$OUT" <<'PY'
import json, sys
tag, out = sys.argv[1:3]
for w in ["dsec", "mvsec", "mvsec_crop", "hires1280", "hires1920", "train"]:
    d = json.load(open(f"{out}/bench_{tag}_{w}.json"))
    r = d["roofline"]; l = d.get("roofline_lookup", {})
    print(f"{w:11s} {d['value']:10.1f} fps  step {d['ms_per_step']*1e3:8.1f} us  build {r['avg_us']:8.1f} us frac {r['frac']:.3f} "
          f"bind {r.get('binding_floor', {}).get('frac')}  lookup {l.get('avg_us')} us frac {l.get('frac')}")
PY
