#!/bin/bash
# bench.py's grouped-vs-separate check on every workload (quick legs only): bash scripts/bench_check_workloads.sh (lines to $OUT, default bench_out/)
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT
for w in full resnet34 resnet34_nodcn nodcn; do
  timeout -k 10 300 python bench.py --full --workload $w --no-cpu-baseline --no-parity --no-h2d --no-roofline > $OUT/$w.json 2> $OUT/$w.err; echo "$w rc=$?"
  python3 - "$OUT/$w.json" <<'PY'
import json, sys
l = json.loads(open(sys.argv[1]).read().strip().splitlines()[-1])
g = l["overlap_check"]["grouped_vs_separate_batches"]
print(l["value"], {k: (round(v, 5) if isinstance(v, float) else v) for k, v in g.items() if k != "bounds"})
PY
done
