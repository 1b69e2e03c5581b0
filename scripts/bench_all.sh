#!/bin/bash
# one bench line per BASELINE.json config that fits one GPU (profiles/r04_bench_<name>.json);
# the headline config is the default command itself: python3 bench.py --full > profiles/r04_bench_full.json.  Lines go to $OUT (default bench_out/)
cd "$GRAFT_REPO_ROOT"
OUT=${OUT:-bench_out}; mkdir -p $OUT
hostname > $OUT/bench_all_host.txt; rocm-smi --showserial 2>/dev/null | grep -i serial >> $OUT/bench_all_host.txt
for cfg in "nodcn --workload nodcn" "att_bs32 --workload att --batch 32" "resnet34 --workload resnet34" "resnet34_nodcn --workload resnet34_nodcn" "full_split --workload full --dtype split --steps 30" "full_f32 --workload full --dtype f32 --steps 10"; do
  set -- $cfg; name=$1; shift
  timeout -k 10 400 python bench.py "$@" --full --no-h2d > $OUT/bench_$name.json 2> $OUT/bench_$name.err || echo "bench $name failed" | tee -a $OUT/bench_all_host.txt
  echo "done $name"
done
