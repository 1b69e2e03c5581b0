#!/bin/bash
# debug: bench.py's two-rank rehearsal (both ranks on cuda:0, gloo) with and without the small-M kernel; a ticker keeps the watchdog quiet
cd "$(dirname "$0")/.."; OUT=${OUT:-bench_out}; mkdir -p $OUT
(while true; do sleep 45; echo tick; done) & T=$!
A="--full --gpus 2 --steps 6 --warmup 2 --batch 8 --inflight 2 --no-cpu-baseline --no-roofline --no-parity"
for e in ""; do
  env $e GP_BENCH_REHEARSE=1 timeout -k 10 150 python -u bench.py $A > $OUT/spawn_$$.json 2> $OUT/spawn_$$.err; echo "[$e] rc=$?"; grep -v amdgpu $OUT/spawn_$$.err | tail -4 | cut -c1-1200
done
kill $T
