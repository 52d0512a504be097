#!/bin/bash
# bench dodge+wavy under env variants: each arg is "NAME=VALUE"
mkdir -p tools_out/var
for v in "$@"; do
  for sc in ${SCENES:-dodge wavy}; do
    extra=""; steps=50
    if [ $sc = wavy ]; then extra="--width 3840 --height 2160 --grid 16 --depth 8"; steps=5; fi
    env $v timeout -k 10 300 python bench.py --full --scene $sc --steps $steps --warmup 3 --no-cpu-baseline --no-tree-scenes --no-work-counters $extra > tools_out/var/bench_${sc}_$v.json 2> tools_out/var/bench_${sc}_$v.err || { tail -3 tools_out/var/bench_${sc}_$v.err; continue; }
    python -c "
import json; d=json.load(open('tools_out/var/bench_${sc}_$v.json')); print('$sc $v', d['value'], 'Mrays/s', d['ms_per_step'], 'ms', d['roofline']['ms_per_frame']['instrumented_frame'])"
  done
done
