#!/bin/bash
# bench the library variants given as arguments (lib names under raytracer-in-cpp_amd/lib) on cube and dodge
mkdir -p tools_out
for lib in "$@"; do
  for sc in cube dodge; do
    RT_LIB=$PWD/raytracer-in-cpp_amd/lib/$lib python bench.py --full --scene $sc --steps 20 --warmup 3 --no-cpu-baseline > tools_out/v.json 2> tools_out/v.err || tail -3 tools_out/v.err
    python -c "
import json; d=json.load(open('tools_out/v.json')); print('$lib $sc', d['ms_per_step'], 'ms', d['roofline']['ms_per_frame']['instrumented_frame'])"
  done
done
