#!/bin/bash
# dev tool (GPU box): bench.py with the shipped library and with every build_variants/libtmat_*.so, alternating, in one call
# usage: bash tools/gpu_lib_ab.sh <repetitions>
cd $GRAFT_REPO_ROOT
T=$(mktemp -d)
for r in $(seq 1 ${1:-2}); do
  for so in "" build_variants/libtmat_*.so; do
    [ -n "$so" ] && [ ! -f "$so" ] && continue
    echo "== [${so:-shipped}]"
    if [ -n "$so" ]; then export TMAT_HIP_LIB=$GRAFT_REPO_ROOT/$so; else unset TMAT_HIP_LIB; fi
    timeout -k 10 400 python3 bench.py --full --steps 3 --warmup 1 --no-alt --no-cpu-baseline > $T/bench.json 2> $T/bench.err || { tail -20 $T/bench.err; exit 1; }
    python3 -c "import json, sys; d=json.loads(open(sys.argv[1]).read()); print(d['value'], d['unit'], d['ms_per_step'], 'dominant', d['roofline']['avg_launch_ms'], 'path', d['roofline']['path_frac'])" $T/bench.json
  done
done
rm -rf $T
