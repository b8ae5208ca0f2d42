#!/bin/bash
# dev tool (GPU box): rocprofv3 kernel trace (no counters) of one forward of 200 patches per narrow model; the narrow launches in launch
# order with their bounds -> <out dir>/narrow_kernel_stats.csv (profiles/narrow_kernel_stats.csv; the table of DESIGN 4.1.8)
# usage: bash tools/gpu_narrow_prof.sh [out dir, default prof_out]
ROOT=$(cd "$(dirname "$0")/.." && pwd)
cd $ROOT
DEST=${1:-prof_out}
mkdir -p $DEST
DEST=$(cd $DEST && pwd)
OUT=$DEST/narrow_prof
rm -rf $OUT && mkdir -p $OUT
echo "model,ksize,stride,cin,cout,side,patches,us,matrix_us,hbm_us,bound,fraction_of_bound,fraction_of_hbm" > $DEST/narrow_kernel_stats.csv
for m in 32 16; do
  (cd /tmp && TMPDIR=/tmp timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/$m -- python3 $ROOT/tools/bench_narrow.py --forward $m > $OUT/run_$m.log 2>&1) || { tail -20 $OUT/run_$m.log; exit 1; }
  T=$(find $OUT/$m -name "*kernel_trace.csv" | head -1)
  python3 tools/bench_narrow.py --table $T --forward $m >> $DEST/narrow_kernel_stats.csv || exit 1
  find $OUT/$m -name "*kernel_stats.csv" | head -1 | xargs -I{} cp {} $DEST/narrow_kernel_stats_rocprof_$m.csv
done
rm -rf $OUT
cat $DEST/narrow_kernel_stats.csv
