#!/bin/bash
# rocprofv3 kernel trace (no counters) of the Z-stack branch on 8 stacks of 24 x 1024 x 1024: the per-stack loop and the batch entry
# point, one process each, two rounds per process.  Writes OUT_DIR/stack_batch_kernel_stats.csv (OUT_DIR: the first argument, default
# prof_out/stack_batch_prof under the repository): the two kernel_stats tables with a leading column path = loop | batch (launches per
# stack = Calls / 16).
#     tools/gpu_stack_batch_prof.sh [OUT_DIR]
set -e -o pipefail
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-$ROOT/prof_out/stack_batch_prof}
mkdir -p $OUT
OUT=$(cd "$OUT" && pwd)
cd $ROOT
for path in old new; do
    timeout -k 10 280 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/trace_$path -- \
        python3 tools/bench_stack.py --batch-only --batch 8 --batch-path $path > $OUT/$path.json 2> $OUT/$path.err
done
python3 - $OUT <<'PY'
import csv, glob, sys
out = sys.argv[1]
rows, header = [], None
for path, name in (("old", "loop"), ("new", "batch")):
    f = sorted(glob.glob(f"{out}/trace_{path}/**/*kernel_stats.csv", recursive=True))[0]
    with open(f) as fh:
        r = list(csv.reader(fh))
    header = ["path"] + r[0]
    rows += [[name] + x for x in r[1:]]
with open(f"{out}/stack_batch_kernel_stats.csv", "w", newline="") as fh:
    w = csv.writer(fh)
    w.writerow(header)
    w.writerows(rows)
ci = header.index("Calls")
for name in ("loop", "batch"):
    print(name, "kernel launches per stack:", sum(int(x[ci]) for x in rows if x[0] == name) / 16.0)
PY
