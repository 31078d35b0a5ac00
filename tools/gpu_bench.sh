#!/bin/bash
# bench --full + kernel-trace profile into $OUT (default: bench_out/ in the repository); every GPU
# step has its own time limit and the chain stops at the first failure.
R="$(cd "$(dirname "$0")/.." && pwd)"
cd "$R" || exit 1
O="$R/${OUT:-bench_out}"
mkdir -p "$O"
timeout -k 10 400 python bench.py --full "$@" > "$O/bench.json" 2> "$O/bench.err" || { echo "bench failed $?"; exit 1; }
cat "$O/bench.json"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d "$O/prof" -o run --output-format csv -- python3 "$R/bench.py" --full --steps 5 --warmup 2 --cpu-baseline 0 --inference 0 > "$O/prof.log" 2>&1 || { echo "rocprof failed $?"; exit 1; }
echo done
