#!/bin/bash
# Diagnostic: rocprofv3 kernel trace of the whole bench (C2 + C3/C4 extras, bench.py --full) -> $OUT/px (bench_out/px);
# summarised by tools/trace_summary.py (per-kernel average durations).
cd "$(dirname "$0")/.." || exit 1
export TMPDIR=/tmp
OUT=${OUT:-bench_out}
mkdir -p "$OUT/px"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/px" -o run -- python3 bench.py --full --steps 3 --warmup 1 --cpu-baseline off > "$OUT/px/b.log" 2>&1
