#!/bin/bash
# GPU box: the round's committed evidence -- tools/profile.sh (kernel trace + stats and the PMC passes of the C2
# bench), then the full bench line (bench.py --full: CPU baseline and extras included). Logs under $OUT (bench_out/).
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-bench_out}
mkdir -p "$OUT" && export TMPDIR=/tmp
bash tools/profile.sh > "$OUT/profile.txt" 2>&1
rc=$?; cat "$OUT/profile.txt"; [ $rc -ne 0 ] && exit $rc
timeout -k 10 600 python -u bench.py --full > "$OUT/bench_full.log" 2>&1
rc=$?; echo "bench rc=$rc"; tail -c 400 "$OUT/bench_full.log"
exit $rc
