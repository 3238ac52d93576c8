#!/bin/bash
# One GPU pass at a milestone: GPU parity tests, the full bench line (bench.py
# --full: headline, roofline, wire observation, surface loops, CPU baseline),
# then the rocprofv3 passes of tools/profile.sh (PROFILE=0 skips them).
# Logs go to $OUT (default bench_out/).
set -u
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -x -q -m gpu --timeout 120 --timeout-method thread > "$OUT/pytest_gpu.log" 2>&1 || { echo pytest failed; tail -30 "$OUT/pytest_gpu.log"; exit 1; }
tail -1 "$OUT/pytest_gpu.log"
timeout -k 10 600 python -u bench.py --full > "$OUT/bench.log" 2> "$OUT/bench.err" || { echo bench failed; tail -20 "$OUT/bench.err"; exit 1; }
tail -1 "$OUT/bench.log"
if [ "${PROFILE:-1}" = 1 ]; then
  bash tools/profile.sh || exit 1
fi
