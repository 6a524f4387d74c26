#!/bin/bash
# One GPU-box session: GPU tests, then the full 1-GPU bench.  Stops at the first GPU fault / timeout.
# Logs go to $BE_CI_OUT (default ci_out/).
set -o pipefail
OUT=${BE_CI_OUT:-ci_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest tests -m gpu -x -v --timeout 300 --timeout-method thread ${PYTEST_ARGS:-} > "$OUT/gpu_tests.log" 2>&1
rc=$?
echo "pytest rc=$rc" >> "$OUT/gpu_tests.log"
tail -3 "$OUT/gpu_tests.log"
case $rc in 0) ;; *) echo "pytest failed rc=$rc"; exit $rc;; esac
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:-} > "$OUT/bench.log" 2>&1
rc=$?
echo "bench rc=$rc" >> "$OUT/bench.log"
tail -2 "$OUT/bench.log"
exit $rc
