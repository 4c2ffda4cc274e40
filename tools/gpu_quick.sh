#!/bin/bash
# One GPU call: the -m gpu suite (or the tests named in $TESTS), smoke(), then the full bench line.
# Each step under its own time limit, stopping at the first failure. Outputs under $OUT/${TAG}_*.
set -o pipefail
TAG=${TAG:-r06}
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
timeout -k 10 900 python -u -m pytest ${TESTS:-tests} -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/${TAG}_gpu_tests.log 2>&1 || { echo TESTS_FAILED; tail -40 $OUT/${TAG}_gpu_tests.log; exit 1; }
tail -2 $OUT/${TAG}_gpu_tests.log
timeout -k 10 120 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1 || { echo SMOKE_FAILED; exit 1; }
tail -1 $OUT/${TAG}_smoke.log
if [ -z "$NO_BENCH" ]; then
  timeout -k 10 300 python bench.py --full > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err || { echo BENCH_FAILED; tail -5 $OUT/${TAG}_bench.err; exit 1; }
  cat $OUT/${TAG}_bench.json
fi
echo QUICK_DONE
