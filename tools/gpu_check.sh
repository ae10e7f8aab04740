#!/bin/bash
# One GPU session: parity tests, bench, rocprofv3 kernel stats.  Usage: tools/gpu_check.sh TAG
# Outputs go to $OUT (default profile_out/).
set -o pipefail
TAG=${1:-run}
OUT=${OUT:-profile_out}
export TMPDIR=/tmp
mkdir -p "$OUT"
timeout -k 10 600 python -u -m pytest tests/ -q -m gpu -x --timeout 120 --timeout-method thread > $OUT/pytest_$TAG.log 2>&1
rc=$?
echo "pytest rc=$rc"; tail -3 $OUT/pytest_$TAG.log
# A fault, abort or time limit ends the session (no further GPU step).
case $rc in 0|1) ;; *) exit $rc ;; esac
timeout -k 10 400 python bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { echo "bench failed"; tail -20 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python bench.py --full --steps 50 --warmup 10 --no-cpu-baseline > $OUT/prof_$TAG.log 2>&1 || { echo "bench prof failed"; exit 1; }
# Roofline pass alone under rocprofv3: its k_blur average must match bench.py's avg_launch_us.
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/roof_$TAG -o run --output-format csv -- python bench.py --roofline-only --steps 100 > $OUT/roof_$TAG.json 2> $OUT/roof_$TAG.err
echo "roofline prof rc=$?"
