#!/bin/bash
# One GPU call's worth of round-2 checks, each step under its own time limit; stops at the first
# GPU fault / timeout.  Usage (on the box): [OUT=dir] tools/gpu_batch.sh STEP...   steps:
#   tests    pytest -m gpu on the files in $TESTS (default: all)
#   bench    bench.py --steps 20 --warmup 6 (the plain run: the headline figure only) -> $OUT/b_default.json
#   full     bench.py --full (defaults, CPU baseline on)                   -> $OUT/b_full.json
#   c2       bench.py --full --primary-only                                -> $OUT/b_c2.json
#   b44      bench.py --bounces 4/4                                        -> $OUT/b_44.json
#   bands1   bench.py --full --bands (the banded path over a one-rank communicator, band_parity) -> $OUT/b_bands1.json
#   counters rocprofv3 -L                                                  -> $OUT/counters.txt
# $OUT (default bench_out, under the repository root) receives the logs.
set -o pipefail
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-bench_out}
mkdir -p "$OUT"
run() {  # name seconds cmd...
    local name=$1 secs=$2; shift 2
    echo "== $name $(date +%T)"
    timeout -k 10 "$secs" "$@"
    local rc=$?
    echo "== $name rc=$rc $(date +%T)"
    if [ $rc -ne 0 ]; then exit $rc; fi
}
for step in "$@"; do
    case $step in
    tests) run tests 900 python -u -m pytest -v --timeout 240 --timeout-method thread -m gpu ${TESTS:-tests} \
               > "$OUT/tests.log" 2>&1 || exit $? ;;
    bench) run bench 200 python -u bench.py --steps 20 --warmup 6 > "$OUT/b_default.json" 2> "$OUT/b_default.err" || exit $? ;;
    full) run full 400 python -u bench.py --full > "$OUT/b_full.json" 2> "$OUT/b_full.err" || exit $? ;;
    c2) run c2 300 python -u bench.py --full --primary-only --cpu-seconds 8 > "$OUT/b_c2.json" 2> "$OUT/b_c2.err" || exit $? ;;
    b44) run b44 200 python -u bench.py --bounces 4/4 --steps 10 --warmup 4 > "$OUT/b_44.json" 2> "$OUT/b_44.err" || exit $? ;;
    bands1) run bands1 300 python -u bench.py --full --bands --steps 10 --warmup 4 --no-cpu-baseline > "$OUT/b_bands1.json" 2> "$OUT/b_bands1.err" || exit $? ;;
    counters) timeout -k 5 60 rocprofv3 -L > "$OUT/counters.txt" 2>&1; true ;;
    *) echo "unknown step $step"; exit 2 ;;
    esac
done
