#!/bin/bash
# EI kernel iteration: GP parity tests, then the EI bench leg (+ rocprof stats).
set -o pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${OUT:-$ROOT/bench_out}"
cd "$ROOT"
mkdir -p "$OUT"
export TMPDIR=/tmp
TAG=${TAG:-ei}
timeout -k 10 300 python -u -m pytest ${TESTS:-tests/test_gp_gpu.py tests/test_optimizer_gpu.py} -m gpu -x -q --timeout 120 --timeout-method thread \
    > "$OUT/ei_tests_$TAG.log" 2>&1 && tail -2 "$OUT/ei_tests_$TAG.log" && \
timeout -k 10 300 python -u bench.py --full --workload ei --steps 20 --warmup 3 --no-cpu-baseline ${BENCH_EXTRA:---no-pmc} \
    > "$OUT/ei_bench_$TAG.json" 2> "$OUT/ei_bench_$TAG.err" && cat "$OUT/ei_bench_$TAG.json" && \
( cd /tmp && timeout -k 10 200 rocprofv3 --kernel-trace --stats -d /tmp/prof_$TAG -o run --output-format csv -- \
    python "$ROOT/bench.py" --full --workload ei --steps 10 --warmup 2 --no-cpu-baseline --no-pmc > "$OUT/ei_prof_$TAG.log" 2>&1 ) && \
mkdir -p "$OUT/prof_$TAG" && find /tmp/prof_$TAG -name "*kernel_stats.csv" -exec cp {} "$OUT/prof_$TAG/" \; && \
grep -h "gp_score" "$OUT/prof_$TAG"/*kernel_stats.csv
