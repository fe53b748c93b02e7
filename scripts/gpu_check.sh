#!/bin/bash
# One GPU session: parity tests, bench, rocprof kernel stats.  Each GPU step has
# its own time limit; steps are chained with && so a failure stops the script.
set -o pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${OUT:-$ROOT/bench_out}"
cd "$ROOT"
mkdir -p "$OUT"
export TMPDIR=/tmp
TESTS=${TESTS:-tests}
timeout -k 10 ${TEST_TIMEOUT:-420} python -u -m pytest $TESTS -m gpu -x -v --timeout 180 --timeout-method thread \
    > "$OUT/gpu_tests.log" 2>&1 && echo "TESTS OK" && \
timeout -k 10 180 python -u -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1 && cat "$OUT/smoke.log" && \
timeout -k 10 240 python -u bench.py --full --steps 20 --warmup 3 > "$OUT/bench.json" 2> "$OUT/bench.err" && \
cat "$OUT/bench.json" && \
( cd /tmp && timeout -k 10 240 rocprofv3 --kernel-trace --stats -d "$OUT/prof" -o ei \
    --output-format csv -- python "$ROOT/bench.py" --full --steps 10 --warmup 2 --no-cpu-baseline \
    > "$OUT/prof.log" 2>&1 ) && echo "PROF OK"
