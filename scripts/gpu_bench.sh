#!/bin/bash
# The whole benchmark (every leg: --full); BENCH_ARGS adds flags.  Output under $OUT.
set -o pipefail
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${OUT:-$ROOT/bench_out}"
cd "$ROOT"
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 400 python -u bench.py --full ${BENCH_ARGS} > "$OUT/bench.json" 2> "$OUT/bench.err" && cat "$OUT/bench.json"
