#!/bin/bash
# Training leg alone under rocprofv3 --kernel-trace --stats (VAR=name, extra env via ENVS)
set -o pipefail
V=${VAR:-a}
ROOT="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
OUT="${OUT:-$ROOT/bench_out}"
cd /tmp && rm -rf /tmp/trp_$V && timeout -k 10 300 rocprofv3 --kernel-trace --stats -d /tmp/trp_$V -o tr --output-format csv -- \
    python "$ROOT/bench.py" --full --workload train --no-cpu-baseline --no-pmc > /tmp/trp_$V.log 2>&1 || { tail -5 /tmp/trp_$V.log; exit 1; }
mkdir -p "$OUT/trprof" && cp $(find /tmp/trp_$V -name "*kernel_stats.csv") "$OUT/trprof/tr_$V.csv"
