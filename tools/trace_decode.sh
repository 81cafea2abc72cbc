#!/bin/bash
# Kernel-trace timeline of the headline decode (rocprofv3 --kernel-trace, no counters):
# per-kernel in-graph durations and the gaps between consecutive kernels.
# Output goes to $QIE_OUT (default bench_out/, relative to the repository root).
set -u
R=$(cd "$(dirname "$0")/.." && pwd); O=$R/${QIE_OUT:-bench_out}; mkdir -p "$O"
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --output-format csv -d "$O/trace" -o tr \
   -- python3 "$R/bench.py" --full --steps 32 --warmup 2 --prefill-iters 1 --no-cpu-baseline ${TRACE_ARGS:-} > "$O/trace.log" 2>&1
rc=$?; echo "rocprof rc=$rc"; [ $rc -eq 0 ] || exit $rc
cd "$R" && python3 tools/trace_gaps.py "$O/trace" > "$O/trace_gaps.txt" && tail -40 "$O/trace_gaps.txt"
