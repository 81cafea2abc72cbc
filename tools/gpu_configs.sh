#!/bin/bash
# The BASELINE.md single-GPU configurations besides the headline (bench.py --full lines), then a
# kernel trace of config 4 (fp8 weights, batch 8) for its in-graph per-kernel durations.
# Logs go to $QIE_OUT (default bench_out/, relative to the repository root).
set -u
R=${GRAFT_REPO_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}
cd "$R"; O=${QIE_OUT:-bench_out}; mkdir -p $O
timeout -k 10 300 python bench.py --full --no-cpu-baseline --fp8 --batch 8 --prompt 1024 --gen 256 --steps 255 > $O/cfg4_fp8.log 2>&1 || exit $?
timeout -k 10 300 python bench.py --full --no-cpu-baseline --batch 8 --prompt 1024 --gen 256 --steps 255 > $O/cfg4_bf16.log 2>&1 || exit $?
timeout -k 10 300 python bench.py --full --no-cpu-baseline --model Qwen2-0.5B --prompt 128 --gen 128 --steps 127 > $O/cfg2.log 2>&1 || exit $?
for f in cfg4_fp8 cfg4_bf16 cfg2; do tail -1 $O/$f.log | cut -c1-400; echo; done
if [ "${TRACE:-1}" = "1" ]; then
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$R/$O/prof_cfg4" -o run \
     -- python3 "$R/bench.py" --full --no-cpu-baseline --fp8 --batch 8 --prompt 1024 --gen 256 --steps 64 --warmup 4 --prefill-iters 1 \
     > "$R/$O/prof_cfg4.log" 2>&1
  rc=$?; echo "rocprof rc=$rc"; exit $rc
fi
