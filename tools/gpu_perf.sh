#!/bin/bash
# Parity tests, then the three decode benches (fp8 B=8, bf16 B=8, bf16 B=1 headline) with
# per-kernel timings (bench.py --full); stops at the first failure.  Logs go to $QIE_OUT
# (default bench_out/ under the repository root).
set -u
cd "$(dirname "$0")/.."
export O=${QIE_OUT:-bench_out}; mkdir -p "$O"
timeout -k 10 600 python -m pytest tests -m gpu -q -x -p no:cacheprovider > $O/pytest_gpu.log 2>&1
rc=$?; tail -3 $O/pytest_gpu.log; [ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python bench.py --full --fp8 --batch 8 --prompt 1024 --gen 256 --no-cpu-baseline > $O/bench_fp8.log 2>&1 || exit $?
timeout -k 10 300 python bench.py --full --batch 8 --prompt 1024 --gen 256 --no-cpu-baseline > $O/bench_b8.log 2>&1 || exit $?
timeout -k 10 300 python bench.py --full --no-cpu-baseline > $O/bench_b1.log 2>&1 || exit $?
python - <<'PY'
import json, os
for f in ("bench_fp8","bench_b8","bench_b1"):
    for l in open(os.path.join(os.environ["O"], f"{f}.log")):
        if l.startswith("{"):
            d=json.loads(l); print(f, d["value"], d["ms_per_step"], {k:(v["avg_us"]) for k,v in d["kernels"].items()})
PY
