"""GPU: bench.py's plain run and its `--dump-outputs`, `--full` options (Qwen2-0.5B, a few steps).

* A plain run prints the headline line only: `ms_per_step` over exactly `--steps` timed steps,
  none of the `--full` legs (kernels / roofline / configs / cpu_baseline).
* `--dump-outputs DIR` writes what the timed steps computed: `token_ids.npy` (float64
  [steps][B]) and `logits.npy` (float32 [B][V]) — equal, id for id and bit for bit, to what
  a caller of the same engine gets from prefill + `decode(steps)` on the same inputs.
* `--full` adds the live kernel timings and the roofline to the same line.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import spec as S, weights as W

pytestmark = pytest.mark.gpu

P, STEPS, WARM, GEN = 24, 6, 2, 8
ARGS = ["--gpus", "1", "--model", "Qwen2-0.5B", "--prompt", str(P), "--gen", str(GEN), "--steps", str(STEPS),
        "--warmup", str(WARM), "--prefill-iters", "1"]
FULL_ONLY = ("kernels", "roofline", "configs", "cpu_baseline")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *ARGS, *extra], capture_output=True,
                       text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_plain_run_is_lean_and_dumps_what_the_timed_steps_computed(tmp_path):
    d = tmp_path / "dump"
    line = _bench("--dump-outputs", str(d))
    assert line["steps"] == STEPS and line["warmup"] == WARM and line["full"] is False
    assert line["ms_per_step"] > 0 and line["unit"] == "tokens/s" and line["higher_is_better"] is True
    assert abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-3 * line["value"]   # B = 1: tok/s = 1 / step time
    assert not [k for k in FULL_ONLY if k in line]
    ids, logits = np.load(d / "token_ids.npy"), np.load(d / "logits.npy")
    spec = S.PRESETS["Qwen2-0.5B"]
    assert ids.dtype == np.float64 and ids.shape == (STEPS, 1)
    assert logits.dtype == np.float32 and logits.shape == (1, spec.vocab)
    # the same engine, weights and prompt as bench.py's run(): prefill, then STEPS greedy steps
    max_ctx = P + max(GEN, STEPS, WARM) + 16
    eng = Q.Engine(spec, max_ctx=max_ctx).init_synthetic(W.SynthParams(seed=0))
    b = eng.batch(1, max_ctx)
    prompt = np.random.default_rng(1).integers(0, spec.vocab, size=(1, P), dtype=np.int32)
    b.prefill(0, prompt[0])
    want = b.decode(STEPS)
    assert np.array_equal(ids, want.astype(np.float64))
    assert np.array_equal(logits.view(np.uint32) >> 16, b.logits().astype(np.uint32))
    assert not (logits.view(np.uint32) & 0xFFFF).any()   # bf16 widened exactly
    b.close()
    eng.close()


def test_full_run_adds_kernel_timings_and_roofline():
    line = _bench("--full", "--no-cpu-baseline", "--no-configs")
    assert line["full"] is True and line["steps"] == STEPS and line["ms_per_step"] > 0
    assert set(line["kernels"]) == {"gate_up_gemv", "down_gemv", "qkv_gemv", "o_gemv", "lm_head_gemv", "attention"}
    assert all(k["avg_us"] > 0 for k in line["kernels"].values())
    assert line["roofline"]["achieved"] == line["kernels"]["gate_up_gemv"]["GBps"]
    assert line["cpu_baseline"] is None and "configs" not in line
