#!/usr/bin/env python3
"""What MXFP4 projection weights buy: Qwen2-7B widths at full depth, synthetic
weights, one process, four engines built once and measured in alternation:

    bf16 | weight_fp8 | weight_fp4 | weight_fp4 + weight_fp8 (fp4 projections, fp8 lm_head)

Per engine and round:
  * qie_batch_time_kernel (event timing inside the library, the decode step's own launches on
    scratch outputs) for gate/up, down, QKV and O at B = 1 and B = 8: µs, algorithmic bytes, TB/s;
  * decode tok/s at B = 1 (context 2,048, contiguous cache) and at B = 8 (paged cache, context 512
    per slot): DECODE_STEPS graph-replayed steps per call, a host clock around the call (it ends
    in a stream synchronise), every slot put back to its position before the next call;
  * one qie_verify step of 16 rows (15 drafts) at B = 1.
ROUNDS rounds with the engines alternating inside each; every figure is the median over the rounds
with its [min, max] — the spread a difference has to exceed to count.  The comparison that matters
is weight_fp4 against weight_fp8: same build, same session, and the fp8 kernels are the parent
commit's.  Every GPU step runs under its own time limit (a watchdog thread: status 124).

  tools/fp4_bench.py [--layers N] [--out FILE]      -> profiles/weight_fp4.json
"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qwen_inference_engine_amd as Q  # noqa: E402
from qwen_inference_engine_amd import spec as S, weights as W  # noqa: E402

ENGINES = {"bf16": {}, "weight_fp8": {"weight_fp8": True}, "weight_fp4": {"weight_fp4": True},
           "fp4_fp8_head": {"weight_fp4": True, "weight_fp8": True}}
KERNELS = {0: "gate_up", 1: "down", 2: "qkv", 3: "o"}
CTX1, CTX8, PAGE = 2048, 512, 128
DECODE_STEPS, KERNEL_ITERS, ROUNDS, WARM = 64, 50, 3, 1
OUT = os.path.join(ROOT, "profiles", "weight_fp4.json")


class step_limit:
    """A time limit around one GPU step: past it a watchdog thread ends the process (status 124)."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _expired(self):
        sys.stderr.write("fp4_bench: %s exceeded its %d s limit\n" % (self.what, self.seconds))
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, self._expired)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


def build(kind, spec):
    eng = Q.Engine(spec, max_ctx=CTX1 + 128, **ENGINES[kind]).init_synthetic(W.SynthParams(seed=0))
    r = np.random.default_rng(3)
    b1 = eng.batch(1, CTX1 + 128)
    ids = [int(t) for t in r.integers(0, spec.vocab, CTX1 + 16)]
    t1 = b1.prefill(0, ids[:CTX1])
    b8 = eng.batch(8, CTX8 + 128, page_tokens=PAGE)
    p8 = [[int(t) for t in r.integers(0, spec.vocab, CTX8)] for _ in range(8)]
    t8 = b8.prefill_batch(0, p8)
    return {"eng": eng, "b1": b1, "t1": [t1], "b8": b8, "t8": list(t8), "draft": ids[CTX1:CTX1 + 15]}


def measure(m):
    out = {}
    for B, b in ((1, m["b1"]), (8, m["b8"])):
        for which, name in KERNELS.items():
            us, by = b.time_kernel(which, KERNEL_ITERS)
            out["%s_B%d" % (name, B)] = {"us": us, "bytes": by, "TBps": by / us * 1e-6}
    for B, b, toks, ctx in ((1, m["b1"], m["t1"], CTX1), (8, m["b8"], m["t8"], CTX8)):
        for rep in range(WARM + 1):
            for s in range(B):
                b.set_position(s, ctx, toks[s])
            t0 = time.perf_counter()
            b.decode(DECODE_STEPS)
            dt = time.perf_counter() - t0
        out["decode_B%d" % B] = {"tok_s": B * DECODE_STEPS / dt, "ms_per_step": dt / DECODE_STEPS * 1e3}
    b = m["b1"]
    for rep in range(WARM + 3):
        b.set_position(0, CTX1, m["t1"][0])
        t0 = time.perf_counter()
        b.verify(0, m["draft"])
        dt = time.perf_counter() - t0
    out["verify_M16"] = {"ms": dt * 1e3}
    b.set_position(0, CTX1, m["t1"][0])
    return out


def summarise(rounds):
    """{figure: {field: {median, min, max}}} over the rounds of one engine."""
    res = {}
    for fig in rounds[0]:
        res[fig] = {}
        for field in rounds[0][fig]:
            v = [r[fig][field] for r in rounds]
            res[fig][field] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than Qwen2-7B's 28 (rehearsal)")
    args = ap.parse_args()
    spec = S.QWEN2_7B if args.layers is None else S.QWEN2_7B.replace(n_layers=args.layers)
    models = {}
    for kind in ENGINES:
        with step_limit(300, "building and prefilling %s" % kind):
            models[kind] = build(kind, spec)
        print("built", kind, flush=True)
    rounds = {k: [] for k in ENGINES}
    for rnd in range(ROUNDS + 1):                       # round 0 warms every shape (captures) and is dropped
        for kind in ENGINES:
            with step_limit(240, "%s round %d" % (kind, rnd)):
                r = measure(models[kind])
            if rnd:
                rounds[kind].append(r)
        print("round", rnd, "done", flush=True)
    doc = {"model": "Qwen2-7B widths, %d layers, synthetic weights" % spec.n_layers,
           "method": "qie_batch_time_kernel (%d launches, events) per projection; decode: %d graph steps per call under "
                     "a host clock, B = 1 at context %d, B = 8 paged (%d-token pages) at context %d; verify: 16 rows at "
                     "context %d; %d rounds after one warm-up round, engines alternating: median [min, max]"
                     % (KERNEL_ITERS, DECODE_STEPS, CTX1, PAGE, CTX8, CTX1, ROUNDS),
           "engines": {k: summarise(v) for k, v in rounds.items()}}
    # the comparison that matters: fp4 against fp8, with the rounds' spread beside it
    cmp = {}
    f8, f4 = doc["engines"]["weight_fp8"], doc["engines"]["weight_fp4"]
    for fig in f8:
        field = "us" if "us" in f8[fig] else ("ms_per_step" if "ms_per_step" in f8[fig] else "ms")
        a, b = f8[fig][field], f4[fig][field]
        cmp[fig] = {"fp8": a["median"], "fp4": b["median"], "fp4_over_fp8": round(b["median"] / a["median"], 4),
                    "faster_beyond_spread": b["max"] < a["min"]}
    doc["fp4_vs_fp8"] = cmp
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    for fig, c in cmp.items():
        print("%-12s fp8 %10.3f  fp4 %10.3f  ratio %.3f  %s" % (fig, c["fp8"], c["fp4"], c["fp4_over_fp8"],
                                                                "beyond spread" if c["faster_beyond_spread"] else ""))
    for m in models.values():
        m["b1"].close()
        m["b8"].close()
        m["eng"].close()


if __name__ == "__main__":
    main()
