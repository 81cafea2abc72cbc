#!/usr/bin/env python3
"""What the codes-only fp4 engine costs or buys at prefill: Qwen2-7B widths,
synthetic weights, one process, the two engines built once and measured in alternation:

    weight_fp4 = 1 (codes + dequantised bf16 copy; M > 16 on the bf16 GEMMs, the parent's path)
    weight_fp4 = 2 (codes only; M > 16 on gemm4_kernel)

Per round: each layer projection at ROWS rows through qie_linear (QKV, O, gate/up, down): ITERS
launches between two synchronisations under a host clock, gemm4_kernel on tiled codes against the
bf16 GEMM on bf16 weights of the same shape; prefill tok/s at P = ROWS for each engine (a host clock
around the call, which ends in a synchronise); Engine.weight_bytes() of both.  ROUNDS rounds after
a warm-up round; every figure is the median with its [min, max] over the rounds, the spread a
difference has to exceed to count.

  tools/fp4_prefill_bench.py [--layers N] [--out FILE]      -> profiles/weight_fp4_prefill.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qwen_inference_engine_amd as Q  # noqa: E402
from qwen_inference_engine_amd import _lib, spec as S, weights as W  # noqa: E402

ROWS, ITERS, ROUNDS, WARM = 2048, 20, 3, 1
H, QD, KD, I = 3584, 3584, 512, 18944
# name: (K, segment rows, epilogue)
PROJ = {"qkv": (H, (QD, KD, KD), _lib.QIE_EPI_STORE), "o": (QD, (H,), _lib.QIE_EPI_RESIDUAL),
        "gate_up": (H, (I, I), _lib.QIE_EPI_SWIGLU), "down": (I, (H,), _lib.QIE_EPI_RESIDUAL)}
FP4 = _lib.QIE_LINEAR_FP4 | _lib.QIE_LINEAR_FP4_T16 | _lib.QIE_LINEAR_FP4_GEMM


def check(lib, rc, what):
    if rc:
        raise RuntimeError("%s: %d %s" % (what, rc, lib.qie_last_error()))


def dmalloc(lib, n):
    p = C.c_void_p()
    check(lib, lib.qie_malloc(C.byref(p), int(n)), "qie_malloc")
    return p


def projection(lib, name):
    """Device buffers and the two argument blocks (bf16 weights, tiled fp4 codes) of one projection."""
    K, segs, epi = PROJ[name]
    N = segs[0] if epi == _lib.QIE_EPI_SWIGLU else sum(segs)
    x, y = dmalloc(lib, ROWS * K * 2), dmalloc(lib, ROWS * N * 2)
    check(lib, lib.qie_synthetic_fill(x, ROWS * K, 1, 7, C.c_float(1.0), C.c_float(0.0), None), "fill x")
    check(lib, lib.qie_memset(y, 0, ROWS * N * 2), "memset y")
    args = {}
    for kind in ("bf16", "fp4"):
        a = _lib.LinearArgsC()
        a.x, a.ldx, a.y, a.ldy, a.M, a.K, a.N, a.epilogue = x, K, y, N, ROWS, K, N, epi
        a.flags = FP4 if kind == "fp4" else 0
        for i, r in enumerate(segs):
            a.seg_rows[i] = r
            a.w[i] = args["bf16"][1][i] if kind == "fp4" else dmalloc(lib, r * K * 2).value
        args[kind] = (a, [a.w[i] for i in range(len(segs))])
    for i, r in enumerate(segs):   # bf16 weights, then their codes, tiled
        wb = args["bf16"][1][i]
        check(lib, lib.qie_synthetic_fill(wb, r * K, 10 + i, 7, C.c_float(0.05), C.c_float(0.0), None), "fill w")
        nb = int(lib.qie_fp4_weight_bytes(r, K))
        plain, tiled = dmalloc(lib, nb), dmalloc(lib, nb)
        check(lib, lib.qie_quantize_fp4(wb, r, K, plain, None), "quantize")
        check(lib, lib.qie_fp4_tile16(plain, r, K, tiled, None), "tile")
        args["fp4"][0].w[i] = tiled.value
    check(lib, lib.qie_synchronize(), "sync")
    return {k: v[0] for k, v in args.items()}


def time_linear(lib, a):
    check(lib, lib.qie_linear(C.byref(a), None), "qie_linear")
    check(lib, lib.qie_synchronize(), "sync")
    t0 = time.perf_counter()
    for _ in range(ITERS):
        check(lib, lib.qie_linear(C.byref(a), None), "qie_linear")
    check(lib, lib.qie_synchronize(), "sync")
    return (time.perf_counter() - t0) / ITERS * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=28)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_fp4_prefill.json"))
    o = ap.parse_args()
    lib = _lib.load()
    spec = S.tiny("qwen2-7b-widths", n_layers=o.layers, hidden=H, n_heads=28, n_kv_heads=4, head_dim=128, ffn=I,
                  vocab=152064, bias=True)
    ids = [int(t) for t in np.random.default_rng(0).integers(0, spec.vocab, ROWS)]
    eng = {m: Q.Engine(spec, max_ctx=ROWS + 64, weight_fp4=m).init_synthetic(W.SynthParams(seed=3, w_scale=0.02))
           for m in (1, 2)}
    bat = {m: e.batch(1, ROWS + 64) for m, e in eng.items()}
    proj = {n: projection(lib, n) for n in PROJ}
    rounds = []
    for r in range(WARM + ROUNDS):
        row = {}
        for n, ab in proj.items():
            row[n + "_us"] = {"mode1_bf16_gemm": time_linear(lib, ab["bf16"]), "gemm4": time_linear(lib, ab["fp4"])}
        row["prefill_tok_s"] = {}
        for m, b in bat.items():
            t0 = time.perf_counter()
            b.prefill(0, ids)
            row["prefill_tok_s"]["mode%d" % m] = ROWS / (time.perf_counter() - t0)
        if r >= WARM:
            rounds.append(row)
    summary = {k: {c: {"median": statistics.median(x[k][c] for x in rounds), "min": min(x[k][c] for x in rounds),
                       "max": max(x[k][c] for x in rounds)} for c in rounds[0][k]} for k in rounds[0]}
    out = {"rows": ROWS, "layers": o.layers, "rounds": ROUNDS, "iters": ITERS, "summary": summary,
           "weight_bytes": {"mode%d" % m: e.weight_bytes() for m, e in eng.items()},
           "method": "host clock around %d qie_linear launches between synchronisations; prefill: host clock around "
                     "one call; one process, engines alternating, median [min, max] over the rounds" % ITERS}
    with open(o.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out["summary"]), json.dumps(out["weight_bytes"]))


if __name__ == "__main__":
    main()
