#!/usr/bin/env python3
"""Decode batches of 8 .. 64 slots at Qwen2-7B widths: what the 17..64-row kernel
(QIE_LINEAR_ROWS64) gives and where it loses.

Synthetic weights, a 4-layer model of Qwen2-7B's widths, bf16 and fp8, every slot placed at
position --ctx (the decode step's cost does not depend on what the cache holds).  Reports
  * decode tok/s of the captured step, B in {8, 16, 32, 64};
  * per-projection microseconds from qie_batch_time_kernel (0 gate/up, 1 down, 2 QKV, 3 O);
  * at B = 32 and 64, each projection as three qie_linear forms alternating in one process:
    the new kernel; the same rows in ceil(B / 16) pieces through the M <= 16 kernels; and (bf16)
    the generic GEMM that M > 16 takes without the flag.  Times are host-clocked batches of
    --reps launches between two synchronisations: median [min, max] over --rounds rounds.
The claim under test, reported true or false per projection: the new kernel is faster than
pieces-of-16 by more than the spread (its max below the pieces' min).
Every step runs under its own wall-clock budget (--budget seconds): a step that exceeds it ends
the run with what was measured.  Writes --out (profiles/batch64.json).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402

import gpu_util as G   # noqa: E402
import qwen_inference_engine_amd as Q   # noqa: E402
from qwen_inference_engine_amd import _lib, spec as S, weights as W   # noqa: E402

R64, FP8, T16 = _lib.QIE_LINEAR_ROWS64, _lib.QIE_LINEAR_FP8, _lib.QIE_LINEAR_FP8_T16
H, QKV, FFN = 3584, (3584, 512, 512), 18944
PROJ = {   # name: (K, segment rows, epilogue)
    "qkv": (H, QKV, _lib.QIE_EPI_STORE), "o": (H, (H,), _lib.QIE_EPI_RESIDUAL),
    "gate_up": (H, (FFN, FFN), _lib.QIE_EPI_SWIGLU), "down": (FFN, (H,), _lib.QIE_EPI_RESIDUAL)}


def mmm(v):
    return {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}


class Budget:
    def __init__(self, seconds):
        self.seconds = seconds

    def step(self, what, fn):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        print(f"[{dt:6.1f}s] {what}", flush=True)
        if dt > self.seconds:
            raise TimeoutError(f"{what}: {dt:.0f}s > {self.seconds}s")
        return out


def engine_numbers(fp8, Bs, ctx, rounds, steps):
    spec = S.ModelSpec("q7b-4l", 4, H, 28, 4, 128, FFN, 152064, False, True, False, 1e-6)
    eng = Q.Engine(spec, max_ctx=ctx + 256, weight_fp8=fp8).init_synthetic(W.SynthParams(seed=0))
    batches = {}
    for B in Bs:
        b = eng.batch(B, ctx + 256)
        for s in range(B):
            b.set_position(s, ctx, 17 + s)
        b.decode(2, want_ids=False)   # capture
        batches[B] = b
    toks = {B: [] for B in Bs}
    for _ in range(rounds):   # alternating
        for B, b in batches.items():
            for s in range(B):
                b.set_position(s, ctx, 17 + s)
            eng.sync()
            t0 = time.perf_counter()
            b.decode(steps, want_ids=False)
            eng.sync()
            toks[B].append(B * steps / (time.perf_counter() - t0))
    out = {}
    for B, b in batches.items():
        out[B] = {"tok_s_4_layers": mmm(toks[B]),
                  "time_kernel_us": {n: round(b.time_kernel(w, 50)[0], 2)
                                     for n, w in (("gate_up", 0), ("down", 1), ("qkv", 2), ("o", 3))}}
        b.close()
    eng.close()
    return out


def operator_forms(qlib, fp8, B, name, rounds, reps):
    K, segs, epi = PROJ[name]
    rng = np.random.default_rng(1)
    N = segs[0] if epi == _lib.QIE_EPI_SWIGLU else sum(segs)
    x = G.dev(G.to_bf16(rng.standard_normal((B, K)).astype(np.float32)))
    y = G.zeros_bf16(B, N)
    plain, tiled = [], []
    for r in segs:
        w = G.to_bf16((0.02 * rng.standard_normal((r, K))).astype(np.float32))
        if not fp8:
            plain.append(G.dev(w))
            continue
        q = G.zeros((int(qlib.qie_fp8_weight_bytes(r, K)),), np.uint8)
        G.check(qlib.qie_quantize_fp8(G.p(G.dev(w)), r, K, G.p(q), None))
        t = G.zeros((q.nbytes,), np.uint8)
        G.check(qlib.qie_fp8_tile16(G.p(q), r, K, G.p(t), None))
        plain.append(q)
        tiled.append(t)

    def args(M, row0, ws, flags):
        a = _lib.LinearArgsC()
        a.x, a.ldx = x.ptr + row0 * K * 2, K
        for i, (d, r) in enumerate(zip(ws, segs)):
            a.w[i], a.seg_rows[i] = d.ptr, r
        a.M, a.K, a.N, a.y, a.ldy, a.epilogue, a.flags = M, K, N, y.ptr + row0 * N * 2, N, epi, flags
        return a

    wflags = (FP8 | T16) if fp8 else 0
    ws = tiled if fp8 else plain
    forms = {"rows64": [args(B, 0, ws, wflags | R64)],
             "pieces16": [args(min(16, B - r0), r0, ws, wflags) for r0 in range(0, B, 16)]}
    if not fp8:
        forms["gemm"] = [args(B, 0, ws, 0)]
    times = {f: [] for f in forms}
    for rnd in range(rounds + 1):
        for f, launches in forms.items():
            G.check(qlib.qie_synchronize())
            t0 = time.perf_counter()
            for _ in range(reps):
                for a in launches:
                    G.check(qlib.qie_linear(C.byref(a), None), f)
            G.check(qlib.qie_synchronize())
            if rnd:   # round 0 warms up
                times[f].append((time.perf_counter() - t0) / reps * 1e6)
    out = {f: mmm(v) for f, v in times.items()}
    out["faster_than_pieces16_beyond_spread"] = out["rows64"]["max"] < out["pieces16"]["min"]
    G.release_all()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ctx", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--budget", type=float, default=120.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch64.json"))
    a = ap.parse_args()
    qlib, budget = _lib.load(), Budget(a.budget)
    res = {"model": "4 layers of Qwen2-7B widths, synthetic weights", "ctx": a.ctx, "rounds": a.rounds,
           "method": "alternating in one process; median [min, max]; operator forms host-clocked over --reps launches"}
    try:
        for fp8 in (False, True):
            wn = "fp8" if fp8 else "bf16"
            res[wn] = {"engine": budget.step(f"{wn} engine", lambda: engine_numbers(fp8, (8, 16, 32, 64), a.ctx, a.rounds, a.steps)),
                       "operator_us": {}}
            for B in (32, 64):
                for name in PROJ:
                    res[wn]["operator_us"][f"B{B}_{name}"] = budget.step(
                        f"{wn} B={B} {name}", lambda: operator_forms(qlib, fp8, B, name, a.rounds, a.reps))
    finally:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
