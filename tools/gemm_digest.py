#!/usr/bin/env python3
"""One SHA-256 per prefill-GEMM case (tools/ab_gemm.py compares variants inside one process and
one library; this compares two LIBRARIES): run it once per build, selected by QIE_LIB, and diff
the two outputs — a refactor of k_gemm.hip must reproduce every digest.  One JSON line per case.

Cases (random bf16 data, fixed seeds; Qwen2-7B shapes):
  * the four projections at 2,048 and 8,192 rows through qie_linear's own launch choice
    (gemm8 unsplit, gemm8 split-K 2, gemm_big<128>), and the smallest shape that splits;
  * QIE_LINEAR_TILE256 / TILE128 / STREAMK forced at tests/test_gpu_ops.py's
    test_linear_big_gemm shapes, every epilogue;
  * fp8 activations (QIE_LINEAR_ACT_FP8), plain and 16-row tiled weights, the four projections
    at 2,048 rows and 256 x 3,584 x 768 (splits in 3);
  * the generic 128x128 kernel at 128 rows, bf16 and fp8 weights.
GD_TIME=1: also time the 2,048-row projections, bf16 and fp8 activations (GD_ITERS launches back
to back around a synchronise, GD_ROUNDS rounds; "us" is the list of per-round means).
GD_ONLY=time: only the timed cases."""
import ctypes as C
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gpu_util as G  # noqa: E402
from qwen_inference_engine_amd import _lib  # noqa: E402
from qwen_inference_engine_amd._lib import LinearArgsC  # noqa: E402

H, I, QKV = 3584, 18944, (3584, 512, 512)
STORE, RESIDUAL, SWIGLU, F32 = _lib.QIE_EPI_STORE, _lib.QIE_EPI_RESIDUAL, _lib.QIE_EPI_SWIGLU, _lib.QIE_EPI_F32
FP8, T16, ACT8 = _lib.QIE_LINEAR_FP8, _lib.QIE_LINEAR_FP8_T16, _lib.QIE_LINEAR_ACT_FP8
TIME = os.environ.get("GD_TIME") == "1"
ONLY_TIME = os.environ.get("GD_ONLY") == "time"
ITERS = int(os.environ.get("GD_ITERS", "20"))
ROUNDS = int(os.environ.get("GD_ROUNDS", "3"))


def rnd(shape, scale, seed):
    a = (np.random.default_rng(seed).standard_normal(shape, dtype=np.float32) * np.float32(scale))
    return (a.view(np.uint32) >> 16).astype(np.uint16)


def run_case(lib, name, M, K, segs, epi, flags=0, bias=False, timed=False):
    """segs: weight rows per segment (SWIGLU: (N, N)).  Weights bf16, or fp8 (plain / tiled) by flags."""
    sw = epi == SWIGLU
    N = segs[0] if sw else sum(segs)
    x = G.dev(rnd((M, K), 1.0, 1))
    a = LinearArgsC()
    keep = []
    for i, r in enumerate(segs):
        w = G.dev(rnd((r, K), 0.02, 10 + i))
        if flags & FP8:
            w8 = G.zeros((int(lib.qie_fp8_weight_bytes(r, K)),), np.uint8)
            G.check(lib.qie_quantize_fp8(G.p(w), r, K, G.p(w8), None))
            if flags & T16:
                wt = G.zeros((w8.nbytes,), np.uint8)
                G.check(lib.qie_fp8_tile16(G.p(w8), r, K, G.p(wt), None))
                w8 = wt
            w = w8
        keep.append(w)
        a.w[i], a.seg_rows[i] = G.p(w), r
        if bias:
            b = G.dev(rnd((r,), 0.1, 20 + i))
            keep.append(b)
            a.bias[i] = G.p(b)
    a.x, a.ldx = G.p(x), K
    if flags & ACT8:
        q, e = G.zeros((M * K,), np.uint8), G.zeros((M,), np.uint8)
        G.check(lib.qie_quantize_rows_fp8(G.p(x), K, M, K, G.p(q), K, G.p(e), None))
        keep += [q, e]
        a.x, a.x_exps = G.p(q), G.p(e)
    res = rnd((M, N), 1.0, 5) if epi != F32 else np.zeros((M, N), np.float32)
    y = G.dev(res)
    a.M, a.K, a.N, a.y, a.ldy, a.epilogue, a.flags = M, K, N, G.p(y), N, epi, flags
    G.check(lib.qie_linear(C.byref(a), None), name)
    G.check(lib.qie_synchronize())
    out = G.host(y) if epi == F32 else G.host_bf16(y)
    rec = {"case": name, "sha256": hashlib.sha256(np.ascontiguousarray(out).tobytes()).hexdigest()}
    if timed:
        us = []
        for _ in range(ROUNDS):
            t0 = time.perf_counter()
            for _ in range(ITERS):
                G.check(lib.qie_linear(C.byref(a), None))
            G.check(lib.qie_synchronize())
            us.append(round((time.perf_counter() - t0) * 1e6 / ITERS, 2))
        rec["us"] = us
    print(json.dumps(rec), flush=True)
    G.release_all()


def main():
    lib = _lib.load()
    proj = [("qkv", H, QKV, STORE, True), ("o", H, (H,), RESIDUAL, False), ("gate_up", H, (I, I), SWIGLU, False),
            ("down", I, (H,), RESIDUAL, False)]
    for name, K, segs, epi, bias in proj:
        run_case(lib, f"bf16_{name}_2048", 2048, K, segs, epi, 0, bias, timed=TIME)
        run_case(lib, f"mxt_{name}_2048", 2048, K, segs, epi, FP8 | T16 | ACT8, bias, timed=TIME)
    if ONLY_TIME:
        return
    for name, K, segs, epi, bias in proj:
        run_case(lib, f"bf16_{name}_8192", 8192, K, segs, epi, 0, bias)
        run_case(lib, f"mx_{name}_2048", 2048, K, segs, epi, FP8 | ACT8, bias)
    epis = [("store3", (200, 72, 40), STORE, True), ("residual", (320,), RESIDUAL, False), ("swiglu", (200, 200), SWIGLU, False),
            ("f32", (264,), F32, False)]
    for M, K in [(256, 896), (300, 96), (520, 32), (257, 3584)]:
        for en, segs, epi, bias in epis:
            for tn, fl in [("t256", _lib.QIE_LINEAR_TILE256), ("t128", _lib.QIE_LINEAR_TILE128), ("sk", _lib.QIE_LINEAR_STREAMK)]:
                run_case(lib, f"{tn}_{M}x{K}_{en}", M, K, segs, epi, fl, bias)
    for en, segs, epi, bias in [("store3", (200, 40, 24), STORE, True), ("residual", (264,), RESIDUAL, False),
                                ("swiglu", (264, 264), SWIGLU, False), ("f32", (264,), F32, False)]:
        run_case(lib, f"splitk_257x8192_{en}", 257, 8192, segs, epi, 0, bias)
    for fl, tag in [(FP8 | ACT8, "mx"), (FP8 | T16 | ACT8, "mxt")]:
        run_case(lib, f"{tag}_256x3584x768", 256, H, (768,), STORE, fl, False)
        run_case(lib, f"{tag}_300x896_swiglu", 300, 896, (208, 208), SWIGLU, fl, False)
    for fl, tag in [(0, "bf16"), (FP8, "fp8w")]:
        for en, segs, epi, bias in [("store3", (512, 128, 128), STORE, True), ("residual", (896,), RESIDUAL, False),
                                    ("swiglu", (640, 640), SWIGLU, False), ("f32", (264,), F32, False)]:
            run_case(lib, f"generic_{tag}_128x3584_{en}", 128, H, segs, epi, fl, bias)


if __name__ == "__main__":
    main()
