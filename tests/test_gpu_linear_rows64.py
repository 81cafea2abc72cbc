"""GPU parity of qie_linear with QIE_LINEAR_ROWS64: the 17..64-row decode kernel (k_decode_rows64.hip).

Against the CPU oracle's product of the exactly dequantised operands, under the bounds the M <= 16
and GEMM variant tests use, through their helpers (test_gpu_ops.py).  Shapes, by the planning rule
of csrc/rows64_plan.hpp (chunks of 256 columns, parts = min(2 cus / col_blocks, chunks / 2, 16)):
  K = 64     the smallest K (one 64-column unit: a ragged first chunk), no split;
  K = 704    11 units = 3 chunks, the last one ragged, no split (chunks / 2 = 1);
  K = 4800   75 units = 19 chunks -> 7 parts of 3 chunks, the last part one ragged chunk: the
             cross-workgroup merge.
N = 87 in segments (48, 16, 23): two column blocks, the second with two live waves and a ragged last
tile; tiled fp8 takes whole tiles: (48, 16, 32).  M: one row past a 16-row tile, a full and a ragged
32, the cap.  x carries NaN rows past M - 1 and a NaN ldx pad; y a sentinel row and pad columns.
"""
import ctypes as C

import numpy as np
import pytest

import gpu_util as G
from test_gpu_fp8 import _fp8_dev
from test_gpu_linear_variants import EPI, NAN_BF16, W_SCALE, _sentinel
from test_gpu_ops import _abs_scale, _linear_args, assert_residual_close, assert_swiglu_close, rand_bf16

from qwen_inference_engine_amd import _lib, weights as W

pytestmark = pytest.mark.gpu

R64, FP8, T16 = _lib.QIE_LINEAR_ROWS64, _lib.QIE_LINEAR_FP8, _lib.QIE_LINEAR_FP8_T16
FORMS = {"bf16": 0, "fp8": FP8, "fp8_t16": FP8 | T16}
MK = [(17, 64), (32, 704), (33, 4800), (64, 4800), (64, 704), (17, 4800)]


def _segs(form, epi):
    last = 32 if form == "fp8_t16" else 23
    return (48, 16, last) if epi == "STORE" else (48 + 16 + last,)


def _weights_dev(qlib, form, w):
    """(device weights in `form`, the bf16 bits the kernel multiplies)."""
    if form == "bf16":
        return G.dev(w), w
    d, dq = _fp8_dev(qlib, w)
    if form == "fp8_t16":
        t = G.zeros((d.nbytes,), np.uint8)
        G.check(qlib.qie_fp8_tile16(G.p(d), w.shape[0], w.shape[1], G.p(t), None), "qie_fp8_tile16")
        d = t
    return d, dq


def _launch(qlib, form, epi, M, K, x, ws, bs, res=None, ldx_pad=8, ldy_pad=3):
    """One launch on x framed by NaN (3 rows past M - 1, the ldx pad) into a framed y; returns y[:M, :N]."""
    N = ws[0].shape[0] if epi == "SWIGLU" else sum(w.shape[0] for w in ws)
    xp = np.full((M + 3, K + ldx_pad), NAN_BF16, np.uint16)
    xp[:M, :K] = x
    y0 = _sentinel((M + 1, N + ldy_pad), np.uint16)
    if res is not None:
        y0[:M, :N] = res
    dws = [_weights_dev(qlib, form, w) for w in ws]
    y = G.dev(y0)
    a = _linear_args(G.dev(xp), [(d, w.shape[0]) for (d, _), w in zip(dws, ws)], [G.dev(b) for b in bs], M, K, N, y,
                     EPI[epi], ldy=N + ldy_pad, ldx=K + ldx_pad, flags=R64 | FORMS[form])
    G.check(qlib.qie_linear(C.byref(a), None), "qie_linear")
    yh = G.host(y)
    keep = np.ones(y0.shape, bool)
    keep[:M, :N] = False
    assert np.array_equal(yh[keep], y0[keep]), "wrote outside y[:M, :N]"
    return np.ascontiguousarray(yh[:M, :N]), [dq for _, dq in dws]


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("epi", ["STORE", "RESIDUAL", "SWIGLU"])
@pytest.mark.parametrize("M,K", MK)
def test_rows64_against_oracle(oracle, qlib, M, K, epi, form):
    seed = M + K
    rows = _segs(form, epi) * (2 if epi == "SWIGLU" else 1)
    x = rand_bf16(oracle, (M, K), seed=seed)
    ws = [rand_bf16(oracle, (r, K), W_SCALE[epi], seed=seed + 10 + i) for i, r in enumerate(rows)]
    bs = [rand_bf16(oracle, (r,), 0.1, seed=seed + 20 + i) for i, r in enumerate(rows)] if epi == "STORE" else []
    res = rand_bf16(oracle, (M, rows[0]), seed=seed + 40) if epi == "RESIDUAL" else None
    got, ws = _launch(qlib, form, epi, M, K, x, ws, bs, res)
    assert np.isfinite(G.bf(got)).all()
    if epi == "STORE":
        want = np.concatenate([oracle.matmul(x, w, b) for w, b in zip(ws, bs)], axis=1)
        G.assert_sum_close(got, want, np.concatenate([_abs_scale(oracle, x, w) for w in ws], axis=1), what="STORE")
    elif epi == "RESIDUAL":
        acc = oracle.matmul(x, ws[0])
        assert_residual_close(got, oracle.resadd(res, acc), acc, _abs_scale(oracle, x, ws[0]))
    else:
        gate, up = oracle.matmul(x, ws[0]), oracle.matmul(x, ws[1])
        assert_swiglu_close(got, oracle.silu_mul(gate, up), gate, up, _abs_scale(oracle, x, ws[0]),
                            _abs_scale(oracle, x, ws[1]))


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("M,K", [(33, 704), (64, 4800)])
def test_rows64_integers_bit_exact(oracle, qlib, M, K, form):
    """Small integers (weights in {-2..2}: exact e4m3 codes under a power-of-two row scale): every
    fp32 sum is exact in any order, so y = bf16(sum + bias) has one right answer.  Row m and column
    n carry their own patterns, so a wrong row <-> tile or column <-> lane mapping shows."""
    r = np.random.default_rng(M * K)
    rows = _segs(form, "STORE")
    xi = r.integers(-3, 4, (M, K)) * (r.random((M, K)) < 0.25)
    wi = [r.integers(-2, 3, (n, K)) for n in rows]
    bi = [r.integers(-8, 9, (n,)) for n in rows]
    f = lambda a: oracle.f32_to_bf16(a.astype(np.float32))
    got, dq = _launch(qlib, form, "STORE", M, K, f(xi), [f(w) for w in wi], [f(b) for b in bi])
    for w, d in zip(wi, dq):
        assert np.array_equal(f(w), d), "the integer weights are not exact in this form"
    want = np.concatenate([xi @ w.T + b for w, b in zip(wi, bi)], axis=1)
    assert np.abs(want).max() < 2 ** 24
    assert np.array_equal(got, G.to_bf16(want.astype(np.float32)))


@pytest.mark.parametrize("what", ["fp4", "fp4_gemm", "keys", "norm", "f32", "m16", "m65"])
def test_rows64_refusals(oracle, qlib, what):
    M = {"m16": 16, "m65": 65}.get(what, 32)
    K, N = 128, 32
    x, w = rand_bf16(oracle, (M, K), seed=1), rand_bf16(oracle, (N, K), 0.05, seed=2)
    y0 = _sentinel((M, N), np.float32 if what == "f32" else np.uint16)
    y = G.dev(y0)
    flags = R64 | {"fp4": _lib.QIE_LINEAR_FP4, "fp4_gemm": _lib.QIE_LINEAR_FP4 | _lib.QIE_LINEAR_FP4_GEMM}.get(what, 0)
    a = _linear_args(G.dev(x), [(G.dev(w), N)], [], M, K, N, y, EPI["F32" if what == "f32" else "STORE"], flags=flags,
                     keys=G.dev(np.zeros(M, np.uint64)) if what == "keys" else None,
                     norm_w=G.dev(oracle.f32_to_bf16(np.ones(K, np.float32))) if what == "norm" else None)
    assert qlib.qie_linear(C.byref(a), None) == -22
    assert b"QIE_LINEAR_ROWS64" in qlib.qie_last_error(), qlib.qie_last_error()
    G.check(qlib.qie_synchronize())
    assert np.array_equal(G.host(y).view(np.uint8), y0.view(np.uint8))
