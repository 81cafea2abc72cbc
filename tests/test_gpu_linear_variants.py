"""GPU parity: every kernel instantiation the M <= 16 linear planner picks, against the CPU oracle.

One qie_linear launch per row of tests/linear_cases.py (tests/test_linear_variants_cpu.py keeps
that table complete).  Per case:
  * the library's own plan for the launch (qie_debug_linear_plan: this device's CU count, the
    library's knobs) must be the instantiation the row declares -- otherwise the case would
    silently test some other kernel;
  * x is padded to ldx with bf16 NaN (any use of the pad poisons the output); y has one extra
    row, and pad columns where ldy > N, prefilled with a sentinel that must survive bit for bit;
  * the result meets the bounds the op tests state, through the same helpers (test_gpu_ops.py):
    STORE assert_sum_close (rel 1e-5, 1 ulp; with a fused norm rel 1e-4 and 1 ulp ref / 2 hf, as
    test_linear_fused_norm_and_argmax), RESIDUAL test_linear_residual's bound, SWIGLU
    test_linear_swiglu's rule, F32 1e-5 of sum|a*w| against a float64 product; fp8 rows against
    the oracle on the dequantised weights.  A fused norm is oracle.rmsnorm, then the product; under
    the epilogues other than STORE on rows whose norm does not depend on the summation order
    (_rows_with_a_stable_norm);
  * fused arg-max keys select oracle.argmax of the kernel's own logits, plus key_col0;
  * rows whose waves walk several tasks are launched twice into fresh outputs, bit-equal.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import gpu_util as G
import linear_cases as LC
from conftest import rng
from test_gpu_fp8 import _fp8_dev
from test_gpu_ops import (_abs_scale, _linear_args, assert_f32_close, assert_residual_close, assert_swiglu_close,
                          rand_bf16)

from qwen_inference_engine_amd import _lib

pytestmark = pytest.mark.gpu

EPI = {"STORE": _lib.QIE_EPI_STORE, "RESIDUAL": _lib.QIE_EPI_RESIDUAL, "SWIGLU": _lib.QIE_EPI_SWIGLU,
       "F32": _lib.QIE_EPI_F32}
W_SCALE = {"STORE": 0.05, "RESIDUAL": 0.02, "SWIGLU": 0.08, "F32": 0.05}   # as the op tests
NAN_BF16 = 0x7FC0


def _weight(oracle, rows, K, scale, seed):
    """[rows, K] bf16 weights: normal like the op tests'; a vocabulary's 65 M elements are drawn
    as bit patterns (random sign and mantissa, magnitudes in [2^-9, 2^-3)), which takes a tenth
    of the time."""
    if rows * K < (1 << 24):
        return rand_bf16(oracle, (rows, K), scale, seed=seed)
    bits = rng(seed).integers(0, 1 << 16, (rows, K), dtype=np.uint16)
    return (bits & 0x807F) | ((118 + (bits >> 7) % 6) << 7).astype(np.uint16)


def _rows_with_a_stable_norm(oracle, M, K, nw, eps, num, seed):
    """x [M, K] (normal bf16 rows, as the op tests') and oracle.rmsnorm of it, with every row
    whose normalised values depend on the fp32 order of the sum of squares redrawn.

    The norm rounds x / rms to bf16, and bf16 x takes few distinct values, so when x / rms sits
    on a rounding boundary for one of them, the last bit of the sum moves a group of elements
    by an ulp together.  Measured with the oracle alone (its summation orders 0, sequential, and
    5, 256 strided partials): at 4 x 1,000 HF rows the two orders differ in 5 of one row's 1,000
    elements, which moves 13 of that row's 41 SwiGLU outputs by up to 10 ulps (the MT 4 GEMV
    equalled order 5 bit for bit); at 1 x 10,248 REF, 6 elements, 1.2e-5 of sum|a*w| in the
    fp32 outputs.  A kernel reduces in a third order, so such a row has no single reference:
    the rows kept here normalise to the same bits in both orders and with the mean square moved
    by +-2e-6 and +-4e-6 (the orders above differ by about 2e-6), and the epilogue bounds then
    apply unchanged.  The shift rides on eps: HF's 1e-6 - 4e-6 is negative, which only moves the
    mean square (about 1 for these rows) down by 3e-6.  Used for the RESIDUAL, SWIGLU and F32
    epilogues only: STORE rows stay unfiltered under their stated fused-norm bound."""
    def alternatives(x):
        oracle.set_sum_order(5)
        try:
            yield oracle.rmsnorm(x, nw, eps, num)
        finally:
            oracle.set_sum_order(0)
        for d in (-4e-6, -2e-6, 2e-6, 4e-6):
            yield oracle.rmsnorm(x, nw, eps + d, num)

    x = rand_bf16(oracle, (M, K), seed=seed)
    for attempt in range(1, 200):
        xn = oracle.rmsnorm(x, nw, eps, num)
        moved = np.zeros(M, bool)
        for alt in alternatives(x):
            moved |= (alt != xn).any(axis=1)
        if not moved.any():
            return x, xn
        x[moved] = rand_bf16(oracle, (M, K), seed=seed + 10000 * attempt)[moved]
    raise AssertionError("no order-stable rows found")


def _sentinel(shape, dtype):
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.uint32)
    if dtype == np.float32:   # quiet NaNs with a counting payload
        return (np.uint32(0x7FC00000) | (i * np.uint32(2654435761) >> np.uint32(10))).view(np.float32).reshape(shape)
    return ((i * np.uint32(40503) + np.uint32(0x5A5A)) & np.uint32(0xFFFF)).astype(np.uint16).reshape(shape)


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _live_plan(qlib, a):
    buf = C.create_string_buffer(512)
    G.check(qlib.qie_debug_linear_plan(C.byref(a), buf, len(buf)), "qie_debug_linear_plan")
    return buf.value.decode()


@pytest.mark.parametrize("case", LC.CASES, ids=[c.name for c in LC.CASES])
def test_linear_variant(oracle, qlib, case):
    c = case
    M, K, N, epi = c.M, c.K, LC.n_cols(c), c.epi
    seed = zlib.crc32(c.name.encode()) % 10000
    fp8 = bool(c.flags & LC.FP8)
    ldx, ldy = K + c.ldx_pad, N + c.ldy_pad

    # ---- inputs
    nw, eps = None, 1e-4
    if c.norm:
        nw = oracle.f32_to_bf16((1 + 0.2 * rng(seed + 30).standard_normal(K)).astype(np.float32))
        eps = 1e-4 if c.norm == "ref" else 1e-6
        if epi == "STORE":   # its fused-norm bound (rel 1e-4, 1 / 2 ulps) already holds a moved element
            x = rand_bf16(oracle, (M, K), seed=seed)
            xin = oracle.rmsnorm(x, nw, eps, c.norm)
        else:                # RESIDUAL / SWIGLU / F32 state no bound for one: order-stable rows
            x, xin = _rows_with_a_stable_norm(oracle, M, K, nw, eps, c.norm, seed)
    else:
        x = xin = rand_bf16(oracle, (M, K), seed=seed)
    xp = np.full((M, ldx), NAN_BF16, np.uint16)
    xp[:, :K] = x
    rows = (N, N) if epi == "SWIGLU" else c.segs
    ws = [_weight(oracle, r, K, W_SCALE[epi], seed + 10 + i) for i, r in enumerate(rows)]
    bs = [rand_bf16(oracle, (r,), 0.1, seed=seed + 20 + i) for i, r in enumerate(rows)] if c.bias else []
    if fp8:   # device codes + scales; the reference multiplies the dequantised rows
        q = [_fp8_dev(qlib, w) for w in ws]
        dws, ws = [d for d, _ in q], [dq for _, dq in q]
    else:
        dws = [G.dev(w) for w in ws]
    res = rand_bf16(oracle, (M, N), seed=seed + 40) if epi == "RESIDUAL" else None
    ydt = np.float32 if epi == "F32" else np.uint16
    y0 = _sentinel((M + 1, ldy), ydt)
    if res is not None:
        y0[:M, :N] = res

    dx, dbs, dnw = G.dev(xp), [G.dev(b) for b in bs], G.dev(nw) if c.norm else None
    segs = list(zip(dws, rows))

    def launch():
        y = G.dev(y0)
        keys = G.dev(np.zeros(M, np.uint64)) if c.key_col0 is not None else None
        a = _linear_args(dx, segs, dbs, M, K, N, y, EPI[epi], norm_w=dnw, eps=eps, num=1 if c.norm == "hf" else 0,
                         keys=keys, ldy=ldy, flags=c.flags, ldx=ldx, key_col0=c.key_col0 or 0)
        plan = _live_plan(qlib, a)
        assert LC.plan_key(plan) == c.plan, f"{c.name}: the library plans {plan}"
        G.check(qlib.qie_linear(C.byref(a), None), "qie_linear")
        ids = None
        if keys is not None:
            ids = G.zeros((M,), np.int32)
            G.check(qlib.qie_keys_to_ids(G.p(keys), M, G.p(ids), None))
            ids = G.host(ids)
        return G.host(y), ids

    yh, ids = launch()
    if c.twice:
        yh2, ids2 = launch()
        assert np.array_equal(_bits(yh), _bits(yh2)), f"{c.name}: two launches differ"
        assert ids is None or np.array_equal(ids, ids2)

    # ---- nothing written outside [M, N]
    untouched = np.ones(y0.shape, bool)
    untouched[:M, :N] = False
    assert np.array_equal(_bits(yh)[untouched], _bits(y0)[untouched]), f"{c.name}: wrote outside y[:M, :N]"
    got = np.ascontiguousarray(yh[:M, :N])

    # ---- the epilogue's bound
    if epi == "STORE":
        want = np.concatenate([oracle.matmul(xin, w, bs[i] if bs else None) for i, w in enumerate(ws)], axis=1)
        scale = np.concatenate([_abs_scale(oracle, xin, w) for w in ws], axis=1)
        print(f"{c.name}: max {G.ulp_diff(got, want).max()} ulps, exact {(got == want).mean():.4f}")
        G.assert_sum_close(got, want, scale, rel=1e-4 if c.norm else 1e-5, ulps=2 if c.norm == "hf" else 1,
                           what=c.name)
    elif epi == "RESIDUAL":
        acc = oracle.matmul(xin, ws[0])
        want = oracle.resadd(res, acc)
        print(f"{c.name}: max {G.ulp_diff(got, want).max()} ulps, exact {(got == want).mean():.4f}")
        assert_residual_close(got, want, acc, _abs_scale(oracle, xin, ws[0]))
    elif epi == "SWIGLU":
        gate, up = oracle.matmul(xin, ws[0]), oracle.matmul(xin, ws[1])
        want = oracle.silu_mul(gate, up)
        print(f"{c.name}: max {G.ulp_diff(got, want).max()} ulps, exact {(got == want).mean():.4f}")
        assert_swiglu_close(got, want, gate, up, _abs_scale(oracle, xin, ws[0]), _abs_scale(oracle, xin, ws[1]))
    else:
        want = oracle.bf16_to_f32(xin).astype(np.float64) @ oracle.bf16_to_f32(ws[0]).astype(np.float64).T
        scale = _abs_scale(oracle, xin, ws[0])
        print(f"{c.name}: max error {np.abs(got - want).max():.3e}, {np.abs(got - want).max() / scale.max():.2e} "
              f"of sum|a*w|")
        assert_f32_close(got, want, scale)

    # ---- fused arg-max: the reference rule on the kernel's own logits
    if ids is not None:
        for m in range(M):
            assert ids[m] == oracle.argmax(got[m]) + c.key_col0, (c.name, m)


@pytest.mark.parametrize("name,M,K,N,epi,words", LC.REFUSALS, ids=[r[0] for r in LC.REFUSALS])
def test_linear_refuses_a_norm_it_cannot_fuse(oracle, qlib, name, M, K, N, epi, words):
    """A fused norm where no kernel can hold the rows (x past the GEMV's 96 KiB of LDS; 16 rows
    past the skinny kernel's 120 KiB, which the GEMM then declines): an error return that names
    the cause, and an untouched output -- never a projection of the un-normed rows."""
    x = rand_bf16(oracle, (M, K), seed=1)
    w = rand_bf16(oracle, (N, K), 0.05, seed=2)
    nw = oracle.f32_to_bf16(np.ones(K, np.float32))
    y0 = _sentinel((M, N), np.uint16)
    y = G.dev(y0)
    a = _linear_args(G.dev(x), [(G.dev(w), N)], [], M, K, N, y, EPI[epi], norm_w=G.dev(nw))
    assert qlib.qie_linear(C.byref(a), None) == -22
    assert words.encode() in qlib.qie_last_error(), qlib.qie_last_error()
    G.check(qlib.qie_synchronize())
    assert np.array_equal(G.host(y), y0)
