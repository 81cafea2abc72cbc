"""The MXFP4 prefill GEMM (csrc/k_gemm_fp4.hip; QIE_LINEAR_FP4 | _FP4_GEMM at M > 16) and the codes-only
engine (weight_fp4 = 2).  Rows are gemm_cases.Case tuples under its protocol: x and biases between NaN
guards, x padded to ldx with NaN, y in gemm_cases.frame(), the live plan asserted, `twice` rows run twice.
Exact cases: integer activations in [-4, 4] and codes under block scales 2^-1 .. 2^1 make every product a
multiple of 1/4 below 48 and every sum below 2^17 (K <= 2,048): exact in fp32 in any order, so F32
equals the float64 product bit for bit and a bf16 epilogue its rounding (gemm_cases.expected)."""
import ctypes as C

import numpy as np
import pytest

import gemm_cases as GC
import gpu_util as G
from conftest import rng
from parity import OrderPair
from test_gpu_engine import SYN, forced_compare
from test_gpu_fp4 import FP4_CONFIGS, _fp4_pair, _tiled
from test_gpu_gemm_variants import _At, _guarded_bias, _guarded_rows, _is_nan, _swiglu_reference
from test_gpu_linear_variants import EPI, W_SCALE, _live_plan, _sentinel, _weight
from test_gpu_ops import (_abs_scale, _linear_args, assert_f32_close, assert_residual_close, assert_swiglu_close,
                          rand_bf16)

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib, weights as W

pytestmark = pytest.mark.gpu

FP4, T16, GEMM = _lib.QIE_LINEAR_FP4, _lib.QIE_LINEAR_FP4_T16, _lib.QIE_LINEAR_FP4_GEMM

def _case(name, M, K, segs, epi, tiled=0, ldx_pad=0, ldy_pad=0, splitk=1):
    return GC.C(name, M, K, segs, epi, f"gemm4_kernel<{epi},{tiled}> splitk={splitk} ", FP4 | GEMM | (T16 if tiled else 0),
                ldx_pad, ldy_pad, bias=(epi == "STORE"), twice=splitk > 1)

def _rows(c):
    return (GC.n_cols(c),) * 2 if c.epi == "SWIGLU" else c.segs

def _launch(qlib, c, x, dws, bs, y0):
    """The framed output of row c on device weights dws (plain layout; tiled here where c asks)."""
    N, ldx, ldy = GC.n_cols(c), c.K + c.ldx_pad, y0.shape[1]
    if c.flags & T16:
        dws = [_tiled(qlib, d, n, c.K) for d, n in zip(dws, _rows(c))]
    dx, dbs = _guarded_rows(x, ldx), [_guarded_bias(b) for b in bs]
    outs = []
    for _ in range(2 if c.twice else 1):
        y = G.dev(y0)
        a = _linear_args(dx, list(zip(dws, _rows(c))), dbs, c.M, c.K, N, _At(y, ldy * y0.dtype.itemsize), EPI[c.epi],
                         ldy=ldy, flags=c.flags, ldx=ldx)
        assert _live_plan(qlib, a).startswith(c.plan), _live_plan(qlib, a)
        G.check(qlib.qie_linear(C.byref(a), None), "qie_linear")
        outs.append(G.host(y))
    assert all(np.array_equal(GC.bits(outs[0]), GC.bits(o)) for o in outs), f"{c.name}: two launches differ"
    outside = np.ones(y0.shape, bool)
    outside[1:c.M + 1, :N] = False
    assert np.array_equal(GC.bits(outs[0])[outside], GC.bits(y0)[outside]), f"{c.name}: wrote outside y[:M, :N]"
    return outs[0]

def _exact_weight(qlib, rows, K, seed):
    r = rng(seed)   # every code byte, scale bytes 126 .. 128; the reference is the library's (own test: test_dequantize_device_exact)
    packed = np.concatenate([r.integers(0, 256, rows * K // 2).astype(np.uint8),
                             r.integers(126, 129, rows * K // 32).astype(np.uint8)])
    d = G.dev(packed)
    out = G.zeros_bf16(rows, K)
    G.check(qlib.qie_dequantize_fp4(G.p(d), rows, K, G.p(out), None))
    return d, G.host_bf16(out)

EXACT = [
    _case("m17_k128_n40_f32", 17, 128, 40, "F32"),
    _case("m17_k384_store3_bias", 17, 384, (32, 16, 24), "STORE", 0, 8, 3),
    _case("m256_k1024_n40_res", 256, 1024, 40, "RESIDUAL", 0, 0, 5),
    _case("m257_k384_n40_swiglu", 257, 384, 40, "SWIGLU", 0, 16),
    _case("m257_k128_n272_t16_f32", 257, 128, 272, "F32", 1, 0, 3),
    _case("m17_k1024_n272_t16_swiglu", 17, 1024, 272, "SWIGLU", 1),
    _case("m256_k384_t16_store3_bias", 256, 384, (32, 16, 224), "STORE", 1, 8),
    _case("m257_k1024_n272_t16_res", 257, 1024, 272, "RESIDUAL", 1),
    _case("split2_m40_k2048_n272_t16_f32", 40, 2048, 272, "F32", 1, splitk=2),
    _case("split2_m257_k2048_n40_store_bias", 257, 2048, 40, "STORE", 0, 0, 3, splitk=2),
]

@pytest.mark.parametrize("c", EXACT, ids=[c.name for c in EXACT])
def test_fp4_gemm_exact(oracle, qlib, c):
    M, K, N = c.M, c.K, GC.n_cols(c)
    r = rng(M + K + N)
    x = GC.to_bf16(r.integers(-4, 5, (M, K)).astype(np.float32))
    q = [_exact_weight(qlib, n, K, 100 + i) for i, n in enumerate(_rows(c))]
    bs = [rand_bf16(oracle, (n,), 0.5, seed=7 + i) for i, n in enumerate(c.segs)] if c.bias else []
    res = rand_bf16(oracle, (M, N), seed=9) if c.epi == "RESIDUAL" else None
    inp = GC.Inputs(x, [w for _, w in q], bs, res, GC.frame(c, res))
    if c.epi == "SWIGLU":   # (expected()'s closed form of silu needs gates >= 17: the oracle's silu instead)
        acc = (GC.bf(x).astype(np.float64) @ GC.bf(np.concatenate(inp.ws)).astype(np.float64).T).astype(np.float32)
        want = oracle.silu_mul(GC.to_bf16(acc[:, :N]), GC.to_bf16(acc[:, N:]))
    else:
        want = GC.expected(c, "F1", inp)
    ok, why = GC.accepted(c, _launch(qlib, c, x, [d for d, _ in q], bs, inp.y0), inp.y0, want)
    assert ok, why

@pytest.mark.parametrize("K,N,tiled", [(384, 48, 1), (1152, 40, 0)])
def test_fp4_gemm_needle_weights_pick_single_columns(qlib, K, N, tiled):
    c = _case(f"needle_k{K}", 33, K, N, "F32", tiled)
    inp = GC.inputs(c, "F2")
    d, dq = _fp4_pair(qlib, inp.ws[0])
    assert np.array_equal(dq, inp.ws[0])
    ok, why = GC.accepted(c, _launch(qlib, c, inp.x, [d], [], inp.y0), inp.y0, GC.expected(c, "F2", inp))
    assert ok, why

RANDOM = [_case(f"random_{e.lower()}", 300, 896, s, e, 0, 8, 3)
          for e, s in (("STORE", (32, 16, 24)), ("RESIDUAL", 41), ("SWIGLU", 40), ("F32", 24))]

@pytest.mark.parametrize("c", RANDOM, ids=[c.name for c in RANDOM])
def test_fp4_gemm_random_data(oracle, qlib, c):
    """gemm_cases' F3 as test_gemm_random holds it, on the dequantised weights: its dot-product bounds, then x
    row r* all NaN (255, the first row tile's last, or M - 1): row r* of y all NaN, the others bit-equal."""
    M, K, N, epi = c.M, c.K, GC.n_cols(c), c.epi
    x = rand_bf16(oracle, (M, K), seed=3)
    q = [_fp4_pair(qlib, _weight(oracle, n, K, W_SCALE[epi], 10 + i)) for i, n in enumerate(_rows(c))]
    dws, ws = [d for d, _ in q], [w for _, w in q]
    bs = [rand_bf16(oracle, (n,), 0.1, seed=20 + i) for i, n in enumerate(c.segs)] if c.bias else []
    res = rand_bf16(oracle, (M, N), seed=40) if epi == "RESIDUAL" else None
    y0 = GC.frame(c, res)
    got = GC.live(c, _launch(qlib, c, x, dws, bs, y0))
    if epi == "STORE":
        want = np.concatenate([oracle.matmul(x, w, bs[i]) for i, w in enumerate(ws)], axis=1)
        G.assert_sum_close(got, want, np.concatenate([_abs_scale(oracle, x, w) for w in ws], axis=1), rel=1e-5, ulps=1, what=epi)
    elif epi == "RESIDUAL":
        acc = oracle.matmul(x, ws[0])
        assert_residual_close(got, oracle.resadd(res, acc), acc, _abs_scale(oracle, x, ws[0]))
    elif epi == "SWIGLU":
        gate, up = oracle.matmul(x, ws[0]), oracle.matmul(x, ws[1])
        sg, su = _abs_scale(oracle, x, ws[0]), _abs_scale(oracle, x, ws[1])
        want = _swiglu_reference(oracle, c, got, oracle.silu_mul(gate, up), gate, up, x, ws, sg, su)
        assert_swiglu_close(got, want, gate, up, sg, su)
    else:
        want = oracle.bf16_to_f32(x).astype(np.float64) @ oracle.bf16_to_f32(ws[0]).astype(np.float64).T
        assert_f32_close(got, want, _abs_scale(oracle, x, ws[0]))
    r = 255 if epi in ("STORE", "SWIGLU") else M - 1
    xn = x.copy()
    xn[r] = GC.NAN_BF16
    yn = GC.live(c, _launch(qlib, c, xn, dws, bs, y0))
    other = np.arange(M) != r
    assert _is_nan(yn[r]).all(), f"row {r} of x is NaN, row {r} of y is not"
    assert np.array_equal(GC.bits(yn)[other], GC.bits(got)[other]), f"a NaN in x row {r} reached other rows"

# (name, M, K, N, segs, epilogue, norm, flags, words)
REFUSALS = [
    ("gemm_without_fp4", 40, 256, 64, (64,), "STORE", 0, GEMM, "needs QIE_LINEAR_FP4"),
    ("gemm_with_fp8", 40, 256, 64, (64,), "STORE", 0, FP4 | GEMM | 1, "combine"),
    ("gemm_with_act_fp8", 40, 256, 64, (64,), "STORE", 0, FP4 | GEMM | 32, "combine"),
    ("k192", 40, 192, 64, (64,), "STORE", 0, FP4 | GEMM, "K % 128 == 0"),
    ("norm", 40, 256, 64, (64,), "STORE", 1, FP4 | GEMM, "no fused norm"),
    ("t16_ragged", 40, 256, 40, (40,), "STORE", 0, FP4 | T16 | GEMM, "whole 16-row tiles"),
    ("ragged_inner_segment", 40, 256, 64, (24, 40), "STORE", 0, FP4 | GEMM, "whole 16-row tiles"),
    ("rows_wrap", 1 << 20, 2048, 64, (64,), "STORE", 0, FP4 | GEMM, "2^32"),
    ("weights_past_range", 40, 32768, 123200, (123200,), "STORE", 0, FP4 | GEMM, "2^31-byte buffer range"),
    ("m17_without_the_flag", 17, 256, 64, (64,), "STORE", 0, FP4, "1 <= M <= 16"),
]

@pytest.mark.parametrize("name,M,K,N,segs,epi,norm,fl,words", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_fp4_gemm_refusals(oracle, qlib, name, M, K, N, segs, epi, norm, fl, words):
    Ma = min(M, 64)   # (the refusal comes before anything is read: the wrapping cases allocate 64 rows / 1 MiB of weights)
    x = G.zeros_bf16(Ma, K)
    w = G.zeros((min(int(qlib.qie_fp4_weight_bytes(N, K)) + int(qlib.qie_fp8_weight_bytes(N, K)), 1 << 20),), np.uint8)
    y0 = _sentinel((Ma, N), np.uint16)
    y = G.dev(y0)
    a = _linear_args(x, [(w, n) for n in segs], [], M, K, N, y, EPI[epi],
                     norm_w=G.dev(oracle.f32_to_bf16(np.ones(K, np.float32))) if norm else None, flags=fl)
    if fl & _lib.QIE_LINEAR_ACT_FP8:
        a.x_exps = G.p(G.zeros((Ma,), np.uint8))
    assert qlib.qie_linear(C.byref(a), None) == -22
    assert words.encode() in qlib.qie_last_error(), qlib.qie_last_error()
    G.check(qlib.qie_synchronize())
    assert np.array_equal(G.host(y), y0)

# ------------------------------------------------------------------------------ the engine
@pytest.mark.parametrize("name,fp8", [(n, False) for n in FP4_CONFIGS] + [("qwen2-bias-hd64", True)])
def test_fp4_codes_only_engine_matches_oracle(oracle, name, fp8):
    # test_fp4_engine_matches_oracle_on_dequantised_model's P = 23 run (same prompts, seeds and cap: the
    # oracle's own disagreement there is at most 2 of 12); the 23-row prefill reads the codes.  fp8: the
    # untied head in fp8 (test_fp4_with_fp8_head_matches_oracle's run), quantised from the load arena
    spec = FP4_CONFIGS[name]
    eng = Q.Engine(spec, max_ctx=128, weight_fp4=2, weight_fp8=fp8).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(spec, SYN).fp4_dequantized(head_fp8=fp8)
    prompt = list(rng(23).integers(0, spec.vocab, 23))
    ids, flips = forced_compare(oracle, eng.batch(1, 128), OrderPair(oracle, hw, 128), prompt, 12)
    assert flips <= 2

class _PrefillThenAppend:
    """A batch whose prefill() is a 300-row prefill and an append of the rest (forced_compare calls prefill)."""

    def __init__(self, b):
        self.b = b

    def __getattr__(self, name):
        return getattr(self.b, name)

    def prefill(self, seq, prompt):
        self.b.prefill(seq, prompt[:300])
        return self.b.append(seq, prompt[300:])

@pytest.mark.parametrize("P", [300, 340])
def test_fp4_codes_only_engine_long_prompt_and_append(oracle, P):
    """Two row tiles, the second ragged (256 + 44), and at P = 340 an append of 40 rows onto them; 11 decode
    steps each.  The oracle alone on this model and prompt (orders 0 and 2, on the CPU, before the cap was
    set) disagrees with itself on 0 of the 12 arg-maxes at P = 300 and 0 of 12 at P = 340: flips <= 2 holds."""
    spec = FP4_CONFIGS["qwen2-bias-hd64"]
    eng = Q.Engine(spec, max_ctx=384, weight_fp4=2).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(spec, SYN).fp4_dequantized()
    prompt = [int(t) for t in rng(300).integers(0, spec.vocab, 340)][:P]
    b = eng.batch(1, 384)
    ids, flips = forced_compare(oracle, _PrefillThenAppend(b) if P > 300 else b, OrderPair(oracle, hw, 384), prompt, 12)
    assert flips <= 2

def test_fp4_codes_only_footprint(oracle, qlib):
    # caller-owned weights: mode 2 holds the codes alone, mode 1 codes + copy, the caller's tensors stay
    with pytest.raises(_lib.QieError, match="rc=-22"):   # (no mode 3)
        Q.Engine(FP4_CONFIGS["tied-h384"], max_ctx=64, weight_fp4=3)
    a256 = lambda n: (n + 255) // 256 * 256
    for name, spec in FP4_CONFIGS.items():
        H, QD, KD, I = spec.hidden, spec.n_heads * spec.head_dim, spec.n_kv_heads * spec.head_dim, spec.ffn
        shapes = [(QD, H), (KD, H), (KD, H), (H, QD), (I, H), (I, H), (H, I)] * spec.n_layers
        codes = sum(a256(int(qlib.qie_fp4_weight_bytes(r, c))) for r, c in shapes)
        copy = sum(a256(2 * r * c) for r, c in shapes)
        hw = W.HostWeights.synthetic(spec, SYN)
        for mode, want in ((2, codes), (1, codes + copy)) if name == "tied-h384" else ():
            dev = {n: G.dev(a) for n, a in hw.tensors.items()}
            eng = Q.Engine(spec, max_ctx=128, weight_fp4=mode).set_weights({n: t.data_ptr() for n, t in dev.items()},
                                                                           keepalive=dev)
            assert eng.weight_bytes() == want
            eng.batch(1, 128).prefill(0, list(rng(23).integers(0, spec.vocab, 23)))
            assert all(np.array_equal(G.host(dev[n]), a) for n, a in hw.tensors.items())
        # engine-owned weights: the compact arena holds embeddings, an untied head, the norms and the biases
        rest = ([spec.vocab * H * 2] * (1 if spec.tie_embeddings else 2) + [H * 2] + spec.n_layers * (
            [H * 2] * 2 + ([QD * 2, KD * 2, KD * 2] if spec.qkv_bias else []) + ([spec.head_dim * 2] * 2 if spec.qk_norm else [])))
        own = [Q.Engine(spec, max_ctx=128, weight_fp4=m).init_synthetic(SYN) for m in (1, 2)]
        arena = C.c_int64()
        G.check(qlib.qie_engine_arena(own[1].h, None, C.byref(arena)))
        assert arena.value == sum(a256(n) for n in rest), name
        assert own[1].weight_bytes() == codes + arena.value < own[0].weight_bytes(), name
        if not spec.tie_embeddings:   # + weight_fp8: the head is held in fp8 alone
            head8 = Q.Engine(spec, max_ctx=128, weight_fp4=2, weight_fp8=True).init_synthetic(SYN)
            assert head8.weight_bytes() == codes + arena.value - a256(spec.vocab * H * 2) + a256(int(qlib.qie_fp8_weight_bytes(spec.vocab, H))), name
