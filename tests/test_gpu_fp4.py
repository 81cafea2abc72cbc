"""GPU: MXFP4 projection weights (qie_ops.h; csrc/k_decode_fp4.hip; qie_engine_opts.weight_fp4).

Every code x 2^k is exactly a bf16, so everything here has one reference: the oracle on the
dequantised bf16 weights (weights.dequantize_mxfp4 of weights.quantize_mxfp4, the written rule).
  * the kernel's own conversion of all 16 codes under exponents from both ends of the range equals
    the numpy dequantisation bit for bit (this also pins the nibble order);
  * device quantiser == host quantiser == the numpy rule; device dequantisation exact;
  * the 16-row tiled layout is the documented permutation, and the kernel on it equals the plain
    layout bit for bit at M = 1, 2, 8, 16, every epilogue, split-K included; row 0 does not depend on M;
  * every row of tests/fp4_cases.py: declared plan asserted on the live arguments, NaN-padded x,
    sentinel-framed y, the bars of test_fp8_batched_decode_kernel through the shared helpers
    (fused-norm rows: test_gpu_linear_variants.py's protocol, see test_fp4_linear_variant);
  * needle weights and small-integer activations: one right answer, compared bit for bit;
  * the engine on every entry point against the oracle on HostWeights.fp4_dequantized().
"""
import ctypes as C
import zlib

import numpy as np
import pytest

import fp4_cases as FC
import gpu_util as G
import linear_cases as LC
from conftest import rng
from parity import OrderPair, max_flips
from test_gpu_engine import CONFIGS, SYN, _teacher_forced_trace, forced_compare, logit_tol, logits_close
from test_gpu_linear_variants import (EPI, NAN_BF16, W_SCALE, _bits, _live_plan, _rows_with_a_stable_norm, _sentinel,
                                      _weight)
from test_gpu_ops import (_abs_scale, _linear, _linear_args, assert_f32_close, assert_residual_close,
                          assert_swiglu_close, rand_bf16)

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib, spec as S, weights as W

pytestmark = pytest.mark.gpu

FP4 = _lib.QIE_LINEAR_FP4
T16 = _lib.QIE_LINEAR_FP4 | _lib.QIE_LINEAR_FP4_T16


# ------------------------------------------------------------------------------ the format
def test_fp4_decode_probe_all_codes(qlib):
    exps = np.array([2, 3, 120, 127, 134, 250, 252], np.uint8)
    out = G.zeros((len(exps), 16), np.uint16)
    G.check(qlib.qie_debug_fp4_decode_bf16(exps.ctypes.data, len(exps), G.p(out)))
    codes = np.tile(np.arange(16, dtype=np.uint8), 2).reshape(1, 32)
    want = np.stack([W.dequantize_mxfp4(codes, np.array([[e]], np.uint8))[0, :16] for e in exps])
    assert np.array_equal(G.host(out), want), (G.host(out), want)


def _fp4_dev(qlib, w):
    """Device codes + scales (plain layout) of bf16 w, quantised on the device."""
    rows, cols = w.shape
    out = G.zeros((int(qlib.qie_fp4_weight_bytes(rows, cols)),), np.uint8)
    G.check(qlib.qie_quantize_fp4(G.p(G.dev(w)), rows, cols, G.p(out), None))
    return out


def _fp4_pair(qlib, w):
    """(device plain codes, dequantised bf16 bits on the host).  The dequantisation comes from the
    device (bit-equal to the numpy rule: test_dequantize_device_exact); numpy's takes seconds at
    the MANY_TILES sizes."""
    rows, cols = w.shape
    d = _fp4_dev(qlib, w)
    out = G.zeros_bf16(rows, cols)
    G.check(qlib.qie_dequantize_fp4(G.p(d), rows, cols, G.p(out), None))
    return d, G.host_bf16(out)


def _tiled(qlib, d, rows, cols):
    out = G.zeros((d.nbytes,), np.uint8)
    G.check(qlib.qie_fp4_tile16(G.p(d), rows, cols, G.p(out), None))
    return out


def _special(oracle, w):
    w[0, :32] = 0                                                            # an all-zero block
    w[1 % len(w), :3] = oracle.f32_to_bf16(np.array([1e4, -3e-3, 7.0], np.float32))   # outliers
    w[2 % len(w), 32:39] = oracle.f32_to_bf16(np.array([6, .25, .75, -1.25, 1.75, -2.5, 3.5], np.float32))   # ties
    return w


@pytest.mark.parametrize("rows,cols", [(7, 64), (33, 896), (5, 18944)])
def test_quantize_device_equals_host_and_rule(oracle, qlib, rows, cols):
    w = _special(oracle, rand_bf16(oracle, (rows, cols), 0.05, seed=rows))
    got = G.host(_fp4_dev(qlib, w))
    G.check(qlib.qie_synchronize())
    host = np.empty(got.size, np.uint8)
    assert qlib.qie_quantize_fp4_host(w.ctypes.data, rows, cols, host.ctypes.data) == 0
    assert np.array_equal(got, host)
    assert np.array_equal(got, W.pack_mxfp4(*W.quantize_mxfp4(w)))


@pytest.mark.parametrize("rows,cols", [(7, 64), (33, 896), (5, 18944)])
def test_dequantize_device_exact(oracle, qlib, rows, cols):
    w = _special(oracle, rand_bf16(oracle, (rows, cols), 0.05, seed=rows + 1))
    _, dq = _fp4_pair(qlib, w)
    assert np.array_equal(dq, W.dequantize_mxfp4(*W.quantize_mxfp4(w)))


@pytest.mark.parametrize("rows,cols", [(16, 128), (48, 896), (64, 3584)])
def test_fp4_tile16_layout(oracle, qlib, rows, cols):
    """qie_fp4_tile16 is qie_ops.h's permutation: code block (t, j) piece l = row 16 t + l % 16, MX
    block 4 j + l // 16 (16 bytes), and the scale bytes under the same (t, j, l) order."""
    d = _fp4_dev(qlib, rand_bf16(oracle, (rows, cols), 0.05, seed=rows))
    plain = G.host(d)
    n = rows * cols // 2
    c = plain[:n].reshape(rows // 16, 16, cols // 128, 4, 16).transpose(0, 2, 3, 1, 4).reshape(-1)   # t, j, g, fr, byte
    s = plain[n:].reshape(rows // 16, 16, cols // 128, 4).transpose(0, 2, 3, 1).reshape(-1)
    assert np.array_equal(G.host(_tiled(qlib, d, rows, cols)), np.concatenate([c, s]))


# ------------------------------------------------------------------------ tiled == plain
@pytest.mark.parametrize("M", [1, 2, 8, 16])
@pytest.mark.parametrize("K,N", [(896, 768), (3584, 768), (5120, 256), (8320, 256), (18944, 512)])
def test_fp4_t16_equals_plain_and_rows_do_not_depend_on_m(oracle, qlib, M, K, N):
    """Every epilogue the shape takes (K > 8,192: split-K, no norm, no SwiGLU), 3-segment STORE with
    biases and keys: tiled == plain bit for bit, and row 0 of the M-row launch == row 0 at M = 1."""
    split = K > 8192
    x = rand_bf16(oracle, (M, K), seed=M + K)
    nw = None if split else G.dev(oracle.f32_to_bf16((1 + 0.2 * rng(12).standard_normal(K)).astype(np.float32)))
    n = (N // 2, N // 4, N // 4)
    ws = [_fp4_dev(qlib, rand_bf16(oracle, (r, K), 0.05, seed=30 + i)) for i, r in enumerate(n)]
    wt = [_tiled(qlib, d, r, K) for d, r in zip(ws, n)]
    bs = [G.dev(rand_bf16(oracle, (r,), 0.1, seed=40 + i)) for i, r in enumerate(n)]
    res = rand_bf16(oracle, (M, n[0]), seed=5)

    def run(weights, fl, m):
        dx = G.dev(x[:m].copy())
        outs = []
        if not split:
            y, keys = G.zeros_bf16(m, N), G.dev(np.zeros(m, np.uint64))
            _linear(qlib, dx, list(zip(weights, n)), bs, m, K, N, y, _lib.QIE_EPI_STORE, norm_w=nw, eps=1e-6, num=0,
                    keys=keys, flags=fl)
            outs += [G.host_bf16(y), G.host(keys)]
            y = G.zeros_bf16(m, n[1])
            _linear(qlib, dx, [(weights[1], n[1]), (weights[2], n[1])], [], m, K, n[1], y, _lib.QIE_EPI_SWIGLU,
                    norm_w=nw, eps=1e-6, num=1, flags=fl)
            outs.append(G.host_bf16(y))
        y = G.zeros_bf16(m, n[0])
        _linear(qlib, dx, [(weights[0], n[0])], [bs[0]], m, K, n[0], y, _lib.QIE_EPI_STORE, flags=fl)
        outs.append(G.host_bf16(y))
        yr = G.dev(res[:m].copy())
        _linear(qlib, dx, [(weights[0], n[0])], [], m, K, n[0], yr, _lib.QIE_EPI_RESIDUAL, flags=fl)
        outs.append(G.host_bf16(yr))
        yf = G.zeros((m, n[0]), np.float32)
        _linear(qlib, dx, [(weights[0], n[0])], [], m, K, n[0], yf, _lib.QIE_EPI_F32, flags=fl)
        outs.append(G.host(yf).view(np.uint32))
        return outs

    plain, tiled, one = run(ws, FP4, M), run(wt, T16, M), run(wt, T16, 1)
    for a, b, c in zip(plain, tiled, one):
        assert np.array_equal(a, b)
        assert np.array_equal(a[:1], c)


# ------------------------------------------------------------------------ every planner form
@pytest.mark.parametrize("case", FC.CASES + FC.MANY_TILES, ids=[c.name for c in FC.CASES + FC.MANY_TILES])
def test_fp4_linear_variant(oracle, qlib, case):
    """tests/test_gpu_linear_variants.py's protocol on fp4 weights; the reference multiplies the
    dequantised rows.  Without a fused norm the bars are test_fp8_batched_decode_kernel's, through
    the shared helpers: assert_sum_close at rel 1e-5 and 1 ulp, the SwiGLU ill-conditioning filter,
    the 2^-7 residual bound, 1e-5 of sum|a*w| in fp32.  With a fused norm the two files differ in
    where the normalised rows come from, and this test follows test_gpu_linear_variants.py, not the
    fp8 test: the reference rows are oracle.rmsnorm's (the fp8 test reads the kernel's own rows back
    through identity weights and checks them to 1 / 2 ulps first), so STORE takes that file's
    fused-norm bound, rel 1e-4 and 1 ulp (ref) / 2 ulps (hf), and the other epilogues run on rows
    whose norm does not depend on the summation order (_rows_with_a_stable_norm) under the
    unchanged bounds."""
    c = case
    M, K, N, epi = c.M, c.K, LC.n_cols(c), c.epi
    seed = zlib.crc32(c.name.encode()) % 10000
    ldx, ldy = K + c.ldx_pad, N + c.ldy_pad
    nw, eps = None, 1e-4
    if c.norm:
        nw = oracle.f32_to_bf16((1 + 0.2 * rng(seed + 30).standard_normal(K)).astype(np.float32))
        eps = 1e-4 if c.norm == "ref" else 1e-6
        if epi == "STORE":
            x = rand_bf16(oracle, (M, K), seed=seed)
            xin = oracle.rmsnorm(x, nw, eps, c.norm)
        else:
            x, xin = _rows_with_a_stable_norm(oracle, M, K, nw, eps, c.norm, seed)
    else:
        x = xin = rand_bf16(oracle, (M, K), seed=seed)
    xp = np.full((M + 1, ldx), NAN_BF16, np.uint16)   # a NaN row past M and NaN columns past K
    xp[:M, :K] = x
    rows = (N, N) if epi == "SWIGLU" else c.segs
    q = [_fp4_pair(qlib, _weight(oracle, r, K, W_SCALE[epi], seed + 10 + i)) for i, r in enumerate(rows)]
    dws, ws = [d for d, _ in q], [dq for _, dq in q]
    bs = [rand_bf16(oracle, (r,), 0.1, seed=seed + 20 + i) for i, r in enumerate(rows)] if c.bias else []
    res = rand_bf16(oracle, (M, N), seed=seed + 40) if epi == "RESIDUAL" else None
    y0 = _sentinel((M + 1, ldy), np.float32 if epi == "F32" else np.uint16)
    if res is not None:
        y0[:M, :N] = res
    dx, dbs, dnw = G.dev(xp), [G.dev(b) for b in bs], G.dev(nw) if c.norm else None

    def launch():
        y = G.dev(y0)
        keys = G.dev(np.zeros(M, np.uint64)) if c.key_col0 is not None else None
        a = _linear_args(dx, list(zip(dws, rows)), dbs, M, K, N, y, EPI[epi], norm_w=dnw, eps=eps,
                         num=1 if c.norm == "hf" else 0, keys=keys, ldy=ldy, flags=c.flags, ldx=ldx,
                         key_col0=c.key_col0 or 0)
        plan = _live_plan(qlib, a)
        assert plan == c.plan + " t16=0", f"{c.name}: the library plans {plan}"
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
    untouched = np.ones(y0.shape, bool)
    untouched[:M, :N] = False
    assert np.array_equal(_bits(yh)[untouched], _bits(y0)[untouched]), f"{c.name}: wrote outside y[:M, :N]"
    got = np.ascontiguousarray(yh[:M, :N])

    if epi == "STORE":
        want = np.concatenate([oracle.matmul(xin, w, bs[i] if bs else None) for i, w in enumerate(ws)], axis=1)
        scale = np.concatenate([_abs_scale(oracle, xin, w) for w in ws], axis=1)
        print(f"{c.name}: max {G.ulp_diff(got, want).max()} ulps, exact {(got == want).mean():.4f}")
        G.assert_sum_close(got, want, scale, rel=1e-4 if c.norm else 1e-5, ulps=2 if c.norm == "hf" else 1, what=c.name)
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
        assert_f32_close(got, want, _abs_scale(oracle, xin, ws[0]))
    if ids is not None:
        for m in range(M):
            assert ids[m] == oracle.argmax(got[m]) + c.key_col0, (c.name, m)


# ------------------------------------------------------------------------ needles
@pytest.mark.parametrize("K,N,tiled", [(896, 48, False), (3584, 64, True), (5120, 32, False), (8320, 64, False),
                                       (18944, 48, True)])
def test_fp4_needle_weights_pick_single_columns(oracle, qlib, K, N, tiled):
    """Row n of W is one needle: code value v_n in {0.5 .. 6} * 2^e_n at column c_n, zeros elsewhere
    (its block's scale is the needle's; every other block is all-zero).  x holds small integers, so
    y[m, n] = x[m, c_n] * W[n, c_n] exactly, with one right answer in fp32: a wrong column, nibble,
    block scale or unit order anywhere shows as a wrong number, which a sum bound over random data
    can hide.  Columns cover every unit, lane group, byte and nibble, both ends included."""
    M = 16
    r = rng(K + N)
    cols = np.concatenate([[0, 1, 31, 32, 127, 128, K - 129, K - 33, K - 2, K - 1],
                           r.integers(0, K, N)])[:N].astype(np.int64)
    cols[N - 1] = K - 1
    vals = np.array([0.5, 1, 1.5, 2, 3, 4, 6, -0.5, -1, -1.5, -2, -3, -4, -6], np.float32)[r.integers(0, 14, N)]
    vals = vals * (2.0 ** r.integers(-6, 7, N)).astype(np.float32)
    wf = np.zeros((N, K), np.float32)
    wf[np.arange(N), cols] = vals
    w = oracle.f32_to_bf16(wf)
    d, dq = _fp4_pair(qlib, w)
    assert np.array_equal(dq, w)                                   # needles are representable: nothing is rounded
    xf = r.integers(-8, 9, (M, K)).astype(np.float32)
    x = oracle.f32_to_bf16(xf)
    if tiled:
        d = _tiled(qlib, d, N, K)
    yf = G.zeros((M, N), np.float32)
    _linear(qlib, G.dev(x), [(d, N)], [], M, K, N, yf, _lib.QIE_EPI_F32, flags=T16 if tiled else FP4)
    want = xf[:, cols] * vals[None, :]
    assert np.array_equal(G.host(yf), want)


# ------------------------------------------------------------------------ refusals (operator)
@pytest.mark.parametrize("name,M,K,N,epi,norm,fl,words", FC.REFUSALS, ids=[r[0] for r in FC.REFUSALS])
def test_fp4_linear_refuses_what_the_kernel_does_not_take(oracle, qlib, name, M, K, N, epi, norm, fl, words):
    x = G.zeros_bf16(M, K)
    w = G.zeros((int(qlib.qie_fp4_weight_bytes(N, K)) + int(qlib.qie_fp8_weight_bytes(N, K)),), np.uint8)
    nw = G.dev(oracle.f32_to_bf16(np.ones(K, np.float32)))
    y0 = _sentinel((M, N), np.uint16)
    y = G.dev(y0)
    segs = [(w, N), (w, N)] if epi == "SWIGLU" else [(w, N)]
    a = _linear_args(x, segs, [], M, K, N, y, EPI[epi], norm_w=nw if norm else None, flags=fl)
    if fl & _lib.QIE_LINEAR_ACT_FP8:
        a.x_exps = G.p(G.zeros((M,), np.uint8))
    assert qlib.qie_linear(C.byref(a), None) == -22
    assert words.encode() in qlib.qie_last_error(), qlib.qie_last_error()
    G.check(qlib.qie_synchronize())
    assert np.array_equal(G.host(y), y0)


# ------------------------------------------------------------------------------ the engine
FP4_CONFIGS = {
    "qwen2-bias-hd64": CONFIGS["qwen2-bias-hd64"],   # 3 layers, hidden 256, ffn 512, hd 64, bias
    "tied-h384": S.tiny("t4-tied", n_layers=2, hidden=384, n_heads=6, n_kv_heads=1, head_dim=64, ffn=640,
                        vocab=777 * 2, tie=True, bias=True),
    "qknorm-hd128": S.tiny("t4-q3", n_layers=2, hidden=256, n_heads=2, n_kv_heads=1, head_dim=128, ffn=384,
                           vocab=1536, bias=False, qk_norm=True),
}
SPEC = FP4_CONFIGS["qwen2-bias-hd64"]


def _ids(seed, n, spec=SPEC):
    return [int(t) for t in rng(seed).integers(0, spec.vocab, n)]


@pytest.mark.parametrize("name", list(FP4_CONFIGS))
@pytest.mark.parametrize("P", [5, 23])
def test_fp4_engine_matches_oracle_on_dequantised_model(oracle, name, P):
    """P = 5: a short prefill on the codes (M <= 16); P = 23: on the dequantised bf16 copy; 12 decode
    steps on the codes.  flips <= 2 is a condition set beforehand, not a measurement: the oracle
    alone on these dequantised models (orders 0 and 2, these prompts, the real synthetic filler)
    disagrees with itself on 0 of the 12 arg-maxes in five of the six runs and on 2 in one
    (qwen2-bias-hd64, P = 23) -- within the cap, so no prompt seed was changed."""
    spec = FP4_CONFIGS[name]
    eng = Q.Engine(spec, max_ctx=128, weight_fp4=True).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(spec, SYN).fp4_dequantized()
    assert hw.spec.tie_embeddings == spec.tie_embeddings
    prompt = list(rng(P).integers(0, spec.vocab, P))
    ids, flips = forced_compare(oracle, eng.batch(1, 128), OrderPair(oracle, hw, 128), prompt, 12)
    assert flips <= 2


def test_fp4_with_fp8_head_matches_oracle(oracle):
    eng = Q.Engine(SPEC, max_ctx=128, weight_fp4=True, weight_fp8=True).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(SPEC, SYN).fp4_dequantized(head_fp8=True)
    assert not hw.spec.tie_embeddings
    prompt = list(rng(23).integers(0, SPEC.vocab, 23))
    ids, flips = forced_compare(oracle, eng.batch(1, 128), OrderPair(oracle, hw, 128), prompt, 12)
    assert flips <= 2


def test_fp4_set_weights_leaves_the_callers_tensors_alone(oracle):
    spec = FP4_CONFIGS["tied-h384"]
    hw = W.HostWeights.synthetic(spec, SYN)
    dev = {n: G.dev(a) for n, a in hw.tensors.items()}
    eng = Q.Engine(spec, max_ctx=128, weight_fp4=True).set_weights({n: t.data_ptr() for n, t in dev.items()},
                                                                   keepalive=dev)
    prompt = list(rng(23).integers(0, spec.vocab, 23))
    ids, flips = forced_compare(oracle, eng.batch(1, 128), OrderPair(oracle, hw.fp4_dequantized(), 128), prompt, 12)
    assert flips <= 2
    eng.sync()
    for n, a in hw.tensors.items():
        assert np.array_equal(G.host(dev[n]).reshape(-1), a.reshape(-1)), f"{n} was written"


def test_fp4_batch8_equals_single(oracle):
    """test_fp8_batch8_equals_single's bar: B = 8 against eight runs of one sequence."""
    eng = Q.Engine(SPEC, max_ctx=96, weight_fp4=True).init_synthetic(SYN)
    prompts = [list(rng(40 + i).integers(0, SPEC.vocab, 4 + 3 * i)) for i in range(8)]
    singles = [_teacher_forced_trace(eng.batch(1, 96), [pr], 7) for pr in prompts]
    s_ids = [r[0][0] for r in singles]
    s_lgs = [r[1][0] for r in singles]
    raw, lgs = _teacher_forced_trace(eng.batch(8, 96), prompts, 7, forced=s_ids)
    flips = 0
    for i in range(8):
        for t in range(7):
            logits_close(lgs[i][t], s_lgs[i][t], f"seq {i} step {t}")
            if raw[i][t] != s_ids[i][t]:
                gap = abs(float(G.bf(s_lgs[i][t][s_ids[i][t]])) - float(G.bf(s_lgs[i][t][raw[i][t]])))
                assert gap <= logit_tol(s_lgs[i][t])
                flips += 1
    assert flips <= 3


def test_fp4_verify_and_verify_batch_match_oracle(oracle):
    """test_gpu_verify.py's and test_gpu_verify_batch.py's protocol (every logits row, emitted id,
    accept length, position, history; then decode steps) on the dequantised model."""
    from test_gpu_verify import _follow_from, _greedy, _start, _verify_checked
    from test_gpu_verify_batch import _draft, _follow_all, _live, _verify_batch_checked
    eng = Q.Engine(SPEC, max_ctx=128, weight_fp4=True).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(SPEC, SYN).fp4_dequantized()
    prompt = _ids(41, 20)
    c, cont, glg = _greedy(oracle, hw, 128, prompt, 15)
    draft = cont[:9] + [int(np.argmin(G.bf(glg[9])))] + _ids(42, 5)     # 15 drafts: a 16-row step
    om = oracle.Model(hw, 128)
    lg_prompt = om.forward(prompt, 0)
    b = eng.batch(1, 128)
    flips = _start(oracle, b, prompt, c, lg_prompt)
    out, f1, _ = _verify_checked(oracle, om, b, 20, c, draft, "fp4 verify")
    if f1 == 0:
        assert len(out) == 10
    flips += f1 + _follow_from(oracle, om, b, 20 + len(out), out[-1], 6, "fp4 verify")
    assert flips <= max_flips(1 + len(out) + 6)
    b.close()
    # three segments of 1 + 8 + 7 = 16 rows on a B = 8 batch
    b = eng.batch(8, 128)
    shape = {1: 0, 4: 7, 6: 6}
    st, f0 = _live(oracle, hw, b, {s: 12 + 3 * s for s in shape}, 15, 100, 128)
    tab = [(1, []), (4, _draft(SPEC, st[4], 7, 7, 3)), (6, _draft(SPEC, st[6], 6, 2, 4))]
    outs, fl = _verify_batch_checked(oracle, b, tab, st, "fp4 verify_batch")
    for (s, _), o, want in zip(tab, outs, (1, 8, 3)):
        if fl[s] == 0:
            assert len(o) == want
    f2 = _follow_all(oracle, b, st, list(shape), 4, "fp4 verify_batch")
    decisions = len(shape) + sum(len(o) for o in outs) + 4 * len(shape)
    assert f0 + sum(fl.values()) + f2 <= max_flips(decisions)
    b.close()


def test_fp4_paged_batcher_equals_batch_decode():
    """The scheduler needs no change: a paged ContinuousBatcher run gives each request the ids of
    the same request run alone in a contiguous Batch."""
    from qwen_inference_engine_amd.scheduler import ContinuousBatcher
    eng = Q.Engine(SPEC, max_ctx=256, weight_fp4=True).init_synthetic(SYN)
    lens, new = [30, 9, 140, 17], [12, 20, 6, 9]
    prompts = [_ids(50 + i, n) for i, n in enumerate(lens)]
    cb = ContinuousBatcher(eng, slots=3, max_ctx=256, page_tokens=128, n_pages=6)
    rids = [cb.submit(p, n) for p, n in zip(prompts, new)]
    while not cb.idle():
        cb.step()
    for rid, p, n in zip(rids, prompts, new):
        b = eng.batch(3, 256)
        want = [b.prefill(0, p)]
        while len(want) < n:
            want.append(b.decode_step()[0])
        b.close()
        assert cb.requests[rid].tokens == want, f"request {rid}"


def test_fp4_world1_peer_comm_leaves_the_push_untaken():
    """comm_always on a world-1 peer communicator: at one row the row-parallel projections are
    offered a peer push, which the MXFP4 kernel does not take (as the fp8 kernels do not); the step
    then runs the exchange on the fp32 partials -- the fused residual's rounding -- and must give
    the plain fp4 engine's logits."""
    prompt = _ids(61, 9)
    comm = Q.Comm.peer_local(1)
    runs = []
    try:
        for kw in ({}, {"comm": comm[0], "comm_always": True}):
            eng = Q.Engine(SPEC, max_ctx=64, weight_fp4=True, **kw).init_synthetic(SYN)
            b = eng.batch(1, 64)
            ids = [b.prefill(0, prompt)]
            for t in range(5):
                if runs and ids[-1] != runs[0][0][len(ids) - 1]:
                    b.set_position(0, len(prompt) + t, runs[0][0][len(ids) - 1])
                ids.append(b.decode_step()[0])
            runs.append((ids, b.logits()[0]))
            b.close()
            eng.close()
    finally:
        for c in comm:
            c.close()
    logits_close(runs[1][1], runs[0][1], "world-1 peer comm")


def test_fp4_time_kernel_counts_code_bytes():
    eng = Q.Engine(SPEC, max_ctx=64, weight_fp4=True).init_synthetic(SYN)
    b = eng.batch(2, 64)
    b.prefill(0, [1, 2, 3])
    b.prefill(1, [4, 5])
    H, I, QD, KD, B = SPEC.hidden, SPEC.ffn, SPEC.n_heads * SPEC.head_dim, SPEC.n_kv_heads * SPEC.head_dim, 2
    pb = 0.5 + 1 / 32
    want = {0: 2 * I * H * pb + B * H * 2 + H * 2 + B * I * 2, 1: H * I * pb + B * I * 2 + B * H * 2,
            2: (QD + 2 * KD) * H * pb + B * H * 2 + B * (QD + 2 * KD) * 2, 3: H * QD * pb + B * QD * 2 + B * H * 2}
    for which, by in want.items():
        us, got = b.time_kernel(which, 3)
        assert us > 0 and got == by, (which, got, by)


@pytest.mark.parametrize("case", ["tp", "prefill_fp8", "hidden448", "mode1"])
def test_fp4_engine_refusals(case):
    lib = _lib.load()
    if case == "mode1":
        eng = Q.Engine(SPEC, max_ctx=64, weight_fp4=True).init_synthetic(SYN)
        b = eng.batch(1, 64)
        with pytest.raises(_lib.QieError, match="fp4 weights") as ei:
            b.set_decode_mode(1)
        assert "rc=-22" in str(ei.value)
        return
    comm = None
    try:
        with pytest.raises(_lib.QieError) as ei:
            if case == "tp":
                comm = Q.Comm.local(2)
                Q.Engine(SPEC, max_ctx=64, comm=comm[0], weight_fp4=True)
            elif case == "prefill_fp8":
                Q.Engine(SPEC, max_ctx=64, weight_fp4=True, weight_fp8=True, prefill_fp8=True)
            else:
                Q.Engine(CONFIGS["tied-g7"], max_ctx=64, weight_fp4=True)   # hidden 448 = 3.5 units
        words = {"tp": "tensor parallelism", "prefill_fp8": "prefill_fp8", "hidden448": "hidden (448)"}[case]
        assert "rc=-22" in str(ei.value) and words in str(ei.value), str(ei.value)
    finally:
        for c in comm or []:
            c.close()
