"""qie_attention_extend_fp8 — the split-context attention on an fp8 KV cache — against
qie_attention_extend on the bf16 cache holding the dequantised rows (bit for bit), a float64 causal
softmax attention of the decoded values, a needle, and the engine's three routes."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import gpu_util as G
from conftest import rng
from qwen_inference_engine_amd import _lib
from test_gpu_kv_fp8 import PARAMS, Cache8, attention64, decode, exact_bf16

L, LAYER, MAXC, SENTINEL = 2, 1, 1152, 0x4D4D
gpu = pytest.mark.gpu


def test_extend_fp8_exported_bound_and_refusing(qlib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert "qie_attention_extend_fp8" in {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert len({n: a for n, _, a in _lib.SIGNATURES}["qie_attention_extend_fp8"]) == 10
    assert qlib.qie_attention_extend_fp8(None, 1, None, 1, None, 0, 4, None, None, None) == -22
    assert b"qie_attention_extend_fp8" in qlib.qie_last_error()


def plant(h, b, first):
    """NaN codes and NaN exponents in every row of sequence b from position `first` on."""
    for t in range(first, h.maxc):
        i, j = h.at(b, t)
        h.k[i, :, :, j], h.v[i, :, :, j], h.ke[i, :, :, j], h.ve[i, :, :, j] = 0x7f, 0x7f, 0xff, 0xff


def bf16_twin(h):
    """The bf16 cache of h's geometry and block table holding h's dequantised rows (call before plant)."""
    c = _lib.KvCacheC()
    h._desc(c, G.dev(exact_bf16(decode(h.k, h.ke))), G.dev(exact_bf16(decode(h.v, h.ve))), h.hd)
    return c


def run(qlib, fp8, c, q, pos, rps, nq, hd):
    """One call with `out` framed by sentinel rows and the workspace filled with 0xFF bytes."""
    M = q.shape[0]
    nbytes = qlib.qie_attention_extend_workspace_bytes(M, nq, hd, MAXC)
    ws = G.zeros_bytes(nbytes)
    if nbytes:
        G.check(qlib.qie_memset(G.p(ws), 0xFF, nbytes))
    out = G.dev(np.full((M + 2, nq * hd), SENTINEL, np.uint16))
    fn = qlib.qie_attention_extend_fp8 if fp8 else qlib.qie_attention_extend
    G.check(fn(G.p(G.dev(q)), M, G.p(G.dev(pos)), rps, C.byref(c), LAYER, nq, G.p(out) + nq * hd * 2, G.p(ws), None))
    got = G.host_bf16(out)
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), "rows outside [0, M) were written"
    return got[1:-1]


@gpu
@pytest.mark.parametrize("pos0,n", [(0, 1), (63, 2), (65, 17), (130, 5), (257, 100), (1000, 40)])
@pytest.mark.parametrize("nq,nkv", [(14, 2), (4, 2)])
@pytest.mark.parametrize("hd,paged", PARAMS)
def test_extend_fp8_bit_equal_and_float64(qlib, hd, paged, nq, nkv, pos0, n):
    """Bound: the fp8 decode attention's own (test_attention_decode_fp8_exact_inputs), q at 2^-9."""
    h = Cache8(1, L, nkv, hd, MAXC, paged, seed=hd + nq)
    end = pos0 + n
    cb = bf16_twin(h)
    plant(h, 0, end)
    c8 = h.upload()
    q = G.to_bf16((rng(pos0 + n).standard_normal((n, nq * hd)) * 2.0 ** -9).astype(np.float32))
    pos = np.arange(pos0, end, dtype=np.int32)
    idx = [h.at(0, t) for t in range(end)]
    ii, jj = np.array([i for i, _ in idx]), np.array([j for _, j in idx])
    K = decode(h.k[ii, LAYER, :, jj], h.ke[ii, LAYER, :, jj]).transpose(1, 0, 2)
    V = decode(h.v[ii, LAYER, :, jj], h.ve[ii, LAYER, :, jj]).transpose(1, 0, 2)
    q64 = G.bf(q).astype(np.float64)   # float64 causal softmax attention, row m over keys [0, pos0 + m]
    want = np.stack([attention64(q64[m], K[:, :pos0 + m + 1], V[:, :pos0 + m + 1], nq, nkv, hd) for m in range(n)])
    bound = 2.0 ** -7 * 2 * max(1.0, np.abs(want).max())
    got16 = run(qlib, False, cb, q, pos, n, nq, hd)
    got8 = run(qlib, True, c8, q, pos, n, nq, hd)
    for what, got in (("bf16", got16), ("fp8", got8)):
        d = np.abs(G.bf(got).astype(np.float64) - want).max()
        print(f"{what}: max |d| {d:.3e}, bound {bound:.3e}")
        assert d <= bound, (what, d, bound)
    assert np.array_equal(got8, got16), f"rows differing: {int((got8 != got16).any(1).sum())} of {n}"


@gpu
@pytest.mark.parametrize("paged", [False, True])
def test_extend_fp8_two_sequences_short_last(qlib, paged):
    """rows_per_seq 5, M 8: the second sequence has 3 rows; prefixes below and above a split edge."""
    hd, nq, nkv, rps, starts, ns = 128, 28, 4, 5, (250, 258), (5, 3)
    assert qlib.qie_attention_extend_split_tokens(8, MAXC) == 256
    h = Cache8(2, L, nkv, hd, MAXC, paged, seed=3)
    ends = [p + m for p, m in zip(starts, ns)]
    cb = bf16_twin(h)
    for b, end in enumerate(ends):
        plant(h, b, end)
    c8 = h.upload()
    q = G.to_bf16((rng(8).standard_normal((8, nq * hd)) * 2.0 ** -9).astype(np.float32))
    pos = np.concatenate([np.arange(p, p + m) for p, m in zip(starts, ns)]).astype(np.int32)
    got16, got8 = run(qlib, False, cb, q, pos, rps, nq, hd), run(qlib, True, c8, q, pos, rps, nq, hd)
    assert np.isfinite(G.bf(got16)).all() and got16.any() and np.array_equal(got8, got16)


@gpu
@pytest.mark.parametrize("needle", [0, 63, 64, 255, 256, 298, 300])
@pytest.mark.parametrize("hd,paged", PARAMS)
def test_extend_fp8_needle(qlib, hd, paged, needle):
    """Rows at 298 .. 300; one key scores >= 128 and every other K row is zero (exp(-128) is 0 in
    fp32), so a row that sees the needle equals its decoded V row bit for bit."""
    nq, nkv, n, pos0 = 4, 2, 3, 298
    h = Cache8(1, L, nkv, hd, MAXC, paged, seed=needle)
    h.k[:] = 0
    u = rng(hd).choice([-1.0, 1.0], hd)
    i, j = h.at(0, needle)
    h.k[i, LAYER, :, j] = np.where(u > 0, 0x60, 0xE0)           # +-32 x 2^-3
    h.ke[i, LAYER, :, j] = 124
    h.ve[i, LAYER, :, j] = [131, 122]                           # the needle's V rows: their own exponents
    h.v[i, LAYER, :, j] |= np.where(h.v[i, LAYER, :, j] & 0x7f, 0, 0x38).astype(np.uint8)   # no zero element
    want = exact_bf16(decode(h.v[i, LAYER, :, j], h.ve[i, LAYER, :, j]))                    # [nkv][hd]
    plant(h, 0, pos0 + n)
    c8 = h.upload()
    q = np.tile(G.to_bf16(np.tile(4 * u, nq).astype(np.float32)), (n, 1))
    got = run(qlib, True, c8, q, np.arange(pos0, pos0 + n, dtype=np.int32), n, nq, hd)
    rows = [m for m in range(n) if pos0 + m >= needle]
    assert rows == ([2] if needle == 300 else [0, 1, 2])
    for m in rows:
        assert np.array_equal(got[m].reshape(nkv, nq // nkv, hd), np.repeat(want[:, None], nq // nkv, 1)), (needle, m)


@gpu
def test_engine_three_routes_across_a_split_and_pages():
    """DESIGN §23.4's three-route rule at 560 tokens on paged engines with max_ctx 1024: the append
    crosses a 512-key split and page edges.  Bound: 4 x the bf16-KV spread measured here, at most 2^-5."""
    import qwen_inference_engine_amd as Q
    from parity import norm_rel
    from test_gpu_engine import CONFIGS, SYN
    from test_gpu_kv_fp8_engine import forced_steps
    spec, P, n = CONFIGS["qwen2-bias-hd64"], 500, 60
    ids = [int(t) for t in rng(5).integers(0, spec.vocab, P + n)]
    spreads = []
    for kv_fp8 in (False, True):
        eng = Q.Engine(spec, max_ctx=1024, kv_fp8=kv_fp8).init_synthetic(SYN)
        logits = []
        for route in range(3):
            b = eng.batch(1, 1024, page_tokens=128)
            b.prefill(0, ids[:P + n] if route == 0 else ids[:P])
            if route == 1:
                b.append(0, ids[P:])
            elif route == 2:
                forced_steps(b, ids, P, n)
            logits.append(b.logits()[0].copy())
            b.close()
        spreads.append(max(norm_rel(logits[i], logits[j]) for i in range(3) for j in range(i)))
    bound = min(2.0 ** -5, 4 * spreads[0])
    print(f"three-route spread: bf16-KV {spreads[0]:.3e}, fp8-KV {spreads[1]:.3e}, bound {bound:.3e}")
    assert spreads[1] <= bound, (spreads, bound)
