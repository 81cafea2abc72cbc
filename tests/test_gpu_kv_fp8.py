"""GPU: the fp8 KV cache's operator tier (qie_ops.h "fp8 KV cache") — writer, expander, copy and
the decode attention on codes — against qie_quantize_rows_fp8, a numpy e4m3 decode table and a
float64 softmax attention over the decoded values."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as G
from conftest import rng
from qwen_inference_engine_amd import _lib
from qwen_inference_engine_amd._lib import KvCacheC, KvCacheFp8C, RowSegsC

pytestmark = pytest.mark.gpu

T = 128   # page_tokens of the paged cases
_c = np.arange(256)
_mag = np.where((_c >> 3) & 15, (1 + (_c & 7) / 8.0) * 2.0 ** (((_c >> 3) & 15) - 7.0), (_c & 7) * 2.0 ** -9)
E4M3 = np.where((_c & 0x7f) == 0x7f, np.nan, np.where(_c & 0x80, -_mag, _mag))   # OCP e4m3fn


def decode(codes, exps):   # float64 e4m3(code) * 2^(e - 127), one exponent per row
    return E4M3[codes] * 2.0 ** (exps.astype(np.float64) - 127)[..., None]


def rand_bf16(shape, seed, scale=1.0):
    return G.to_bf16((rng(seed).standard_normal(shape) * scale).astype(np.float32))


class Cache8:
    """Host image of an fp8 cache (and of a bf16 cache of the same geometry): arrays indexed
    [sequence or page][layer][kv head][token in run]([d]); at(s, t) gives the first and last index."""
    def __init__(self, B, L, nkv, hd, maxc, paged, seed=0):
        self.B, self.L, self.nkv, self.hd, self.maxc, self.paged = B, L, nkv, hd, maxc, paged
        self.mp = (maxc + T - 1) // T
        n0, self.run = (1 + B * self.mp, T) if paged else (B, maxc)
        self.table = 1 + rng(seed).permutation(B * self.mp).astype(np.int32).reshape(B, self.mp)
        r = rng(seed + 1)
        self.k = r.integers(0, 256, (n0, L, nkv, self.run, hd), dtype=np.uint8)
        self.v = r.integers(0, 256, (n0, L, nkv, self.run, hd), dtype=np.uint8)
        for a in (self.k, self.v):
            a[(a & 0x7f) == 0x7f] = 0x38                      # no NaN codes among the data
        self.ke = r.integers(121, 134, (n0, L, nkv, self.run), dtype=np.uint8)   # 2^-6 .. 2^6
        self.ve = r.integers(121, 134, (n0, L, nkv, self.run), dtype=np.uint8)

    def at(self, s, t):
        return (self.table[s, t // T], t % T) if self.paged else (s, t)

    def _desc(self, c, k, v, elems_per_tok):
        c.k, c.v = G.p(k), G.p(v)
        c.seq_stride = self.L * self.nkv * self.run * elems_per_tok
        c.n_layers, c.n_kv_heads, c.head_dim, c.max_ctx = self.L, self.nkv, self.hd, self.maxc
        if self.paged:
            self.dt = G.dev(self.table)
            c.block_table, c.page_tokens, c.max_pages = G.p(self.dt), T, self.mp

    def upload(self):
        self.dk, self.dv, self.dke, self.dve = G.dev(self.k), G.dev(self.v), G.dev(self.ke), G.dev(self.ve)
        c = KvCacheFp8C()
        self._desc(c.c, self.dk, self.dv, self.hd)
        c.k_exps, c.v_exps, c.exp_stride = G.p(self.dke), G.p(self.dve), self.L * self.nkv * self.run
        return c

    def download(self):
        return G.host(self.dk), G.host(self.dv), G.host(self.dke), G.host(self.dve)

    def bf16(self):   # a zeroed bf16 cache of the same geometry and block table
        h = np.zeros(self.k.shape, np.uint16)
        dk, dv = G.dev(h), G.dev(h)
        c = KvCacheC()
        self._desc(c, dk, dv, self.hd)
        return c, dk, dv


def stage_cache(B, nkv, hd, maxc, fill):
    h = np.full((B, 1, nkv, maxc, hd), fill, np.uint16)
    dk, dv = G.dev(h), G.dev(h)
    c = KvCacheC()
    c.k, c.v, c.seq_stride = G.p(dk), G.p(dv), nkv * maxc * hd
    c.n_layers, c.n_kv_heads, c.head_dim, c.max_ctx = 1, nkv, hd, maxc
    return c, dk, dv, h


def quantize_rows(qlib, rows_bf16):   # qie_quantize_rows_fp8: [n, hd] bf16 -> codes [n, hd], exps [n]
    n, hd = rows_bf16.shape
    q, e = G.zeros((n, hd), np.uint8), G.zeros((max(n, 16),), np.uint8)
    G.check(qlib.qie_quantize_rows_fp8(G.p(G.dev(rows_bf16)), hd, n, hd, G.p(q), hd, G.p(e), None))
    return G.host(q), G.host(e)[:n]


def exact_bf16(x):   # bf16 bits of float64 values that are exactly bf16 (asserted)
    b = G.to_bf16(x.astype(np.float32))
    assert np.array_equal(G.bf(b).astype(np.float64), x)
    return b


PARAMS = [pytest.param(hd, pg, id=f"hd{hd}-{'paged' if pg else 'contig'}") for hd in (64, 128) for pg in (False, True)]


# ------------------------------------------------------------------ 1. writer
@pytest.mark.parametrize("num,qkn", [("ref", False), ("hf", True)])
@pytest.mark.parametrize("hd,paged", PARAMS)
def test_qkv_post_fp8_equals_quantized_qkv_post(oracle, qlib, hd, paged, num, qkn):
    nq, nkv, L, layer, maxc, B = 4, 2, 2, 1, 256, 2
    QD, KD = nq * hd, nkv * hd
    cs, sn = oracle.rope_table(maxc, hd, 1e6, num)
    dcs, dsn = G.dev(cs), G.dev(sn)
    qn, kn = (G.dev(rand_bf16((hd,), s, 0.3)) for s in (1, 2))
    forms = [(1, 1, None), (17, 17, None), (17, 0, ([0, 5, 17], [1, 0])), (130, 65, None), (130, 0, ([0, 130], [1]))]
    for M, rps, segs in forms:
        qkv = rand_bf16((M, QD + 2 * KD), hd + M)
        qkv[0, QD:QD + hd] = 0                                             # an all-zero K row
        qkv[0, QD + KD:] = rand_bf16((KD,), 3, 0.1)
        qkv[0, QD + KD + 5] = G.to_bf16(np.float32([28.0]))[0]             # amax = 448 * 2^-4 exactly
        qkv[0, QD + KD + hd + 7] = G.to_bf16(np.float32([-28.125]))[0]     # ... and one bf16 step above
        if segs:
            sg = RowSegsC()
            sg.n = len(segs[1])
            sg.row0[:len(segs[0])], sg.seq[:sg.n] = segs[0], segs[1]
            seq = np.concatenate([np.full(b - a, s) for a, b, s in zip(segs[0], segs[0][1:], segs[1])])
            first = np.concatenate([np.full(b - a, a) for a, b in zip(segs[0], segs[0][1:])])
        else:
            seq, first = np.arange(M) // rps, (np.arange(M) // rps) * rps
        pos = (3 + np.arange(M) - first).astype(np.int32)                  # M = 130: across the page boundary
        c8h = Cache8(B, L, nkv, hd, maxc, paged, seed=M)
        for a, fill in ((c8h.k, 0xAB), (c8h.v, 0xAB), (c8h.ke, 0xCD), (c8h.ve, 0xCD)):
            a[:] = fill                                                    # sentinels everywhere
        c8 = c8h.upload()
        cb, bk, bv = c8h.bf16()
        st, sk, sv, st_h = stage_cache(B, nkv, hd, maxc, 0x1234)
        q8, qb = G.zeros_bf16(M, QD), G.zeros_bf16(M, QD)
        args = (G.p(qn) if qkn else None, G.p(kn) if qkn else None, G.p(dcs), G.p(dsn), nq)
        tail = (layer, 1e-6, 0 if num == "ref" else 1)
        dq, dp = G.dev(qkv), G.dev(pos)
        G.check(qlib.qie_qkv_post_fp8(G.p(dq), M, G.p(dp), max(rps, 1), C.byref(sg) if segs else None, *args,
                                      C.byref(c8), C.byref(st), *tail, G.p(q8), None))
        if segs:
            G.check(qlib.qie_qkv_post_ragged(G.p(dq), M, G.p(dp), C.byref(sg), *args, C.byref(cb), *tail, G.p(qb), None))
        else:
            G.check(qlib.qie_qkv_post(G.p(dq), M, G.p(dp), rps, *args, C.byref(cb), *tail, G.p(qb), None))
        assert np.array_equal(G.host(q8), G.host(qb)), (M, "q")
        want = [a.copy() for a in (c8h.k, c8h.v, c8h.ke, c8h.ve)]
        want_st = [st_h.copy(), st_h.copy()]
        for kv, dbf in enumerate((bk, bv)):
            hb = G.host(dbf)
            rows = np.stack([hb[c8h.at(seq[m], pos[m])[0], layer, :, c8h.at(seq[m], pos[m])[1]] for m in range(M)])
            codes, exps = quantize_rows(qlib, rows.reshape(M * nkv, hd))
            deq = exact_bf16(decode(codes, exps)).reshape(M, nkv, hd)
            for m in range(M):
                i, j = c8h.at(seq[m], pos[m])
                want[kv][i, layer, :, j] = codes.reshape(M, nkv, hd)[m]
                want[2 + kv][i, layer, :, j] = exps.reshape(M, nkv)[m]
                want_st[kv][seq[m], 0, :, pos[m]] = deq[m]
        for got, w, what in zip(c8h.download() + (G.host(sk), G.host(sv)), want + want_st,
                                ("k codes", "v codes", "k exps", "v exps", "stage k", "stage v")):
            assert np.array_equal(got, w), (M, rps, what)
        assert want[2][c8h.at(seq[0], pos[0])[0], layer, 0, c8h.at(seq[0], pos[0])[1]] == 127   # zero row: scale 1
        G.release_all()


# ------------------------------------------------------- 2. dequantise / copy
@pytest.mark.parametrize("hd,paged", PARAMS)
def test_kv_dequantize_and_copy_fp8(qlib, hd, paged):
    nkv, L, layer, maxc, B, pos0, n = 2, 2, 1, 256, 2, 100, 60    # rows 100 .. 159: across the page boundary
    h = Cache8(B, L, nkv, hd, maxc, paged, seed=hd)
    c8 = h.upload()
    st, sk, sv, st_h = stage_cache(B, nkv, hd, maxc, 0x1234)
    G.check(qlib.qie_kv_dequantize_fp8(C.byref(c8), 0, layer, pos0, n, C.byref(st), 1, 0, None))
    assert qlib.qie_kv_dequantize_fp8(C.byref(c8), 0, layer, pos0, 0, C.byref(st), 1, 0, None) == 0
    for codes, exps, got in ((h.k, h.ke, sk), (h.v, h.ve, sv)):
        want = st_h.copy()
        for t in range(pos0, pos0 + n):
            i, j = h.at(0, t)
            want[1, 0, :, t] = exact_bf16(decode(codes[i, layer, :, j], exps[i, layer, :, j]))
        assert np.array_equal(G.host(got), want)
    G.check(qlib.qie_kv_copy_fp8(C.byref(c8), 0, C.byref(c8), 1, pos0, n, None))
    assert qlib.qie_kv_copy_fp8(C.byref(c8), 0, C.byref(c8), 0, pos0, n, None) == -22   # the same sequence
    for src, got in zip((h.k, h.v, h.ke, h.ve), h.download()):
        want = src.copy()
        for t in range(pos0, pos0 + n):
            (i0, j0), (i1, j1) = h.at(0, t), h.at(1, t)
            want[i1, :, :, j1] = src[i0, :, :, j0]
        assert np.array_equal(got, want)


# ----------------------------------------------- 3. decode attention, exact inputs
def attention64(q, K, V, nq, nkv, hd):   # float64; q [nq * hd], K / V [nkv][ctx][hd]
    out = np.empty((nq, hd))
    for h in range(nq):
        s = K[h // (nq // nkv)] @ q[h * hd:(h + 1) * hd] / np.sqrt(hd)
        w = np.exp(s - s.max())
        out[h] = (w / w.sum()) @ V[h // (nq // nkv)]
    return out.reshape(-1)


@pytest.mark.parametrize("form", ["ref", "qknorm", "hf", "preroped"])
@pytest.mark.parametrize("nq,nkv", [(28, 4), (4, 2)])
@pytest.mark.parametrize("hd,paged", PARAMS)
def test_attention_decode_fp8_exact_inputs(oracle, qlib, hd, paged, nq, nkv, form):
    """Bound: test_attention_decode's own.  The reference includes the row the kernel appended."""
    L, layer, maxc, B = 2, 1, 4224, 3
    QD, KD = nq * hd, nkv * hd
    num = "hf" if form == "hf" else "ref"
    qkn = form == "qknorm"
    eps = 1e-4 if num == "ref" else 1e-6
    # q is kept small (2^-9; with qk-norm through its weight) so that the scores over K values of up
    # to 448 * 2^6 stay O(10): a softmax with many keys in play, not a one-hot
    qn = rand_bf16((hd,), 1, 2.0 ** -9) if qkn else None
    kn = rand_bf16((hd,), 2, 0.3) if qkn else None
    cs, sn = oracle.rope_table(maxc, hd, 1e6, num)
    dcs, dsn, dqn, dkn = G.dev(cs), G.dev(sn), G.dev(qn) if qkn else None, G.dev(kn) if qkn else None
    base = Cache8(B, L, nkv, hd, maxc, paged, seed=hd + nq)
    cb, bk, bv = base.bf16()
    ws = G.zeros_bytes(qlib.qie_attention_decode_workspace_bytes(B, nq, nkv, hd, maxc))
    ws16 = G.zeros_bytes(qlib.qie_attention_decode_workspace_bytes(B, nq, nkv, hd, maxc))
    for ctxs in ([1, 127, 128], [129, 257, 300], [4200]):
        nb = len(ctxs)
        pos = np.array(ctxs, np.int32) - 1
        h = Cache8(B, L, nkv, hd, maxc, paged, seed=hd + nq)
        for b, ctx in enumerate(ctxs):                      # NaN codes and exponents past the context
            for t in range(ctx - 1, min(maxc, ctx + 300)):
                i, j = h.at(b, t)
                h.k[i, :, :, j], h.v[i, :, :, j], h.ke[i, :, :, j], h.ve[i, :, :, j] = 0x7f, 0x7f, 0xff, 0xff
        c8 = h.upload()
        qkv = rand_bf16((nb, QD + 2 * KD), 5 + ctxs[0])
        qkv[:, :QD] = rand_bf16((nb, QD), 6 + ctxs[0], 2.0 ** -9)
        q, k = qkv[:, :QD].copy(), qkv[:, QD:QD + KD].copy()
        if qkn:
            q = oracle.qknorm(q, qn, nq, hd, eps, num)
        q = oracle.rope(q, cs, sn, pos, nq, hd, num)
        flags = 0 if num == "ref" else 1
        if form == "preroped":
            k = oracle.rope(k, cs, sn, pos, nkv, hd, num)
            qkv = np.concatenate([q, k, qkv[:, QD + KD:]], axis=1)
            flags = _lib.QIE_ATTN_PREROPED
        out, out16 = G.zeros_bf16(nb, QD), G.zeros_bf16(nb, QD)
        call = (G.p(G.dev(qkv)), nb, G.p(G.dev(pos)), G.p(dqn), G.p(dkn), G.p(dcs), G.p(dsn), nq)
        for rep in range(2):   # the second call checks the counters were left zeroed
            G.check(qlib.qie_attention_decode_fp8(*call, C.byref(c8), layer, eps, flags, G.p(out), G.p(ws), None))
        G.check(qlib.qie_attention_decode(*call, C.byref(cb), layer, eps, flags, G.p(out16), G.p(ws16), None))
        got = G.bf(G.host(out)).astype(np.float64)
        gk, gv, gke, gve = h.download()
        hb16 = (G.host(bk), G.host(bv))
        for b, ctx in enumerate(ctxs):
            idx = [h.at(b, t) for t in range(ctx)]
            ii, jj = np.array([i for i, _ in idx]), np.array([j for _, j in idx])
            K = decode(gk[ii, layer, :, jj], gke[ii, layer, :, jj]).transpose(1, 0, 2)
            V = decode(gv[ii, layer, :, jj], gve[ii, layer, :, jj]).transpose(1, 0, 2)
            assert np.isfinite(K).all() and np.isfinite(V).all()
            want = attention64(G.bf(q[b]).astype(np.float64), K, V, nq, nkv, hd)
            d = np.abs(got[b] - want)
            print(f"ctx {ctx}: max |d| {d.max():.3e}, bound {2 ** -7 * max(1.0, np.abs(want).max()) * 2:.3e}")
            assert d.max() <= 2 ** -7 * max(1.0, np.abs(want).max()) * 2, f"ctx {ctx}: {d.max()}"
            # the appended row = the bf16 kernel's appended row through qie_quantize_rows_fp8
            i, j = idx[-1]
            for g8, ge8, hb in ((gk, gke, hb16[0]), (gv, gve, hb16[1])):
                codes, exps = quantize_rows(qlib, hb[i, layer, :, j])
                assert np.array_equal(g8[i, layer, :, j], codes) and np.array_equal(ge8[i, layer, :, j], exps), ctx
            # ... and nothing past it was written
            i, j = h.at(b, ctx)
            assert (gk[i, :, :, j] == 0x7f).all() and (gve[i, :, :, j] == 0xff).all()
        assert not G.host(ws)[:B * nkv * 4].any()


# ------------------------------------------------------------------ 4. needle
@pytest.mark.parametrize("hd,paged", PARAMS)
def test_attention_decode_fp8_needle(qlib, oracle, hd, paged):
    """One key takes all the weight (score >= 128, every other K row zero: exp(-128) is 0 in fp32), so
    the output is that key's decoded V row bit for bit — a wrong exponent, row or byte order shows."""
    nq, nkv, L, layer, maxc, ctx = 4, 2, 2, 1, 384, 300
    QD, KD = nq * hd, nkv * hd
    cs, sn = oracle.rope_table(maxc, hd, 1e6, "ref")
    dcs, dsn = G.dev(cs), G.dev(sn)
    u = rng(hd).choice([-1.0, 1.0], hd)
    pos = np.array([ctx - 1], np.int32)
    ws = G.zeros_bytes(qlib.qie_attention_decode_workspace_bytes(1, nq, nkv, hd, maxc))
    for needle in (0, 127, 128, ctx - 2, ctx - 1):
        h = Cache8(1, L, nkv, hd, maxc, paged, seed=needle)
        h.k[:] = 0
        qkv = np.zeros((1, QD + 2 * KD), np.uint16)
        qkv[0, :QD] = G.to_bf16(np.tile(4 * u, nq).astype(np.float32))
        # no V element of the needle is zero: 1 * (-0) + 0 * v is +0, the one bit a sum cannot keep
        qkv[0, QD + KD:] = G.to_bf16(rng(needle).choice([-3.0, -1.5, 1.0, 2.0, 3.0], KD).astype(np.float32))
        if needle == ctx - 1:                                  # the new token itself
            qkv[0, QD:QD + KD] = G.to_bf16(np.tile(4 * u, nkv).astype(np.float32))
        else:
            i, j = h.at(0, needle)
            h.k[i, layer, :, j] = np.where(u > 0, 0x60, 0xE0)   # +-32 ...
            h.ke[i, layer, :, j] = 124                          # ... x 2^-3
            h.ve[i, layer, :, j] = [131, 122]                   # the needle's V rows: their own exponents
            h.v[i, layer, :, j] |= np.where(h.v[i, layer, :, j] & 0x7f, 0, 0x38).astype(np.uint8)
        c8 = h.upload()
        out = G.zeros_bf16(1, QD)
        G.check(qlib.qie_attention_decode_fp8(G.p(G.dev(qkv)), 1, G.p(G.dev(pos)), None, None, G.p(dcs), G.p(dsn), nq,
                                              C.byref(c8), layer, 1e-6, _lib.QIE_ATTN_PREROPED, G.p(out), G.p(ws), None))
        _, gv, _, gve = h.download()
        i, j = h.at(0, needle)
        want = exact_bf16(decode(gv[i, layer, :, j], gve[i, layer, :, j]))       # [nkv][hd]
        assert np.array_equal(G.host(out).reshape(nkv, nq // nkv, hd), np.repeat(want[:, None], nq // nkv, 1)), needle
        G.release_all()
