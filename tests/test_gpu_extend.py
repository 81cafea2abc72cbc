"""GPU: qie_attention_extend — a block of new rows over a cached prefix — against the
oracle's self_attension.cu restatement (oracle.attention with q_abs_base = pos0).

The bar is test_gpu_ops.test_attention_prefill_causal's own: max |d| <= 2**-6 on inputs
from rand_bf16 at scale 1.0 (the arithmetic is that kernel's: bf16 MFMA products, fp32
scores and softmax, P in two bf16 parts; the split merge adds fp32 rounding only)."""
import ctypes as C
import functools

import numpy as np
import pytest

import gpu_util as G
from test_gpu_paged import Paged, _contig, rand_bf16

pytestmark = pytest.mark.gpu

BAR = 2 ** -6
L, LAYER, MAXC, T = 2, 1, 1152, 128
HEADS = [(64, 4, 4), (64, 14, 2), (128, 28, 4), (128, 16, 2)]   # G = 1, 7, 7, 8
ROWS = [(1, 1), (63, 2), (64, 16), (65, 17), (127, 33), (130, 5), (257, 100), (1000, 40)]
SENTINEL = 0x4D4D


@functools.lru_cache(maxsize=None)
def _kv(oracle, hd, nkv, B):
    """Host K/V caches [B][L][nkv][MAXC][hd], shared (read-only) by every case of a head shape."""
    kc = rand_bf16(oracle, (B, L, nkv, MAXC, hd), seed=hd + nkv + B)
    vc = rand_bf16(oracle, (B, L, nkv, MAXC, hd), seed=hd + nkv + B + 1)
    kc.setflags(write=False)
    vc.setflags(write=False)
    return kc, vc


def _cache(oracle, kc_h, vc_h, paged):
    """(descriptor, keepalive) of the cache, contiguous or paged with shuffled 128-token pages."""
    B, _, nkv, maxc, hd = kc_h.shape
    if paged:
        pg = Paged(oracle, kc_h, vc_h, T, seed=7)
        return pg.cache(), pg
    kc, vc = G.dev(kc_h), G.dev(vc_h)
    return _contig(kc, vc, L, nkv, hd, maxc), (kc, vc)


def _extend(qlib, c, q, pos, rps, nq, hd, poison=False, maxc=MAXC):
    """Runs the operator with `out` framed by one sentinel row on each side; returns [M][nq*hd]."""
    M = q.shape[0]
    nbytes = qlib.qie_attention_extend_workspace_bytes(M, nq, hd, maxc)
    ws = G.zeros_bytes(nbytes)
    if poison:
        assert nbytes > 0, "the poisoned case must be a multi-split one"
        G.check(qlib.qie_memset(G.p(ws), 0xFF, nbytes))   # NaNs in every partial slot
    out = G.dev(np.full((M + 2, nq * hd), SENTINEL, np.uint16))
    G.check(qlib.qie_attention_extend(G.p(G.dev(q)), M, G.p(G.dev(pos)), rps, C.byref(c), LAYER, nq,
                                      G.p(out) + nq * hd * 2, G.p(ws), None), "qie_attention_extend")
    got = G.host_bf16(out)
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), "rows outside [0, M) were written"
    return got[1:-1]


def _want(oracle, q, kc_h, vc_h, b, pos0, nq, nkv, hd):
    n = q.shape[0]
    return oracle.attention(q, kc_h[b, LAYER, :, :pos0 + n], vc_h[b, LAYER, :, :pos0 + n], nq, nkv, hd, True, pos0)


def _check(got, want, what):
    d = np.abs(G.bf(got) - G.bf(want))
    print(f"{what}: max |d| {d.max():.3e}")
    assert np.isfinite(G.bf(got)).all(), what
    assert d.max() <= BAR, f"{what}: {d.max()}"


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("pos0,n", ROWS)
@pytest.mark.parametrize("hd,nq,nkv", HEADS)
def test_extend_matches_oracle(oracle, qlib, hd, nq, nkv, pos0, n, paged):
    kc_h, vc_h = _kv(oracle, hd, nkv, 1)
    c, keep = _cache(oracle, kc_h, vc_h, paged)
    q = rand_bf16(oracle, (n, nq * hd), seed=pos0 + n)
    pos = np.arange(pos0, pos0 + n, dtype=np.int32)
    got = _extend(qlib, c, q, pos, n, nq, hd)
    _check(got, _want(oracle, q, kc_h, vc_h, 0, pos0, nq, nkv, hd), f"hd {hd} nq {nq} nkv {nkv} pos0 {pos0} n {n}")


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("hd,nq,nkv,n", [(64, 4, 4, 16), (64, 14, 2, 3)])
def test_extend_split_invisible_to_early_rows(oracle, qlib, hd, nq, nkv, n, paged):
    """One 16-row group straddles a split boundary: with the library's split length S for this
    call, the rows start at S - 2 (G = 1: rows 0, 1 of the group) or S - 1 (G = 7: the first
    token's 7 rows), so split 1 holds visible keys for the later rows of the group and none
    for the earlier ones — their (-inf, 0) partial must not disturb the merge."""
    S = qlib.qie_attention_extend_split_tokens(n, MAXC)
    assert S % 64 == 0 and S + n < MAXC and qlib.qie_attention_extend_workspace_bytes(n, nq, hd, MAXC) > 0
    G_ = nq // nkv
    pos0 = S - 2 if G_ == 1 else S - 1
    assert pos0 < S <= pos0 + n - 1 and (S - pos0) * G_ < 16 <= n * G_   # boundary inside the first 16-row group
    kc_h, vc_h = _kv(oracle, hd, nkv, 1)
    c, keep = _cache(oracle, kc_h, vc_h, paged)
    q = rand_bf16(oracle, (n, nq * hd), seed=91)
    got = _extend(qlib, c, q, np.arange(pos0, pos0 + n, dtype=np.int32), n, nq, hd, poison=True)
    _check(got, _want(oracle, q, kc_h, vc_h, 0, pos0, nq, nkv, hd), f"split {S} pos0 {pos0}")


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("hd,nq,nkv", [(64, 14, 2), (128, 16, 2)])
def test_extend_two_sequences(oracle, qlib, hd, nq, nkv, paged):
    """rows_per_seq = n, two sequences with different prefixes in one call."""
    n, starts = 20, (70, 300)
    kc_h, vc_h = _kv(oracle, hd, nkv, 2)
    c, keep = _cache(oracle, kc_h, vc_h, paged)
    q = rand_bf16(oracle, (2 * n, nq * hd), seed=17)
    pos = np.concatenate([np.arange(p, p + n, dtype=np.int32) for p in starts])
    got = _extend(qlib, c, q, pos, n, nq, hd)
    for b, p in enumerate(starts):
        _check(got[b * n:(b + 1) * n], _want(oracle, q[b * n:(b + 1) * n], kc_h, vc_h, b, p, nq, nkv, hd),
               f"sequence {b} pos0 {p}")


@pytest.mark.parametrize("paged", [False, True])
def test_extend_short_last_sequence(oracle, qlib, paged):
    """M is not a multiple of rows_per_seq: the last sequence has fewer rows (13 of 20)."""
    hd, nq, nkv, n, n2, starts = 64, 14, 2, 20, 13, (70, 300)
    kc_h, vc_h = _kv(oracle, hd, nkv, 2)
    c, keep = _cache(oracle, kc_h, vc_h, paged)
    q = rand_bf16(oracle, (n + n2, nq * hd), seed=19)
    pos = np.concatenate([np.arange(starts[0], starts[0] + n), np.arange(starts[1], starts[1] + n2)]).astype(np.int32)
    got = _extend(qlib, c, q, pos, n, nq, hd)
    _check(got[:n], _want(oracle, q[:n], kc_h, vc_h, 0, starts[0], nq, nkv, hd), "sequence 0")
    _check(got[n:], _want(oracle, q[n:], kc_h, vc_h, 1, starts[1], nq, nkv, hd), "sequence 1 (short)")


def test_extend_long_context_takes_longer_splits(oracle, qlib):
    """max_ctx past 64 splits of 512 keys doubles the split length (the split count is
    bounded): 40 rows at the end of a 33,000-key cache, one kv head to keep it small."""
    hd, nq, nkv, maxc, pos0, n = 64, 2, 1, 33000, 32900, 40
    assert qlib.qie_attention_extend_split_tokens(n, maxc) == 1024
    kc_h = rand_bf16(oracle, (1, 1, nkv, maxc, hd), seed=31)
    vc_h = rand_bf16(oracle, (1, 1, nkv, maxc, hd), seed=32)
    kc, vc = G.dev(kc_h), G.dev(vc_h)
    c = _contig(kc, vc, 1, nkv, hd, maxc)
    q = rand_bf16(oracle, (n, nq * hd), seed=33)
    ws = G.zeros_bytes(qlib.qie_attention_extend_workspace_bytes(n, nq, hd, maxc))
    out = G.zeros_bf16(n, nq * hd)
    G.check(qlib.qie_attention_extend(G.p(G.dev(q)), n, G.p(G.dev(np.arange(pos0, pos0 + n, dtype=np.int32))), n,
                                      C.byref(c), 0, nq, G.p(out), G.p(ws), None))
    want = oracle.attention(q, kc_h[0, 0, :, :pos0 + n], vc_h[0, 0, :, :pos0 + n], nq, nkv, hd, True, pos0)
    _check(G.host_bf16(out), want, "33k-key cache")


@pytest.mark.parametrize("paged", [False, True])
def test_extend_poisoned_workspace(oracle, qlib, paged):
    """Three splits of 512 keys at max_ctx 1,152, the rows see two of them: every partial slot
    the merge reads is written by the call itself (the workspace starts as NaNs)."""
    hd, nq, nkv, pos0, n = 128, 28, 4, 1000, 40
    kc_h, vc_h = _kv(oracle, hd, nkv, 1)
    c, keep = _cache(oracle, kc_h, vc_h, paged)
    q = rand_bf16(oracle, (n, nq * hd), seed=23)
    got = _extend(qlib, c, q, np.arange(pos0, pos0 + n, dtype=np.int32), n, nq, hd, poison=True)
    _check(got, _want(oracle, q, kc_h, vc_h, 0, pos0, nq, nkv, hd), "poisoned workspace")


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("P", [33, 130])
@pytest.mark.parametrize("hd,nq,nkv", [(64, 4, 4), (64, 14, 2), (128, 28, 4)])
def test_extend_single_split_equals_prefill_bitwise(oracle, qlib, hd, nq, nkv, P, paged):
    """P rows at positions 0..P-1 on a 512-key cache: qie_attention takes its MFMA prefill
    kernel (rows_per_seq >= 32), qie_attention_extend has exactly one split, and both walk the
    key tiles with the one attn_mfma_walk.  A row's result depends only on which key tiles it
    sees and on its own masked scores, not on how rows are packed into 16-row groups and
    workgroups (consecutive tokens there, flattened (token, head) pairs here): equal bit for bit."""
    maxc = 512
    assert qlib.qie_attention_extend_workspace_bytes(P, nq, hd, maxc) == 0   # one split, no merge
    kc_h = rand_bf16(oracle, (1, L, nkv, maxc, hd), seed=hd + nkv + P)
    vc_h = rand_bf16(oracle, (1, L, nkv, maxc, hd), seed=hd + nkv + P + 1)
    c, keep = _cache(oracle, kc_h, vc_h, paged)
    q = rand_bf16(oracle, (P, nq * hd), seed=P)
    pos = np.arange(P, dtype=np.int32)
    got = _extend(qlib, c, q, pos, P, nq, hd, maxc=maxc)
    out = G.zeros_bf16(P, nq * hd)
    G.check(qlib.qie_attention(G.p(G.dev(q)), P, G.p(G.dev(pos)), P, C.byref(c), LAYER, nq, G.p(out), None, None),
            "qie_attention")
    want = G.host_bf16(out)
    d = np.abs(G.bf(got) - G.bf(want))
    print(f"hd {hd} nq {nq} nkv {nkv} P {P} paged {paged}: rows differing {int((got != want).any(axis=1).sum())}, "
          f"max |d| {d.max():.3e}")
    assert np.isfinite(G.bf(want)).all() and want.any()
    assert np.array_equal(got, want)


def test_extend_bad_arguments(qlib):
    d = G.zeros_bf16(1 << 16)
    pos = G.dev(np.zeros(1, np.int32))
    out = G.zeros_bf16(1, 1024)
    for hd, nq, nkv in [(96, 4, 2), (64, 5, 2)]:   # head_dim not 64 / 128; nq % nkv != 0
        c = _contig(d, d, 1, nkv, hd, 64)
        assert qlib.qie_attention_extend(G.p(d), 1, G.p(pos), 1, C.byref(c), 0, nq, G.p(out), None, None) == -22
