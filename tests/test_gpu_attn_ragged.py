"""GPU: the ragged operator tier — qie_attention_ragged and qie_qkv_post_ragged — whose rows
are up to 8 segments of any lengths, each of its own cache sequence (qie_row_segs).

qie_attention_ragged against the oracle under test_gpu_extend's bar (2**-6 on rand_bf16 inputs
at scale 1.0: the arithmetic is that kernel's), bit for bit against qie_attention_extend on each
segment alone (inside a segment the rows are packed as the extend kernel packs a sequence's, so
with equal split lengths the same tiles are walked for the same 16-row groups), and key by key
through attn_cases' exact families.  qie_qkv_post_ragged bit for bit against per-segment
qie_qkv_post calls on a twin cache.  `out` is framed by sentinel rows, the workspace starts as
0xFF bytes."""
import ctypes as C

import numpy as np
import pytest

import attn_cases as A
import gpu_util as G
from test_gpu_attention_keys import SENTINEL, Dev
from test_gpu_extend import HEADS, L, LAYER, MAXC, _cache, _check, _extend, _kv, _want
from test_gpu_paged import _contig, rand_bf16

from qwen_inference_engine_amd import _lib

pytestmark = pytest.mark.gpu

PAGED = pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])


def _segs(lengths, seqs):
    t = _lib.RowSegsC()
    t.n = len(lengths)
    row0 = np.concatenate([[0], np.cumsum(lengths)])
    for z in range(_lib.QIE_RAGGED_MAX_SEGS + 1):
        t.row0[z] = int(row0[min(z, len(lengths))])
    for z, s in enumerate(seqs):
        t.seq[z] = int(s)
    return t


def _ragged(qlib, c, q, pos, segs, nq, hd, maxc, layer=LAYER, what="qie_attention_ragged"):
    """Runs the operator with `out` framed by a sentinel row on each side and every partial slot
    of the workspace a NaN; returns [M][nq*hd]."""
    M = q.shape[0]
    nbytes = qlib.qie_attention_extend_workspace_bytes(M, nq, hd, maxc)
    ws = G.zeros_bytes(nbytes)
    if nbytes:
        G.check(qlib.qie_memset(G.p(ws), 0xFF, nbytes))
    out = G.dev(np.full((M + 2, nq * hd), SENTINEL, np.uint16))
    G.check(qlib.qie_attention_ragged(G.p(G.dev(q)), G.p(G.dev(pos)), C.byref(segs), C.byref(c), layer, nq,
                                      G.p(out) + nq * hd * 2, G.p(ws), None), what)
    got = G.host_bf16(out)
    assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), "rows outside [0, M) were written"
    return got[1:-1]


def _seq_cache(c, keep, b, paged):
    """The descriptor whose sequence 0 is sequence b of cache c."""
    if paged:
        return keep.cache(b)
    cz = _lib.KvCacheC()
    C.memmove(C.byref(cz), C.byref(c), C.sizeof(cz))
    cz.k, cz.v = c.k + b * c.seq_stride * 2, c.v + b * c.seq_stride * 2
    return cz


def _positions(starts, lengths):
    return np.concatenate([np.arange(p, p + n) for p, n in zip(starts, lengths)]).astype(np.int32)


# (pos0, n, cache sequence): a non-identity slot map, a one-row segment, a fresh segment and one
# that crosses key 512
ORACLE_SEGS = [(0, 5, 3), (70, 33, 0), (300, 1, 2), (500, 40, 1)]


@PAGED
@pytest.mark.parametrize("hd,nq,nkv", HEADS)
def test_ragged_matches_oracle(oracle, qlib, hd, nq, nkv, paged):
    kc_h, vc_h = _kv(oracle, hd, nkv, 4)
    c, keep = _cache(oracle, kc_h, vc_h, paged)
    starts, lengths, seqs = zip(*ORACLE_SEGS)
    M = sum(lengths)
    q = rand_bf16(oracle, (M, nq * hd), seed=41)
    got = _ragged(qlib, c, q, _positions(starts, lengths), _segs(lengths, seqs), nq, hd, MAXC)
    r = 0
    for p0, n, b in ORACLE_SEGS:
        _check(got[r:r + n], _want(oracle, q[r:r + n], kc_h, vc_h, b, p0, nq, nkv, hd),
               f"hd {hd} nq {nq} nkv {nkv} segment (pos0 {p0}, n {n}, sequence {b})")
        r += n


# (max_ctx, lengths, pos0s, the split both ops must use): one split whatever its length; every segment and the total
# above 32 rows (512-key splits); the total at most 32 (256-key splits)
BITWISE = [(256, (3, 17, 130), (0, 60, 100), 256),
           (1152, (33, 40, 100), (1000, 0, 257), 512),
           (1152, (5, 20), (600, 250), 256)]


@PAGED
@pytest.mark.parametrize("maxc,lengths,starts,split", BITWISE, ids=["one_split", "split512", "split256"])
@pytest.mark.parametrize("hd,nq,nkv", [(64, 14, 2), (128, 28, 4), (64, 4, 4)])
def test_ragged_equals_extend_per_segment_bitwise(oracle, qlib, hd, nq, nkv, maxc, lengths, starts, split, paged):
    M, B = sum(lengths), len(lengths)
    for n in lengths + (M,):   # both ops cut the context alike: into one split, or at the same keys
        if maxc <= split:
            assert qlib.qie_attention_extend_workspace_bytes(n, nq, hd, maxc) == 0
        else:
            assert qlib.qie_attention_extend_split_tokens(n, maxc) == split
            assert qlib.qie_attention_extend_workspace_bytes(n, nq, hd, maxc) > 0
    kc_h = rand_bf16(oracle, (B, L, nkv, maxc, hd), seed=hd + nkv + maxc)
    vc_h = rand_bf16(oracle, (B, L, nkv, maxc, hd), seed=hd + nkv + maxc + 1)
    c, keep = _cache(oracle, kc_h, vc_h, paged)
    seqs = [(z + 1) % B for z in range(B)]   # not the identity
    q = rand_bf16(oracle, (M, nq * hd), seed=M)
    pos = _positions(starts, lengths)
    got = _ragged(qlib, c, q, pos, _segs(lengths, seqs), nq, hd, maxc)
    assert np.isfinite(G.bf(got)).all() and got.any()
    r = 0
    for z, n in enumerate(lengths):
        want = _extend(qlib, _seq_cache(c, keep, seqs[z], paged), q[r:r + n], pos[r:r + n], n, nq, hd, maxc=maxc)
        diff = int((got[r:r + n] != want).any(axis=1).sum())
        print(f"hd {hd} nq {nq} nkv {nkv} maxc {maxc} segment {z} ({n} rows at {starts[z]}): rows differing {diff}")
        assert np.array_equal(got[r:r + n], want), f"segment {z}"
        r += n


def _case_segs(c):
    """A case's (M, rows_per_seq) as segments: segment z = rows [z*rps, min((z+1)*rps, M)), sequence z."""
    lengths = [min(c.rps, c.M - r) for r in range(0, c.M, c.rps)]
    return _segs(lengths, range(len(lengths)))


def _run_keys(qlib, oracle, shape, family, paged, trap):
    n = 0
    for c in A.cases("extend", shape, family, trap=trap, oracle=oracle, sweeps=trap is None):
        d = Dev(oracle, c, paged)
        assert qlib.qie_attention_extend_workspace_bytes(c.M, c.nq, c.hd, c.maxc) > 0
        got = _ragged(qlib, d.desc, c.q, c.pos, _case_segs(c), c.nq, c.hd, c.maxc, layer=A.LAYER, what=c.name)
        ok = A.accepted(c, got)
        assert ok.all(), (f"{int((~ok).sum())} of {ok.size} (row, head)s, paged {paged}: "
                          + A.describe(c, got, *np.argwhere(~ok)[0]))
        G.release_all()
        n += 1
    print(f"ragged {shape} {family} paged {paged} trap {trap}: {n} launches exact")


@pytest.mark.parametrize("trap", [None, "nan"], ids=["plain", "nan"])
@PAGED
@pytest.mark.parametrize("family", ["needle", "ramp_up", "ramp_down"])
@pytest.mark.parametrize("shape", A.SHAPES["extend"], ids=lambda s: f"{s[0]}-{s[1]}-{s[2]}")
def test_ragged_sees_every_key(oracle, qlib, shape, family, paged, trap):
    """attn_cases' exact families for the extend kernel, run through the ragged op; the
    two_seqs_short_last layout is a real ragged case (20 + 13 rows)."""
    assert len(A.SHAPES["extend"]) == 3
    _run_keys(qlib, oracle, shape, family, paged, trap)


# ------------------------------------------------------------------ qie_qkv_post_ragged
QKV_LENGTHS, QKV_SEQS, QKV_POS0 = (7, 1, 20), (2, 0, 1), (30, 140, 250)
QKV_MAXC, QKV_B = 320, 3


def _qkv_post(qlib, ragged, qkv, M, pos, how, qn, kn, cs, sn, nq, c, eps, num, q_out):
    fn = qlib.qie_qkv_post_ragged if ragged else qlib.qie_qkv_post
    return fn(G.p(qkv), M, G.p(pos), C.byref(how) if ragged else how, G.p(qn), G.p(kn), G.p(cs), G.p(sn), nq, C.byref(c),
              LAYER, eps, num, G.p(q_out), None)


@PAGED
@pytest.mark.parametrize("hd,nq,nkv,hf", [(64, 14, 2, False), (128, 16, 2, True)], ids=["hd64-ref-bias", "hd128-hf-qknorm"])
def test_qkv_post_ragged_equals_per_segment_calls(oracle, qlib, hd, nq, nkv, hf, paged):
    """q_out and the WHOLE cache (or pool) equal those of one qie_qkv_post call per segment on a
    twin cache: the segment's rows landed in its own sequence and no other row changed."""
    M, eps = sum(QKV_LENGTHS), 1e-6
    width = (nq + 2 * nkv) * hd
    qkv_h = rand_bf16(oracle, (M, width), seed=hd)
    if not hf:   # REF with bias rows: the projection's bias already added (a constant row offset)
        qkv_h = oracle.f32_to_bf16(G.bf(qkv_h) + G.bf(rand_bf16(oracle, (1, width), 0.5, seed=hd + 1)))
    cs_h, sn_h = np.zeros((QKV_MAXC, hd // 2), np.float32), np.zeros((QKV_MAXC, hd // 2), np.float32)
    G.check(qlib.qie_rope_table_host(cs_h.ctypes.data_as(C.POINTER(C.c_float)), sn_h.ctypes.data_as(C.POINTER(C.c_float)),
                                     QKV_MAXC, hd, 10000.0, 1 if hf else 0))
    cs, sn = G.dev(cs_h), G.dev(sn_h)
    qn = G.dev(rand_bf16(oracle, (hd,), seed=5)) if hf else None
    kn = G.dev(rand_bf16(oracle, (hd,), seed=6)) if hf else None
    kc_h = rand_bf16(oracle, (QKV_B, L, nkv, QKV_MAXC, hd), seed=hd + 2)
    vc_h = rand_bf16(oracle, (QKV_B, L, nkv, QKV_MAXC, hd), seed=hd + 3)
    pos_h = _positions(QKV_POS0, QKV_LENGTHS)
    qkv, pos = G.dev(qkv_h), G.dev(pos_h)

    def state(keep):
        if paged:
            return G.host_bf16(keep.dk).copy(), G.host_bf16(keep.dv).copy()
        return G.host_bf16(keep[0]).copy(), G.host_bf16(keep[1]).copy()

    ca, keep_a = _cache(oracle, kc_h, vc_h, paged)
    qa = G.dev(np.full((M, nq * hd), SENTINEL, np.uint16))
    G.check(_qkv_post(qlib, True, qkv, M, pos, _segs(QKV_LENGTHS, QKV_SEQS), qn, kn, cs, sn, nq, ca, eps, int(hf), qa),
            "qie_qkv_post_ragged")
    cb, keep_b = _cache(oracle, kc_h, vc_h, paged)
    k0, v0 = state(keep_b)
    qb = G.dev(np.full((M, nq * hd), SENTINEL, np.uint16))
    r = 0
    for n, b in zip(QKV_LENGTHS, QKV_SEQS):
        cz = _seq_cache(cb, keep_b, b, paged)
        G.check(qlib.qie_qkv_post(G.p(qkv) + r * width * 2, n, G.p(pos) + r * 4, n, G.p(qn), G.p(kn), G.p(cs), G.p(sn),
                                  nq, C.byref(cz), LAYER, eps, int(hf), G.p(qb) + r * nq * hd * 2, None), "qie_qkv_post")
        r += n
    got_q, want_q = G.host_bf16(qa), G.host_bf16(qb)
    assert not (want_q == SENTINEL).all(axis=1).any() and np.isfinite(G.bf(want_q)).all()
    assert np.array_equal(got_q, want_q), "q_out"
    (ka, va), (kb, vb) = state(keep_a), state(keep_b)
    assert (kb != k0).any() and (vb != v0).any(), "the twin's cache was not written"
    assert np.array_equal(ka, kb) and np.array_equal(va, vb), "the caches differ"


def test_ragged_bad_arguments_write_nothing(oracle, qlib):
    hd, nq, nkv, M, maxc = 64, 4, 2, 12, 256
    kc_h = rand_bf16(oracle, (2, L, nkv, maxc, hd), seed=1)
    kc, vc = G.dev(kc_h), G.dev(kc_h)
    c = _contig(kc, vc, L, nkv, hd, maxc)
    q = G.dev(rand_bf16(oracle, (M, nq * hd), seed=2))
    qkv = G.dev(rand_bf16(oracle, (M, (nq + 2 * nkv) * hd), seed=3))
    pos = G.dev(np.arange(M, dtype=np.int32))
    cs = G.dev(np.ones((maxc, hd // 2), np.float32))
    out = G.dev(np.full((M, nq * hd), SENTINEL, np.uint16))
    good = _segs((5, 7), (0, 1))

    def table(n=2, row0=(0, 5, 12), seq=(0, 1)):
        t = _segs((5, 7), (0, 1))
        t.n = n
        for z in range(_lib.QIE_RAGGED_MAX_SEGS + 1):
            t.row0[z] = row0[min(z, len(row0) - 1)]
        for z, s in enumerate(seq):
            t.seq[z] = s
        return t

    bad = {"n = 0": table(n=0), "n = 9": table(n=9), "row0[0] != 0": table(row0=(1, 5, 12)),
           "row0 not increasing": table(row0=(0, 5, 5)), "row0 decreasing": table(row0=(0, 7, 5)),
           "repeated seq": table(seq=(1, 1))}

    def attn(t, cache=c, heads=nq):
        return qlib.qie_attention_ragged(G.p(q), G.p(pos), C.byref(t), C.byref(cache), LAYER, heads, G.p(out), None, None)

    def post(t, rows=M, cache=c):
        return qlib.qie_qkv_post_ragged(G.p(qkv), rows, G.p(pos), C.byref(t), None, None, G.p(cs), G.p(cs), nq,
                                        C.byref(cache), LAYER, 1e-6, 0, G.p(out), None)

    for what, t in bad.items():
        assert attn(t) == -22, f"qie_attention_ragged: {what}"
        assert post(t) == -22, f"qie_qkv_post_ragged: {what}"
    assert post(good, rows=M + 1) == -22 and post(good, rows=M - 1) == -22, "row0[n] != M"
    c96 = _contig(kc, vc, L, nkv, 96, maxc)
    assert attn(good, cache=c96) == -22, "head_dim 96"
    assert attn(good, heads=5) == -22, "nq % nkv != 0"
    assert qlib.qie_attention_ragged(G.p(q), G.p(pos), C.byref(good), C.byref(c), L, nq, G.p(out), None, None) == -22
    G.check(qlib.qie_synchronize())
    assert (G.host_bf16(out) == SENTINEL).all(), "a refused call wrote its output"
    assert np.array_equal(G.host_bf16(kc).reshape(kc_h.shape), kc_h), "a refused call wrote the cache"
    assert attn(good) == 0 and post(good) == 0   # the same buffers with a well-formed table
