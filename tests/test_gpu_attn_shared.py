"""GPU: qie_attention_decode_shared (k_attn_shared.hip) — decode attention that reads a group's
shared prompt prefix once, through the leader's rows — against a float64 softmax, against
qie_attention_decode on caches where every member holds its own copy of the prefix, with the
members' own prefix rows poisoned, and on needle cases (attn_cases.py's construction) whose one
dominant key sits in the shared prefix or in a member's suffix.

Two layouts.  `short` (max_ctx 512: splits of one 128-key step) is the issue's table.  `long`
(max_ctx 16,512: splits of 384 keys, three steps) is one group of eight members — 56 or 64 stacked
rows, all four row tiles — whose prefix walks run several steps: both V buffers and the first
one again, the rescale of O, and members masked from the second or third step of a walk on."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import attn_cases as A
import gpu_util as G
from conftest import rng
from test_gpu_paged import Paged, _contig

from qwen_inference_engine_amd import _lib

pytestmark = pytest.mark.gpu

L, LAYER, T = A.L, A.LAYER, 128


def layout(maxc, stride, share, pos):
    pos = np.array(pos, np.int32)
    return SimpleNamespace(maxc=maxc, stride=stride, share=share, pos=pos, B=len(share),
                           keys=(int(pos.max()) + T) // T * T)   # the rows that hold data: a whole page past every pos


# slot: (leader, n_shared), pos — a leader with a suffix crossing a step, a member whose suffix is
# only the new key, a plain slot between members, a member that skips the prefix's second step and
# crosses a step in its suffix, and a second group
SHORT = layout(512, 40, [(0, 256), (0, 256), (2, 0), (0, 128), (4, 128), (4, 128)], [300, 256, 5, 258, 200, 128])
# prefix splits [0, 384) and [384, 768): member 2 drops out after the first step of the first, member 6
# after its second, member 4 after the first step of the second, member 3 skips the second whole;
# suffix splits of one to three steps, a suffix that is only the new key (1, 6)
LONG = layout(16512, 90, [(0, 768), (0, 768), (0, 128), (0, 384), (0, 512), (0, 768), (0, 256), (0, 640)],
              [900, 768, 700, 1200, 640, 1000, 256, 770])
CASES = [(SHORT, hd, nq, nkv, pg) for hd in (64, 128) for nq, nkv in ((2, 2), (7, 1), (8, 1)) for pg in (False, True)]
CASES += [(LONG, 64, 7, 1, True), (LONG, 64, 8, 1, False), (LONG, 128, 7, 1, False), (LONG, 128, 8, 1, True)]
IDS = [f"{'short' if y is SHORT else 'long'}-{hd}-{nq}-{nkv}-{'paged' if pg else 'contig'}" for y, hd, nq, nkv, pg in CASES]


def cache_of(y, rows):
    """[B][L][nkv][maxc][hd] bits: `rows` [B][L][nkv][keys][hd] in front, zeros (never visible) behind."""
    out = np.zeros(rows.shape[:3] + (y.maxc, rows.shape[4]), np.uint16)
    out[:, :, :, :y.keys] = rows
    return out


def copy_prefix(y, K):
    """Every member's own rows [0, n_shared) become its leader's: the caller's guarantee."""
    for m, (l, n) in enumerate(y.share):
        K[m, :, :, :n] = K[l, :, :, :n]
    return K


def poisoned(y, K):
    """... and what only a kernel that reads the prefix through the leader survives: NaN there."""
    K = K.copy()
    for m, (l, n) in enumerate(y.share):
        if l != m:
            K[m, :, :, :n] = A.NAN
    return K


def ref64(y, q, K, V, nq, nkv, hd):
    """float64 softmax(q k / sqrt(hd)) v per (slot, head) over keys [0, pos] of the slot's own rows
    (K, V [B][nkv][maxc][hd] bits with the new row in place); returns (out, 1 - largest weight)."""
    out, slack = np.empty((y.B, nq, hd)), np.empty((y.B, nq))
    for m in range(y.B):
        for h in range(nq):
            g, n = h // (nq // nkv), int(y.pos[m]) + 1
            s = A.f64(K[m, g, :n]) @ A.f64(q[m, h * hd:(h + 1) * hd]) / np.float64(np.sqrt(np.float32(hd)))
            w = np.exp(s - s.max())
            w /= w.sum()
            out[m, h], slack[m, h] = w @ A.f64(V[m, g, :n]), 1 - w.max()
    return out.reshape(y.B, nq * hd), slack


class Run:
    """One set of inputs on the device, contiguous or paged; call() runs either operator."""

    def __init__(self, oracle, qlib, y, Kh, Vh, qkv, nq, nkv, hd, paged, num=0, eps=1e-4, qn=None, kn=None, cs=None, sn=None):
        self.qlib, self.y, self.nq, self.nkv, self.hd, self.paged, self.num, self.eps = qlib, y, nq, nkv, hd, paged, num, eps
        if paged:
            self.pg = Paged(oracle, Kh, Vh, T, seed=3)
            self.desc = self.pg.cache()
        else:
            self.kc, self.vc = G.dev(Kh), G.dev(Vh)
            self.desc = _contig(self.kc, self.vc, L, nkv, hd, y.maxc)
        self.args = [G.dev(x) if x is not None else None for x in (qkv, y.pos, qn, kn, cs, sn)]
        t = (_lib.PrefixShareC * y.B)(*[_lib.PrefixShareC(l, n) for l, n in y.share])
        self.table = G.dev(np.frombuffer(bytes(t), np.int32).copy())

    def call(self, shared, B_=None, ws=True, layer=LAYER, nq=None):
        q, y, hd = self.qlib, self.y, self.hd
        size = (q.qie_attention_decode_shared_workspace_bytes if shared else q.qie_attention_decode_workspace_bytes)
        w = G.zeros_bytes(size(y.B, self.nq, self.nkv, hd, y.maxc))
        if shared:   # the workspace need not be initialised: NaNs in every partial slot
            G.check(q.qie_memset(G.p(w), 0xFF, w.nbytes))
        out = G.dev(np.full((y.B, self.nq * hd), 0x4D4D, np.uint16))
        qkv, pos, qn, kn, cs, sn = (G.p(x) for x in self.args)
        tail = (qn, kn, cs, sn, nq or self.nq, C.byref(self.desc), layer, self.eps, self.num, G.p(out),
                G.p(w) if ws else None, None)
        B_ = y.B if B_ is None else B_
        rc = (q.qie_attention_decode_shared(qkv, B_, pos, G.p(self.table), *tail) if shared
              else q.qie_attention_decode(qkv, B_, pos, *tail))
        return rc, G.host_bf16(out)

    def cache(self):
        if self.paged:
            return self.pg.gather(self.pg.dk), self.pg.gather(self.pg.dv)
        shape = (self.y.B, L, self.nkv, self.y.maxc, self.hd)
        return G.host_bf16(self.kc).reshape(shape), G.host_bf16(self.vc).reshape(shape)


@pytest.mark.parametrize("y,hd,nq,nkv,paged", CASES, ids=IDS)
def test_shared_decode_against_float64_and_plain_decode(oracle, qlib, y, hd, nq, nkv, paged):
    B, POS, QD, KD = y.B, y.pos, nq * hd, nkv * hd
    r = rng(hd + nq)
    bf16 = lambda shape: oracle.f32_to_bf16(r.standard_normal(shape).astype(np.float32))
    Kh, Vh = (copy_prefix(y, cache_of(y, bf16((B, L, nkv, y.keys, hd)))) for _ in range(2))
    qkv = bf16((B, QD + 2 * KD))
    qn, kn = (oracle.f32_to_bf16((1 + 0.3 * r.standard_normal(hd)).astype(np.float32)) for _ in range(2))
    cs, sn = oracle.rope_table(y.maxc, hd, 1e6, "ref")
    q = oracle.rope(oracle.qknorm(qkv[:, :QD].copy(), qn, nq, hd, 1e-4, "ref"), cs, sn, POS, nq, hd, "ref")
    k = oracle.rope(oracle.qknorm(qkv[:, QD:QD + KD].copy(), kn, nkv, hd, 1e-4, "ref"), cs, sn, POS, nkv, hd, "ref")
    Kw, Vw = Kh[:, LAYER, :, :y.keys].copy(), Vh[:, LAYER, :, :y.keys].copy()
    for m in range(B):
        Kw[m, :, POS[m]], Vw[m, :, POS[m]] = k[m].reshape(nkv, hd), qkv[m, QD + KD:].reshape(nkv, hd)
    want, _ = ref64(y, q, Kw, Vw, nq, nkv, hd)
    bound = 2 ** -7 * np.maximum(1.0, np.abs(want).max(axis=1, keepdims=True)) * 2   # test_attention_decode_fused's

    mk = lambda K, V: Run(oracle, qlib, y, K, V, qkv, nq, nkv, hd, paged, qn=qn, kn=kn, cs=cs, sn=sn)
    plain, shared = mk(Kh, Vh), mk(Kh, Vh)
    rc, got_plain = plain.call(False)
    G.check(rc)
    rc, got = shared.call(True)
    G.check(rc)
    for name, o in (("qie_attention_decode", got_plain), ("shared", got)):
        d = np.abs(A.f64(o) - want)
        print(f"{name}: max |d| {d.max():.3e}, worst d / bound {(d / bound).max():.3f}")
        assert (d <= bound).all(), f"{name}: slot {np.argwhere(d > bound)[0][0]}"
    # the appended rows are qie_attention_decode's, bit for bit, and nothing else moved
    (pk, pv), (sk, sv) = plain.cache(), shared.cache()
    assert np.array_equal(sk, pk) and np.array_equal(sv, pv)
    for m in range(B):
        assert np.array_equal(sv[m, LAYER, :, POS[m]].reshape(-1), qkv[m, QD + KD:])
        Kh[m, LAYER, :, POS[m]], Vh[m, LAYER, :, POS[m]] = sk[m, LAYER, :, POS[m]], sv[m, LAYER, :, POS[m]]
    assert np.array_equal(sk, Kh) and np.array_equal(sv, Vh)
    if not paged:   # the poison run: bit-equal outputs
        rc, got_p = mk(poisoned(y, Kh), poisoned(y, Vh)).call(True)
        G.check(rc)
        assert np.array_equal(got_p, got)


@pytest.mark.parametrize("where", ["prefix", "suffix"])
@pytest.mark.parametrize("y,hd,nq,nkv,paged", CASES, ids=IDS)
def test_shared_decode_needles(oracle, qlib, y, hd, nq, nkv, paged, where):
    """The K row of one key is the bits of the query row (QIE_ATTN_PREROPED: no rotation in
    between), every other key N(0, 0.25**2), V rows distinct codes: the output is that key's V row,
    bit for bit.  prefix: the key lies below the slot's n_shared where it can — then in its LEADER's
    rows only: the member's own copy, contiguous or paged, is NaN; suffix: it is the new key at pos,
    which every slot appends itself."""
    B, POS, Gq, r = y.B, y.pos, nq // nkv, rng(7 * hd + nq)
    Kh, Vh = (cache_of(y, x) for x in A._base(hd, nkv, B, y.keys, "needle", 11))
    q = A.to_bf16((r.standard_normal((B, nq, hd)) * (4.0 if hd == 64 else 3.0)).astype(np.float32))
    k_new = A.to_bf16((r.standard_normal((B, nkv, hd)) * 0.25).astype(np.float32))
    v_new = A.vcode(B * L * nkv * y.keys + np.arange(B * nkv), hd).reshape(B, nkv, hd)   # codes past the cache's
    target = np.empty((B, nq), np.int64)
    for m, (l, n) in enumerate(y.share):
        mi = sum(1 for j in range(m) if y.share[j][0] == l)   # the slot's rank in its group
        for h in range(nq):
            if where == "suffix":
                q[m, h] = q[m, h - h % Gq]   # the heads of a kv group target one key: one query
                k_new[m, h // Gq], target[m, h] = q[m, h], POS[m]
            else:   # distinct keys per (member, head) of a group; past n_shared the key is in the slot's own rows
                target[m, h] = t = min(1 + y.stride * mi + 4 * (h % Gq), int(POS[m]) - 1)
                q[m, h] = q[m, min(j for j in range(h - h % Gq, h + 1) if target[m, j] == t)]   # one key, one query
                Kh[l if t < n else m, LAYER, h // Gq, t] = q[m, h]
    Kh, Vh = copy_prefix(y, Kh), copy_prefix(y, Vh)
    Kw, Vw = Kh[:, LAYER, :, :y.keys].copy(), Vh[:, LAYER, :, :y.keys].copy()
    for m in range(B):
        Kw[m, :, POS[m]], Vw[m, :, POS[m]] = k_new[m], v_new[m]
    _, slack = ref64(y, q.reshape(B, -1), Kw, Vw, nq, nkv, hd)
    assert (slack <= A.MARGIN).all(), "the inputs do not isolate one key"
    want = np.stack([np.concatenate([Vw[m, h // Gq, target[m, h]] for h in range(nq)]) for m in range(B)])
    qkv = np.concatenate([q.reshape(B, -1), k_new.reshape(B, -1), v_new.reshape(B, -1)], axis=1)
    cs, sn = oracle.rope_table(y.maxc, hd, 1e6, "ref")
    rc, got = Run(oracle, qlib, y, poisoned(y, Kh), poisoned(y, Vh), qkv, nq, nkv, hd, paged, num=_lib.QIE_ATTN_PREROPED,
                  cs=cs, sn=sn).call(True)
    G.check(rc)
    assert np.array_equal(got, want), f"first wrong (slot, head): {np.argwhere((got != want).reshape(B, nq, hd).any(-1))[0]}"


@pytest.mark.parametrize("case", ["B0", "B9", "no_ws", "layer", "group"])
def test_shared_decode_refusals(oracle, qlib, case):
    """-22 and nothing launched: the output keeps its fill."""
    y, nq, nkv, hd = SHORT, 8, 1, 64
    z = np.zeros((y.B, L, nkv, y.maxc, hd), np.uint16)
    cs, sn = oracle.rope_table(y.maxc, hd, 1e6, "ref")
    run = Run(oracle, qlib, y, z, z, np.zeros((y.B, (nq + 2 * nkv) * hd), np.uint16), nq, nkv, hd, False, cs=cs, sn=sn)
    kw = {"B0": dict(B_=0), "B9": dict(B_=9), "no_ws": dict(ws=False), "layer": dict(layer=L), "group": dict(nq=9)}[case]
    rc, out = run.call(True, **kw)
    assert rc == -22 and (out == 0x4D4D).all()
