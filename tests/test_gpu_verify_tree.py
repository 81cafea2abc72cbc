"""GPU: tree verification: a chain is qie_verify bit for bit, the masked attention
against a float64 softmax over the visible keys, the compaction, the engine, the refusals."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as G
import slot_sampling_ref as R
from conftest import rng
from parity import max_flips
from test_gpu_engine import CONFIGS, SYN
from test_gpu_extend import BAR
from test_gpu_paged import Paged, _contig, rand_bf16
from test_gpu_verify import MODE1_SPEC, MX_SPEC, _follow_from

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib, weights as W

pytestmark = pytest.mark.gpu

SPEC = CONFIGS["qwen2-bias-hd64"]
STAR = [0] * 15
TWO_CHAINS = [0] + list(range(1, 7)) + [0] + list(range(8, 14))
BINARY = [(i - 1) // 2 for i in range(1, 16)]
TREES = {"star": STAR, "two_chains": TWO_CHAINS, "binary": BINARY}


def _path(parents, i):   # node i's root path, root first
    out = [i]
    while out[-1]:
        out.append(parents[out[-1] - 1])
    return out[::-1]


def _state(b):
    pos = b.positions().copy()
    return (pos, b.history(0, int(pos[0]) + 1).copy(), b.logits().copy())


@pytest.mark.parametrize("sampled", [False, True])
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("name", ["qwen2-bias-hd64", "qwen3-qknorm-hd128"])
def test_chain_equals_verify_bitwise(name, paged, sampled):
    spec = CONFIGS[name]
    smp = Q.Sampling(top_k=40, temperature=0.8, top_p=0.9, seed=5) if sampled else Q.GREEDY
    eng = Q.Engine(spec, max_ctx=320).init_synthetic(SYN)
    kw = dict(page_tokens=128) if paged else {}
    for p in (60, 120, 250):   # the rows straddle a 64-key tile, a 128-token page, a 256-key split
        prompt = [int(t) for t in rng(p).integers(0, spec.vocab, p)]
        a, b = eng.batch(1, 320, **kw), eng.batch(1, 320, **kw)
        c = a.prefill(0, prompt, smp)
        assert b.prefill(0, prompt, smp) == c
        cont = [int(t) for t in a.decode(15, smp)[:, 0]]
        cont[9] = (cont[9] + 1) % spec.vocab   # M = 16 stops inside the chain
        for M in (1, 2, 16):
            a.set_position(0, p, c)
            b.set_position(0, p, c)
            want, got = a.verify(0, cont[:M - 1], smp), b.verify_tree(0, cont[:M - 1], list(range(M - 1)), smp)
            assert got == want and np.array_equal(a.verify_logits(), b.verify_logits()), (p, M)
            for x, y in zip(_state(a), _state(b)):
                assert np.array_equal(x, y), (p, M)
            assert a.decode_step(smp)[0] == b.decode_step(smp)[0] and np.array_equal(a.logits(), b.logits()), (p, M)


def _attend_tree(qlib, c, q, p, parents, nq, hd, maxc):
    M = q.shape[0]
    anc = np.array([sum(1 << j for j in _path(parents, i)) for i in range(M)], np.int32)
    ws = G.zeros_bytes(qlib.qie_attention_extend_workspace_bytes(M, nq, hd, maxc))
    out = G.zeros_bf16(M, nq * hd)
    G.check(qlib.qie_attention_extend_tree(G.p(G.dev(q)), M, G.p(G.dev(np.arange(p, p + M, dtype=np.int32))),
                                           G.p(G.dev(anc)), 0, C.byref(c), 0, nq, G.p(out), G.p(ws), None))
    return G.host_bf16(out)


def _cache(oracle, kc, vc, paged):
    if paged:
        pg = Paged(oracle, kc, vc, 128, seed=3)
        return pg.cache(), pg
    dk, dv = G.dev(kc), G.dev(vc)
    return _contig(dk, dv, kc.shape[1], kc.shape[2], kc.shape[4], kc.shape[3]), (dk, dv)


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("hd,nq,nkv", [(64, 14, 2), (128, 16, 2)])
@pytest.mark.parametrize("shape", list(TREES))
def test_masked_attention_sees_exactly_the_ancestors(oracle, qlib, shape, hd, nq, nkv, paged):
    """Per leaf: every new row off the leaf's root path holds NaN in V and 3e4 in K; every row on the
    path equals the float64 softmax over the prefix and its ancestors.  The rows straddle key 256."""
    parents, p, maxc, g, M = TREES[shape], 250, 320, nq // nkv, len(TREES[shape]) + 1
    k0, v0 = rand_bf16(oracle, (1, 1, nkv, maxc, hd), seed=hd), rand_bf16(oracle, (1, 1, nkv, maxc, hd), seed=hd + 1)
    q = rand_bf16(oracle, (M, nq * hd), seed=7)
    qf, kf, vf = (G.bf(x).astype(np.float64) for x in (q, k0, v0))
    worst = 0.0
    for leaf in (i for i in range(M) if i not in parents):
        path = _path(parents, leaf)
        kc, vc = k0.copy(), v0.copy()
        off = [p + j for j in range(M) if j not in path]
        kc[0, 0, :, off] = oracle.f32_to_bf16(np.full(1, 3e4, np.float32))[0]
        vc[0, 0, :, off] = 0x7FC0
        c, keep = _cache(oracle, kc, vc, paged)
        got = G.bf(_attend_tree(qlib, c, q, p, parents, nq, hd, maxc))
        for i in path:
            keys = list(range(p)) + [p + j for j in _path(parents, i)]
            for h in range(nq):
                s = kf[0, 0, h // g, keys] @ qf[i, h * hd:(h + 1) * hd] / np.sqrt(hd)
                w = np.exp(s - s.max())
                want = (w / w.sum()) @ vf[0, 0, h // g, keys]
                row = got[i, h * hd:(h + 1) * hd]
                assert np.isfinite(row).all(), (shape, leaf, i, h)
                worst = max(worst, float(np.abs(row - want).max()))
    assert worst <= BAR, worst


@pytest.mark.parametrize("shape", list(TREES))
def test_masked_attention_needle(oracle, qlib, shape):
    """The last row's q is 64 x one ancestor's K row: every other probability underflows to 0, so the
    output is that ancestor's V row bit for bit, although hidden siblings hold K = 3e4 and NaN V."""
    parents, p, maxc, hd, nq, nkv, M = TREES[shape], 250, 320, 64, 4, 2, len(TREES[shape]) + 1
    kc, vc = rand_bf16(oracle, (1, 1, nkv, maxc, hd), seed=1), rand_bf16(oracle, (1, 1, nkv, maxc, hd), seed=2)
    t, path = M - 1, _path(parents, M - 1)
    off = [p + j for j in range(M) if j not in path]
    kc[0, 0, :, off] = oracle.f32_to_bf16(np.full(1, 3e4, np.float32))[0]
    vc[0, 0, :, off] = 0x7FC0
    needle = path[len(path) // 2]
    q = rand_bf16(oracle, (M, nq * hd), seed=3)
    for h in range(nq):
        q[t, h * hd:(h + 1) * hd] = oracle.f32_to_bf16((64 * G.bf(kc[0, 0, h // 2, p + needle])).astype(np.float32))
    c, keep = _cache(oracle, kc, vc, False)
    got = _attend_tree(qlib, c, q, p, parents, nq, hd, maxc)
    for h in range(nq):
        assert np.array_equal(got[t, h * hd:(h + 1) * hd], vc[0, 0, h // 2, p + needle]), (shape, h)


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("p,path", [(60, (1, 2, 3)), (60, (2, 5, 9, 15)), (200, (15,)), (126, (3, 5, 9))])
def test_kv_compact_moves_the_path(oracle, qlib, p, path, hd, paged):
    L, nkv, maxc = 2, 3, 256
    kc = (np.arange(L * nkv * maxc * hd, dtype=np.uint32) * 7 % 65521).astype(np.uint16).reshape(1, L, nkv, maxc, hd)
    vc = (kc + 1).astype(np.uint16)
    want_k, want_v = kc.copy(), vc.copy()
    for d, node in enumerate(path, 1):
        want_k[0, :, :, p + d], want_v[0, :, :, p + d] = kc[0, :, :, p + node], vc[0, :, :, p + node]
    c, keep = _cache(oracle, kc, vc, paged)
    words = G.dev(np.array([p, len(path), 0] + list(path), np.int32))
    G.check(qlib.qie_kv_compact(C.byref(c), 0, G.p(words), G.p(words) + 4, G.p(words) + 8, None))
    got_k, got_v = (keep.gather(keep.dk), keep.gather(keep.dv)) if paged else (G.host_bf16(x) for x in keep)
    got_k, got_v, a = got_k.reshape(kc.shape), got_v.reshape(vc.shape), len(path)
    assert np.array_equal(got_k[..., :p + a + 1, :], want_k[..., :p + a + 1, :])   # rows below p untouched
    assert np.array_equal(got_v[..., :p + a + 1, :], want_v[..., :p + a + 1, :])
    assert np.array_equal(got_k[..., p + a + 1:, :], kc[..., p + a + 1:, :])       # sources past the path kept


@pytest.mark.parametrize("entry", [False, True])
@pytest.mark.parametrize("paged", [False, True])
def test_engine_accepts_the_second_branch(oracle, paged, entry):
    """Nodes 1-3 are a wrong branch, nodes 4-6 the twin's own continuation; the decode steps after it
    meet test_gpu_verify's bar.  entry: a repetition penalty, checked on each row's root-path window."""
    eng = Q.Engine(SPEC, max_ctx=256).init_synthetic(SYN)
    kw = dict(page_tokens=128) if paged else {}
    P = 126 if paged else 30
    prompt = [int(t) for t in rng(77).integers(0, SPEC.vocab, P)]
    e = Q.SlotSampling(top_k=1, repetition_penalty=1.3, penalty_last_n=20) if entry else None
    twin, b = eng.batch(1, 256, **kw), eng.batch(1, 256, **kw)
    for x in (twin, b):
        x.set_sampling(0, e)
    c = twin.prefill(0, prompt)
    g = [int(twin.decode_step()[0]) for _ in range(4)]   # the twin's four tokens after c
    assert b.prefill(0, prompt) == c
    ids = [(t + 1) % SPEC.vocab for t in g[:3]] + g[:3]
    parents = [0, 1, 2, 0, 4, 5]
    out = b.verify_tree(0, ids, parents)
    vl = b.verify_logits()
    if entry:   # the accepted rows' choices under the contract, each on its own root-path window
        hist = b.history(0, 256)
        for d, i in enumerate((0, 4, 5, 6)):
            tail = [ids[j - 1] for j in _path(parents, i)[1:]]
            assert out[d] == R.choose(oracle, vl[i], e, R.window_ids(e, hist, P + d, tail), 0)[0], i
    assert out == g, (out, g)
    assert int(b.positions()[0]) == int(twin.positions()[0]) == P + 4
    assert np.array_equal(b.history(0, P + 5), twin.history(0, P + 5))
    assert np.array_equal(b.logits()[0], vl[6])
    if not entry:
        om = oracle.Model(W.HostWeights.synthetic(SPEC, SYN), 256)
        om.forward(prompt + [c] + g[:3], 0)
        assert _follow_from(oracle, om, b, P + 4, g[3], 4, "after the tree") <= max_flips(4)
    else:
        assert [int(b.decode_step()[0]) for _ in range(3)] == [int(twin.decode_step()[0]) for _ in range(3)]


@pytest.mark.parametrize("case", ["kv_fp8", "prefill_fp8", "decode_mode_1", "pool"])
def test_refusals_leave_the_batch_alone(case):
    spec, kw, bkw, rc, P = SPEC, {}, {}, "rc=-22", 10
    if case == "kv_fp8":
        kw = dict(kv_fp8=True)
    elif case == "prefill_fp8":
        spec, kw = MX_SPEC, dict(weight_fp8=True, prefill_fp8=True)
    elif case == "decode_mode_1":
        spec = MODE1_SPEC
    else:
        bkw, rc, P = dict(page_tokens=128, n_pages=2), "rc=-28", 120   # rows 120 .. 135 need a second page
    ctx = 256 if case == "pool" else 64
    eng = Q.Engine(spec, max_ctx=ctx, **kw).init_synthetic(SYN)
    prompt = [int(t) for t in rng(9).integers(0, spec.vocab, P)]

    def start():
        x = eng.batch(1, ctx, **bkw)
        x.prefill(0, prompt)
        if case == "decode_mode_1":
            x.set_decode_mode(1)
        return x

    twin, b = start(), start()
    before = _state(b)
    with pytest.raises(_lib.QieError, match=rc):
        b.verify_tree(0, [1] * 15, STAR)
    for x, y in zip(before, _state(b)):
        assert np.array_equal(x, y)
    for _ in range(4):
        assert b.decode_step()[0] == twin.decode_step()[0] and np.array_equal(b.logits(), twin.logits())
