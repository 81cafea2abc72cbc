"""GPU: sampling from the whole vocabulary, top_k = QIE_TOP_K_ALL (the contract at
qie_sample_rows in qie_ops.h), through qie_sample and qie_sample_rows on strided rows.  The CPU
oracle's sampler caps at 256 candidates: it is the reference where at most 256 carry weight and
the source of the uniform draw elsewhere; thresholds are checked against a float64 softmax."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as G
from test_gpu_engine import CONFIGS, SYN
from test_gpu_slot_sampling import _table

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd._lib import QIE_TOP_K_ALL, SampleRowsArgsC

pytestmark = pytest.mark.gpu

SS = Q.SlotSampling
BG = np.float32(-300.0)   # background logit: its weight against any support value here is exactly 0
VS, MS, ENTRIES = [1000, 4097, 151936], [1, 3], ["sample", "rows"]
BR8 = np.array([int(f"{i:08b}"[::-1], 2) for i in range(256)])


def draw(qlib, how, lg, V, entries, steps, hist=None, q=None):
    """ids of the rows lg [M][ld >= V] under entries (a list of SlotSampling; `sample`: all alike)."""
    M, ld = lg.shape
    ids, step, dl = G.dev(np.full((M,), -7, np.int32)), G.dev(np.asarray(steps, np.int32)), G.dev(lg)
    if how == "sample":
        e = entries[0]
        s = Q.Sampling(e.top_k, e.temperature, e.top_p, e.seed).to_c()
        ws = G.zeros_bytes(qlib.qie_sample_workspace_bytes(M, V))
        G.check(qlib.qie_sample(G.p(dl), M, V, ld, C.byref(s), G.p(step), G.p(ids), G.p(ws), None), "qie_sample")
    else:
        a = SampleRowsArgsC()
        hist = np.zeros((M, 8), np.int32) if hist is None else np.ascontiguousarray(hist, np.int32)
        a.logits, a.M, a.V, a.ld = G.p(dl), M, V, ld
        a.table, a.slot0, a.slot_stride = G.p(_table(entries)), 0, 1
        a.hist, a.hist_stride = G.p(G.dev(hist)), hist.shape[1]
        a.q_dev = G.p(G.dev(np.asarray([0] * M if q is None else q, np.int32)))
        a.step_dev, a.out_ids = G.p(step), G.p(ids)
        a.ws = G.p(G.zeros_bytes(qlib.qie_sample_rows_workspace_bytes(M, V)))
        G.check(qlib.qie_sample_rows(C.byref(a), None), "qie_sample_rows")
    G.check(qlib.qie_synchronize())
    return [int(t) for t in G.host(ids)]


def support(V, N, seed):
    """N ids: 0, V - 1, both sides of every 4,096 boundary, the rest scattered."""
    forced = sorted({0, V - 1} | {b - d for b in range(4096, V, 4096) for d in (0, 1)})
    rest = np.setdiff1d(np.arange(V), forced)
    return np.concatenate([forced, np.random.default_rng(seed).choice(rest, N - len(forced), replace=False)]).astype(np.int64)


def rows_of(oracle, V, M, N, values):
    """M strided rows (ld = V + 13: odd, so rows start unaligned) of background with N support ids."""
    lg = np.full((M, V + 13), BG, np.float32)
    sup = [support(V, N, 10 * V + m) for m in range(M)]
    for m in range(M):
        lg[m, np.random.default_rng(m).permutation(sup[m])] = values
    return oracle.f32_to_bf16(lg), sup


@pytest.mark.parametrize("how", ENTRIES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("V", VS)
def test_support_of_at_most_256_equals_the_oracle(oracle, qlib, V, M, how):
    N = 200   # distinct bf16 values in [-3.1, 3.1], several 256-key groups
    bits = np.concatenate([0x3F80 + 2 * np.arange(N // 2), 0xBF80 + 2 * np.arange(N // 2)]).astype(np.uint16)
    vals = oracle.bf16_to_f32(bits)
    lg, _ = rows_of(oracle, V, M, N, vals)
    for T in (0.7, 1.5):
        assert np.exp(np.float32((BG - vals.max()) / np.float32(T))) == 0
        for top_p in (1.0, 0.9):
            for step in range(8):
                steps = [step + m for m in range(M)]
                got = draw(qlib, how, lg, V, [SS(QIE_TOP_K_ALL, T, top_p, seed=4321)] * M, steps)
                want = [oracle.sample(lg[m, :V], 256, T, top_p, 4321 + steps[m]) for m in range(M)]
                assert got == want, (T, top_p, step)


@pytest.mark.parametrize("how", ENTRIES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("V", VS)
def test_equal_maxima_beyond_256_follow_the_uniform(oracle, qlib, V, M, how):
    """N > 256 equal candidates: every sum is an integer, so the drawn rank is the uniform's.
    (Before ALL mode existed, top_k = -1 was greedy: every rank was 0.)"""
    N = min(1024, V)
    lg, sup = rows_of(oracle, V, M, N, np.float32(1.0))
    assert np.exp(BG - np.float32(1.0)) == 0
    order = [sorted(s, key=lambda i: (-BR8[i & 255], i)) for s in sup]   # descending sel_key
    flat = oracle.f32_to_bf16(np.ones(256, np.float32))
    ranks = []
    for i in range(64 // M + 1):
        seed, steps = 1000 + i // 8, [M * i + m for m in range(M)]
        got = draw(qlib, how, lg, V, [SS(QIE_TOP_K_ALL, 1.0, 1.0, seed=seed)] * M, steps)
        for m in range(M):
            assert got[m] in sup[m]
            r = order[m].index(got[m])
            # the oracle's pick i of 256 equal logits says uniform in (i/256, (i+1)/256]; rank r says
            # (r/N, (r+1)/N]: the two must overlap (N a multiple of 256: r * 256 // N == i)
            i256 = 255 - int(BR8[oracle.sample(flat, 256, 1.0, 1.0, seed + steps[m])])
            assert r * 256 < (i256 + 1) * N and i256 * N < (r + 1) * 256, (i, m, r, i256)
            ranks.append(r)
    assert len(ranks) >= 64 and max(ranks) >= 256


@pytest.mark.parametrize("how", ENTRIES)
@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("V", VS)
def test_thresholds_leave_what_a_float64_softmax_leaves(oracle, qlib, V, M, how):
    edges = [e for e in (0, 4095, 4096, V - 1) if e < V]
    r = np.random.default_rng(V)
    for e in edges:
        lg = np.zeros((M, V + 13), np.float32)
        lg[:, :V] = r.standard_normal((M, V))
        lg[:, e] = 9.0
        lg = oracle.f32_to_bf16(lg)
        p = np.exp(oracle.bf16_to_f32(lg[:, :V]).astype(np.float64))
        p /= p.sum(axis=1, keepdims=True)
        assert (p.argmax(axis=1) == e).all() and p[:, e].min() > 2 * 0.01   # the top bin alone reaches top_p
        cuts = [SS(QIE_TOP_K_ALL, 1.0, 0.01)] + ([SS(QIE_TOP_K_ALL, 1.0, 1.0, min_p=1.0)] if how == "rows" else [])
        for entry in cuts:
            for step in range(4):
                assert draw(qlib, how, lg, V, [entry] * M, [step] * M) == [e] * M, (e, entry, step)
    # a tie AT the top-p cut: weights 1, 1/e, 1/e and top_p = 0.7 -> the tied bin stays whole
    a, b, c = (5, 4095, 4096) if V > 4096 else (5, 1, V - 1)
    lg = np.full((M, V + 13), BG, np.float32)
    lg[:, a], lg[:, b], lg[:, c] = 2.0, 1.0, 1.0
    seen = set()
    for step in range(32):
        seen |= set(draw(qlib, how, oracle.f32_to_bf16(lg), V, [SS(QIE_TOP_K_ALL, 1.0, 0.7, seed=7)] * M, [step] * M))
    assert seen == {a, b, c}


@pytest.mark.parametrize("V", VS)
def test_rows_mix_modes_and_all_rows_honour_penalties_and_bias(oracle, qlib, V):
    lg = np.zeros((3, V + 13), np.float32)
    lg[:, :V] = np.random.default_rng(V + 1).standard_normal((3, V)) * 3
    lg = oracle.f32_to_bf16(lg)
    others = [SS(40, 0.8, 0.9, seed=5), SS(1)]
    for step in range(4):
        mixed = draw(qlib, "rows", lg, V, [SS(QIE_TOP_K_ALL, 1.0, 0.95, seed=5)] + others, [step] * 3)
        plain = draw(qlib, "rows", lg, V, [others[0]] + others, [step] * 3)
        assert mixed[1:] == plain[1:] and 0 <= mixed[0] < V
    # two candidates A (5.0) and B (4.0) around a slice edge: A banned by a -inf bias; A pushed to
    # -45 by a presence penalty, where min_p = 0.5 leaves B alone (float64: w(A) = e^-49 < 0.5)
    A, B = (4096, 4095) if V > 4096 else (V - 1, 0)
    two = np.full((1, V + 13), BG, np.float32)
    two[0, A], two[0, B] = 5.0, 4.0
    two = oracle.f32_to_bf16(two)
    hist = np.full((1, 8), A, np.int32)
    assert np.exp(np.float64(-45.0 - 4.0)) < 0.5
    for entry in (SS(QIE_TOP_K_ALL, 1.0, 1.0, bias={A: float("-inf")}),
                  SS(QIE_TOP_K_ALL, 1.0, 1.0, min_p=0.5, presence_penalty=50.0)):
        got = {draw(qlib, "rows", two, V, [entry], [step], hist, [3])[0] for step in range(16)}
        assert got == {B}, entry
    assert A in {draw(qlib, "rows", two, V, [SS(QIE_TOP_K_ALL, 1.0, 1.0)], [s], hist, [3])[0] for s in range(16)}


ALL = Q.Sampling(top_k=QIE_TOP_K_ALL, temperature=1.0, top_p=0.95, seed=99)
TOPK = Q.Sampling(top_k=40, temperature=0.8, top_p=0.9, seed=99)


@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_engine_steps_equal_qie_sample_on_their_logits(oracle, qlib, paged, graph):
    spec = CONFIGS["qwen2-bias-hd64"]
    V = spec.vocab
    eng = Q.Engine(spec, max_ctx=128, use_graph=graph).init_synthetic(SYN)
    b = eng.batch(2, 128, page_tokens=128 if paged else None)

    def want(lg, smp, step):
        e = SS(smp.top_k, smp.temperature, smp.top_p, seed=smp.seed)
        return draw(qlib, "sample", np.ascontiguousarray(lg), V, [e] * 2, [step] * 2)

    try:
        for s in range(2):
            b.prefill(s, [3 + s, 17, 256, 999, 42], ALL)
        ids = []
        for step in range(1, 10):
            # steps 4-6: slot 0 under an ALL-mode entry beside the call's top-k (one re-capture
            # when it is set, one when it is cleared, replays in between)
            call = ALL if step <= 3 else TOPK
            if step in (4, 7):
                b.set_sampling(0, SS(ALL.top_k, ALL.temperature, ALL.top_p, seed=ALL.seed) if step == 4 else None)
            got = [int(t) for t in b.decode_step(call)]
            lg = b.logits()
            w = want(lg, call, step)
            if 4 <= step <= 6:
                w[0] = want(lg, ALL, step)[0]
            assert got == w, (step, got, w)
            ids += got
        assert all(0 <= t < V for t in ids)
        if graph:
            b.set_sampling(0, SS(ALL.top_k, ALL.temperature, ALL.top_p, seed=ALL.seed))
            n0 = b.verify_captures()
            outs = [b.verify(0, [1, 2], TOPK), b.verify(0, [1, 2], TOPK)]
            assert b.verify_captures() == n0 + 1 and all(0 <= t < V for o in outs for t in o)
    finally:
        b.close()
        eng.close()
