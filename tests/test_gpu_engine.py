"""GPU end-to-end parity: the libqie engine (prefill + hipGraph decode) against the CPU
oracle's full forward on identical synthetic weights and prompts.

Bar (written per check):
* logits: every step's bf16 logits within 4 bf16 ulps of the largest |logit| of the
  oracle's (fp32 summation order differs inside every dot product, 2-80 layers deep),
  and norm-relative within tests/parity.py's bar: max(1e-3, 2 x the oracle's own
  order-0 vs order-2 spread on the same step) — 1e-3 alone is below the reference
  algorithm's own order sensitivity (3e-3 .. 9e-3 on these models);
* greedy ids: TEACHER-FORCED — at every step the engine's arg-max must equal the
  oracle's unless the oracle's own logits put the two tokens within that same tolerance
  (a near-tie, where any fp32 reordering may flip a bf16 arg-max); the oracle's token is
  then forced into the engine (qie_batch_set_position) so later steps stay comparable.
  Near-tie flips are counted and bounded;
* engine invariants (graph == eager, batch == single, weights.bin == synthetic init,
  device-tensor weights, rewind) are bit-exact.
"""
import numpy as np
import pytest

import gpu_util as G
from conftest import rng
from parity import OrderPair, check_step, max_flips, oracle_trace

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import spec as S, weights as W

pytestmark = pytest.mark.gpu

CONFIGS = {
    "qwen2-bias-hd64": S.tiny("t-q2", n_layers=3, hidden=256, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512,
                              vocab=1000, bias=True),
    "qwen3-qknorm-hd128": S.tiny("t-q3", n_layers=2, hidden=512, n_heads=8, n_kv_heads=2, head_dim=128, ffn=768,
                                 vocab=1536, bias=False, qk_norm=True),
    "tied-g7": S.tiny("t-tied", n_layers=2, hidden=448, n_heads=7, n_kv_heads=1, head_dim=64, ffn=640,
                      vocab=777 * 2, tie=True, bias=True),
}
SYN = W.SynthParams(seed=11, w_scale=0.08, norm_scale=0.25, bias_scale=0.05)
LOGIT_ULPS = 4


def make_pair(spec, oracle, max_ctx=128, use_graph=True, syn=SYN):
    eng = Q.Engine(spec, max_ctx=max_ctx, use_graph=use_graph).init_synthetic(syn)
    hw = W.HostWeights.synthetic(spec, syn)
    return eng, hw, oracle.Model(hw, max_ctx)


def logit_tol(want):
    return LOGIT_ULPS * 2.0 ** -7 * max(1.0, float(np.abs(G.bf(want)).max()))


def logits_close(got, want, what=""):
    g, w = G.bf(got).astype(np.float64), G.bf(want).astype(np.float64)
    assert np.abs(g - w).max() <= logit_tol(want), f"{what}: max |dlogit| {np.abs(g - w).max()} > {logit_tol(want)}"


def forced_compare(oracle, b, pair, prompt, n_new, seq=0):
    """Teacher-forced greedy comparison under tests/parity.py's bar (`pair` a
    parity.OrderPair): the oracle trace first, then the engine forced onto its ids.
    Returns (oracle ids, near-tie flips)."""
    ids, outs = oracle_trace(oracle, pair, prompt, n_new)
    pair.calibrate(b.e.spec.vocab)
    t_e = b.prefill(seq, prompt)
    flips = 0
    for i in range(n_new):
        lg0 = outs[i][0]
        lg_e = b.logits()[seq]
        logits_close(lg_e, lg0, f"step {i}")
        flips += check_step(lg_e, lg0, pair, t_e, ids[i], f"step {i}")
        if t_e != ids[i]:
            b.set_position(seq, len(prompt) + i, ids[i])
        if i + 1 < n_new:
            t_e = b.decode_step()[seq]
    return ids, flips


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("num", ["ref", "hf"])
@pytest.mark.parametrize("P", [5, 23])
def test_greedy_generation_matches_oracle(oracle, name, num, P):
    spec = CONFIGS[name].with_numerics(num)
    eng, hw, om = make_pair(spec, oracle)
    prompt = list(rng(P).integers(0, spec.vocab, P))
    n_new = 16
    ids, flips = forced_compare(oracle, eng.batch(1, 128), OrderPair(oracle, hw, 128), prompt, n_new)
    assert flips <= max_flips(n_new), f"{flips} near-tie flips in {n_new} steps"


def _teacher_forced_trace(b, prompts, n_new, forced=None):
    """Per-sequence (engine choices, per-step logits) of a batch, every sequence forced to
    `forced[i][step]` after each step when given (qie_batch_set_position)."""
    B = len(prompts)
    raw = [[b.prefill(i, pr)] for i, pr in enumerate(prompts)]
    lgs = [[] for _ in range(B)]
    for t in range(n_new):
        lg = b.logits()
        for i in range(B):
            lgs[i].append(lg[i])
            if forced is not None and raw[i][-1] != forced[i][t]:
                b.set_position(i, len(prompts[i]) + t, int(forced[i][t]))
        if t + 1 < n_new:
            nxt = b.decode_step()
            for i in range(B):
                raw[i].append(nxt[i])
    return raw, lgs


def test_graph_equals_eager_and_batch_equals_single(oracle):
    """graph == eager bit-exactly (same kernels); batch (B = 3: the skinny MFMA kernel)
    vs one sequence at a time (B = 1: the GEMV kernel) differ only in fp32 summation
    order: logits within the 4-ulp bar, ids equal except at near-ties (teacher-forced)."""
    spec = CONFIGS["qwen2-bias-hd64"]
    prompts = [list(rng(i).integers(0, spec.vocab, n)) for i, n in enumerate([7, 19, 3])]
    outs = {}
    for graph in (True, False):
        eng = Q.Engine(spec, max_ctx=96, use_graph=graph).init_synthetic(SYN)
        singles = [_teacher_forced_trace(eng.batch(1, 96), [pr], 11) for pr in prompts]
        s_ids = [r[0][0] for r in singles]
        s_lgs = [r[1][0] for r in singles]
        raw, lgs = _teacher_forced_trace(eng.batch(3, 96), prompts, 11, forced=s_ids)
        flips = 0
        for i in range(3):
            for t in range(11):
                logits_close(lgs[i][t], s_lgs[i][t], f"seq {i} step {t}")
                if raw[i][t] != s_ids[i][t]:
                    gap = abs(float(G.bf(s_lgs[i][t][s_ids[i][t]])) - float(G.bf(s_lgs[i][t][raw[i][t]])))
                    assert gap <= logit_tol(s_lgs[i][t]), f"seq {i} step {t}: gap {gap}"
                    flips += 1
        assert flips <= 3
        outs[graph] = (raw, np.stack([np.stack(x) for x in lgs]))
    assert outs[True][0] == outs[False][0]
    assert np.array_equal(outs[True][1], outs[False][1])


def test_time_kernel_leaves_the_step_alone_and_counts_its_bytes():
    """qie_batch_time_kernel (bench.py --full's per-kernel timing) between decode steps: its
    launches write scratch only, so the steps around it give the ids and logits of the same run
    without it, bit for bit; and every `bytes` it returns is the traffic of that projection at
    these shapes (bf16: weights once, the B input rows, the norm weight where the launch norms,
    the B output rows; attention: K and V of each slot's context, q in and out)."""
    spec = CONFIGS["qwen2-bias-hd64"]
    B, P = 2, (7, 11)
    prompts = [list(rng(i).integers(0, spec.vocab, n)) for i, n in enumerate(P)]
    H, I, V = spec.hidden, spec.ffn, spec.vocab
    QD, KD = spec.n_heads * spec.head_dim, spec.n_kv_heads * spec.head_dim
    want_bytes = [
        2.0 * I * H * 2 + B * H * 2 + H * 2 + B * I * 2,                    # 0 gate/up
        float(H * I * 2 + B * I * 2 + B * H * 2),                            # 1 down
        float((QD + 2 * KD) * H * 2 + B * H * 2 + B * (QD + 2 * KD) * 2),    # 2 QKV
        float(H * QD * 2 + B * QD * 2 + B * H * 2),                          # 3 O
        float(V * H * 2 + B * H * 2 + B * V * 2),                            # 4 lm_head
        float(sum((p + 2 + 1) * KD * 2 * 2 for p in P) + B * QD * 2 * 2),    # 5 attention, 2 steps after the prompts
    ]
    runs = []
    for timed in (False, True):
        eng = Q.Engine(spec, max_ctx=64).init_synthetic(SYN)
        b = eng.batch(B, 64)
        for i, pr in enumerate(prompts):
            b.prefill(i, pr)
        ids = [b.decode_step() for _ in range(2)]
        if timed:
            got_bytes = [b.time_kernel(which, 2)[1] for which in range(6)]
        ids += [b.decode_step() for _ in range(2)]
        runs.append((ids, b.logits()))
        b.close()
        eng.close()
    assert runs[0][0] == runs[1][0]
    assert np.array_equal(runs[0][1], runs[1][1])
    assert got_bytes == want_bytes


def test_weights_bin_loader_equals_synthetic(oracle, tmp_path):
    spec = CONFIGS["qwen3-qknorm-hd128"]
    hw = W.HostWeights.synthetic(spec, SYN)
    hw.write_weights_bin(str(tmp_path / "weights.bin"), str(tmp_path / "meta_data.txt"))
    prompt = [1, 2, 3, 4, 5, 6, 7, 8, 9]
    e1 = Q.Engine(spec, max_ctx=64).init_synthetic(SYN)
    e2 = Q.Engine(spec, max_ctx=64).load_weights_bin(str(tmp_path / "weights.bin"), str(tmp_path / "meta_data.txt"),
                                                     chunk_bytes=1 << 16)
    r, lg = [], []
    for e in (e1, e2):
        b = e.batch(1, 64)
        r.append([b.prefill(0, prompt)] + list(b.decode(8)[:, 0]))
        lg.append(b.logits())
    assert r[0] == r[1]
    assert np.array_equal(lg[0], lg[1])


def test_set_weights_from_device_tensors(oracle):
    spec = CONFIGS["tied-g7"]
    hw = W.HostWeights.synthetic(spec, SYN)
    dev = {n: G.dev(a) for n, a in hw.tensors.items()}
    e1 = Q.Engine(spec, max_ctx=64).set_weights({n: t.data_ptr() for n, t in dev.items()}, keepalive=dev)
    e2 = Q.Engine(spec, max_ctx=64).init_synthetic(SYN)
    r = []
    for e in (e1, e2):
        b = e.batch(1, 64)
        r.append(([b.prefill(0, [5, 4, 3, 2, 1])] + list(b.decode(7)[:, 0]), b.logits()))
    assert r[0][0] == r[1][0] and np.array_equal(r[0][1], r[1][1])


def test_rewind_reproduces(oracle):
    spec = CONFIGS["qwen2-bias-hd64"]
    e = Q.Engine(spec, max_ctx=64).init_synthetic(SYN)
    b = e.batch(1, 64)
    prompt = [9, 8, 7, 6, 5, 4]
    t0 = b.prefill(0, prompt)
    a = list(b.decode(10)[:, 0])
    b.set_position(0, len(prompt), t0)
    assert list(b.decode(10)[:, 0]) == a
    hist = b.history(0, len(prompt) + 11)
    assert list(hist[:len(prompt)]) == prompt and hist[len(prompt)] == t0 and list(hist[len(prompt) + 1:]) == a


def test_topk_sampling_schedule_on_engine_logits(oracle):
    """Reference sampling schedule — prefill k=50, T=1.0, seed 1234; decode step s k=50,
    T=0.7, seed 1234+s (qwen_main.cu:241, 381-388) — applied by the oracle's restated
    sampler to the ENGINE's own logits must give the engine's token at every step."""
    spec = CONFIGS["qwen2-bias-hd64"]
    eng = Q.Engine(spec, max_ctx=128).init_synthetic(SYN)
    b = eng.batch(1, 128)
    prompt = [11, 22, 33, 44, 55, 66, 77]
    tok = b.prefill(0, prompt, Q.Sampling(top_k=50, temperature=1.0, seed=1234))
    assert tok == oracle.sample(b.logits()[0], 50, 1.0, 1.0, 1234)
    for s in range(1, 12):
        tok = b.decode_step(Q.Sampling(top_k=50, temperature=0.7, seed=1234))[0]
        assert tok == oracle.sample(b.logits()[0], 50, 0.7, 1.0, 1234 + s), s


@pytest.mark.slow
def test_qwen2_0_5b_config1_greedy_matches_oracle(oracle):
    """BASELINE config 1 shape (Qwen2-0.5B, prompt 16, gen 16, greedy) at full size."""
    spec = S.QWEN2_0_5B
    eng, hw, om = make_pair(spec, oracle, max_ctx=64, syn=W.SynthParams(seed=0))
    prompt = list(rng(1).integers(0, spec.vocab, 16))
    ids, flips = forced_compare(oracle, eng.batch(1, 64), OrderPair(oracle, hw, 64), prompt, 16)
    assert flips <= 2


def test_qwen2_0_5b_config2_p128_g128_forced_decisions(oracle):
    """BASELINE config 2 end to end: the full Qwen2-0.5B (24 layers, tied head) with a
    128-token prompt (M = 128 prefill dispatch) and 127 hipGraph decode steps at ctx
    129..255 (the one-split decode attention), 128 greedy decisions on a forced
    continuation against or_forward in summation orders 0 / 1 / 2 (tests/parity.py
    forced_decisions; peaked head = boosted rows of the tied embedding)."""
    from parity import PEAKED, forced_decisions
    spec = S.QWEN2_0_5B
    syn = W.SynthParams(seed=0, **PEAKED)
    eng = Q.Engine(spec, max_ctx=272).init_synthetic(syn)
    b = eng.batch(1, 272)
    prompt = [int(t) for t in rng(128).integers(0, spec.vocab, 128)]
    rep = forced_decisions(oracle, W.HostWeights.synthetic(spec, syn), b, prompt, 128, progress=True)
    print("config 2 forced decisions:", rep)
    assert rep["ok"], rep


@pytest.mark.slow
def test_qwen2_7b_widths_two_layers_match_oracle(oracle):
    """Full Qwen2-7B widths (H 3584, I 18944, 28/4 heads, V 152064), 2 layers: any
    7B-shape-specific kernel bug shows here at the tight tolerance, independent of the
    drift that 28 layers of fp32 reordering accumulate in the full model."""
    spec = S.QWEN2_7B.replace(n_layers=2)
    eng, hw, om = make_pair(spec, oracle, max_ctx=64, syn=W.SynthParams(seed=0))
    prompt = list(rng(2).integers(0, spec.vocab, 24))
    ids, flips = forced_compare(oracle, eng.batch(1, 64), OrderPair(oracle, hw, 64), prompt, 6)
    assert flips <= 2


@pytest.mark.slow
@pytest.mark.parametrize("name", ["Qwen3-14B", "Qwen2-72B"])
def test_wide_hidden_two_layers_match_oracle(oracle, name):
    """Hidden sizes above 4,096 (Qwen3-14B, the reference's own model: H 5120, 40 / 8 heads =
    GQA group 5, qk-norm, no bias; Qwen2-72B: H 8192, 64 / 8 heads), 2 layers: the batch-1
    GEMVs fuse the RMSNorm at these widths through a different prologue variant than at
    7B widths (before round 2's fix the x-first variant for K > 4,096 dropped the norm)."""
    spec = S.PRESETS[name].replace(n_layers=2)
    eng, hw, om = make_pair(spec, oracle, max_ctx=48, syn=W.SynthParams(seed=0))
    prompt = list(rng(14).integers(0, spec.vocab, 12))
    ids, flips = forced_compare(oracle, eng.batch(1, 48), OrderPair(oracle, hw, 48), prompt, 6)
    assert flips <= 2


@pytest.mark.parametrize("paged", [False, True])
def test_short_prefill_after_long_prefill(oracle, paged):
    """Prompts of <= 8 tokens run the split prefill attention, which needs a workspace
    that longer prompts do not; a short prefill after a long one in the same batch must
    size it (it once wrote its split partials past a 16-byte buffer).  Ids and logits equal
    the same short prompt in a fresh batch, bit for bit."""
    spec = CONFIGS["qwen2-bias-hd64"]
    eng = Q.Engine(spec, max_ctx=256).init_synthetic(SYN)
    pt = 128 if paged else None
    b = eng.batch(2, 256, page_tokens=pt)
    b.prefill(0, list(rng(1).integers(0, spec.vocab, 40)))
    short = list(rng(2).integers(0, spec.vocab, 3))
    got = [b.prefill(1, short)] + [int(t) for t in b.decode(6)[:, 1]]
    lg = b.logits()[1]
    f = eng.batch(2, 256, page_tokens=pt)
    want = [f.prefill(1, short)] + [int(t) for t in f.decode(6)[:, 1]]
    assert got == want
    assert np.array_equal(lg, f.logits()[1])


def test_prefill_scratch_regrowth_is_invisible():
    """The prefill rows are one block that grows (freed, then made anew): on one batch, prefills of
    5, 40 and 5 tokens into the same slot (made, regrown, reused) give the id and the logits of
    three fresh batches doing one prefill each, bit for bit."""
    spec = CONFIGS["qwen2-bias-hd64"]
    eng = Q.Engine(spec, max_ctx=128).init_synthetic(SYN)
    b = eng.batch(1, 128)
    for i, P in enumerate((5, 40, 5)):
        prompt = [int(t) for t in rng(60 + i).integers(0, spec.vocab, P)]
        got, lg = b.prefill(0, prompt), b.logits()
        f = eng.batch(1, 128)
        assert got == f.prefill(0, prompt), f"prefill {i} (P = {P})"
        assert np.array_equal(lg, f.logits()), f"prefill {i} (P = {P})"
        f.close()


def test_captured_work_survives_prefill_regrowth():
    """Captured work may point only into blocks that are never reallocated.  B = 2 with graphs:
    prefill slot 0 (P = 5), 2 decode steps (captures the decode graph), a verify with 3 drafts
    (captures that step); then a P = 40 prefill of slot 1 frees and reallocates the prefill rows;
    2 more decode steps and the verify again replay the captured work.  Ids and logits of every
    step equal the same sequence on an eager engine, bit for bit."""
    spec = CONFIGS["qwen2-bias-hd64"]
    p0 = [int(t) for t in rng(70).integers(0, spec.vocab, 5)]
    p1 = [int(t) for t in rng(71).integers(0, spec.vocab, 40)]
    draft = [int(t) for t in rng(72).integers(0, spec.vocab, 3)]

    def run(use_graph):
        eng = Q.Engine(spec, max_ctx=128, use_graph=use_graph).init_synthetic(SYN)
        b = eng.batch(2, 128)
        out = [("prefill0", [b.prefill(0, p0)], b.logits()[:1])]
        for phase in (0, 1):
            if phase == 1:
                out.append(("prefill1", [b.prefill(1, p1)], b.logits()))
            rows = slice(0, 1 + phase)   # slot 1 is idle (its logits unwritten) before its prefill
            for i in range(2):
                out.append((f"decode{phase}.{i}", b.decode_step()[rows], b.logits()[rows]))
            out.append((f"verify{phase}", b.verify(0, draft), b.verify_logits()))
            out.append((f"after_verify{phase}", [], b.logits()[rows]))
        return out

    for (what, ids_g, lg_g), (_, ids_e, lg_e) in zip(run(True), run(False)):
        assert list(ids_g) == list(ids_e), what
        assert np.array_equal(lg_g, lg_e), what


@pytest.mark.parametrize("L", [5, 40])
@pytest.mark.parametrize("paged", [False, True])
def test_prefill_batch_matches_oracle(oracle, L, paged):
    """qie_prefill_batch: 3 equal-length prompts into slots 1..3 of a 4-slot batch in one
    pass (one GEMM over 3L rows; L = 5 runs the split attention, L = 40 the causal MFMA
    kernel, both with rows_per_seq = L).  Every slot is teacher-forced against its own
    oracle trace under tests/parity.py's bar through 6 decode steps; slot 0 stays idle.
    Positions and token history are exact."""
    spec = CONFIGS["qwen3-qknorm-hd128"]
    eng, hw, _ = make_pair(spec, oracle, max_ctx=96)
    prompts = [[int(t) for t in rng(40 + z).integers(0, spec.vocab, L)] for z in range(3)]
    n_new = 6
    traces, pairs = [], []
    for pr in prompts:
        pair = OrderPair(oracle, hw, 96)
        traces.append(oracle_trace(oracle, pair, pr, n_new))
        pairs.append(pair.calibrate(spec.vocab))
    b = eng.batch(4, 96, page_tokens=128 if paged else None)
    t_e = b.prefill_batch(1, prompts)
    assert list(b.positions()[1:]) == [L] * 3
    for z in range(3):
        assert list(b.history(1 + z, L + 1)) == prompts[z] + [t_e[z]]
    flips = 0
    for i in range(n_new):
        lg = b.logits()
        for z in range(3):
            ids, outs = traces[z]
            logits_close(lg[1 + z], outs[i][0], f"seq {z} step {i}")
            flips += check_step(lg[1 + z], outs[i][0], pairs[z], t_e[z], ids[i], f"seq {z} step {i}")
            if t_e[z] != ids[i]:
                b.set_position(1 + z, L + i, ids[i])
        if i + 1 < n_new:
            t_e = b.decode_step()[1:]
    assert flips <= max_flips(3 * n_new)
