"""GPU: batches of 9 .. 64 slots.  B <= 16 decodes through the M <= 16 planner as
before; B > 16 runs its four layer projections on the 17..64-row kernel (QIE_LINEAR_ROWS64) and its
head in pieces of 16 rows.

Every slot of a batch is held to the same prompt run alone in a B = 1 batch of the same engine:
logits within parity.py's bar (max(1e-3, 2 x the oracle's own order spread), calibrated on the
model), tokens equal but for near-ties under its flip rule (a slot is followed up to its first
flip; the runs are free-running).  The spec has K = 896 everywhere, so the fp8 engine tiles its
projections (QIE_LINEAR_FP8_T16) and the kernel reads the tiled layout.
"""
import numpy as np
import pytest

import gpu_util as G
import parity
from conftest import rng
from test_gpu_slot_sampling import run_rows

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib, spec as S, weights as W

pytestmark = pytest.mark.gpu

SPEC = S.tiny("t-b64", n_layers=2, hidden=896, n_heads=14, n_kv_heads=2, head_dim=64, ffn=896, vocab=1000)
SYN = W.SynthParams(seed=11, w_scale=0.08, norm_scale=0.25, bias_scale=0.05)
CTX, STEPS = 128, 6
PROMPTS = [[int(t) for t in rng(100 + i).integers(0, SPEC.vocab, 5 + i % 8)] for i in range(84)]


def _run(b, prompts, steps=STEPS, step=None):
    """Prefill prompts[i] into slot i, then `steps` greedy steps: (tokens [1 + steps][B], logits alike)."""
    toks = [[b.prefill(i, p) for i, p in enumerate(prompts)]]
    lgs = [b.logits().copy()]
    for _ in range(steps):
        toks.append((step or b.decode_step)())
        lgs.append(b.logits().copy())
    return np.array(toks), np.array(lgs)


@pytest.fixture(scope="module", params=[False, True], ids=["bf16", "fp8"])
def model(request, oracle):
    """The engine, the parity bar of its model, and every prompt's run alone in a B = 1 batch."""
    fp8 = request.param
    eng = Q.Engine(SPEC, max_ctx=CTX, weight_fp8=fp8).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(SPEC, SYN)
    pair = parity.OrderPair(oracle, hw.fp8_dequantized() if fp8 else hw, CTX).calibrate(SPEC.vocab, n_prompt=12, n_steps=4)
    b1 = eng.batch(1, CTX)
    alone = [_run(b1, [p]) for p in PROMPTS[:64]]
    b1.close()
    yield eng, pair, alone, fp8
    eng.close()


@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("B", [9, 16, 17, 40, 64])
def test_every_slot_decodes_as_it_does_alone(model, B, paged):
    eng, pair, alone, _ = model
    b = eng.batch(B, CTX, page_tokens=128 if paged else None)
    try:
        toks, lgs = _run(b, PROMPTS[:B])
    finally:
        b.close()
    flips = 0
    for s in range(B):
        at, al = alone[s]
        for k in range(STEPS + 1):
            if parity.check_step(lgs[k, s], al[k, 0], pair, int(toks[k, s]), int(at[k, 0]), f"B={B} slot {s} step {k}"):
                flips += 1
                break   # the two runs feed different tokens from here on
    assert flips <= parity.max_flips(B * (STEPS + 1))


def test_b40_graph_equals_eager(model):
    eng, _, _, fp8 = model
    eager = Q.Engine(SPEC, max_ctx=CTX, weight_fp8=fp8, use_graph=False).init_synthetic(SYN)
    bg, be = eng.batch(40, CTX), eager.batch(40, CTX)
    try:
        (tg, lg), (te, le) = _run(bg, PROMPTS[:40]), _run(be, PROMPTS[:40])
        assert np.array_equal(tg, te) and np.array_equal(lg, le)
    finally:
        bg.close(), be.close(), eager.close()


def test_b40_refilled_slots_do_not_disturb_the_others(model):
    eng = model[0]
    a, twin = eng.batch(40, CTX, page_tokens=128), eng.batch(40, CTX, page_tokens=128)
    try:
        for b in (a, twin):
            _run(b, PROMPTS[:40], steps=2)
        for s in range(1, 40, 2):
            a.release(s)
            a.prefill(s, PROMPTS[40 + s])
        for _ in range(3):
            ta, tt = a.decode_step(), twin.decode_step()
            assert np.array_equal(np.array(ta)[0::2], np.array(tt)[0::2])
            assert np.array_equal(a.logits()[0::2], twin.logits()[0::2])
    finally:
        a.close(), twin.close()


def test_b40_slot_entries_draw_what_the_rows_draw(model, qlib):
    """Two slots with entries (one over the whole vocabulary): the step's id is qie_sample_rows' on
    the step's own logit row, history and counter, one row at a time."""
    eng = model[0]
    entries = {3: Q.SlotSampling(top_k=40, temperature=0.9, top_p=0.95, seed=7),
               29: Q.SlotSampling(top_k=_lib.QIE_TOP_K_ALL, temperature=1.1, top_p=0.9, seed=8)}
    b = eng.batch(40, CTX)
    try:
        for s, e in entries.items():
            b.set_sampling(s, e)
        _run(b, PROMPTS[:40], steps=0)
        for step in range(1, 4):
            pos, hists = b.positions(), {s: b.history(s, CTX) for s in entries}
            got, lg = b.decode_step(), b.logits()
            for s, e in entries.items():
                want = run_rows(qlib, G.dev(lg[s:s + 1]), 1, SPEC.vocab, [e], hists[s][None, :], [int(pos[s])], [step])
                assert got[s] == max(want[0], 0), (step, s)
    finally:
        b.close()


def test_refusals_leave_the_batch_decoding(model):
    eng, _, _, fp8 = model
    with pytest.raises(_lib.QieError, match=r"rc=-22.*B <= 64"):
        eng.batch(65, CTX)
    if not fp8:
        e4 = Q.Engine(SPEC, max_ctx=CTX, weight_fp4=True).init_synthetic(SYN)
        with pytest.raises(_lib.QieError, match=r"rc=-22.*weight_fp4"):
            e4.batch(17, CTX)
        e4.batch(16, CTX).close()
        e4.close()
    for B, mode, words in ((9, 2, "at most 8"), (17, 1, "persistent decode step does not cover")):
        b = eng.batch(B, CTX, page_tokens=128)
        try:
            before = _run(b, PROMPTS[:B], steps=2)
            with pytest.raises(_lib.QieError, match=rf"rc=-22.*{words}"):
                b.set_decode_mode(mode)
            assert b.decode_mode == 0
            after = _run(b, PROMPTS[:B], steps=2)
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        finally:
            b.close()
