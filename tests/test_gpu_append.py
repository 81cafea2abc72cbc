"""GPU: qie_prefill_append — n new ids into a live sequence over its cached rows — against
the CPU oracle (oracle.Model.forward(prompt, 0), then single-token forwards fed the engine's
own tokens, as test_gpu_paged.test_batcher_batched_admission_matches_oracle).

Bars are test_gpu_engine.py's: logits within LOGIT_ULPS = 4 bf16 ulps of max |logit|
(logit_tol), every token the oracle's arg-max or a near-tie within that tolerance, flips
<= parity.max_flips(decisions).  Bit-exact checks compare two runs of the same kernels."""
import numpy as np
import pytest

import gpu_util as G
from conftest import rng
from parity import max_flips
from test_gpu_engine import CONFIGS, SYN, logit_tol

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib, spec as S, weights as W

pytestmark = pytest.mark.gpu

SPEC = CONFIGS["qwen2-bias-hd64"]


def _ids(seed, n, spec=SPEC):
    return [int(t) for t in rng(seed).integers(0, spec.vocab, n)]


def _check_logits(oracle, got, lg, tok, what):
    """The logit bar and the token rule; returns 1 for a tolerated near-tie flip."""
    d = np.abs(G.bf(got).astype(np.float64) - G.bf(lg))
    assert d.max() <= logit_tol(lg), f"{what}: max |dlogit| {d.max()} > {logit_tol(lg)}"
    want = oracle.argmax(lg)
    if tok != want:
        gap = abs(float(G.bf(lg[want])) - float(G.bf(lg[tok])))
        assert gap <= logit_tol(lg), f"{what}: engine {tok} vs oracle {want}, gap {gap}"
        return 1
    return 0


def _follow(oracle, b, om, lg, tok, n_steps, seq=0, what=""):
    """Checks (tok, b.logits()) against the oracle logits lg, then n_steps decode steps, the
    oracle fed the engine's own tokens.  Returns the flips."""
    flips = _check_logits(oracle, b.logits()[seq], lg, tok, f"{what} first")
    for t in range(n_steps):
        lg = om.forward([tok])
        tok = b.decode_step()[seq]
        flips += _check_logits(oracle, b.logits()[seq], lg, tok, f"{what} step {t}")
    return flips


def _rc(exc):
    return str(exc.value)


@pytest.mark.parametrize("P0,n", [(5, 1), (5, 37), (40, 9)])
@pytest.mark.parametrize("num", ["ref", "hf"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_append_matches_oracle(oracle, name, num, P0, n):
    spec = CONFIGS[name].with_numerics(num)
    eng = Q.Engine(spec, max_ctx=128).init_synthetic(SYN)
    om = oracle.Model(W.HostWeights.synthetic(spec, SYN), 128)
    prompt = _ids(100 * P0 + n, P0 + n, spec)
    b = eng.batch(1, 128)
    b.prefill(0, prompt[:P0])
    assert int(b.positions()[0]) == P0
    tok = b.append(0, prompt[P0:])                     # pos0 = the current position
    assert int(b.positions()[0]) == P0 + n
    hist = b.history(0, P0 + n + 1)
    assert list(hist[:P0 + n]) == prompt and int(hist[P0 + n]) == tok
    flips = _follow(oracle, b, om, om.forward(prompt, 0), tok, 8, what=f"{name} {num} {P0}+{n}")
    assert flips <= max_flips(9)
    assert int(b.positions()[0]) == P0 + n + 8


def test_append_across_a_split_boundary(oracle):
    """An engine whose context takes several attention splits (max_ctx 320: two of 256 keys for
    an append of <= 32 rows, one of 512 above): 20 rows from position 250 straddle the first
    boundary, then 40 more rows run the long-split form."""
    from qwen_inference_engine_amd import _lib as L_
    spec = CONFIGS["tied-g7"]
    assert L_.load().qie_attention_extend_split_tokens(20, 320) < 270
    eng = Q.Engine(spec, max_ctx=320).init_synthetic(SYN)
    om = oracle.Model(W.HostWeights.synthetic(spec, SYN), 320)
    prompt = _ids(77, 310, spec)
    b = eng.batch(1, 320)
    b.prefill(0, prompt[:250])
    tok = b.append(0, prompt[250:270])
    flips = _follow(oracle, b, om, om.forward(prompt[:270], 0), tok, 2, what="split boundary")
    tok = b.append(0, prompt[270:], pos0=270)
    flips += _follow(oracle, b, om, om.forward(prompt, 0), tok, 2, what="long split")
    assert flips <= max_flips(6)


def test_chunked_prefill_matches_oracle(oracle):
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)
    om = oracle.Model(W.HostWeights.synthetic(SPEC, SYN), 128)
    prompt = _ids(7, 100)
    b = eng.batch(1, 128)
    tok = b.prefill(0, prompt, chunk=32)               # 32 + 32 + 32 + 4
    assert int(b.positions()[0]) == 100 and list(b.history(0, 100)) == prompt
    assert _follow(oracle, b, om, om.forward(prompt, 0), tok, 0, what="chunked") <= max_flips(1)
    # chunk=None is the plain call
    b1, b2 = eng.batch(1, 128), eng.batch(1, 128)
    assert b1.prefill(0, prompt, chunk=None) == b2.prefill(0, prompt)
    assert np.array_equal(b1.logits(), b2.logits())


def test_append_paged_keeps_pages_and_grows(oracle):
    eng = Q.Engine(SPEC, max_ctx=256).init_synthetic(SYN)
    om = oracle.Model(W.HostWeights.synthetic(SPEC, SYN), 256)
    prompt = _ids(11, 140)
    b = eng.batch(1, 256, page_tokens=128)
    b.prefill(0, prompt[:120])
    assert b.page_stats()[1][0] == 1
    first = int(b.block_table(0, 1)[0])
    tok = b.append(0, prompt[120:])
    assert b.page_stats()[1][0] == 2 and int(b.block_table(0, 1)[0]) == first
    assert _follow(oracle, b, om, om.forward(prompt, 0), tok, 8, what="paged") <= max_flips(9)


def test_append_pool_exhausted_leaves_sequence_intact():
    """-28 with nothing launched: the slot keeps its page and decodes like an untouched twin."""
    eng = Q.Engine(SPEC, max_ctx=256).init_synthetic(SYN)
    prompt = _ids(12, 120)
    ref = eng.batch(1, 256, page_tokens=128, n_pages=2)   # scratch page + 1
    t0 = ref.prefill(0, prompt)
    want = [(ref.decode_step()[0], ref.logits()) for _ in range(7)]   # rows 120 .. 126: the one page
    pb = eng.batch(1, 256, page_tokens=128, n_pages=2)
    assert pb.prefill(0, prompt) == t0
    stats = pb.page_stats()
    with pytest.raises(_lib.QieError) as ex:
        pb.append(0, _ids(13, 20))                       # rows 120 .. 139 need a second page
    assert "rc=-28" in _rc(ex)
    assert pb.page_stats()[0] == stats[0] and pb.page_stats()[1][0] == stats[1][0]
    assert int(pb.positions()[0]) == 120
    for t, lg in want:
        assert pb.decode_step()[0] == t and np.array_equal(pb.logits(), lg)


def test_append_overwrites_rows_from_pos0():
    """Rows written by decode steps since pos0 do not matter: append at pos0 after 3 decode
    steps equals append at pos0 right after the prefill, bit for bit."""
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)
    head, tail = _ids(21, 30), _ids(22, 12)
    outs = []
    for steps in (3, 0):
        b = eng.batch(1, 128)
        b.prefill(0, head)
        for _ in range(steps):
            b.decode_step()
        tok = b.append(0, tail, pos0=30)
        lg = [b.logits()]
        toks = [tok]
        for _ in range(4):
            toks.append(b.decode_step()[0])
            lg.append(b.logits())
        outs.append((toks, lg, list(b.history(0, 47))))
    assert outs[0][0] == outs[1][0] and outs[0][2] == outs[1][2]
    for a, c in zip(outs[0][1], outs[1][1]):
        assert np.array_equal(a, c)


def test_append_leaves_other_slot_alone():
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)
    p0, p1 = _ids(31, 20), _ids(32, 27)
    runs = []
    for do_append in (True, False):
        b = eng.batch(2, 128)
        b.prefill(0, p0)
        b.prefill(1, p1)
        if do_append:
            b.append(0, _ids(33, 18))
        got = []
        for _ in range(8):
            t = b.decode_step()[1]
            got.append((t, b.logits()[1].copy()))
        runs.append(got)
    for (t1, l1), (t2, l2) in zip(*runs):
        assert t1 == t2 and np.array_equal(l1, l2)


@pytest.mark.parametrize("mode", ["weight_fp8", "comm_always"])
def test_append_fp8_weights_and_comm(oracle, mode):
    """The shared layer loop's other routes: fp8 weights (against the dequantised model, as
    test_gpu_fp8.py) and the exchange path at world 1 (comm_always, as test_gpu_tp.py)."""
    hw = W.HostWeights.synthetic(SPEC, SYN)
    comm = None
    if mode == "weight_fp8":
        eng = Q.Engine(SPEC, max_ctx=128, weight_fp8=True).init_synthetic(SYN)
        hw = hw.fp8_dequantized()
    else:
        comm = Q.Comm.rccl(Q.Comm.unique_id(), 1, 0, 0)
        eng = Q.Engine(SPEC, max_ctx=128, comm=comm, comm_always=True).init_synthetic(SYN)
    om = oracle.Model(hw, 128)
    prompt = _ids(41, 14 + 37)
    b = eng.batch(1, 128)
    try:
        b.prefill(0, prompt[:14])
        tok = b.append(0, prompt[14:])
        flips = _follow(oracle, b, om, om.forward(prompt, 0), tok, 8, what=mode)
    finally:
        # the communicator holds streams of its own: nothing of it may outlive the test (the
        # in-process peer ranks of test_gpu_tp.py need the process's hardware queues)
        b.close()
        eng.close()
        if comm is not None:
            comm.close()
    assert flips <= max_flips(9)


def test_append_refused_on_prefill_fp8_engine():
    spec = S.tiny("t-mx", n_layers=2, hidden=256, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, vocab=1024,
                  bias=True)
    eng = Q.Engine(spec, max_ctx=128, weight_fp8=True, prefill_fp8=True).init_synthetic(SYN)
    b = eng.batch(1, 128)
    b.prefill(0, _ids(51, 16, spec))
    with pytest.raises(_lib.QieError) as ex:
        b.append(0, _ids(52, 8, spec))
    assert "rc=-22" in _rc(ex) and "prefill_fp8" in _rc(ex)


@pytest.mark.parametrize("case", ["pos0_zero", "pos0_past_current", "reaches_max_ctx", "released_slot", "no_ids"])
def test_append_bad_arguments(case):
    """-22 before anything is launched; the live sequence then decodes as an untouched twin."""
    eng = Q.Engine(SPEC, max_ctx=64).init_synthetic(SYN)
    prompt = _ids(61, 10)
    def start():
        x = eng.batch(2, 64)
        x.prefill(0, prompt)
        if case == "released_slot":
            x.prefill(1, prompt)
            x.release(1)
        return x

    twin = start()
    want = [(twin.decode_step()[0], twin.logits()[0].copy()) for _ in range(8)]
    b = start()
    seq, ids, pos0 = 0, _ids(62, 4), 10
    if case == "pos0_zero":
        pos0 = 0
    elif case == "pos0_past_current":
        pos0 = 11
    elif case == "reaches_max_ctx":
        ids = _ids(63, 54)                               # 10 + 54 = max_ctx
    elif case == "released_slot":
        seq = 1
    else:
        ids = []
    with pytest.raises(_lib.QieError) as ex:
        b.append(seq, ids, pos0=pos0)
    assert "rc=-22" in _rc(ex)
    assert int(b.positions()[0]) == 10
    for t, lg in want:
        assert b.decode_step()[0] == t and np.array_equal(b.logits()[0], lg)


def test_batcher_chunked_prefill_matches_oracle(oracle):
    """Prompts of 21, 33, 70 and 100 tokens through 2 slots with 32-token prefill chunks: the
    long ones take one chunk per step while the other slot keeps decoding; every request's
    tokens and logits follow the oracle."""
    from qwen_inference_engine_amd.scheduler import ContinuousBatcher
    eng = Q.Engine(SPEC, max_ctx=256).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(SPEC, SYN)
    cb = ContinuousBatcher(eng, slots=2, max_ctx=256, page_tokens=128, keep_logits=True, prefill_chunk=32)
    prompts = [_ids(400 + i, n) for i, n in enumerate((21, 33, 70, 100))]
    rids = [cb.submit(p, 6 + 2 * i) for i, p in enumerate(prompts)]
    cb.run()
    flips = n_tok = 0
    for rid, pr in zip(rids, prompts):
        r = cb.requests[rid]
        assert len(r.tokens) == len(r.logits) == 6 + 2 * rid
        om = oracle.Model(hw, 256)
        lg = om.forward(pr, 0)
        for t, (tok, got) in enumerate(zip(r.tokens, r.logits)):
            flips += _check_logits(oracle, got, lg, tok, f"request {rid} token {t}")
            if t + 1 < len(r.tokens):
                lg = om.forward([tok])
        n_tok += len(r.tokens)
    assert flips <= max_flips(n_tok)
