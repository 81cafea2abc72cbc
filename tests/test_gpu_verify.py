"""GPU: qie_verify — up to 15 drafted tokens scored in one pass — against the
CPU oracle teacher-forced on the same rows (oracle.Model.forward one token at a time).

Bars are test_gpu_engine.py's and test_gpu_append.py's: every logits row within LOGIT_ULPS = 4
bf16 ulps of max |logit| (logit_tol), every emitted token the oracle's arg-max or a near-tie
within that tolerance, flips <= parity.max_flips(decisions).  The accept length is checked
exactly from the engine's own outputs; bit-exact checks compare two runs of the same kernels."""
import numpy as np
import pytest

import gpu_util as G
from conftest import rng
from parity import max_flips
from test_gpu_append import _check_logits
from test_gpu_engine import CONFIGS, SYN, logit_tol

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib, spec as S, weights as W

pytestmark = pytest.mark.gpu

SPEC = CONFIGS["qwen2-bias-hd64"]


def _ids(seed, n, spec=SPEC):
    return [int(t) for t in rng(seed).integers(0, spec.vocab, n)]


def _accept_len(draft, out):
    """The rule, from the engine's own ids: the longest prefix with d_j == out[j - 1]."""
    a = 0
    while a < len(draft) and a < len(out) and draft[a] == out[a]:
        a += 1
    return a


def _verify_checked(oracle, om, b, p, cur, draft, what, seq=0):
    """b.verify(seq, draft) of a sequence at position p with current token `cur`, whose oracle
    twin `om` holds the K/V rows [0, p).  Checks every logits row and emitted id against the
    oracle teacher-forced on cur, d_1 .. d_n, the accept length, position, history and the
    batch's logits row.  Returns (emitted ids, flips, oracle logits per row)."""
    rows = [cur] + list(draft)
    lgs = [om.forward([t], p + i) for i, t in enumerate(rows)]
    out = b.verify(seq, draft)
    vl = b.verify_logits()
    assert vl.shape == (len(rows), b.e.spec.vocab)
    for i, lg in enumerate(lgs):
        d = np.abs(G.bf(vl[i]).astype(np.float64) - G.bf(lg))
        assert d.max() <= logit_tol(lg), f"{what} row {i}: max |dlogit| {d.max()} > {logit_tol(lg)}"
    flips = 0
    for i, t in enumerate(out):
        flips += _check_logits(oracle, vl[i], lgs[i], t, f"{what} row {i}")
    a = len(out) - 1
    assert 0 <= a <= len(draft) and a == _accept_len(draft, out), (what, draft, out)
    assert a == len(draft) or draft[a] != out[a]
    assert int(b.positions()[seq]) == p + a + 1
    hist = b.history(seq, p + a + 2)
    assert int(hist[p]) == cur and [int(t) for t in hist[p + 1:]] == out, (what, hist[p:], out)
    assert np.array_equal(b.logits()[seq], vl[a]), f"{what}: batch logits row != verify row {a}"
    return out, flips, lgs


def _follow_from(oracle, om, b, pos, tok, n_steps, what, seq=0):
    """n_steps decode steps from (pos, tok), the oracle re-fed from that position with the
    engine's own tokens.  Returns the flips."""
    flips = 0
    lg = om.forward([tok], pos)
    for t in range(n_steps):
        tok = b.decode_step()[seq]
        flips += _check_logits(oracle, b.logits()[seq], lg, tok, f"{what} step {t}")
        if t + 1 < n_steps:
            lg = om.forward([tok])
    return flips


def _greedy(oracle, hw, max_ctx, prompt, n):
    """The oracle's first token after `prompt` and its n-token greedy continuation, with the
    logits that chose each: (c, [g_1 .. g_n], [lg_0 .. lg_n]), lg_i choosing g_(i+1)."""
    om = oracle.Model(hw, max_ctx)
    c = oracle.argmax(om.forward(prompt, 0))
    toks, lgs, t = [], [], c
    for _ in range(n + 1):
        lgs.append(om.forward([t]))
        t = oracle.argmax(lgs[-1])
        toks.append(t)
    return c, toks[:n], lgs


def _start(oracle, b, prompt, c, lg_prompt):
    """Prefill; the engine's first token may differ from the oracle's at a near-tie: counted and
    forced (qie_batch_set_position), as test_gpu_engine.forced_compare does."""
    tok = b.prefill(0, prompt)
    flips = _check_logits(oracle, b.logits()[0], lg_prompt, tok, "prefill")
    if tok != c:
        b.set_position(0, len(prompt), c)
    return flips


# ---------------------------------------------------------------------------- 1. the oracle
@pytest.mark.parametrize("n", [0, 1, 7, 15])
@pytest.mark.parametrize("num", ["ref", "hf"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_verify_matches_oracle(oracle, name, num, n):
    """Drafts: the oracle's own greedy continuation for j tokens, then its ARG-MIN logit (never
    a near-tie: the reference alone emits exactly j + 1 tokens), then random ids."""
    spec = CONFIGS[name].with_numerics(num)
    eng = Q.Engine(spec, max_ctx=128).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(spec, SYN)
    P = 20
    prompt = _ids(1000 + n, P, spec)
    c, cont, glg = _greedy(oracle, hw, 128, prompt, n)
    lg_prompt = oracle.Model(hw, 128).forward(prompt, 0)
    flips = decisions = 0
    for j in sorted({0, n // 2, n}):
        draft = cont[:j]
        if j < n:
            draft = draft + [int(np.argmin(G.bf(glg[j])))] + _ids(7 * n + j, n - j - 1, spec)
        assert len(draft) == n
        b = eng.batch(1, 128)
        f0 = _start(oracle, b, prompt, c, lg_prompt)
        om = oracle.Model(hw, 128)
        om.forward(prompt, 0)
        what = f"{name} {num} n={n} j={j}"
        out, f1, _ = _verify_checked(oracle, om, b, P, c, draft, what)
        if f1 == 0:
            assert len(out) == j + 1, (what, out)     # no near-tie among the rows: the reference's count
        f2 = _follow_from(oracle, om, b, P + len(out), out[-1], 6, what)
        flips += f0 + f1 + f2
        decisions += 1 + len(out) + 6
    assert flips <= max_flips(decisions), f"{flips} flips in {decisions} decisions"


# ------------------------------------------------------------------ 2. across a split boundary
def test_verify_across_a_split_boundary(oracle):
    """max_ctx 320 takes two 256-key attention splits for a call of 16 rows: rows at positions
    250 .. 265 straddle key 256."""
    spec = CONFIGS["tied-g7"]
    assert _lib.load().qie_attention_extend_split_tokens(16, 320) == 256
    eng = Q.Engine(spec, max_ctx=320).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(spec, SYN)
    prompt = _ids(78, 250, spec)
    c, cont, _ = _greedy(oracle, hw, 320, prompt, 15)
    om = oracle.Model(hw, 320)
    lg_prompt = om.forward(prompt, 0)
    b = eng.batch(1, 320)
    flips = _start(oracle, b, prompt, c, lg_prompt)
    out, f1, _ = _verify_checked(oracle, om, b, 250, c, cont, "split boundary")
    if f1 == 0:
        assert len(out) == 16
    flips += f1 + _follow_from(oracle, om, b, 250 + len(out), out[-1], 3, "split boundary")
    assert flips <= max_flips(1 + len(out) + 3)


# ------------------------------------------------------------ 3. paged, across a page boundary
def _paged_case(oracle):
    eng = Q.Engine(SPEC, max_ctx=256).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(SPEC, SYN)
    prompt = _ids(14, 120)
    c, cont, glg = _greedy(oracle, hw, 256, prompt, 15)
    draft = cont[:2] + [int(np.argmin(G.bf(glg[2])))] + _ids(15, 12)   # the 3rd one wrong
    return eng, hw, prompt, c, draft


def test_verify_paged_takes_and_keeps_the_second_page(oracle):
    eng, hw, prompt, c, draft = _paged_case(oracle)
    om = oracle.Model(hw, 256)
    lg_prompt = om.forward(prompt, 0)
    b = eng.batch(1, 256, page_tokens=128)
    flips = _start(oracle, b, prompt, c, lg_prompt)
    assert b.page_stats()[1][0] == 1
    first = int(b.block_table(0, 1)[0])
    out, f1, _ = _verify_checked(oracle, om, b, 120, c, draft, "paged")   # rows 120 .. 135
    if f1 == 0:
        assert len(out) == 3
    # the page taken for rows 128 .. 135 stays with the slot although they were rejected
    assert b.page_stats()[1][0] == 2 and int(b.block_table(0, 1)[0]) == first
    flips += f1 + _follow_from(oracle, om, b, 120 + len(out), out[-1], 8, "paged")
    assert b.page_stats()[1][0] == 2 and int(b.block_table(0, 1)[0]) == first
    assert flips <= max_flips(1 + len(out) + 8)


def test_verify_pool_exhausted_leaves_sequence_intact(oracle):
    """-28 with nothing launched: the slot keeps its page and decodes like an untouched twin."""
    eng, hw, prompt, c, draft = _paged_case(oracle)
    ref = eng.batch(1, 256, page_tokens=128, n_pages=2)     # scratch page + 1
    t0 = ref.prefill(0, prompt)
    want = [(ref.decode_step()[0], ref.logits()) for _ in range(7)]   # rows 120 .. 126: the one page
    pb = eng.batch(1, 256, page_tokens=128, n_pages=2)
    assert pb.prefill(0, prompt) == t0
    stats = pb.page_stats()
    with pytest.raises(_lib.QieError) as ex:
        pb.verify(0, draft)                                   # rows 120 .. 135 need a second page
    assert "rc=-28" in str(ex.value)
    assert pb.page_stats()[0] == stats[0] and pb.page_stats()[1][0] == stats[1][0]
    assert int(pb.positions()[0]) == 120
    for t, lg in want:
        assert pb.decode_step()[0] == t and np.array_equal(pb.logits(), lg)


# -------------------------------------------------------------------- 4. graph replay == eager
def test_verify_graph_equals_eager_and_repeats():
    prompt = _ids(21, 30)
    runs = {}
    for graph in (True, False):
        eng = Q.Engine(SPEC, max_ctx=128, use_graph=graph).init_synthetic(SYN)
        b = eng.batch(1, 128)
        t0 = b.prefill(0, prompt)
        # drafts: what plain decode steps emit (so most are accepted), one spoiled
        twin = eng.batch(1, 128)
        twin.prefill(0, prompt)
        cont = [int(t) for t in twin.decode(12)[:, 0]]
        d1 = cont[:7]
        d1[4] = (d1[4] + 1) % SPEC.vocab
        got = []
        o1 = b.verify(0, d1)                                   # captures (graph engine)
        got.append((o1, b.verify_logits(), b.logits()))
        p1 = 30 + len(o1)
        d2 = cont[len(o1):len(o1) + 7]
        o2 = b.verify(0, d2)                                   # the same (M, sampling): a replay
        got.append((o2, b.verify_logits(), b.logits()))
        assert len(o1) <= 5 and len(o1) - 1 == _accept_len(d1, o1)   # draft 5 was spoiled
        # back to position p1 with its token: the same call again is the same bits
        b.set_position(0, p1, o1[-1])
        o3 = b.verify(0, d2)
        got.append((o3, b.verify_logits(), b.logits()))
        assert o3 == o2 and np.array_equal(got[1][1], got[2][1]) and np.array_equal(got[1][2], got[2][2])
        assert int(b.positions()[0]) == p1 + len(o2)
        runs[graph] = (t0, got)
    assert runs[True][0] == runs[False][0]
    for (oa, va, la), (ob, vb, lb) in zip(runs[True][1], runs[False][1]):
        assert oa == ob and np.array_equal(va, vb) and np.array_equal(la, lb)


# ---------------------------------------------------------------------------------- 5. sampled
@pytest.mark.parametrize("mode", ["plain", "comm_always"])
def test_verify_sampled_rows_draw_what_decode_steps_would(oracle, mode):
    """Row j's id == the oracle's restated sampler on the engine's own row-j logits with counter
    step0 + j (test_gpu_engine.test_topk_sampling_schedule_on_engine_logits' convention: the
    prefill draws with the seed, decode step s with seed + s).  comm_always: the rows are
    sampled from the gathered logits of the exchange path (world 1)."""
    smp = Q.Sampling(top_k=40, temperature=0.8, top_p=0.9, seed=99)
    comm = Q.Comm.rccl(Q.Comm.unique_id(), 1, 0, 0) if mode == "comm_always" else None
    eng = Q.Engine(SPEC, max_ctx=128, comm=comm, comm_always=comm is not None).init_synthetic(SYN)
    prompt, junk = _ids(31, 12), _ids(32, 7)
    step0, p = 4, 12 + 3
    live = []

    def fresh():
        """A sequence after the prefill and 3 sampled decode steps: counter step0, position p."""
        b = eng.batch(1, 128)
        live.append(b)
        tok = b.prefill(0, prompt, smp)
        assert tok == oracle.sample(b.logits()[0], 40, 0.8, 0.9, 99)
        for s in range(1, 4):
            tok = b.decode_step(smp)[0]
            assert tok == oracle.sample(b.logits()[0], 40, 0.8, 0.9, 99 + s)
        return b

    try:
        # three drafts the rows WILL draw, found one at a time: a row's logits depend on the rows
        # before it only, so the same 8-row call with a longer right prefix repeats its draws
        good = []
        for _ in range(3):
            t = fresh().verify(0, good + junk[len(good):], smp)
            assert len(t) >= len(good) + 1 and t[:len(good)] == good
            good.append(t[len(good)])
        draft = good + junk[3:]
        b = fresh()
        out = b.verify(0, draft, smp)
        vl = b.verify_logits()
        assert vl.shape[0] == 8
        a = len(out) - 1
        assert a >= 3 and a == _accept_len(draft, out) and (a == 7 or draft[a] != out[a])
        for j, t in enumerate(out):
            assert t == oracle.sample(vl[j], 40, 0.8, 0.9, 99 + step0 + j), j
        assert int(b.positions()[0]) == p + a + 1
        tok = b.decode_step(smp)[0]
        assert tok == oracle.sample(b.logits()[0], 40, 0.8, 0.9, 99 + step0 + len(out))
    finally:
        for x in live:
            x.close()
        eng.close()
        if comm is not None:
            comm.close()


# ----------------------------------------------------------------------------- 6. other routes
@pytest.mark.parametrize("mode", ["weight_fp8", "comm_always"])
def test_verify_fp8_weights_and_comm(oracle, mode):
    hw = W.HostWeights.synthetic(SPEC, SYN)
    comm = None
    if mode == "weight_fp8":
        eng = Q.Engine(SPEC, max_ctx=128, weight_fp8=True).init_synthetic(SYN)
        hw = hw.fp8_dequantized()
    else:
        comm = Q.Comm.rccl(Q.Comm.unique_id(), 1, 0, 0)
        eng = Q.Engine(SPEC, max_ctx=128, comm=comm, comm_always=True).init_synthetic(SYN)
    prompt = _ids(41, 20)
    c, cont, glg = _greedy(oracle, hw, 128, prompt, 7)
    draft = cont[:5] + [int(np.argmin(G.bf(glg[5])))] + _ids(42, 1)
    om = oracle.Model(hw, 128)
    lg_prompt = om.forward(prompt, 0)
    b = eng.batch(1, 128)
    try:
        flips = _start(oracle, b, prompt, c, lg_prompt)
        out, f1, _ = _verify_checked(oracle, om, b, 20, c, draft, mode)
        if f1 == 0:
            assert len(out) == 6
        flips += f1 + _follow_from(oracle, om, b, 20 + len(out), out[-1], 6, mode)
    finally:
        # the communicator holds streams of its own: nothing of it may outlive the test
        b.close()
        eng.close()
        if comm is not None:
            comm.close()
    assert flips <= max_flips(1 + len(out) + 6)


# ------------------------------------------------------------------- 7. isolation and errors
def test_verify_leaves_other_slot_alone():
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)
    p0, p1 = _ids(51, 20), _ids(52, 27)
    runs = []
    for do_verify in (True, False):
        b = eng.batch(2, 128)
        b.prefill(0, p0)
        b.prefill(1, p1)
        if do_verify:
            b.verify(0, _ids(53, 9))
        got = []
        for _ in range(8):
            t = b.decode_step()[1]
            got.append((t, b.logits()[1].copy()))
        runs.append(got)
    for (t1, l1), (t2, l2) in zip(*runs):
        assert t1 == t2 and np.array_equal(l1, l2)


MODE1_SPEC = S.tiny("t-v-pk", n_layers=2, hidden=1024, n_heads=8, n_kv_heads=2, head_dim=128, ffn=2048, vocab=4096,
                    bias=False, qk_norm=True)
MX_SPEC = S.tiny("t-v-mx", n_layers=2, hidden=256, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, vocab=1024,
                 bias=True)


@pytest.mark.parametrize("case", ["idle_slot", "sixteen_drafts", "id_is_vocab", "reaches_max_ctx", "prefill_fp8",
                                  "decode_mode_1"])
def test_verify_bad_arguments(case):
    """-22 before anything is launched; the live sequence then decodes as an untouched twin."""
    spec, kw = SPEC, {}
    if case == "prefill_fp8":
        spec, kw = MX_SPEC, dict(weight_fp8=True, prefill_fp8=True)
    elif case == "decode_mode_1":
        spec = MODE1_SPEC
    eng = Q.Engine(spec, max_ctx=64, **kw).init_synthetic(SYN)
    prompt = _ids(61, 10, spec)

    def start():
        x = eng.batch(1 if case == "decode_mode_1" else 2, 64)
        x.prefill(0, prompt)
        if case == "decode_mode_1":
            x.set_decode_mode(1)
        return x

    twin = start()
    want = [(twin.decode_step()[0], twin.logits()[0].copy()) for _ in range(8)]
    b = start()
    seq, draft, word = 0, _ids(62, 4, spec), "qie_verify"
    if case == "idle_slot":
        seq, word = 1, "no live sequence"
    elif case == "sixteen_drafts":
        draft, word = _ids(63, 16, spec), "16 drafts"
    elif case == "id_is_vocab":
        draft[2], word = spec.vocab, "out of range"
    elif case == "reaches_max_ctx":
        b.set_position(0, 58, prompt[0])                       # 58 + 5 + 1 = max_ctx
        twin = start()
        twin.set_position(0, 58, prompt[0])
        want = [(twin.decode_step()[0], twin.logits()[0].copy()) for _ in range(4)]
        draft, word = _ids(64, 5, spec), "max_ctx"
    elif case == "prefill_fp8":
        word = "prefill_fp8"
    else:
        word = "decode mode 1"
    pos = int(b.positions()[0])
    with pytest.raises(_lib.QieError) as ex:
        b.verify(seq, draft)
    assert "rc=-22" in str(ex.value) and word in str(ex.value), str(ex.value)
    assert int(b.positions()[0]) == pos
    for t, lg in want:
        assert b.decode_step()[0] == t and np.array_equal(b.logits()[0], lg)


# --------------------------------------------------------------------------------- 8. end to end
def _teacher_forced_stream(oracle, hw, max_ctx, prompt, out, what):
    """Every token of `out` is the oracle's arg-max (or a near-tie within logit_tol) given the
    prompt and the tokens before it.  Returns the flips."""
    om = oracle.Model(hw, max_ctx)
    lg = om.forward(prompt, 0)
    flips = 0
    for i, t in enumerate(out):
        want = oracle.argmax(lg)
        if t != want:
            gap = abs(float(G.bf(lg[want])) - float(G.bf(lg[t])))
            assert gap <= logit_tol(lg), f"{what} token {i}: engine {t} vs oracle {want}, gap {gap}"
            flips += 1
        if i + 1 < len(out):
            lg = om.forward([t])
    return flips


@pytest.mark.parametrize("drafter", ["ngram", "same_weights", "other_seed"])
def test_speculative_decoder_end_to_end(oracle, drafter):
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(SPEC, SYN)
    b = eng.batch(1, 128)
    deng = None
    if drafter == "ngram":
        d = Q.NgramDrafter()
        prompt = _ids(71, 6) * 4                               # a repetitive prompt: lookups hit
    else:
        syn = SYN if drafter == "same_weights" else W.SynthParams(seed=12, w_scale=0.08, norm_scale=0.25,
                                                                  bias_scale=0.05)
        deng = Q.Engine(SPEC, max_ctx=128).init_synthetic(syn)
        d = Q.ModelDrafter(deng.batch(1, 128))
        prompt = _ids(72, 20)
    calls = []
    real_verify = b.verify
    b.verify = lambda seq, draft, sampling=Q.GREEDY: (calls.append((list(draft), real_verify(seq, draft, sampling)))
                                                      or calls[-1][1])
    dec = Q.SpeculativeDecoder(b, d, k=4)
    out = dec.generate(prompt, 40)
    assert len(out) == 40 and dec.stats["emitted"] == 40
    assert all(len(o) >= 1 for _, o in calls) and dec.stats["verify_calls"] == len(calls)
    assert 1 + sum(len(o) for _, o in calls) == 40
    assert dec.stats["drafted"] == sum(len(dr) for dr, _ in calls)
    assert dec.stats["accepted"] == sum(len(o) - 1 for _, o in calls)
    assert int(b.positions()[0]) == len(prompt) + 39
    assert [int(t) for t in b.history(0, len(prompt) + 40)] == prompt + out
    assert _teacher_forced_stream(oracle, hw, 128, prompt, out, drafter) <= max_flips(40)
    if drafter == "same_weights":
        # the drafter runs the same model on the GEMV route: a rejection is a near-tie between
        # that route and the M-row route
        rejected = sum(1 for dr, o in calls if len(o) - 1 < len(dr))
        assert rejected <= max_flips(dec.stats["drafted"]), (rejected, dec.stats)
        assert dec.stats["accepted"] >= dec.stats["drafted"] - 4 * rejected
    if drafter == "other_seed":
        assert dec.stats["drafted"] > 0                        # rejected rows were written, and left no trace
