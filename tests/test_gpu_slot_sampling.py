"""GPU: per-slot sampling entries — qie_sample_rows against the numpy restatement
of its contract (tests/slot_sampling_ref.py: float32 penalties and bias, bf16 rounding, then the
CPU oracle's arg-max / sampler), ids exactly equal; and the engine tier (decode, prefill, verify,
fork, idle slots, tensor parallelism, the batcher) against the same reference applied to the
engine's own logit rows, histories and step counters."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

import gpu_util as G
import slot_sampling_ref as R
from conftest import rng
from test_gpu_engine import CONFIGS, SYN
from test_gpu_tp import run_ranks

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd._lib import SamplingC, SampleRowsArgsC, SlotSamplingC
from qwen_inference_engine_amd.scheduler import ContinuousBatcher

pytestmark = pytest.mark.gpu

SS = Q.SlotSampling
SPEC = CONFIGS["qwen2-bias-hd64"]
NEG_INF = float("-inf")
MIN_P_MARGIN = 1e-3   # far outside any expf ulp difference


def _ids(seed, n, spec=SPEC):
    return [int(t) for t in rng(seed).integers(0, spec.vocab, n)]


# ------------------------------------------------------------------------ operator harness
def _table(entries):
    """Device table of entries (None: no entry, n_bias = -1)."""
    arr = (SlotSamplingC * len(entries))()
    for i, e in enumerate(entries):
        if e is None:
            arr[i].n_bias, arr[i].repetition_penalty = -1, 1.0
        else:
            arr[i] = e.to_c()
    return G.dev(np.frombuffer(bytes(arr), np.uint8).copy())


def run_rows(qlib, dl, M, V, entries, hist, q, steps, slot0=0, stride=1, tail=None, tail_len=None, fallback=None):
    a = SampleRowsArgsC()
    ws = G.zeros_bytes(qlib.qie_sample_rows_workspace_bytes(M, V))
    ids = G.dev(np.full((M,), -7, np.int32))
    a.logits, a.M, a.V, a.ld = G.p(dl), M, V, V
    a.table, a.slot0, a.slot_stride = G.p(_table(entries)), slot0, stride
    fb = None
    if fallback is not None:
        fb = fallback.to_c()
        a.fallback = C.pointer(fb)
    hist = np.ascontiguousarray(hist, np.int32)
    a.hist, a.hist_stride = G.p(G.dev(hist)), hist.shape[1]
    a.q_dev = G.p(G.dev(np.asarray(q, np.int32)))
    if tail is not None:
        a.tail_dev, a.tail_len_dev = G.p(G.dev(np.asarray(tail, np.int32))), G.p(G.dev(np.asarray(tail_len, np.int32)))
    a.step_dev, a.out_ids, a.ws = G.p(G.dev(np.asarray(steps, np.int32))), G.p(ids), G.p(ws)
    G.check(qlib.qie_sample_rows(C.byref(a), None), "qie_sample_rows")
    G.check(qlib.qie_synchronize())
    return [int(t) for t in G.host(ids)]


MAX_CTX = 200
STEPS = [0, 1, 7]
Q_POS = [0, 129, MAX_CTX - 1]   # histories of length 1, 130 and max_ctx


def op_rows(oracle, V, kind):
    r = rng(V)
    if kind == "ties":
        return oracle.f32_to_bf16(r.integers(0, 6, (3, V)).astype(np.float32))
    return oracle.f32_to_bf16((r.standard_normal((3, V)) * 3).astype(np.float32))


def op_history(oracle, lg, V):
    """Three history rows of max_ctx words: ids with many duplicates drawn from each row's own 40
    best (so the penalties move the candidates), ids >= V and negative ids among them; for a
    vocabulary past one slice, the ids on both sides of the slice boundary."""
    r = rng(V + 1)
    hist = np.zeros((3, MAX_CTX), np.int32)
    for m in range(3):
        top, _ = oracle.topk(lg[m], 40)
        pool = np.concatenate([top[:12], r.integers(0, V, 6), [V, V + 5, 1 << 24, -1, -4096, 2 ** 31 - 1]])
        if V > 4096:
            pool = np.concatenate([pool, [4095, 4096, 4095, 4096]])
        hist[m] = r.choice(pool, MAX_CTX).astype(np.int64).astype(np.int32)
        if V > 4096:
            hist[m, Q_POS[m]] = 4096
            if Q_POS[m] > 0:
                hist[m, Q_POS[m] - 1] = 4095
    hist[1, 126:130] = hist[1, 125]   # a run of one id that penalty_last_n = 2 cuts in the middle
    return hist


def op_entries(lg, oracle, kind):
    best = [int(oracle.argmax(lg[m])) for m in range(3)]
    T = 0.7
    base = dict(top_k=50, temperature=T, seed=1234)
    return {
        "neutral": SS(**base),
        "repetition": SS(repetition_penalty=1.3, **base),
        "presence": SS(presence_penalty=0.75, **base),
        "frequency": SS(frequency_penalty=0.3, **base),
        "all three": SS(repetition_penalty=1.2, presence_penalty=0.5, frequency_penalty=0.2, **base),
        "last_n mid-duplicate": SS(frequency_penalty=0.4, penalty_last_n=2, **base),
        "start past q": SS(repetition_penalty=1.5, presence_penalty=2.0, penalty_start=MAX_CTX + 5, **base),
        "bias": SS(bias={best[0]: NEG_INF, best[1]: -1.5, best[2]: 2.25, 3: 0.5}, **base),
        "min-p": SS(top_k=50, temperature=T, min_p=0.06 if kind == "normal" else 0.15, seed=77),
        "greedy + penalties": SS(top_k=1, repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2),
        "greedy banned arg-max": SS(top_k=1, bias={b: NEG_INF for b in set(best)}),
        "temperature 0 is greedy": SS(top_k=50, temperature=0.0, frequency_penalty=0.5),
        "combined k=256": SS(top_k=256, temperature=0.9, top_p=0.9, min_p=0.02 if kind == "normal" else 0.03,
                             seed=4321, repetition_penalty=1.15, presence_penalty=0.4, frequency_penalty=0.1,
                             penalty_start=3, penalty_last_n=150, bias={best[0]: NEG_INF, best[1]: 1.0, 9: -0.75}),
    }


def op_expected(oracle, V, kind):
    """(rows, history, {name: (entry, [want id per row])}); asserts, on the CPU, that no min-p
    decision of the reference sits within MIN_P_MARGIN of its threshold."""
    lg = op_rows(oracle, V, kind)
    hist = op_history(oracle, lg, V)
    cases = {}
    for name, e in op_entries(lg, oracle, kind).items():
        want = []
        for m in range(3):
            tok, margin = R.choose(oracle, lg[m], e, R.window_ids(e, hist[m], Q_POS[m]), STEPS[m])
            assert margin >= MIN_P_MARGIN, (name, m, margin)
            want.append(tok)
        cases[name] = (e, want)
    return lg, hist, cases


# --------------------------------------------------------------------------- 1. the operator
@pytest.mark.parametrize("V", [1000, 4097, 151936])
@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_sample_rows_equals_the_reference(oracle, qlib, V, kind):
    lg, hist, cases = op_expected(oracle, V, kind)
    dl = G.dev(lg)
    for name, (e, want) in cases.items():
        got = run_rows(qlib, dl, 3, V, [e] * 3, hist, Q_POS, STEPS)
        assert got == want, (name, got, want)
    # the penalties did move choices: the reference differs from the neutral entry somewhere
    assert any(w != cases["neutral"][1] for _, w in cases.values())
    # rows may share one slot (a verify step's rows): a tail replaces the window's last ids
    e = cases["all three"][0]
    tail, tl = [int(hist[2, 5]), int(hist[2, 5]), 4096 % V], [0, 1, 3]
    qs = [60, 61, 63]
    got = run_rows(qlib, dl, 3, V, [None, None, e], hist, qs, STEPS, slot0=2, stride=0, tail=tail, tail_len=tl)
    want = [R.choose(oracle, lg[m], e, R.window_ids(e, hist[2], qs[m], tail[:tl[m]]), STEPS[m])[0] for m in range(3)]
    assert got == want


def test_no_selectable_element_yields_minus_one(oracle, qlib):
    V = 1000
    lg = oracle.f32_to_bf16(np.full((2, V), NEG_INF, np.float32))
    lg[1, 5] = 0x7FC0
    hist = np.zeros((2, 8), np.int32)
    for e in (SS(top_k=1), SS(top_k=50, temperature=0.7)):
        assert run_rows(qlib, G.dev(lg), 2, V, [e, e], hist, [3, 3], [0, 0]) == [-1, -1]


# ------------------------------------------------------------- 2. a neutral entry is qie_sample
@pytest.mark.parametrize("V", [1000, 151936])
@pytest.mark.parametrize("kind", ["normal", "ties"])
def test_neutral_entry_is_qie_sample(oracle, qlib, V, kind):
    M = 3
    lg = op_rows(oracle, V, kind)
    dl = G.dev(lg)
    hist = op_history(oracle, lg, V)
    ws = G.zeros_bytes(qlib.qie_sample_workspace_bytes(M, V))
    ids = G.zeros((M,), np.int32)
    step = G.dev(np.array(STEPS, np.int32))
    for k, T, tp in [(1, 1.0, 1.0), (50, 0.7, 1.0), (50, 1.0, 1.0), (5, 1.3, 1.0), (256, 0.9, 1.0), (50, 0.8, 0.9)]:
        s = SamplingC()
        s.top_k, s.temperature, s.top_p, s.seed = k, T, tp, 1234
        G.check(qlib.qie_sample(G.p(dl), M, V, V, C.byref(s), G.p(step), G.p(ids), G.p(ws), None))
        G.check(qlib.qie_synchronize())
        want = [int(t) for t in G.host(ids)]
        e = SS(top_k=k, temperature=T, top_p=tp, seed=1234)
        assert run_rows(qlib, dl, M, V, [e] * M, hist, Q_POS, STEPS) == want, (k, T, tp)
        # ... and so is a row without an entry under the call's sampling
        fb = Q.Sampling(top_k=k, temperature=T, top_p=tp, seed=1234)
        assert run_rows(qlib, dl, M, V, [None] * M, hist, Q_POS, STEPS, fallback=fb) == want, (k, T, tp)


# ------------------------------------------------------------------------------ engine harness
CALL = Q.Sampling(top_k=40, temperature=0.8, top_p=0.9, seed=99)


def as_entry(s):
    return SS(top_k=s.top_k, temperature=s.temperature, top_p=s.top_p, seed=s.seed)


def want_id(oracle, b, slot, entry, q, step, hist=None, logits=None, call=CALL):
    """The reference on the engine's own logit row of `slot`, its history and step counter."""
    e = entry if entry is not None else as_entry(call)
    hist = b.history(slot, b.max_ctx) if hist is None else hist
    row = (b.logits() if logits is None else logits)[slot]
    tok, margin = R.choose(oracle, row, e, R.window_ids(e, hist, q), step)
    return max(tok, 0)   # the step's finalisation maps "no choice" to id 0


# ------------------------------------------------------------------ 3. engine, mixed batch
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("graph", [False, True])
def test_engine_mixed_batch_follows_each_slots_entry(oracle, paged, graph):
    prompts = [_ids(1, 9), _ids(2, 12), _ids(3, 7)]
    prompts[0][3] = prompts[0][1]   # a repeated prompt id
    entries = [SS(top_k=1, repetition_penalty=1.3),
               SS(top_k=50, temperature=0.7, seed=4242, presence_penalty=0.6, frequency_penalty=0.3,
                  penalty_start=len(prompts[1])),
               None]
    eng = Q.Engine(SPEC, max_ctx=256, use_graph=graph).init_synthetic(SYN)
    b = eng.batch(3, 256, page_tokens=128 if paged else None)
    try:
        for s, e in enumerate(entries):
            if e is not None:
                b.set_sampling(s, e)
        assert b.slot_sampling(0) == dataclasses.replace(entries[0], repetition_penalty=float(np.float32(1.3)))
        assert b.slot_sampling(2) is None
        for s, pr in enumerate(prompts):
            tok = b.prefill(s, pr, CALL)
            assert tok == want_id(oracle, b, s, entries[s], len(pr) - 1, 0), ("prefill", s)
        moved = 0
        for step in range(1, 9):
            if step == 5:   # values are read from the table, not captured: no re-capture, new ids
                entries[1] = dataclasses.replace(entries[1], temperature=1.3, bias={777: 200.0})
                entries[0] = dataclasses.replace(entries[0], bias={555: 200.0})
                b.set_sampling(1, entries[1])
                b.set_sampling(0, entries[0])
            pos = b.positions()
            hists = [b.history(s, 256) for s in range(3)]
            got = b.decode_step(CALL)
            lg = b.logits()
            for s in range(3):
                want = want_id(oracle, b, s, entries[s], int(pos[s]), step, hists[s], lg)
                assert got[s] == want, (step, s, got[s], want)
                moved += want != want_id(oracle, b, s, None, int(pos[s]), step, hists[s], lg)
            if step == 5:
                assert got[0] == 555 and got[1] == 777
        assert moved > 0   # the entries decided ids the call's sampling would not have
    finally:
        b.close()
        eng.close()


# ------------------------------------------------------------------ 4. unset is unchanged
@pytest.mark.parametrize("smp", [Q.GREEDY, CALL], ids=["greedy", "sampled"])
def test_cleared_and_neutral_entries_change_nothing(smp):
    prompts = [_ids(11, 10), _ids(12, 6)]
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)

    def run(prepare):
        b = eng.batch(2, 128)
        try:
            prepare(b)
            ids, lgs = [], []
            for s, pr in enumerate(prompts):
                ids.append(b.prefill(s, pr, smp))
            lgs.append(b.logits())
            for _ in range(6):
                ids.extend(b.decode_step(smp))
                lgs.append(b.logits())
            return ids, np.stack(lgs)
        finally:
            b.close()

    def set_and_clear(b):
        b.set_sampling(0, SS(top_k=50, temperature=0.7, repetition_penalty=1.3, bias={4: NEG_INF}))
        b.set_sampling(1, SS(presence_penalty=1.0))
        b.set_sampling(0, None)
        b.set_sampling(1, None)
        assert b.slot_sampling(0) is None and b.slot_sampling(1) is None

    def neutral_twin(b):   # slot 1 carries the call's own values as its entry
        b.set_sampling(1, as_entry(smp))

    try:
        plain = run(lambda b: None)
        for prepare in (set_and_clear, neutral_twin):
            ids, lgs = run(prepare)
            assert ids == plain[0], prepare.__name__
            assert np.array_equal(lgs, plain[1]), prepare.__name__
    finally:
        eng.close()


# ------------------------------------------------------------------------------ 5. verify
@pytest.mark.parametrize("mode", ["plain", "comm_always"])
def test_verify_rows_see_the_history_a_decode_step_would(oracle, mode):
    """qie_verify on a slot with a sampled entry returns what plain decode steps return from a
    fork of the same state with the same entry.  The entry boosts what the window holds
    (negative presence / frequency penalties beside the repetition penalty), so the sequence
    repeats itself and a row's choice depends on the drafts before it."""
    entry = SS(top_k=40, temperature=0.8, top_p=0.95, seed=99, repetition_penalty=1.3, presence_penalty=-6.0,
               frequency_penalty=-1.0)
    comm = Q.Comm.rccl(Q.Comm.unique_id(), 1, 0, 0) if mode == "comm_always" else None
    eng = Q.Engine(SPEC, max_ctx=128, comm=comm, comm_always=comm is not None).init_synthetic(SYN)
    prompt = _ids(31, 12)
    live = []

    def fresh():
        """Slot 0 after the prefill and 3 decode steps; slot 1 a fork of it (entry included)."""
        b = eng.batch(2, 128)
        live.append(b)
        b.set_sampling(0, entry)
        b.prefill(0, prompt, CALL)
        for _ in range(3):
            b.decode_step(CALL)
        b.fork(0, 1)
        assert b.slot_sampling(1) == b.slot_sampling(0) and b.slot_sampling(1) is not None
        return b

    try:
        twin = fresh()
        steps = [twin.decode_step(CALL) for _ in range(16)]
        assert all(s[0] == s[1] for s in steps)   # the fork decodes what its source decodes
        toks = [s[0] for s in steps]
        repeats = 0
        for n_draft, wrong_at in [(0, None), (3, None), (15, None), (15, 6)]:
            b = fresh()
            seen = set(int(t) for t in b.history(0, int(b.positions()[0]) + 1))
            draft = toks[:n_draft]
            repeats += sum(1 for i, d in enumerate(draft) if d in seen or d in draft[:i])
            if wrong_at is not None:
                draft = draft[:wrong_at] + [(draft[wrong_at] + 1) % SPEC.vocab] + draft[wrong_at + 1:]
            out = b.verify(0, draft, CALL)
            vl = b.verify_logits()
            n = len(out)
            assert n == (n_draft + 1 if wrong_at is None else wrong_at + 1), (n_draft, wrong_at, out)
            # the fork (slot 1) takes as many plain decode steps
            plain = [b.decode_step(CALL)[1] for _ in range(n)]
            assert out == plain == toks[:n], (n_draft, wrong_at, out, plain)
            # ... and each accepted row is the reference on its own logits and window
            p = len(prompt) + 3
            h = twin.history(0, 128)
            for i in range(n):
                w, _ = R.choose(oracle, vl[i], entry, R.window_ids(entry, h, p + i), 4 + i)
                assert out[i] == w, (n_draft, i)
        assert repeats > 0   # a draft repeated an id of the history: the tail counts mattered
    finally:
        for x in live:
            x.close()
        eng.close()
        if comm is not None:
            comm.close()


# -------------------------------------------------------------------------------- 6. fork
def test_fork_copies_the_entry(oracle):
    entry = SS(top_k=50, temperature=0.9, seed=7, repetition_penalty=1.2, frequency_penalty=0.3)
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)
    b = eng.batch(3, 128)
    try:
        b.set_sampling(0, entry)
        b.set_sampling(2, SS(top_k=1, bias={3: 50.0}))   # replaced by the fork
        b.prefill(0, _ids(41, 10), CALL)
        b.decode_step(CALL)
        b.decode_step(CALL)                               # slot 0: position 12, step counter 3
        b.fork(0, 1)
        b.fork(0, 2, step_offset=5)
        assert b.slot_sampling(1) == b.slot_sampling(0) == b.slot_sampling(2)
        pos = b.positions()
        hists = [b.history(s, 128) for s in range(3)]
        got = b.decode_step(CALL)
        lg = b.logits()
        assert np.array_equal(lg[0], lg[1]) and np.array_equal(lg[0], lg[2])
        assert got[1] == got[0] == want_id(oracle, b, 0, entry, int(pos[0]), 3, hists[0], lg)
        assert got[2] == want_id(oracle, b, 2, entry, int(pos[2]), 3 + 5, hists[2], lg)
        # a source without an entry leaves the destination without one
        b.set_sampling(0, None)
        b.fork(0, 1)
        assert b.slot_sampling(1) is None
    finally:
        b.close()
        eng.close()


# ------------------------------------------------------------------ 7. idle and released slots
@pytest.mark.parametrize("paged", [False, True])
def test_idle_slots_with_entries_disturb_nothing(paged):
    """A released slot and a never-used slot keep entries with penalties: their windows run over
    whatever their history rows hold, clamped, and the live slots' ids are what they are
    without those entries."""
    heavy = SS(top_k=50, temperature=0.7, repetition_penalty=1.5, presence_penalty=1.0, frequency_penalty=0.5,
               penalty_last_n=4000, bias={0: NEG_INF})
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)

    def run(with_entries):
        b = eng.batch(4, 128, page_tokens=128 if paged else None)
        try:
            if with_entries:
                b.set_sampling(2, heavy)
                b.set_sampling(3, dataclasses.replace(heavy, top_k=1, penalty_start=100))
            ids = [b.prefill(0, _ids(51, 9), CALL), b.prefill(1, _ids(52, 14), CALL)]
            b.prefill(2, _ids(53, 30), CALL)
            b.decode_step(CALL)
            b.release(2)
            for _ in range(6):
                got = b.decode_step(CALL)
                ids += [got[0], got[1]]
            if with_entries:
                assert b.slot_sampling(2) is not None   # release left it alone
            return ids
        finally:
            b.close()

    try:
        assert run(True) == run(False)
    finally:
        eng.close()


# --------------------------------------------------------------------- 8. tensor parallel
def test_tensor_parallel_ranks_sample_the_gathered_row_alike(oracle):
    prompt = _ids(61, 9)
    entries = [SS(top_k=50, temperature=0.7, seed=5, repetition_penalty=1.3, frequency_penalty=0.4, bias={7: NEG_INF}),
               SS(top_k=1, presence_penalty=0.8)]

    def fn(rank, comm):
        eng = Q.Engine(SPEC, max_ctx=96, comm=comm).init_synthetic(SYN)
        b = eng.batch(2, 96)
        for s, e in enumerate(entries):
            b.set_sampling(s, e)
        trace = []
        for s in range(2):
            tok = b.prefill(s, prompt, CALL)
            trace.append((s, tok, len(prompt) - 1, 0, b.history(s, 96), b.logits()[s]))
        for step in range(1, 5):
            pos, hists = b.positions(), [b.history(s, 96) for s in range(2)]
            got = b.decode_step(CALL)
            lg = b.logits()
            trace += [(s, int(got[s]), int(pos[s]), step, hists[s], lg[s]) for s in range(2)]
        return trace

    res = run_ranks(2, fn)
    assert [t[1] for t in res[0]] == [t[1] for t in res[1]]
    for s, tok, q, step, hist, row in res[0]:
        w, _ = R.choose(oracle, row, entries[s], R.window_ids(entries[s], hist, q), step)
        assert tok == w, (s, step)


# ------------------------------------------------------------------------------ 9. batcher
@pytest.mark.parametrize("kw", [{"prefill_chunk": 8}, {"prefix_cache_pages": 4}],
                         ids=["chunked", "prefix-cache"])
def test_batcher_requests_sample_as_they_do_alone(kw):
    """Three requests with different entries share a batcher; each one's tokens are those of the
    same request served alone by a batcher of the same configuration.  With the prefix cache a
    primer request first leaves the shared 128-id prefix cached in either batcher, so the
    requests are admitted through it both times."""
    shared = _ids(71, 128)
    reqs = [(shared + _ids(72, 9), SS(top_k=50, temperature=0.7, seed=11, repetition_penalty=1.3), True),
            (shared + _ids(73, 21), SS(top_k=1, presence_penalty=0.7, frequency_penalty=0.2), False),
            (_ids(74, 17), SS(top_k=40, temperature=1.1, top_p=0.9, min_p=0.05, seed=3, bias={5: NEG_INF}), True),
            (_ids(75, 11), None, True)]
    eng = Q.Engine(SPEC, max_ctx=384).init_synthetic(SYN)

    def serve(which):
        cb = ContinuousBatcher(eng, slots=4, max_ctx=384, sampling=CALL, **kw)
        try:
            if "prefix_cache_pages" in kw:
                cb.submit(shared + [1, 2, 3], 1)
                cb.run()
            rids = [cb.submit(reqs[i][0], 6, sampling=reqs[i][1], penalize_prompt=reqs[i][2]) for i in which]
            cb.run()
            if "prefix_cache_pages" in kw:
                assert cb.prefix_hits >= sum(1 for i in which if i < 2)
            assert all(cb.batch.slot_sampling(s) is None for s in range(4))   # cleared at finish
            return [cb.requests[r].tokens for r in rids]
        finally:
            cb.close()

    try:
        together = serve([0, 1, 2, 3])
        for i in range(4):
            assert serve([i]) == [together[i]], i
    finally:
        eng.close()


# ------------------------------------------------------------------------ 10. bad arguments
def test_bad_entries_are_refused_and_change_nothing(qlib):
    eng = Q.Engine(SPEC, max_ctx=64).init_synthetic(SYN)
    b = eng.batch(2, 64)
    try:
        good = SS(top_k=50, temperature=0.7, min_p=0.1, repetition_penalty=1.3, bias={3: -1.0})
        b.set_sampling(1, good)
        kept = b.slot_sampling(1)
        nan, inf = float("nan"), float("inf")
        bad = [dict(bias={SPEC.vocab: 0.0}), dict(bias={-1: 0.0}), dict(bias={3: nan}), dict(bias={3: inf}),
               dict(temperature=nan), dict(temperature=inf), dict(repetition_penalty=inf), dict(presence_penalty=nan),
               dict(frequency_penalty=-inf), dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0),
               dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=nan), dict(penalty_start=-1), dict(penalty_last_n=-2)]
        structs = [dataclasses.replace(good, **kw).to_c() for kw in bad]
        for n_bias in (-1, 33):
            c = good.to_c()
            c.n_bias = n_bias
            structs.append(c)
        dup = good.to_c()
        dup.n_bias, dup.bias_ids[0], dup.bias_ids[1] = 2, 9, 9
        structs.append(dup)
        for i, c in enumerate(structs):
            assert qlib.qie_batch_set_slot_sampling(b.h, 1, C.byref(c)) == -22, i
            assert b.slot_sampling(1) == kept, i
        for seq in (-1, 2):
            c = good.to_c()
            assert qlib.qie_batch_set_slot_sampling(b.h, seq, C.byref(c)) == -22
            assert qlib.qie_batch_slot_sampling(b.h, seq, C.byref(c), None) == -22
        assert b.slot_sampling(0) is None and b.slot_sampling(1) == kept
    finally:
        b.close()
        eng.close()
