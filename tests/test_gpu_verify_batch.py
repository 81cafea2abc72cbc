"""GPU: qie_verify_batch — every slot's drafts verified in one pass — against the
CPU oracle teacher-forced on each slot's rows.

Bars are test_gpu_verify.py's: every logits row within logit_tol (4 bf16 ulps of max |logit|) of
the oracle, every emitted id the oracle's arg-max or a near tie within it, flips <=
parity.max_flips(decisions), the accept length exact from the engine's own outputs.  Drafts are
built as there: the oracle's greedy continuation for j tokens, then its ARG-MIN logit (never a
near tie), then random ids — so with no flip among a segment's rows its count is exactly j + 1.
Bit-exact checks compare two runs of the same kernels."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as G
import slot_sampling_ref as R
from conftest import rng
from parity import max_flips
from test_gpu_append import _check_logits
from test_gpu_engine import CONFIGS, SYN, logit_tol
from test_gpu_verify import MODE1_SPEC, MX_SPEC, _accept_len, _greedy, _teacher_forced_stream

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib, weights as W
from qwen_inference_engine_amd.engine import SlotSampling as SS
from qwen_inference_engine_amd.scheduler import ContinuousBatcher

pytestmark = pytest.mark.gpu

SPEC = CONFIGS["qwen2-bias-hd64"]
_ENGINES = {}


def engine(name="qwen2-bias-hd64", num="ref", max_ctx=128, **kw):
    key = (name, num, max_ctx, tuple(sorted(kw.items())))
    if key not in _ENGINES:
        _ENGINES[key] = Q.Engine(CONFIGS[name].with_numerics(num), max_ctx=max_ctx, **kw).init_synthetic(SYN)
    return _ENGINES[key]


def _ids(seed, n, spec=SPEC):
    return [int(t) for t in rng(seed).integers(0, spec.vocab, n)]


def _live(oracle, hw, b, plens, n_greedy, seed, max_ctx):
    """Prefills slot s with a prompt of plens[s] ids.  Returns (state per slot, flips): the oracle
    twin `om` holding rows [0, p), the position p, the current token (the oracle's: a near-tie of
    the engine's first token is counted and forced, as test_gpu_engine.forced_compare does), and
    the oracle's greedy continuation with the logits that chose it."""
    spec = b.e.spec
    st, flips = {}, 0
    for s, plen in plens.items():
        prompt = _ids(seed + 17 * s, plen, spec)
        c, cont, glg = _greedy(oracle, hw, max_ctx, prompt, n_greedy)
        om = oracle.Model(hw, max_ctx)
        lgp = om.forward(prompt, 0)
        tok = b.prefill(s, prompt)
        flips += _check_logits(oracle, b.logits()[s], lgp, tok, f"prefill slot {s}")
        if tok != c:
            b.set_position(s, plen, c)
        st[s] = dict(om=om, p=plen, cur=c, cont=cont, glg=glg, prompt=prompt)
    return st, flips


def _draft(spec, s, n, j, seed):
    """n drafts of which exactly the first j are the oracle's own choices."""
    d = list(s["cont"][:j])
    if j < n:
        d += [int(np.argmin(G.bf(s["glg"][j])))] + _ids(seed, n - j - 1, spec)
    assert len(d) == n
    return d


def _verify_batch_checked(oracle, b, table, st, what, sampling=Q.GREEDY):
    """b.verify_batch(table) with every segment checked as test_gpu_verify._verify_checked checks
    one: each logits row and emitted id against the oracle teacher-forced on that slot's rows,
    the accept length, position, history and the batch's logits row.  Advances st.  Returns
    (outs, flips per slot)."""
    lgs = {}
    for slot, draft in table:
        s = st[slot]
        lgs[slot] = [s["om"].forward([t], s["p"] + i) for i, t in enumerate([s["cur"]] + list(draft))]
    outs = b.verify_batch(table, sampling)
    vl = b.verify_logits()
    assert vl.shape == (sum(len(d) + 1 for _, d in table), b.e.spec.vocab) and len(outs) == len(table)
    pos, bl = b.positions(), b.logits()
    flips, r0 = {}, 0
    for (slot, draft), out in zip(table, outs):
        s, f = st[slot], 0
        p, cur = s["p"], s["cur"]
        for i, lg in enumerate(lgs[slot]):
            d = np.abs(G.bf(vl[r0 + i]).astype(np.float64) - G.bf(lg))
            assert d.max() <= logit_tol(lg), f"{what} slot {slot} row {i}: max |dlogit| {d.max()} > {logit_tol(lg)}"
        for i, t in enumerate(out):
            f += _check_logits(oracle, vl[r0 + i], lgs[slot][i], t, f"{what} slot {slot} row {i}")
        a = len(out) - 1
        assert 0 <= a <= len(draft) and a == _accept_len(draft, out), (what, slot, draft, out)
        assert a == len(draft) or draft[a] != out[a]
        assert int(pos[slot]) == p + a + 1, (what, slot)
        hist = b.history(slot, p + a + 2)
        assert int(hist[p]) == cur and [int(t) for t in hist[p + 1:]] == out, (what, slot, hist[p:], out)
        assert np.array_equal(bl[slot], vl[r0 + a]), f"{what} slot {slot}: batch logits row != step row {r0 + a}"
        flips[slot] = f
        s["p"], s["cur"] = p + a + 1, out[-1]
        r0 += len(draft) + 1
    return outs, flips


def _follow_all(oracle, b, st, slots, n_steps, what):
    """n_steps decode steps, every slot of `slots` checked with its oracle re-fed from its own
    position with the engine's tokens.  Returns the flips."""
    flips = 0
    lg = {s: st[s]["om"].forward([st[s]["cur"]], st[s]["p"]) for s in slots}
    for t in range(n_steps):
        ids, bl = b.decode_step(), b.logits()
        for s in slots:
            flips += _check_logits(oracle, bl[s], lg[s], ids[s], f"{what} slot {s} step {t}")
            st[s]["p"], st[s]["cur"] = st[s]["p"] + 1, ids[s]
            if t + 1 < n_steps:
                lg[s] = st[s]["om"].forward([ids[s]])
    return flips


# ---------------------------------------------------------------------- 1. the oracle, three tables
TABLES = {"3seg_0_7_6": {1: 0, 4: 7, 6: 6}, "8x1": {s: 1 for s in range(8)}, "2seg_0_14": {0: 0, 3: 14}}


@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("num", ["ref", "hf"])
@pytest.mark.parametrize("name", ["qwen2-bias-hd64", "qwen3-qknorm-hd128"])
def test_verify_batch_matches_oracle(oracle, name, num, table):
    """On a B = 8 batch.  The segments with drafts take turns accepting everything, rejecting
    the first draft and rejecting in the middle (variant v moves the turn on by one)."""
    eng = engine(name, num)
    spec = eng.spec
    hw = W.HostWeights.synthetic(spec, SYN)
    shape = TABLES[table]
    flips = decisions = 0
    for v in ((0,) if table == "8x1" else (0, 1, 2)):
        b = eng.batch(8, 128)
        st, f0 = _live(oracle, hw, b, {s: 12 + 3 * s for s in shape}, 15, 100, 128)
        tab, want, k = [], {}, v
        for s, n in shape.items():
            j = (n, 0, n // 2)[k % 3] if n else 0
            k += 1 if n else 0
            tab.append((s, _draft(spec, st[s], n, j, 7 * s + v)))
            want[s] = j + 1
        what = f"{name} {num} {table} v{v}"
        outs, fl = _verify_batch_checked(oracle, b, tab, st, what)
        for (s, _), out in zip(tab, outs):
            if fl[s] == 0:
                assert len(out) == want[s], (what, s, out)     # no near-tie among its rows: the reference's count
        f2 = _follow_all(oracle, b, st, list(shape), 4, what)
        flips += f0 + sum(fl.values()) + f2
        decisions += len(shape) + sum(len(o) for o in outs) + 4 * len(shape)
        b.close()
    assert flips <= max_flips(decisions), f"{flips} flips in {decisions} decisions"


# ------------------------------------------------------------------------------- 2. bystanders
def test_verify_batch_leaves_other_slots_alone():
    """Live slots outside the table keep position, history, logits row and — shown by sampled
    decode steps, which draw from seed + counter — their step counter, and then decode exactly
    like the slots of a twin batch on which the call was never made."""
    eng = engine()
    smp = Q.Sampling(top_k=40, temperature=0.8, top_p=0.9, seed=5)
    prompts = {s: _ids(200 + s, 10 + 4 * s) for s in range(4)}
    runs = []
    for do_verify in (True, False):
        b = eng.batch(4, 128)
        for s, pr in prompts.items():
            b.prefill(s, pr, smp)
        b.decode_step(smp)
        before = (b.positions().copy(), [b.history(s, 128).copy() for s in (1, 3)], b.logits()[[1, 3]].copy())
        if do_verify:
            outs = b.verify_batch([(0, _ids(210, 6)), (2, _ids(211, 8))], smp)
            assert all(len(o) >= 1 for o in outs)
            pos = b.positions()
            assert pos[1] == before[0][1] and pos[3] == before[0][3]
            assert pos[0] == before[0][0] + len(outs[0]) and pos[2] == before[0][2] + len(outs[1])
            for i, s in enumerate((1, 3)):
                assert np.array_equal(b.history(s, 128), before[1][i])
            assert np.array_equal(b.logits()[[1, 3]], before[2])
        got = []
        for _ in range(6):
            ids = b.decode_step(smp)
            got.append(([ids[1], ids[3]], b.logits()[[1, 3]].copy()))
        runs.append(got)
        b.close()
    for (t1, l1), (t2, l2) in zip(*runs):
        assert t1 == t2 and np.array_equal(l1, l2)


# ------------------------------------------------------------------ 3. one segment is qie_verify
@pytest.mark.parametrize("graph", [True, False])
def test_one_segment_equals_qie_verify(graph):
    """Twin batches, the same M: the same linear kernels and split length, and the ragged
    attention and post-projection are bit-equal to the single forms there."""
    eng = engine(use_graph=graph)
    prompts = {s: _ids(300 + s, 9 + 5 * s) for s in range(4)}
    got = []
    for batched in (True, False):
        b = eng.batch(4, 128)
        for s, pr in prompts.items():
            b.prefill(s, pr)
        res = []
        for slot, draft in [(2, _ids(310, 7)), (0, []), (3, _ids(311, 15)), (2, _ids(312, 3))]:
            out = b.verify_batch([(slot, draft)])[0] if batched else b.verify(slot, draft)
            res.append((out, b.verify_logits().copy(), b.positions().copy(), b.history(slot, 128).copy(),
                        b.logits().copy()))
        res.append(([int(t) for t in b.decode_step()], None, b.positions().copy(), None, b.logits().copy()))
        got.append(res)
        b.close()
    for x, y in zip(*got):
        assert x[0] == y[0]
        for u, w in zip(x[1:], y[1:]):
            assert (u is None and w is None) or np.array_equal(u, w)


# ------------------------------------------------------------------------------ 4. independence
def test_a_segment_does_not_depend_on_the_other_segments_ids():
    eng = engine()
    prompts = {s: _ids(400 + s, 8 + 3 * s) for s in range(8)}
    mine = _ids(410, 5)
    got = []
    for seed in (420, 430):
        b = eng.batch(8, 128)
        for s, pr in prompts.items():
            b.prefill(s, pr)
        outs = b.verify_batch([(1, _ids(seed, 4)), (4, mine), (6, _ids(seed + 1, 4))])
        got.append((outs[1], b.verify_logits()[5:11].copy(), b.logits()[4].copy(), outs[0], outs[2]))
        b.close()
    assert got[0][0] == got[1][0]
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][2], got[1][2])


# --------------------------------------------------------------------------------------- 5. paged
def _paged_setup(oracle, n_pages=0):
    eng = engine(max_ctx=256)
    hw = W.HostWeights.synthetic(SPEC, SYN)
    b = eng.batch(2, 256, page_tokens=128, n_pages=n_pages)
    st, f0 = _live(oracle, hw, b, {0: 120, 1: 20}, 15, 500, 256)
    d0 = _draft(SPEC, st[0], 10, 2, 501)     # rows 120 .. 130: the third draft wrong
    d1 = _draft(SPEC, st[1], 4, 4, 502)      # rows 20 .. 24; 16 rows together
    return eng, b, st, f0, [(0, d0), (1, d1)]


def test_verify_batch_paged_takes_and_keeps_the_second_page(oracle):
    eng, b, st, flips, tab = _paged_setup(oracle)
    assert b.page_stats()[1].tolist() == [1, 1]
    first = [int(b.block_table(s, 1)[0]) for s in (0, 1)]
    free = b.page_stats()[0]
    outs, fl = _verify_batch_checked(oracle, b, tab, st, "paged")
    if fl[0] == 0:
        assert len(outs[0]) == 3
    if fl[1] == 0:
        assert len(outs[1]) == 5
    # the page taken for rows 128 .. 130 stays with slot 0 although they were rejected
    assert b.page_stats()[1].tolist() == [2, 1] and b.page_stats()[0] == free - 1
    assert [int(b.block_table(s, 1)[0]) for s in (0, 1)] == first
    flips += sum(fl.values()) + _follow_all(oracle, b, st, [0, 1], 6, "paged")
    assert b.page_stats()[1].tolist() == [2, 1]
    assert flips <= max_flips(2 + sum(len(o) for o in outs) + 12)
    b.close()


def test_verify_batch_pool_exhausted_leaves_every_slot_intact(oracle):
    """A pool one page short (scratch + one page per slot): -28 with nothing launched; page
    accounting, positions and the following decode steps of both slots are an untouched twin's."""
    runs = []
    for attempt in (False, True):
        eng, b, st, _, tab = _paged_setup(oracle, n_pages=3)
        stats = b.page_stats()
        if attempt:
            with pytest.raises(_lib.QieError) as ex:
                b.verify_batch(tab)
            assert "rc=-28" in str(ex.value) and "qie_verify_batch" in str(ex.value)
        now = b.page_stats()
        assert now[0] == stats[0] == 0 and now[1].tolist() == stats[1].tolist()
        assert b.positions().tolist() == [120, 20]
        runs.append([(b.decode_step(), b.logits().copy()) for _ in range(7)])   # rows 120 .. 126: no new page
        b.close()
    for (t1, l1), (t2, l2) in zip(*runs):
        assert t1 == t2 and np.array_equal(l1, l2)


def test_verify_batch_copies_a_shared_page_of_its_write_range():
    """Slot 1 is a fork of slot 0 at 280 (pages 0 and 1 shared), rewound to 120: set_position
    gave it page 0 of its own, page 1 is still shared — and rows 120 .. 135 of the step reach into
    it.  The step's reservation gives slot 1 a private page there; the source's rows do not move."""
    eng = engine(max_ctx=320)
    b = eng.batch(2, 320, page_tokens=128)
    prompt = _ids(600, 280)
    b.prefill(0, prompt)
    b.fork(0, 1)
    b.set_position(1, 120, prompt[120])
    L = SPEC.n_layers
    snap = [b.kv_rows(0, l, 280) for l in range(L)]
    old0, old1 = b.block_table(0, 3).tolist(), b.block_table(1, 3).tolist()
    assert old1[1] == old0[1] and old1[0] != old0[0] and b.page_refs()[old0[1]] == 2
    free = b.page_stats()[0]
    twin = eng.batch(2, 320, page_tokens=128)          # the same rows on pages nobody shares
    twin.prefill(1, prompt)
    twin.set_position(1, 120, prompt[120])
    draft = _ids(601, 15)
    outs = b.verify_batch([(1, draft)])
    want = twin.verify_batch([(1, draft)])
    assert outs == want and np.array_equal(b.verify_logits(), twin.verify_logits())
    new1 = b.block_table(1, 3).tolist()
    assert new1[0] == old1[0] and new1[1] not in (0, old1[1]) and b.block_table(0, 3).tolist() == old0
    refs = b.page_refs()
    assert refs[old0[1]] == 1 and refs[new1[1]] == 1 and b.page_stats()[0] == free - 1
    for l in range(L):
        k, v = b.kv_rows(0, l, 280)
        assert np.array_equal(k, snap[l][0]) and np.array_equal(v, snap[l][1]), l
    b.close()
    twin.close()


# ------------------------------------------------------------------------------ 6. split boundary
def test_verify_batch_across_a_split_boundary(oracle):
    """max_ctx 320 takes two 256-key attention splits for a call of 16 rows: slot 0's rows at
    positions 250 .. 260 straddle key 256, slot 1's (30 .. 34) lie in the first split."""
    spec = CONFIGS["tied-g7"]
    assert _lib.load().qie_attention_extend_split_tokens(16, 320) == 256
    eng = engine("tied-g7", max_ctx=320)
    hw = W.HostWeights.synthetic(spec, SYN)
    b = eng.batch(2, 320)
    st, flips = _live(oracle, hw, b, {0: 250, 1: 30}, 10, 700, 320)
    tab = [(0, _draft(spec, st[0], 10, 10, 701)), (1, _draft(spec, st[1], 4, 2, 702))]
    assert sum(len(d) + 1 for _, d in tab) == 16
    outs, fl = _verify_batch_checked(oracle, b, tab, st, "split boundary")
    if fl[0] == 0:
        assert len(outs[0]) == 11
    if fl[1] == 0:
        assert len(outs[1]) == 3
    flips += sum(fl.values()) + _follow_all(oracle, b, st, [0, 1], 3, "split boundary")
    assert flips <= max_flips(2 + sum(len(o) for o in outs) + 6)
    b.close()


# -------------------------------------------------------------------------- 7. per-slot sampling
CALL = Q.Sampling(top_k=40, temperature=0.8, top_p=0.9, seed=99)


def _as_entry(s):
    return SS(top_k=s.top_k, temperature=s.temperature, top_p=s.top_p, seed=s.seed)


@pytest.mark.parametrize("kind", ["greedy", "sampled"])
def test_verify_batch_rows_sample_under_their_own_slots_entry(oracle, kind):
    """Slot 3 (the SECOND segment: its drafts do not begin the draft array) has an entry whose
    penalties boost what the window holds, so a row's choice depends on the drafts before it,
    and a -inf bias; slot 1 has none and samples under the call's sampling.  Every row's id is the
    reference (tests/slot_sampling_ref.py) on the step's own logits row, that slot's history and
    that segment's drafts; qie_verify slot by slot on a twin batch meets the same reference on
    its own rows.  The drafts are found one round at a time: a row's logits depend on the rows
    before it only, so a longer right prefix repeats the draws."""
    eng = engine()
    call = Q.GREEDY if kind == "greedy" else CALL
    prompts = {1: _ids(800, 14), 3: _ids(801, 11)}
    prompts[3][5] = prompts[3][2]
    ban = 123
    entry = SS(top_k=1 if kind == "greedy" else 40, temperature=0.8, top_p=0.95, seed=7, repetition_penalty=1.3,
               presence_penalty=-6.0, frequency_penalty=-1.0, bias={ban: float("-inf")})
    entries = {1: None, 3: entry}
    N = {1: 4, 3: 6}
    live = []

    def fresh():
        b = eng.batch(4, 128)
        live.append(b)
        b.set_sampling(3, entry)
        for s, pr in prompts.items():
            b.prefill(s, pr, call)
        return b

    def reference(b_hist, vl, r0, slot, draft, n_rows):
        e = entries[slot] if entries[slot] is not None else _as_entry(call)
        p = len(prompts[slot])
        ids = []
        for i in range(n_rows):
            w, _ = R.choose(oracle, vl[r0 + i], e, R.window_ids(e, b_hist[slot], p + i, draft[:i]), 1 + i)
            ids.append(max(w, 0))
        return ids

    try:
        good = {1: [], 3: []}
        junk = {s: _ids(810 + s, N[s]) for s in N}
        for _ in range(max(N.values())):
            out = fresh().verify_batch([(s, good[s] + junk[s][len(good[s]):]) for s in (1, 3)], call)
            for s, o in zip((1, 3), out):
                assert o[:len(good[s])] == good[s][:len(o)]
                if len(good[s]) < N[s]:
                    good[s].append(o[len(good[s])])
        b = fresh()
        hist = {s: b.history(s, 128) for s in (1, 3)}
        # the last draft of each segment spoiled: every row before it is emitted
        tab = [(s, good[s][:-1] + [(good[s][-1] + 1) % SPEC.vocab]) for s in (1, 3)]
        outs = b.verify_batch(tab, call)
        vl = b.verify_logits()
        assert [len(o) for o in outs] == [N[1], N[3]] and outs[0] == good[1] and outs[1] == good[3]
        r0 = 0
        for (s, d), o in zip(tab, outs):
            assert o == reference(hist, vl, r0, s, d, len(o)), (kind, s)
            r0 += len(d) + 1
        assert ban not in outs[1]
        # qie_verify, slot by slot, on a twin: the same reference on its own rows
        t = fresh()
        for s, d in tab:
            o = t.verify(s, d, call)
            assert o == reference(hist, t.verify_logits(), 0, s, d, len(o)), (kind, s, "single")
        # the next decode step continues each slot's counter: 1 + rows emitted
        pos = b.positions()
        hist = {s: b.history(s, 128) for s in (1, 3)}
        ids, bl = b.decode_step(call), b.logits()
        for s in (1, 3):
            e = entries[s] if entries[s] is not None else _as_entry(call)
            w, _ = R.choose(oracle, bl[s], e, R.window_ids(e, hist[s], int(pos[s])), 1 + N[s])
            assert ids[s] == max(w, 0), (kind, s, "decode")
    finally:
        for x in live:
            x.close()


# -------------------------------------------------------------------------- 8. graph replay == eager
def test_verify_batch_graph_equals_eager_and_replays():
    prompts = {s: _ids(900 + s, 10 + 2 * s) for s in range(8)}
    shape = [(0, 3), (2, 5), (5, 0), (7, 4)]
    runs = {}
    for graph in (True, False):
        eng = engine(use_graph=graph)
        b = eng.batch(8, 128)
        for s, pr in prompts.items():
            b.prefill(s, pr)
        twin = eng.batch(8, 128)
        for s, pr in prompts.items():
            twin.prefill(s, pr)
        cont = twin.decode(24)                                # drafts: what plain steps emit, one spoiled
        twin.close()
        got = []
        at = {s: 0 for s, _ in shape}
        for call in range(3):                                    # the same table, different drafts: replays
            tab = []
            for s, n in shape:
                d = [int(t) for t in cont[at[s]:at[s] + n, s]]
                if n and (s + call) % 2:
                    d[n // 2] = (d[n // 2] + 1) % SPEC.vocab
                tab.append((s, d))
            outs = b.verify_batch(tab)
            # the first call captures the table's step, the later ones replay it: no re-capture
            assert b.verify_captures() == (1 if graph else 0), (graph, call)
            for (s, d), o in zip(tab, outs):
                assert len(o) - 1 == _accept_len(d, o)
                at[s] += len(o)
            got.append((outs, b.verify_logits().copy(), b.logits().copy(), b.positions().copy()))
        got.append((b.decode_step(), None, b.logits().copy(), b.positions().copy()))
        runs[graph] = got
        b.close()
    for (oa, va, la, pa), (ob, vb, lb, pb) in zip(runs[True], runs[False]):
        assert oa == ob and np.array_equal(la, lb) and np.array_equal(pa, pb)
        assert (va is None and vb is None) or np.array_equal(va, vb)


def test_verify_batch_graph_keys_the_calls_sampling_for_slots_without_an_entry(oracle):
    """A table that mixes a slot with an entry (2) and slots without (0, 5): the rows of the
    latter sample under the CALL's sampling, which a captured step holds by value.  The same table
    under two samplings and then greedy, on one batch: graph == eager bit for bit, every id of a
    slot without an entry is the reference on its own logits row under THAT call's sampling, each
    new sampling captures once and a repeated one replays.  With an entry on every slot of the
    table the call's sampling is not part of the step: another sampling replays."""
    prompts = {s: _ids(950 + s, 9 + s) for s in (0, 2, 5)}
    entry = SS(top_k=30, temperature=0.9, top_p=0.95, seed=3, repetition_penalty=1.2)
    calls = [Q.Sampling(top_k=40, temperature=0.8, top_p=0.9, seed=99), Q.Sampling(top_k=20, temperature=1.3, top_p=1.0, seed=7),
             Q.Sampling(top_k=40, temperature=0.8, top_p=0.9, seed=99), Q.GREEDY]
    want_captures = [1, 2, 2, 3]
    runs = {}
    for graph in (True, False):
        eng = engine(use_graph=graph)
        b = eng.batch(8, 128)
        b.set_sampling(2, entry)
        for s, pr in prompts.items():
            b.prefill(s, pr, calls[0])
        got, steps = [], {s: 1 for s in prompts}
        for i, call in enumerate(calls):
            pos = b.positions().copy()
            hist = {s: b.history(s, 128) for s in prompts}
            tab = [(s, _ids(960 + 10 * i + s, 3)) for s in prompts]      # random drafts: (nearly) all rejected
            outs = b.verify_batch(tab, call)
            vl = b.verify_logits()
            assert b.verify_captures() == (want_captures[i] if graph else 0), (graph, i)
            for z, ((s, d), o) in enumerate(zip(tab, outs)):
                if s == 2:
                    continue
                for j, t in enumerate(o):                                  # (steps: 1 after the prefill, + rows emitted)
                    e = _as_entry(call)
                    w, _ = R.choose(oracle, vl[4 * z + j], e, R.window_ids(e, hist[s], int(pos[s]) + j, d[:j]),
                                    steps[s] + j)
                    assert t == max(w, 0), (graph, i, s, j)
            for (s, _), o in zip(tab, outs):
                steps[s] += len(o)
            got.append((outs, vl.copy(), b.logits().copy()))
        if graph:                                                          # every slot of the table has an entry
            b.set_sampling(0, entry)
            b.set_sampling(5, entry)
            n0 = b.verify_captures()
            b.verify_batch([(s, []) for s in prompts], calls[0])
            b.verify_batch([(s, []) for s in prompts], calls[1])
            assert b.verify_captures() == n0 + 1
        runs[graph] = got
        b.close()
    for (oa, va, la), (ob, vb, lb) in zip(runs[True], runs[False]):
        assert oa == ob and np.array_equal(va, vb) and np.array_equal(la, lb)


# ------------------------------------------------------------------------------ 9. the exchange path
def test_verify_batch_comm_always(oracle):
    hw = W.HostWeights.synthetic(SPEC, SYN)
    comm = Q.Comm.rccl(Q.Comm.unique_id(), 1, 0, 0)
    eng = Q.Engine(SPEC, max_ctx=128, comm=comm, comm_always=True).init_synthetic(SYN)
    b = eng.batch(4, 128)
    try:
        st, flips = _live(oracle, hw, b, {0: 14, 1: 9, 3: 21}, 8, 1000, 128)
        tab = [(0, _draft(SPEC, st[0], 6, 6, 1001)), (1, _draft(SPEC, st[1], 3, 0, 1002)),
               (3, _draft(SPEC, st[3], 4, 2, 1003))]
        outs, fl = _verify_batch_checked(oracle, b, tab, st, "comm_always")
        for (s, _), o, n in zip(tab, outs, (7, 1, 3)):
            if fl[s] == 0:
                assert len(o) == n
        flips += sum(fl.values()) + _follow_all(oracle, b, st, [0, 1, 3], 4, "comm_always")
        assert flips <= max_flips(3 + sum(len(o) for o in outs) + 12)
    finally:
        b.close()
        eng.close()
        comm.close()


# -------------------------------------------------------------------------------- 10. -22 cases
@pytest.mark.parametrize("case", ["seventeen_rows", "repeated_slot", "decreasing_slots", "idle_slot", "id_is_vocab",
                                  "reaches_max_ctx", "no_segments", "decode_mode_1", "prefill_fp8"])
def test_verify_batch_bad_arguments(case):
    """-22 before anything is launched; every live slot then decodes as an untouched twin's."""
    spec, kw, B = SPEC, {}, 4
    if case == "prefill_fp8":
        spec, kw = MX_SPEC, dict(weight_fp8=True, prefill_fp8=True)
    elif case == "decode_mode_1":
        spec, B = MODE1_SPEC, 1
    eng = Q.Engine(spec, max_ctx=64, **kw).init_synthetic(SYN)
    live = [0] if B == 1 else [0, 1, 2]

    def start():
        x = eng.batch(B, 64)
        for s in live:
            x.prefill(s, _ids(1100 + s, 8 + s, spec))
        if case == "decode_mode_1":
            x.set_decode_mode(1)
        if case == "reaches_max_ctx":
            x.set_position(1, 58, 3)                              # 58 + 5 + 1 = max_ctx
        return x

    twin = start()
    want = [(twin.decode_step(), twin.logits().copy()) for _ in range(4)]
    twin.close()
    b = start()
    d = lambda seed, n: _ids(seed, n, spec)
    tab, word = [(0, d(1, 4)), (1, d(2, 3))], "qie_verify_batch"
    if case == "seventeen_rows":
        tab, word = [(0, d(1, 7)), (1, d(2, 4)), (2, d(3, 3))], "exceed the 16 rows"
    elif case == "repeated_slot":
        tab, word = [(0, d(1, 2)), (1, d(2, 2)), (1, d(3, 2))], "strictly increasing"
    elif case == "decreasing_slots":
        tab, word = [(2, d(1, 2)), (0, d(2, 2))], "strictly increasing"
    elif case == "idle_slot":
        tab, word = [(0, d(1, 2)), (3, d(2, 2))], "no live sequence"
    elif case == "id_is_vocab":
        tab, word = [(0, d(1, 4)), (2, d(2, 2) + [spec.vocab])], "out of range"
    elif case == "reaches_max_ctx":
        tab, word = [(0, d(1, 4)), (1, d(2, 5))], "max_ctx"
    elif case == "decode_mode_1":
        tab, word = [(0, d(1, 4))], "decode mode 1"
    elif case == "prefill_fp8":
        word = "prefill_fp8"
    pos = b.positions().copy()
    if case == "no_segments":
        seg = (_lib.VerifySegC * 8)(*[_lib.VerifySegC(s, 0) for s in range(8)])
        out, n = (C.c_int32 * 4)(), (C.c_int32 * 1)()
        assert b.lib.qie_verify_batch(b.h, seg, 0, None, None, out, n) == -22
        assert b.lib.qie_verify_batch(b.h, seg, B + 1, None, None, out, n) == -22
    else:
        with pytest.raises(_lib.QieError) as ex:
            b.verify_batch(tab)
        assert "rc=-22" in str(ex.value) and word in str(ex.value), str(ex.value)
    assert np.array_equal(b.positions(), pos)
    for t, lg in want:
        assert b.decode_step() == t and np.array_equal(b.logits(), lg)
    b.close()
    eng.close()


# ------------------------------------------------------------------------------ 11. verify_logprobs
def _log_softmax64(rows):
    l = G.bf(rows).astype(np.float64)
    m = l.max(axis=-1, keepdims=True)
    return l - m - np.log(np.exp(l - m).sum(axis=-1, keepdims=True))


@pytest.mark.parametrize("mode", ["plain", "comm_always"])
def test_verify_logprobs_equal_float64_on_the_steps_rows(mode):
    """qie_logprob_rows on GIVEN logits: 1e-4 absolute of float64 (test_gpu_score.py's bar for
    it); -1 gives exactly 0.0.  After verify_batch and after verify."""
    comm = Q.Comm.rccl(Q.Comm.unique_id(), 1, 0, 0) if mode == "comm_always" else None
    eng = Q.Engine(SPEC, max_ctx=128, comm=comm, comm_always=comm is not None).init_synthetic(SYN)
    b = eng.batch(4, 128)
    try:
        for s in range(3):
            b.prefill(s, _ids(1200 + s, 10 + s))
        with pytest.raises(_lib.QieError):
            b.verify_logprobs([])                                  # no verify step's rows yet
        b.verify_batch([(0, _ids(1210, 5)), (2, _ids(1211, 7))])
        vl = b.verify_logits()
        ids = _ids(1212, 14)
        ids[3] = ids[9] = -1
        ids[0] = int(np.argmax(G.bf(vl[0])))
        lp = b.verify_logprobs(ids)
        want = _log_softmax64(vl)
        assert lp.shape == (14,) and lp.dtype == np.float32
        for m, t in enumerate(ids):
            if t < 0:
                assert lp[m] == 0.0
            else:
                assert abs(float(lp[m]) - want[m, t]) <= 1e-4, (m, t, lp[m], want[m, t])
        with pytest.raises(ValueError):
            b.verify_logprobs(ids[:5])
        with pytest.raises(_lib.QieError) as ex:
            b.verify_logprobs(ids[:13] + [SPEC.vocab])
        assert "rc=-22" in str(ex.value)
        b.verify(1, _ids(1213, 3))
        vl = b.verify_logits()
        ids = [5, -1, 77, 900]
        lp = b.verify_logprobs(ids)
        want = _log_softmax64(vl)
        assert lp[1] == 0.0 and all(abs(float(lp[m]) - want[m, ids[m]]) <= 1e-4 for m in (0, 2, 3))
    finally:
        b.close()
        eng.close()
        if comm is not None:
            comm.close()


# ------------------------------------------------------------------------------ 12. the batcher
def test_batcher_with_a_drafter_end_to_end(oracle):
    """Three requests of different lengths on prompts that repeat themselves, NgramDrafter.
    Every stream is the oracle's teacher-forced (flips bar), kept log-probabilities are those of
    the kept logit rows, something was accepted, and every page is back at the end."""
    eng = engine()
    hw = W.HostWeights.synthetic(SPEC, SYN)
    cb = ContinuousBatcher(eng, slots=4, max_ctx=128, page_tokens=128, drafter=Q.NgramDrafter(), draft_tokens=4,
                             keep_logits=True, keep_logprobs=True)
    free0 = cb.batch.page_stats()[0]
    reqs = [(_ids(1300, 6) * 4, 70), (_ids(1301, 4) * 5, 45), (_ids(1302, 9) * 2, 90)]
    rids = [cb.submit(p, n) for p, n in reqs]
    out = cb.run()
    flips = decisions = 0
    for rid, (p, n) in zip(rids, reqs):
        r = cb.requests[rid]
        assert len(out[rid]) == n == len(r.logits) == len(r.logprobs)
        flips += _teacher_forced_stream(oracle, hw, 128, p, out[rid], f"request {rid}")
        decisions += n
        want = _log_softmax64(np.stack(r.logits))
        for i, t in enumerate(out[rid]):
            assert abs(r.logprobs[i] - want[i, t]) <= 1e-4, (rid, i)
            assert t == int(np.argmax(G.bf(r.logits[i]))) or G.bf(r.logits[i])[t] == G.bf(r.logits[i]).max()
    assert flips <= max_flips(decisions), f"{flips} flips in {decisions} decisions"
    st = cb.stats
    assert st["verify_calls"] > 0 and 0 < st["accepted"] <= st["drafted"], st
    assert st["emitted"] == sum(n for _, n in reqs)
    assert cb.batch.page_stats()[0] == free0 and not cb.batch.page_refs().any()
    cb.close()
