"""CPU: the host side of batched speculative decoding — qie_verify_batch and
qie_verify_logprobs are declared, exported and bound and refuse a null batch without a GPU; the
row-dealing policy (draft_cap, deal_verify_rows); and ContinuousBatcher with a drafter over a
stand-in for a Batch whose "model" is a fixed token function: the streams are those of the same
batcher without a drafter, stop ids and max_new_tokens are honoured exactly, the stats add up."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

from qwen_inference_engine_amd import _lib
from qwen_inference_engine_amd.engine import verify_segments
from qwen_inference_engine_amd.scheduler import (VERIFY_MAX_ROWS, VERIFY_MAX_SEGS, ContinuousBatcher, deal_verify_rows,
                                                 draft_cap)
from qwen_inference_engine_amd.speculative import NgramDrafter

NEW = {"qie_verify_batch", "qie_verify_logprobs", "qie_batch_debug_verify_captures"}


# ------------------------------------------------------------------------------------- the ABI
def test_header_declares_and_library_exports_the_batched_step(qlib):
    text = open(os.path.join(ROOT, "include", "qie", "qie_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"^int\s+%s\s*\(" % name, code, flags=re.M), name
    assert re.search(r"typedef\s+struct\s+qie_verify_seg\s*\{\s*int32_t\s+seq\s*,\s*n_draft\s*;\s*\}", code)
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert NEW | {"qie_sample_rows_mapped"} <= exported
    assert NEW | {"qie_sample_rows_mapped"} <= {n for n, _, _ in _lib.SIGNATURES}
    assert C.sizeof(_lib.VerifySegC) == 8
    assert (VERIFY_MAX_ROWS, VERIFY_MAX_SEGS) == (_lib.QIE_VERIFY_MAX_ROWS, _lib.QIE_RAGGED_MAX_SEGS)


def test_null_batch_is_refused_without_a_gpu(qlib):
    seg = (_lib.VerifySegC * 1)(_lib.VerifySegC(0, 0))
    out, n = (C.c_int32 * 4)(), (C.c_int32 * 1)(7)
    assert qlib.qie_verify_batch(None, seg, 1, None, None, out, n) == -22
    assert b"qie_verify_batch" in qlib.qie_last_error()
    assert n[0] == 7
    lp = (C.c_float * 1)(3.0)
    assert qlib.qie_verify_logprobs(None, out, lp) == -22
    assert b"qie_verify_logprobs" in qlib.qie_last_error()
    assert lp[0] == 3.0
    assert qlib.qie_sample_rows_mapped(None, None, None, None) == -22
    assert qlib.qie_batch_debug_verify_captures(None) == -22


def test_verify_segments_shapes():
    assert verify_segments([(1, [3, 4]), (5, ())]) == [(1, [3, 4]), (5, [])]
    with pytest.raises(ValueError):
        verify_segments([])
    with pytest.raises(ValueError):
        verify_segments([(1, [2], 3)])


# ------------------------------------------------------------------------------------ the policy
def test_draft_cap():
    # min(draft_tokens, max_new_tokens - emitted - 1, context room), never negative
    assert draft_cap(4, 100, 1, 10, 1000) == 4
    assert draft_cap(4, 10, 7, 10, 1000) == 2          # 2 drafts + the bonus token fill the budget
    assert draft_cap(4, 10, 9, 10, 1000) == 0          # the last token: its one row only
    assert draft_cap(4, 10, 10, 10, 1000) == 0
    assert draft_cap(15, 100, 1, 120, 128) == 6        # 120 + 6 + 1 < 128
    assert draft_cap(15, 100, 1, 126, 128) == 0 and draft_cap(15, 100, 1, 127, 128) == 0
    assert draft_cap(0, 100, 1, 10, 1000) == 0


def _rows(table):
    return sum(len(d) + 1 for _, d in table)


def test_deal_no_drafts_is_the_plain_step():
    assert deal_verify_rows([]) == []
    assert deal_verify_rows([(0, []), (3, []), (4, [])]) == []


def test_deal_everything_fits():
    prop = [(1, [10, 11]), (4, []), (6, [20, 21, 22])]
    assert deal_verify_rows(prop) == [(1, [10, 11]), (4, []), (6, [20, 21, 22])]


def test_deal_round_robin_in_slot_order():
    # three segments: 13 spare rows, dealt one at a time 0, 2, 5, 0, 2, 5, ... ; slot 2 runs out at 2
    prop = [(0, list(range(100, 115))), (2, [7, 8]), (5, list(range(200, 215)))]
    table = deal_verify_rows(prop)
    assert [s for s, _ in table] == [0, 2, 5]
    assert [len(d) for _, d in table] == [6, 2, 5]
    assert _rows(table) == 16
    assert all(d == dict(prop)[s][:len(d)] for s, d in table)   # a prefix of the proposal, in order
    # eight slots with four ids each: 8 spare rows, one each
    prop = [(s, [s * 10 + i for i in range(4)]) for s in range(8)]
    table = deal_verify_rows(prop)
    assert [d for _, d in table] == [[s * 10] for s in range(8)] and _rows(table) == 16
    # one spare row short of a full round: the first slots in order get it
    prop = [(s, [1, 2, 3]) for s in range(6)]
    table = deal_verify_rows(prop)
    assert [len(d) for _, d in table] == [2, 2, 2, 2, 1, 1] and _rows(table) == 16


def test_deal_never_exceeds_rows_or_segments():
    for n_slots in range(1, VERIFY_MAX_SEGS + 1):
        for k in (0, 1, 4, 15):
            prop = [(2 * s, list(range(k if s % 3 else 15))) for s in range(n_slots)]
            table = deal_verify_rows(prop)
            assert [s for s, _ in table] == [2 * s for s in range(n_slots)]   # every slot once, in order
            assert _rows(table) <= VERIFY_MAX_ROWS and all(len(d) <= 15 for _, d in table)
            assert _rows(table) == min(16, n_slots + sum(len(d) for _, d in prop))   # no spare row left idle
    with pytest.raises(ValueError):                            # a batch has at most 8 slots
        deal_verify_rows([(s, [1]) for s in range(VERIFY_MAX_SEGS + 1)])


# ------------------------------------------------------------------- the batcher over a fake batch
VOCAB = 64


def model(prev):
    """The fake model: the token after `prev` (a permutation with cycles, so streams repeat)."""
    return (prev * 5 + 3) % 17


class _Spec:
    vocab = VOCAB


class FakeBatch:
    def __init__(self, B, max_ctx, page_tokens=16, n_pages=64):
        self.e = type("E", (), {"spec": _Spec()})()
        self.B, self.max_ctx, self.page_tokens, self.free0 = B, max_ctx, page_tokens, n_pages
        self.cur = [None] * B
        self.pos = [0] * B
        self.calls = []          # ("decode",) / ("verify", table) / ("prefill", slot) / ...

    def page_stats(self):
        return self.free0, [0] * self.B, self.page_tokens

    def prefill(self, slot, ids, sampling=None):
        self.calls.append(("prefill", slot))
        self.cur[slot], self.pos[slot] = model(ids[-1]), len(ids)
        return self.cur[slot]

    def prefill_batch(self, seq0, prompts, sampling=None):
        return [self.prefill(seq0 + i, p) for i, p in enumerate(prompts)]

    def append(self, slot, ids, pos0, sampling=None):
        self.calls.append(("append", slot))
        self.cur[slot], self.pos[slot] = model(ids[-1]), pos0 + len(ids)
        return self.cur[slot]

    def decode_step(self, sampling=None):
        self.calls.append(("decode",))
        out = [0] * self.B
        for s in range(self.B):
            if self.cur[s] is not None:
                self.cur[s] = out[s] = model(self.cur[s])
                self.pos[s] += 1
        return out

    def verify_batch(self, items, sampling=None):
        items = [(s, list(d)) for s, d in items]
        self.calls.append(("verify", items))
        assert 1 <= len(items) <= 8 and sum(len(d) + 1 for _, d in items) <= 16
        assert all(a[0] < b[0] for a, b in zip(items, items[1:]))
        res = []
        for s, d in items:
            assert self.cur[s] is not None and self.pos[s] + len(d) + 1 < self.max_ctx
            assert all(0 <= t < VOCAB for t in d)
            out = [model(self.cur[s])]
            for t in d:
                if t != out[-1]:
                    break
                out.append(model(out[-1]))
            self.cur[s] = out[-1]
            self.pos[s] += len(out)
            res.append(out)
        return res

    def release(self, slot):
        self.calls.append(("release", slot))
        self.cur[slot] = None

    def set_sampling(self, slot, e):
        pass

    def close(self):
        pass


class FakeEngine:
    def __init__(self):
        self.batches = []

    def batch(self, slots, max_ctx, page_tokens=16, n_pages=0):
        self.batches.append(FakeBatch(slots, max_ctx or 256, page_tokens))
        return self.batches[-1]


PROMPTS = [[1, 2, 3], [9, 4], [5, 5, 5, 6], [2], [11, 12, 13, 14, 15], [7, 0], [3, 3], [8], [16, 1], [4, 10]]


def _serve(drafter, reqs, slots=4, draft_tokens=4, **kw):
    eng = FakeEngine()
    cb = ContinuousBatcher(eng, slots=slots, max_ctx=256, page_tokens=16, drafter=drafter, draft_tokens=draft_tokens,
                           **kw)
    rids = [cb.submit(p, n, stop_ids=stop) for p, n, stop in reqs]
    order = []
    while not cb.idle():
        order.append(cb.step())
    return cb, eng.batches[0], {r: cb.requests[r].tokens for r in rids}, order


def _chain(prompt, n, stop=()):
    out, t = [], prompt[-1]
    for _ in range(n):
        t = model(t)
        out.append(t)
        if t in stop:
            break
    return out


REQS = [(p, n, ()) for p, n in zip(PROMPTS, [30, 7, 19, 1, 12, 40, 2, 25, 9, 16])]


@pytest.mark.parametrize("slots", [1, 4, 8])
def test_batcher_streams_equal_the_streams_without_a_drafter(slots):
    plain_cb, plain_b, plain, _ = _serve(None, REQS, slots=slots)
    assert not any(c[0] == "verify" for c in plain_b.calls)
    assert plain_cb.stats["verify_calls"] == 0
    for dr in (NgramDrafter(), NgramDrafter):            # one shared object, and a factory per request
        cb, b, got, order = _serve(dr, REQS, slots=slots)
        assert got == plain
        for rid, (p, n, _) in enumerate(REQS):
            assert got[rid] == _chain(p, n)                # never over-emits
        st = cb.stats
        tables = [c[1] for c in b.calls if c[0] == "verify"]
        assert st["verify_calls"] == len(tables) > 0
        assert st["drafted"] == sum(len(d) for t in tables for _, d in t)
        assert 0 < st["accepted"] <= st["drafted"]
        assert st["emitted"] == sum(len(t) for t in got.values()) == sum(len(s) for s in order)
        # the weight passes: fewer than without a drafter (the model repeats itself, lookups hit)
        passes = lambda calls: sum(1 for c in calls if c[0] in ("decode", "verify"))
        assert passes(b.calls) < passes(plain_b.calls)
        if dr is NgramDrafter:
            assert cb._drafters == {}                      # dropped with their requests


def test_batcher_emits_in_slot_order_each_slots_tokens_in_order():
    cb, b, got, order = _serve(NgramDrafter(), REQS[:4], slots=4)
    assert len(order) > 2
    for step in order[1:]:                                 # (the first step also emits the prefills' tokens)
        rids = [rid for rid, _ in step]
        assert rids == sorted(rids)                        # (rid == slot here: four requests, four slots)
    for rid, toks in got.items():
        assert [t for step in order for r, t in step if r == rid] == toks


def test_batcher_without_drafts_makes_the_plain_calls():
    class Silent:
        def propose(self, history, k):
            return []
    _, pb, plain, _ = _serve(None, REQS)
    _, b, got, _ = _serve(Silent(), REQS)
    assert got == plain and b.calls == pb.calls            # exactly the calls made without a drafter
    # draft_tokens = 0: the same
    _, b, got, _ = _serve(NgramDrafter(), REQS, draft_tokens=0)
    assert got == plain and b.calls == pb.calls


def test_batcher_honours_stop_ids_and_budgets_exactly():
    # the chain from 3 runs 1, 8, 9, 14, 5, 11, ... : stop at 14 inside an accepted run
    assert _chain([3], 6) == [1, 8, 9, 14, 5, 11]
    reqs = [([3, 1, 8, 9, 14, 5, 11, 7, 4, 6, 16, 15, 10, 2, 13, 0, 3], 40, (14,)),
            ([3, 1, 8, 9, 3], 5, ()), ([1, 8, 9, 14, 5, 1], 3, (9,))]
    _, pb, plain, _ = _serve(None, reqs)
    cb, b, got, _ = _serve(NgramDrafter(), reqs, draft_tokens=8)
    assert got == plain
    assert got[0] == [1, 8, 9, 14] and got[1] == _chain([3], 5) and got[2] == [8, 9]
    assert cb.stats["accepted"] > 0
    # the stop id came inside a longer accepted run: the slot was released, never rewound
    assert ("release", 0) in b.calls
    # no table asked for more rows than a request's budget leaves (request 2: at most 3 - 1 - 1)
    for c in b.calls:
        if c[0] == "verify":
            for s, d in c[1]:
                assert len(d) <= reqs[s][1] - 2, (s, d)


def test_batcher_keeps_a_chunking_slot_out_of_the_table():
    eng = FakeEngine()
    cb = ContinuousBatcher(eng, slots=2, max_ctx=256, page_tokens=16, drafter=NgramDrafter(), prefill_chunk=32,
                           draft_tokens=2)
    cycle = [1, 8, 9, 14, 5, 11, 7, 4, 6, 16, 15, 10, 2, 13, 0, 3]
    long_prompt = [20 + i for i in range(100)]                     # 4 pieces
    a = cb.submit(cycle + [1], 40)                                 # every lookup hits
    cb.step()
    c = cb.submit(long_prompt, 6)
    seen = False
    while not cb.idle():
        chunking = {r.slot for r in cb.slots if r is not None and len(r.chunks) > 1}   # before this step's piece
        n0 = len(eng.batches[0].calls)
        cb.step()
        for call in eng.batches[0].calls[n0:]:
            if call[0] == "verify" and chunking:
                seen = True
                assert not chunking & {s for s, _ in call[1]}
    assert seen
    assert cb.requests[a].tokens == _chain([1], 40) and cb.requests[c].tokens == _chain(long_prompt, 6)


def test_draft_tokens_range():
    with pytest.raises(ValueError):
        ContinuousBatcher(FakeEngine(), slots=2, max_ctx=64, drafter=NgramDrafter(), draft_tokens=16)
