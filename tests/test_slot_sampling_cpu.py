"""CPU: per-slot sampling — the numpy restatement of the contract on hand-computed rows, the
ctypes mirror of qie_slot_sampling against the C header, and the batcher's per-request entries
on a fake Batch."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import slot_sampling_ref as R
from conftest import ROOT

from qwen_inference_engine_amd import SlotSampling, _lib
from qwen_inference_engine_amd.scheduler import ContinuousBatcher

NEG_INF = float("-inf")


def bf(oracle, xs):
    return oracle.f32_to_bf16(np.array(xs, np.float32))


def val(oracle, bits):
    return [float(x) for x in oracle.bf16_to_f32(np.asarray(bits, np.uint16))]


# ----------------------------------------------------------------------------- the contract
def test_neutral_entry_leaves_the_row_bit_identical(oracle):
    row = oracle.f32_to_bf16((np.random.default_rng(1).standard_normal(300) * 3).astype(np.float32))
    row[7], row[8], row[9] = 0x7FC0, 0xFF80, 0x8000   # NaN, -inf, -0: bits kept too
    got = R.process(oracle, row, SlotSampling(top_k=40, temperature=0.7), [1, 2, 2, 7, 8, 9, 299])
    assert np.array_equal(got, row)


def test_each_penalty_alone_on_positive_negative_and_zero_logits(oracle):
    row = bf(oracle, [2.0, -2.0, 0.0, 3.0, -1.5, 0.0])
    ids = [0, 1, 2]   # 3, 4, 5 are not in the window
    # repetition 2: positive halves, negative doubles, zero stays
    got = R.process(oracle, row, SlotSampling(repetition_penalty=2.0), ids)
    assert val(oracle, got) == [1.0, -4.0, 0.0, 3.0, -1.5, 0.0]
    # presence 0.5: subtracted once
    got = R.process(oracle, row, SlotSampling(presence_penalty=0.5), ids)
    assert val(oracle, got) == [1.5, -2.5, -0.5, 3.0, -1.5, 0.0]
    # frequency 0.25, one occurrence each
    got = R.process(oracle, row, SlotSampling(frequency_penalty=0.25), ids)
    assert val(oracle, got) == [1.75, -2.25, -0.25, 3.0, -1.5, 0.0]


def test_counts_above_one(oracle):
    row = bf(oracle, [2.0, -2.0, 0.0, 3.0])
    ids = [0, 0, 0, 1, 1, 3, 999, -4]   # ids outside [0, V) are ignored
    e = SlotSampling(repetition_penalty=2.0, presence_penalty=0.5, frequency_penalty=0.25)
    # 0: 2/2 - (0.5 + 0.75) = -0.25   1: -2*2 - (0.5 + 0.5) = -5   3: 3/2 - (0.5 + 0.25) = 0.75
    assert val(oracle, R.process(oracle, row, e, ids)) == [-0.25, -5.0, 0.0, 0.75]
    # the presence penalty does not grow with the count, the frequency penalty does
    assert val(oracle, R.process(oracle, row, SlotSampling(presence_penalty=1.0), ids)) == [1.0, -3.0, 0.0, 2.0]
    assert val(oracle, R.process(oracle, row, SlotSampling(frequency_penalty=1.0), ids)) == [-1.0, -4.0, 0.0, 2.0]


def test_result_is_rounded_to_bf16(oracle):
    row = bf(oracle, [1.0])
    got = R.process(oracle, row, SlotSampling(repetition_penalty=3.0), [0])
    # 1/3 in fp32, then bf16 round-to-nearest-even: 0x3EAB (0.333984375)
    assert int(got[0]) == 0x3EAB


def test_window_clipping(oracle):
    hist = np.array([5, 6, 7, 8, 9, 6, 6, 3, 3, 3], np.int32)   # max_ctx 10
    assert R.window_ids(SlotSampling(), hist, 6) == [5, 6, 7, 8, 9, 6, 6]
    assert R.window_ids(SlotSampling(penalty_start=4), hist, 6) == [9, 6, 6]
    # last_n cuts the run of 6s in the middle
    assert R.window_ids(SlotSampling(penalty_last_n=2), hist, 6) == [6, 6]
    assert R.window_ids(SlotSampling(penalty_last_n=1), hist, 6) == [6]
    assert R.window_ids(SlotSampling(penalty_start=2, penalty_last_n=100), hist, 6) == [7, 8, 9, 6, 6]
    assert R.window_ids(SlotSampling(penalty_start=5, penalty_last_n=4), hist, 6) == [6, 6]
    # start past q: empty; q past the row: clamped to max_ctx
    assert R.window_ids(SlotSampling(penalty_start=7), hist, 6) == []
    assert R.window_ids(SlotSampling(penalty_start=8), hist, 40) == [3, 3]
    # a verify row: the last ids come from the drafts, not from the history's stale words
    assert R.window_ids(SlotSampling(), hist, 6, tail=[1, 2]) == [5, 6, 7, 8, 9, 1, 2]
    assert R.window_ids(SlotSampling(penalty_last_n=1), hist, 6, tail=[1, 2]) == [2]
    assert R.window_ids(SlotSampling(penalty_last_n=3), hist, 6, tail=[1, 2]) == [9, 1, 2]
    # the count follows the clipped window
    row = bf(oracle, [0.0] * 10)
    e = SlotSampling(frequency_penalty=1.0, penalty_last_n=2)
    assert val(oracle, R.process(oracle, row, e, R.window_ids(e, hist, 6)))[6] == -2.0


def test_bias_and_a_banned_argmax(oracle):
    row = bf(oracle, [1.0, 4.0, 3.0, -1.0])
    assert oracle.argmax(row) == 1
    e = SlotSampling(bias={1: NEG_INF, 3: 0.5, 0: -0.25})
    got = R.process(oracle, row, e, [])
    assert val(oracle, got) == [0.75, NEG_INF, 3.0, -0.5]
    assert R.choose(oracle, row, e, [], 0)[0] == 2
    # penalty first, then the bias
    e = SlotSampling(repetition_penalty=2.0, bias={1: 1.0})
    assert val(oracle, R.process(oracle, row, e, [1]))[1] == 3.0
    # every element banned: no choice
    e = SlotSampling(bias={i: NEG_INF for i in range(4)})
    assert R.choose(oracle, row, e, [], 0)[0] == -1


def test_min_p_keeps_a_prefix(oracle):
    # weights at T = 1 relative to the best: 1, e^-1, e^-2, e^-4
    row = bf(oracle, [0.0, -4.0, -1.0, -2.0])
    e = SlotSampling(top_k=4, temperature=1.0, min_p=0.1, seed=5)
    kept, margin = R.min_p_keep(oracle, row, e)
    assert kept == 3 and margin > 0.2
    for step in range(4):
        assert R.choose(oracle, row, e, [], step)[0] == oracle.sample(row, 3, 1.0, 1.0, 5 + step)
    assert R.min_p_keep(oracle, row, SlotSampling(top_k=4, min_p=0.0)) == (4, float("inf"))
    assert R.min_p_keep(oracle, row, SlotSampling(top_k=4, min_p=0.9))[0] == 1


# ------------------------------------------------------------------------------ the C struct
FIELDS = ["top_k", "temperature", "top_p", "min_p", "seed", "repetition_penalty", "presence_penalty",
          "frequency_penalty", "penalty_start", "penalty_last_n", "n_bias", "bias_ids", "bias"]


def test_ctypes_mirror_matches_the_header(tmp_path):
    src = tmp_path / "layout.c"
    lines = "".join(f'    printf("{f} %zu\\n", offsetof(qie_slot_sampling, {f}));\n' for f in FIELDS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "qie/qie_types.h"\nint main(void) {\n'
                   '    printf("sizeof %zu\\n", sizeof(qie_slot_sampling));\n'
                   '    printf("bias_max %d\\n", QIE_SLOT_BIAS_MAX);\n' + lines + "    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([os.environ.get("CC", "cc"), "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-o", str(exe), str(src)])
    out = dict(l.split() for l in subprocess.check_output([str(exe)]).decode().splitlines())
    assert int(out["sizeof"]) == C.sizeof(_lib.SlotSamplingC)
    assert int(out["bias_max"]) == _lib.QIE_SLOT_BIAS_MAX
    assert [f for f, _ in _lib.SlotSamplingC._fields_] == FIELDS
    for f in FIELDS:
        assert int(out[f]) == getattr(_lib.SlotSamplingC, f).offset, f


def test_slot_sampling_round_trips_through_the_struct():
    e = SlotSampling(top_k=50, temperature=0.7, top_p=0.9, min_p=0.05, seed=(1 << 63) + 5, repetition_penalty=1.3,
                     presence_penalty=0.5, frequency_penalty=0.25, penalty_start=7, penalty_last_n=64,
                     bias={3: -1.5, 9: NEG_INF})
    c = e.to_c()
    assert c.n_bias == 2 and list(c.bias_ids[:2]) == [3, 9] and c.seed == (1 << 63) + 5
    back = SlotSampling.from_c(c)
    assert back.bias == {3: -1.5, 9: NEG_INF} and back.top_k == 50 and back.penalty_last_n == 64
    assert back.repetition_penalty == np.float32(1.3)
    with pytest.raises(ValueError):
        SlotSampling(bias={i: 0.0 for i in range(33)}).to_c()


def test_entry_points_declared_and_bound():
    bound = {n: args for n, _, args in _lib.SIGNATURES}
    for name, n_args in [("qie_batch_set_slot_sampling", 3), ("qie_batch_slot_sampling", 4),
                         ("qie_sample_rows", 2), ("qie_sample_rows_workspace_bytes", 2)]:
        assert len(bound[name]) == n_args


# ------------------------------------------------------------------------------ the batcher
class _FakeBatch:
    """Records the calls of the ContinuousBatcher; one token per call, a fixed pool."""

    def __init__(self, slots=3, with_entries=True):
        self.B, self.max_ctx, self.calls = slots, 4096, []
        if with_entries:
            self.set_sampling = self._set_sampling

    def _set_sampling(self, seq, sampling):
        self.calls.append(("set", seq, sampling))

    def page_stats(self):
        return 63, np.zeros(self.B, np.int32), 128

    def page_refs(self):
        return np.zeros(64, np.int32)

    def block_table(self, seq, n):
        return np.arange(1, n + 1, dtype=np.int32)

    def save_prefix(self, seq, n):
        self.calls.append(("save", seq, n))
        return object()

    def load_prefix(self, prefix, dst, token, n):
        self.calls.append(("load", dst, n))

    def prefill(self, seq, ids, sampling=None):
        self.calls.append(("prefill", seq, len(ids)))
        return 100 + seq

    def prefill_batch(self, seq0, prompts, sampling=None):
        self.calls.append(("prefill_batch", seq0, len(prompts)))
        return [100 + seq0 + i for i in range(len(prompts))]

    def append(self, seq, ids, pos0, sampling=None):
        self.calls.append(("append", seq, pos0, len(ids)))
        return 200 + seq

    def decode_step(self, sampling=None):
        self.calls.append(("decode",))
        return [300 + i for i in range(self.B)]

    def release(self, seq):
        self.calls.append(("release", seq))


class _FakeEngine:
    def __init__(self, b):
        self.b = b

    def batch(self, *a, **k):
        return self.b


def _first(calls, pred):
    return next(i for i, c in enumerate(calls) if pred(c))


@pytest.mark.parametrize("kw", [{}, {"prefill_chunk": 8}, {"prefix_cache_pages": 8},
                                {"prefill_chunk": 64, "prefix_cache_pages": 8}])
def test_batcher_sets_the_entry_before_anything_is_prefilled_and_clears_it_at_finish(kw):
    fb = _FakeBatch()
    cb = ContinuousBatcher(_FakeEngine(fb), slots=3, max_ctx=4096, **kw)
    ea, eb = SlotSampling(top_k=50, temperature=0.7, seed=3), SlotSampling(repetition_penalty=1.3)
    base = list(range(300))
    if "prefix_cache_pages" in kw:   # a first request leaves base[:256] in the prefix cache
        cb.submit(base, 1)
        cb.run()
        fb.calls.clear()
    ra = cb.submit(base[:260] + [7, 8], 3, sampling=ea)                       # slot 0
    rb = cb.submit(list(range(20)), 2, sampling=eb, penalize_prompt=False)    # slot 1
    rc = cb.submit(list(range(5)), 2)                                         # slot 2: the batcher's sampling
    cb.run()
    calls = fb.calls
    if "prefix_cache_pages" in kw:
        assert ("load", 0, 256) in calls   # the admission went through the prefix cache
    if kw.get("prefill_chunk") == 8:
        assert sum(1 for c in calls if c[0] == "append" and c[1] == 1) == 2   # 20 ids: 8 + 8 + 4
    sets = [c for c in calls if c[0] == "set"]
    # one set and one clear per request with an entry, none for the request without
    assert [(c[1], c[2] is None) for c in sets if c[1] == 0] == [(0, False), (0, True)]
    assert [(c[1], c[2] is None) for c in sets if c[1] == 1] == [(1, False), (1, True)]
    assert not [c for c in sets if c[1] == 2]
    assert sets[0][2] == ea
    # penalize_prompt=False: the window starts behind the prompt
    assert [c[2] for c in sets if c[1] == 1][0] == SlotSampling(repetition_penalty=1.3, penalty_start=20)
    for slot in (0, 1):
        i_set = _first(calls, lambda c: c[0] == "set" and c[1] == slot and c[2] is not None)
        i_work = _first(calls, lambda c: (c[0] in ("prefill", "append", "load") and c[1] == slot) or
                        (c[0] == "prefill_batch" and c[1] <= slot < c[1] + c[2]))
        assert i_set < i_work, (slot, calls)
        i_clear = _first(calls, lambda c: c[0] == "set" and c[1] == slot and c[2] is None)
        i_rel = _first(calls, lambda c: c == ("release", slot))
        assert i_work < i_clear < i_rel
    assert len(cb.requests[ra].tokens) == 3 and len(cb.requests[rb].tokens) == 2 and len(cb.requests[rc].tokens) == 2


@pytest.mark.parametrize("kw", [{}, {"prefill_chunk": 8}])
def test_batcher_without_entries_makes_the_calls_it_made(kw):
    """A Batch without set_sampling serves: nothing of the feature is touched, and the calls are
    the sequence written down here from the batcher as it was."""
    fb = _FakeBatch(with_entries=False)
    cb = ContinuousBatcher(_FakeEngine(fb), slots=3, max_ctx=4096, **kw)
    cb.submit(list(range(12)), 2)
    cb.submit(list(range(12)), 2)
    cb.submit(list(range(5)), 3)
    cb.run()
    if not kw:
        want = [("prefill_batch", 0, 2), ("prefill", 2, 5), ("decode",), ("release", 0), ("release", 1),
                ("decode",), ("release", 2)]
    else:   # 12 ids: 8 at admission, 4 appended in the same step's successor
        want = [("prefill", 0, 8), ("prefill", 1, 8), ("prefill", 2, 5), ("decode",),
                ("append", 0, 8, 4), ("append", 1, 8, 4), ("decode",), ("release", 0), ("release", 1), ("release", 2)]
    assert fb.calls == want
