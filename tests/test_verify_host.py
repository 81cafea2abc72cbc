"""CPU: the host side of speculative decoding — the qie_verify ABI is declared,
exported and bound; it refuses a null batch without a GPU; the n-gram drafter's lookup rule;
and SpeculativeDecoder's accept-length / max_new / stop-id / stats bookkeeping over a scripted
stand-in for a Batch."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

from qwen_inference_engine_amd import _lib
from qwen_inference_engine_amd.speculative import NgramDrafter, SpeculativeDecoder


def test_header_declares_and_library_exports_verify(qlib):
    text = open(os.path.join(ROOT, "include", "qie", "qie_engine.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^int\s+qie_verify\s*\(", code, flags=re.M)
    assert re.search(r"^int\s+qie_verify_logits\s*\(", code, flags=re.M)
    m = re.search(r"^#define\s+QIE_VERIFY_MAX_ROWS\s+(\d+)", code, flags=re.M)
    assert m and int(m.group(1)) == 16 == _lib.QIE_VERIFY_MAX_ROWS
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"qie_verify", "qie_verify_logits"} <= exported
    assert {"qie_verify", "qie_verify_logits"} <= {n for n, _, _ in _lib.SIGNATURES}


def test_verify_null_batch_is_refused_without_a_gpu(qlib):
    import ctypes as C
    out, n = (C.c_int32 * 4)(), C.c_int32(7)
    assert qlib.qie_verify(None, 0, None, 0, None, out, C.byref(n)) == -22
    assert b"qie_verify" in qlib.qie_last_error()
    assert n.value == 7
    assert qlib.qie_verify_logits(None, None) == -22
    assert b"qie_verify_logits" in qlib.qie_last_error()


# ------------------------------------------------------------------------------ NgramDrafter
def test_ngram_longest_match_wins():
    #            0  1  2  3  4  5  6  7  8  9 10
    h = [9, 1, 2, 3, 7, 5, 3, 8, 1, 2, 3]
    # suffix (1, 2, 3) occurred at 1..3 -> continues 7; the shorter suffix (3) alone would take
    # its most recent earlier occurrence at 6 -> 8
    assert NgramDrafter(3, 1).propose(h, 2) == [7, 5]
    assert NgramDrafter(1, 1).propose(h, 2) == [8, 1]


def test_ngram_most_recent_occurrence():
    h = [4, 5, 10, 4, 5, 20, 4, 5]
    assert NgramDrafter(2, 1).propose(h, 1) == [20]
    assert NgramDrafter(2, 1).propose(h, 3) == [20, 4, 5]


def test_ngram_truncates_at_k_and_at_the_end():
    h = [1, 2, 3, 4, 5, 6, 1, 2]
    assert NgramDrafter(3, 1).propose(h, 3) == [3, 4, 5]
    assert NgramDrafter(3, 1).propose(h, 15) == [3, 4, 5, 6, 1, 2]   # what follows, no more
    assert NgramDrafter(3, 1).propose(h, 0) == []


def test_ngram_no_match_and_min_ngram():
    assert NgramDrafter().propose([1, 2, 3, 4], 4) == []
    assert NgramDrafter().propose([], 4) == [] and NgramDrafter().propose([5], 4) == []
    h = [1, 2, 9, 8, 2]                       # only the 1-gram (2) recurs
    assert NgramDrafter(3, 1).propose(h, 2) == [9, 8]
    assert NgramDrafter(3, 2).propose(h, 2) == []
    with pytest.raises(ValueError):
        NgramDrafter(1, 2)


# ------------------------------------------------------------------------ SpeculativeDecoder
class _Spec:
    vocab = 100


class _Eng:
    spec = _Spec()


class FakeBatch:
    """A Batch whose model emits the scripted stream `target` after any prompt: verify applies
    qie_verify's accept rule to it, and records every call."""

    def __init__(self, target, max_ctx=1 << 20):
        self.e, self.max_ctx = _Eng(), max_ctx
        self.target = list(target)
        self.n = 0              # tokens of the stream emitted so far
        self.calls = []         # drafts of every verify call
        self.rewinds = []

    def prefill(self, seq, ids, sampling=None):
        self.P = len(ids)
        self.n = 1
        return self.target[0]

    def verify(self, seq, draft, sampling=None):
        assert len(draft) <= 15 and all(0 <= t < _Spec.vocab for t in draft)
        self.calls.append(list(draft))
        out = [self.target[self.n]]
        for j, d in enumerate(draft):
            if d != out[-1]:
                break
            out.append(self.target[self.n + j + 1])
        self.n += len(out)
        return out

    def set_position(self, seq, pos, tok):
        self.rewinds.append((pos, tok))
        self.n = pos - self.P + 1


class ScriptDrafter:
    """Proposes the true continuation with the listed mistakes: wrong[i] = offset of the bad
    draft in call i (None: all right; -1: an empty proposal)."""

    def __init__(self, target, P, wrong):
        self.target, self.P, self.wrong, self.i = list(target), P, list(wrong), 0

    def propose(self, history, k):
        w = self.wrong[self.i] if self.i < len(self.wrong) else None
        self.i += 1
        if w == -1:
            return []
        n = len(history) - self.P
        d = self.target[n:n + k]
        if w is not None and w < len(d):
            d[w] = (d[w] + 1) % _Spec.vocab
        return d


TARGET = [(7 * i + 3) % 50 for i in range(64)]   # no stop id 99 in it
PROMPT = [1, 2, 3]


def _run(wrong, max_new, k=4, stop=(), target=TARGET):
    b = FakeBatch(target)
    dec = SpeculativeDecoder(b, ScriptDrafter(target, len(PROMPT), wrong), k=k)
    return b, dec, dec.generate(PROMPT, max_new, stop_ids=stop)


def test_decoder_all_drafts_right():
    b, dec, out = _run([], 11)
    assert out == TARGET[:11]
    # 1 from the prefill, then 5 per call (4 drafts + the bonus token): 1 + 5 + 5
    assert b.calls == [TARGET[1:5], TARGET[6:10]]
    assert dec.stats == dict(verify_calls=2, drafted=8, accepted=8, emitted=11)


def test_decoder_first_draft_wrong():
    b, dec, out = _run([0, 0, 0], 4)
    assert out == TARGET[:4]
    assert [len(c) for c in b.calls] == [2, 1, 0]        # k shrinks with the room left: 4 - 1 - 1, ...
    assert dec.stats == dict(verify_calls=3, drafted=3, accepted=0, emitted=4)


def test_decoder_wrong_in_the_middle():
    b, dec, out = _run([2, None], 12)
    assert out == TARGET[:12]
    # call 0: drafts 0, 1 accepted, draft 2 wrong -> 3 tokens; call 1: 4 accepted -> 5; call 2
    assert [len(c) for c in b.calls] == [4, 4, 2]
    assert dec.stats == dict(verify_calls=3, drafted=10, accepted=2 + 4 + 2, emitted=12)


def test_decoder_empty_proposal_still_emits_one():
    b, dec, out = _run([-1, -1, None], 6)
    assert out == TARGET[:6]
    assert b.calls == [[], [], TARGET[3:5]]              # room for 3 more: 2 drafts + the bonus token
    assert dec.stats == dict(verify_calls=3, drafted=2, accepted=2, emitted=6)


def test_decoder_never_exceeds_max_new():
    for max_new in (1, 2, 5, 6, 7):
        b, dec, out = _run([], max_new)
        assert out == TARGET[:max_new]
        assert all(len(c) <= 4 for c in b.calls)
        assert 1 + sum(len(c) + 1 for c in b.calls) == max_new   # every call was sized to the room left
    assert _run([], 0)[2] == []


def test_decoder_stops_at_a_stop_id_and_rewinds_the_batch():
    target = list(TARGET)
    target[3] = 99
    b, dec, out = _run([], 20, stop=(99,), target=target)
    assert out == target[:4]
    # the one call emitted 5 tokens, the stop id third among them: the batch is put back onto it
    assert b.rewinds == [(len(PROMPT) + 3, 99)] and b.n == 4
    assert dec.stats == dict(verify_calls=1, drafted=4, accepted=4, emitted=4)
    # a stop id as the prefill's token ends at once
    target = [99] + TARGET
    b, dec, out = _run([], 20, stop=(99,), target=target)
    assert out == [99] and b.calls == []


def test_decoder_respects_the_context_limit():
    b = FakeBatch(TARGET, max_ctx=len(PROMPT) + 6)
    dec = SpeculativeDecoder(b, ScriptDrafter(TARGET, len(PROMPT), []), k=4)
    out = dec.generate(PROMPT, 40)
    assert out == TARGET[:len(out)]
    # a call of n drafts at position p needs p + n + 1 < max_ctx
    p = len(PROMPT)
    for c in b.calls:
        assert p + len(c) + 1 < b.max_ctx
        p += len(c) + 1
    assert len(out) >= 2
