"""CPU: the host side of scoring — the declaration / binding of the new entry points, the
target / chunk planning of Batch.score, and the batcher's logprob bookkeeping on a fake batch."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

from qwen_inference_engine_amd import _lib
from qwen_inference_engine_amd.engine import Batch
from qwen_inference_engine_amd.scheduler import ContinuousBatcher, Request, prefill_chunks, score_pieces


def _declared(header, name):
    text = open(os.path.join(ROOT, "include", "qie", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b(?:int|int64_t)\s+%s\s*\(([^)]*)\)\s*;" % name, text)
    assert m, f"{header} does not declare {name}"
    return len([a for a in m.group(1).split(",") if a.strip()])


@pytest.mark.parametrize("header,name,n_args", [
    ("qie_engine.h", "qie_score", 11),
    ("qie_engine.h", "qie_batch_logprobs", 3),
    ("qie_ops.h", "qie_logprob_rows", 8),
    ("qie_ops.h", "qie_score_rows_workspace_bytes", 2),
    ("qie_ops.h", "qie_score_rows", 11),
])
def test_scoring_entry_points_declared_and_bound(header, name, n_args):
    bound = {n: args for n, _, args in _lib.SIGNATURES}
    assert name in bound
    assert len(bound[name]) == _declared(header, name) == n_args


def test_score_flag_matches_the_header():
    text = open(os.path.join(ROOT, "include", "qie", "qie_engine.h")).read()
    m = re.search(r"#define\s+QIE_SCORE_UNFUSED\s+(\d+)", text)
    assert m and int(m.group(1)) == _lib.QIE_SCORE_UNFUSED == 1


def test_scoring_source_is_built():
    mk = open(os.path.join(ROOT, "qwen_inference_engine_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS_HIP\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    assert "k_score.hip" in srcs
    assert os.path.exists(os.path.join(ROOT, "qwen_inference_engine_amd", "csrc", "k_score.hip"))


def test_score_pieces_targets():
    ids = list(range(100, 145))   # 45 ids
    assert score_pieces(ids) == [(0, ids, ids[1:] + [-1])]
    pieces = score_pieces(ids, 16)
    assert [(pos, len(p)) for pos, p, _ in pieces] == prefill_chunks(45, 16) == [(0, 16), (16, 16), (32, 13)]
    for (pos, p, t), nxt in zip(pieces, pieces[1:] + [None]):
        assert len(t) == len(p) and t[:-1] == p[1:]
        # the last row of a middle piece targets the next piece's first id; the text's last row nothing
        assert t[-1] == (nxt[1][0] if nxt else -1)
    assert sum((t for _, _, t in pieces), []) == ids[1:] + [-1]
    # at a position: the pieces continue a live sequence there
    assert [pos for pos, _, _ in score_pieces(ids, 16, pos0=100)] == [100, 116, 132]
    assert score_pieces([7]) == [(0, [7], [-1])]
    assert score_pieces([7, 8], 1) == [(0, [7], [8]), (1, [8], [-1])]


def test_score_pieces_rejects_nonsense():
    for ids, chunk, pos0 in [([], None, 0), ([1, 2], 0, 0), ([1, 2], None, -1)]:
        with pytest.raises(ValueError):
            score_pieces(ids, chunk, pos0)


class _FakeBatch:
    """Batch.score over a recorded score_rows: row i's logprob is -(position + 1), its greedy id
    the target or 999."""

    def __init__(self):
        self.calls = []

    def score_rows(self, seq, ids, targets, pos0=0, sampling=None, unfused=False):
        self.calls.append((seq, list(ids), list(targets), pos0, unfused))
        lp = np.array([-(pos0 + i + 1) if t >= 0 else 0.0 for i, t in enumerate(targets)], np.float32)
        gr = np.array([t if t >= 0 else 999 for t in targets], np.int32)
        return lp, gr, 4242

    score = Batch.score
    perplexity = Batch.perplexity


def test_batch_score_stitches_the_pieces():
    fb = _FakeBatch()
    ids = list(range(10, 55))
    lp, gr, nxt = fb.score(2, ids, chunk=16, unfused=True)
    assert [(c[0], c[3], len(c[1]), c[4]) for c in fb.calls] == [(2, 0, 16, True), (2, 16, 16, True), (2, 32, 13, True)]
    assert list(lp) == [-(i + 1) for i in range(44)] and lp.dtype == np.float32
    assert list(gr) == ids[1:] + [999] and nxt == 4242
    fb.calls.clear()
    lp2, _, _ = fb.score(0, ids, pos0=7)
    assert fb.calls == [(0, ids, ids[1:] + [-1], 7, False)] and len(lp2) == 44
    assert fb.perplexity(0, [1, 2, 3]) == float(np.exp(1.5))   # mean of -1, -2


class _FakeLpBatch:
    """Two slots; logprobs(ids) returns -(slot + 1) - id / 1000 for the slots asked."""

    def __init__(self):
        self.B, self.max_ctx, self.asked = 2, 512, []

    def page_stats(self):
        return 8, np.zeros(2, np.int32), 128

    def prefill(self, slot, prompt, sampling=None):
        return 100 + slot

    def append(self, slot, ids, pos0, sampling=None):
        return 200 + slot

    def decode_step(self, sampling=None):
        return [300, 301]

    def logprobs(self, ids):
        self.asked.append(list(ids))
        return np.array([0.0 if t < 0 else -(i + 1) - t / 1000 for i, t in enumerate(ids)], np.float32)

    def release(self, slot):
        pass


class _FakeEngine:
    def __init__(self, b):
        self.b = b

    def batch(self, *a, **k):
        return self.b


def test_batcher_records_one_logprob_per_token():
    fb = _FakeLpBatch()
    cb = ContinuousBatcher(_FakeEngine(fb), slots=2, max_ctx=512, keep_logprobs=True, prefill_chunk=8)
    a = cb.submit(list(range(5)), 2)     # whole: admission token, then one decode token
    c = cb.submit(list(range(12)), 2)    # two chunks: completion token, then one decode token
    cb.run()
    ra, rc = cb.requests[a], cb.requests[c]
    assert ra.tokens == [100, 300] and rc.tokens == [201, 301]
    assert ra.logprobs == pytest.approx([-1.1, -1.3]) and rc.logprobs == pytest.approx([-2.201, -2.301])
    # only the emitting slots were asked about, the others skipped with -1
    assert fb.asked[0] == [100, -1] and all(len(q) == 2 for q in fb.asked)
    assert Request(0, [1], 1).logprobs == []
    # off by default: nothing is asked
    fb2 = _FakeLpBatch()
    cb2 = ContinuousBatcher(_FakeEngine(fb2), slots=2, max_ctx=512)
    r = cb2.submit([1, 2, 3], 2)
    cb2.run()
    assert fb2.asked == [] and cb2.requests[r].logprobs == []
