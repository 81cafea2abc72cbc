"""CPU: the host side of ragged prefill — the grouping function and the argument check
(qwen_inference_engine_amd.scheduler), the exact calls a ContinuousBatcher(ragged_prefill=True)
makes on test_prefix_host's fake Batch (which keeps pages and counts and asserts where the engine
would refuse), Batch.prefill_ragged's own ValueErrors, and the library's new symbols."""
import subprocess

import pytest

from test_prefix_host import T, FakeBatch, FakeEngine, ids

from qwen_inference_engine_amd import _lib
from qwen_inference_engine_amd.engine import Batch
from qwen_inference_engine_amd.scheduler import ContinuousBatcher, Request, ragged_group, ragged_segments


class RaggedFake(FakeBatch):
    """One recorded call; each segment does to the pool what its single call does."""

    def prefill_ragged(self, segments, sampling=None):
        segments = ragged_segments(segments)
        assert 1 < len(segments) <= 8, "a group of one is the plain call"
        self.calls.append(("prefill_ragged",) + tuple((s, len(i), p) for s, i, p in segments))
        n = len(self.calls)
        toks = [self.append(s, i, p) if p else self.prefill(s, i) for s, i, p in segments]
        del self.calls[n:]
        return toks


def _batcher(slots, n_pages=64, **kw):
    fb = RaggedFake(slots, 1024, n_pages)
    return fb, ContinuousBatcher(FakeEngine(fb), slots=slots, max_ctx=1024, ragged_prefill=True, **kw)


def _no_decode(calls):
    return [c for c in calls if c[0] != "decode"]


# ------------------------------------------------------------------ pure functions
def test_ragged_group_orders_pieces_by_slot():
    rs = [Request(0, ids(40, 1), 1, slot=2), Request(1, ids(9, 2), 1, slot=0), Request(2, ids(100, 3), 1, slot=5)]
    got = ragged_group([(rs[0], 32, 8), (rs[1], 0, 9), (rs[2], 64, 32)])
    assert got == [(0, ids(9, 2), 0), (2, ids(40, 1)[32:40], 32), (5, ids(100, 3)[64:96], 64)]
    assert ragged_group([]) == []
    assert ragged_segments(got) == got   # what the grouping yields passes the call's own check


def test_ragged_segments_check():
    assert ragged_segments([(1, [4, 5]), (3, (6,), 7), (4, [8], None)]) == [(1, [4, 5], 0), (3, [6], 7), (4, [8], 0)]
    for bad in ([], [(0, [])], [(0, [1]), (0, [2])], [(2, [1]), (1, [2])], [(0,)], [(0, [1], 0, 0)]):
        with pytest.raises(ValueError):
            ragged_segments(bad)


def test_batch_prefill_ragged_raises_on_its_own():
    """Before the library is touched: the object has no handle at all."""
    b = Batch.__new__(Batch)
    for bad in ([], [(0, [])], [(1, [3]), (1, [4])], [(2, [3]), (0, [4])]):
        with pytest.raises(ValueError):
            b.prefill_ragged(bad)


def test_library_exports_the_ragged_symbols(qlib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"qie_attention_ragged", "qie_qkv_post_ragged", "qie_prefill_ragged"} <= exported
    assert qlib.qie_abi_version() == 1
    import ctypes as C
    assert C.sizeof(_lib.RowSegsC) == 4 * (1 + 9 + 8) and C.sizeof(_lib.PrefillSegC) == 12


# ------------------------------------------------------------------ the batcher's calls
def test_admitted_group_is_one_call_and_a_group_of_one_stays_plain():
    fb, cb = _batcher(4)
    lens = [16, 16, 9, 200]
    rids = [cb.submit(ids(n, i), 2) for i, n in enumerate(lens)]
    out = cb.step()
    assert [c for c in fb.calls if "prefill" in c[0]] == [
        ("prefill_ragged", (0, 16, 0), (1, 16, 0), (2, 9, 0), (3, 200, 0))]
    assert fb.calls[0][0] == "prefill_ragged"
    assert out[:4] == [(rid, 1000 + rid) for rid in rids]   # first tokens in admission order
    cb.run()
    n0 = len(fb.calls)
    cb.submit(ids(33, 9), 1)                                # alone: the plain call
    cb.run()
    assert _no_decode(fb.calls[n0:]) == [("prefill", 0, 33), ("release", 0)]


def test_chunked_prompts_first_pieces_and_advances_go_together():
    """prefill_chunk = 32, prompts of 9, 70, 33, 40: the admission is one call over the whole
    prompt and the three first pieces; each later step advances every chunked slot in one call
    (one piece left: the plain append); a non-final piece emits nothing."""
    fb, cb = _batcher(4, prefill_chunk=32)
    rids = [cb.submit(ids(n, i), 3) for i, n in enumerate((9, 70, 33, 40))]
    out = cb.step()
    assert _no_decode(fb.calls) == [("prefill_ragged", (0, 9, 0), (1, 32, 0), (2, 32, 0), (3, 32, 0))]
    assert [rid for rid, _ in out] == [rids[0], rids[0]]   # its first token and one decoded; nothing of the chunked
    n0 = len(fb.calls)
    out = cb.step()
    assert _no_decode(fb.calls[n0:]) == [("prefill_ragged", (1, 32, 32), (2, 1, 32), (3, 8, 32)), ("release", 0)]
    assert [rid for rid, _ in out[:2]] == [rids[2], rids[3]]   # their last pieces, in slot order
    n0 = len(fb.calls)
    cb.step()
    assert _no_decode(fb.calls[n0:])[0] == ("append", 1, 6, 64)
    cb.run()
    assert all(len(cb.requests[r].tokens) == 3 for r in rids)


def test_ragged_false_makes_todays_calls():
    fb = RaggedFake(4, 1024, 64)
    cb = ContinuousBatcher(FakeEngine(fb), slots=4, max_ctx=1024, prefill_chunk=32)
    for i, n in enumerate((16, 16, 70)):
        cb.submit(ids(n, i), 2)
    cb.step()
    assert _no_decode(fb.calls) == [("prefill", 2, 32), ("prefill_batch", 0, 2), ("release", 0), ("release", 1)]
    n0 = len(fb.calls)
    cb.step()
    assert _no_decode(fb.calls[n0:])[0] == ("append", 2, 32, 32)
    assert not any(c[0] == "prefill_ragged" for c in fb.calls)


def test_prefix_cache_flush_groups_whole_prompts():
    """prefix_cache_pages > 0: the whole prompts without a match flush as one call and are saved
    afterwards; a prompt that begins like a cached one loads its prefix and appends alone."""
    fb, cb = _batcher(4, prefix_cache_pages=8)
    base = ids(2 * T, 1)
    a, b_, c = base + [5], ids(40, 2), ids(T + 3, 3)
    for p in (a, b_, c):
        cb.submit(p, 1)
    cb.step()
    assert _no_decode(fb.calls) == [
        ("prefill_ragged", (0, 2 * T + 1, 0), (1, 40, 0), (2, T + 3, 0)),
        ("save_prefix", 0, 2 * T), ("save_prefix", 2, T), ("release", 0), ("release", 1), ("release", 2)]
    n0 = len(fb.calls)
    cb.submit(base + ids(50, 4), 1)       # matches 2 pages: load + append, a group of one
    cb.submit(ids(20, 5), 1)
    cb.submit(ids(21, 6), 1)
    cb.run()
    new = _no_decode(fb.calls[n0:])
    assert new[:3] == [("load_prefix", 0, 2 * T), ("append", 0, 50, 2 * T), ("release", 0)]
    assert ("prefill_ragged", (0, 20, 0), (1, 21, 0)) in new
    assert cb.prefix_hits == 1


def test_prefix_cache_with_chunks_advances_in_one_call():
    fb, cb = _batcher(3, prefill_chunk=64, prefix_cache_pages=8)
    for i, n in enumerate((150, 100)):
        cb.submit(ids(n, i + 1), 2)
    cb.step()                             # chunked prompts start one by one (cached admission)
    assert _no_decode(fb.calls) == [("prefill", 0, 64), ("prefill", 1, 64)]
    n0 = len(fb.calls)
    cb.step()
    assert _no_decode(fb.calls[n0:])[0] == ("prefill_ragged", (0, 64, 64), (1, 36, 64))
    cb.run()
    assert ("save_prefix", 0, T) in fb.calls
