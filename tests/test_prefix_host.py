"""CPU: the host logic of prefix reuse (qwen_inference_engine_amd.scheduler): the pure
prefix-match function, and the ContinuousBatcher's admission arithmetic with a prefix cache on a
fake Batch that keeps pages and counts as DESIGN.md §18 describes them (LIFO free list, a count
per page, pages drawn by the call that writes them) and raises where the engine would return -28.
With prefix_cache_pages=0 the batcher must make exactly the calls it made before the cache
existed: checked on a fake that records every call."""
import pytest

from qwen_inference_engine_amd.scheduler import ContinuousBatcher, longest_prefix_match

T = 128


def ids(n, seed=0):
    return [(seed * 7919 + i * 31 + 3) % 1000 for i in range(n)]


# ------------------------------------------------------------------ the match function
def test_match_none():
    assert longest_prefix_match(ids(300, 1), [], T) == (0, -1)
    assert longest_prefix_match(ids(300, 1), [ids(256, 2)], T) == (0, -1)


def test_match_shorter_than_a_page():
    a = ids(300, 1)
    assert longest_prefix_match(a, [a[:127] + [9999] + a[128:256]], T) == (0, -1)   # 127 equal ids
    assert longest_prefix_match(a[:100], [a[:256]], T) == (0, -1)                   # a prompt below one page


def test_match_exactly_one_page():
    a = ids(300, 1)
    assert longest_prefix_match(a, [a[:128]], T) == (128, 0)
    assert longest_prefix_match(a, [a[:128] + ids(128, 5)], T) == (128, 0)      # diverges in page 2
    assert longest_prefix_match(a, [a[:255]], T) == (128, 0)                    # the entry's partial page is not shared


def test_match_whole_prompt_cached_leaves_one_id():
    a = ids(256, 1)
    assert longest_prefix_match(a, [a], T) == (128, 0)            # capped: (255 // 128) * 128
    assert longest_prefix_match(a + [5], [a], T) == (256, 0)      # one id left to append
    assert longest_prefix_match(a[:129], [a], T) == (128, 0)
    assert longest_prefix_match(a[:128], [a], T) == (0, -1)       # cap 0: nothing but the last id's page
    assert longest_prefix_match([], [a], T) == (0, -1)


def test_match_picks_the_longest_entry():
    a = ids(600, 1)
    assert longest_prefix_match(a, [a[:128], a[:384], a[:256]], T) == (384, 1)
    assert longest_prefix_match(a, [a[:256], a[:256] + ids(128, 9)], T) == (256, 0)   # first of equals
    assert longest_prefix_match(a, [ids(256, 4), a[:512]], T) == (512, 1)


# ------------------------------------------------------------------ a fake Batch with a real pool
class PoolExhausted(Exception):
    pass


class FakePrefix:
    def __init__(self, fb, pages, ids_):
        self.fb, self.pages, self.ids, self.n_tokens = fb, pages, ids_, len(pages) * T

    def drop(self):
        for p in self.pages:
            self.fb._drop(p)
        self.pages = []


class FakeBatch:
    def __init__(self, slots, max_ctx, n_pages):
        self.B, self.max_ctx, self.n_pages = slots, max_ctx, n_pages
        self.free = list(range(n_pages - 1, 0, -1))
        self.refs = [0] * n_pages
        self.rows = [[] for _ in range(slots)]
        self.pos = [None] * slots
        self.calls = []
        self.min_free = len(self.free)

    def _take(self):
        if not self.free:
            raise PoolExhausted(self.calls[-1])
        p = self.free.pop()
        self.refs[p] = 1
        self.min_free = min(self.min_free, len(self.free))
        return p

    def _drop(self, p):
        self.refs[p] -= 1
        if self.refs[p] == 0:
            self.free.append(p)

    def _grow(self, s, ntok):
        while len(self.rows[s]) < -(-ntok // T):
            self.rows[s].append(self._take())

    def _write(self, s, lo, hi):
        for i in range(lo // T, min(hi // T, len(self.rows[s]) - 1) + 1):
            assert self.refs[self.rows[s][i]] == 1, f"slot {s} writes into shared page index {i}: a private copy"
        self._grow(s, hi + 1)

    def _release(self, s):
        for p in reversed(self.rows[s]):
            self._drop(p)
        self.rows[s], self.pos[s] = [], None

    def page_stats(self):
        return len(self.free), [len(r) for r in self.rows], T

    def page_refs(self):
        return list(self.refs)

    def block_table(self, seq, n):
        return list(self.rows[seq][:n])

    def prefill(self, seq, ids_, sampling=None):
        self.calls.append(("prefill", seq, len(ids_)))
        self._release(seq)
        self._grow(seq, len(ids_))
        self.pos[seq] = len(ids_)
        return 1000 + seq

    def prefill_batch(self, seq0, prompts, sampling=None):
        self.calls.append(("prefill_batch", seq0, len(prompts)))
        for z, p in enumerate(prompts):
            self._release(seq0 + z)
        for z, p in enumerate(prompts):
            self._grow(seq0 + z, len(p))
            self.pos[seq0 + z] = len(p)
        return [1000 + seq0 + z for z in range(len(prompts))]

    def append(self, seq, ids_, pos0=None, sampling=None):
        self.calls.append(("append", seq, len(ids_), pos0))
        assert self.pos[seq] is not None and 1 <= pos0 <= self.pos[seq]
        self._write(seq, pos0, pos0 + len(ids_) - 1)
        self.pos[seq] = pos0 + len(ids_)
        return 1500 + seq

    def save_prefix(self, seq, n):
        self.calls.append(("save_prefix", seq, n))
        assert n > 0 and n % T == 0 and n <= self.pos[seq]
        pages = self.rows[seq][:n // T]
        for p in pages:
            self.refs[p] += 1
        return FakePrefix(self, list(pages), None)

    def load_prefix(self, prefix, dst, token, n_tokens=None):
        self.calls.append(("load_prefix", dst, n_tokens))
        assert n_tokens % T == 0 and 0 < n_tokens <= len(prefix.pages) * T
        self._release(dst)
        for p in prefix.pages[:n_tokens // T]:
            self.refs[p] += 1
            self.rows[dst].append(p)
        self.pos[dst] = n_tokens

    def decode_step(self, sampling=None):
        self.calls.append(("decode",))
        for s in range(self.B):
            if self.pos[s] is not None:
                self._write(s, self.pos[s], self.pos[s])
                self.pos[s] += 1
        return [2000 + i for i in range(self.B)]

    def release(self, seq):
        self.calls.append(("release", seq))
        self._release(seq)


class FakeEngine:
    def __init__(self, fb):
        self.fb = fb

    def batch(self, slots, max_ctx, page_tokens=None, n_pages=0):
        return self.fb


def _save_sets_ids(cb):
    """FakePrefix carries no ids of its own; the batcher keeps them in its entries."""
    return [e.ids for e in cb.cache]


def test_batcher_reuses_a_cached_prefix_and_never_runs_dry():
    """Three requests; the second and third begin with the first's 256 ids.  Pool of 6 usable
    pages: the first needs 3 (300 + 40 ids), the second 3 - 2 shared, so both fit at once; the
    third arrives after both finished and fits because its match costs it nothing."""
    fb = FakeBatch(2, 512, 7)
    cb = ContinuousBatcher(FakeEngine(fb), slots=2, max_ctx=512, prefix_cache_pages=4)
    base = ids(256, 1)
    p1, p2, p3 = base + ids(44, 2), base + ids(30, 3), base + ids(100, 4)
    r1, r2 = cb.submit(p1, 40), cb.submit(p2, 60)
    cb.step()
    # the first prompt prefills whole and is saved before the second is looked up
    assert fb.calls[:4] == [("prefill", 0, 300), ("save_prefix", 0, 256), ("load_prefix", 1, 256),
                            ("append", 1, 30, 256)]
    assert cb.prefix_hits == 1 and cb.prefix_tokens_reused == 256
    assert cb.requests[r1].pages == 3 and cb.requests[r2].pages == 1 and cb.requests[r2].matched == 256
    assert fb.rows[0][:2] == fb.rows[1][:2] and fb.refs[fb.rows[0][0]] == 3   # two slots + the cache
    assert _save_sets_ids(cb) == [base]                 # the second's aligned part is covered: one entry
    cb.run()
    assert len(fb.free) == 6 - 2                        # the cache alone holds the two pages
    r3 = cb.submit(p3, 130)                             # 4 pages in all, 2 of them cached
    cb.run()
    assert cb.prefix_hits == 2 and cb.prefix_tokens_reused == 512
    assert cb.requests[r3].pages == 2 and len(cb.requests[r3].tokens) == 130
    cb.drop_cache()
    assert len(fb.free) == 6 and not any(fb.refs)
    assert not any(c[0] == "save_prefix" and c[2] != 256 for c in fb.calls)


def test_batcher_evicts_least_recently_used_and_matched_entry_last():
    """5 usable pages, three cached one-page prefixes A, B, C (saved in that order, A then hit
    again).  A request matching A that needs 4 more pages does not fit beside the cache's 3:
    B (least recently used) goes, then C; A, the match, stays and is used."""
    fb = FakeBatch(1, 1024, 6)
    cb = ContinuousBatcher(FakeEngine(fb), slots=1, max_ctx=1024, prefix_cache_pages=5)
    pa, pb, pc = ids(128, 1), ids(128, 2), ids(128, 3)
    for p in (pa, pb, pc):
        cb.submit(p + [1], 1)
        cb.run()
    assert [e.ids for e in cb.cache] == [pa, pb, pc] and len(fb.free) == 2
    cb.submit(pa + [2, 3], 1)
    cb.run()                                            # a hit on A: most recently used now
    assert cb.prefix_hits == 1
    cb.submit(pa + ids(300, 9), 80)                     # pages(508) = 4, one matched: 3 needed, 2 free
    cb.run()
    assert [e.ids for e in cb.cache][0] == pa and pb not in [e.ids for e in cb.cache]
    assert cb.prefix_hits == 2
    # the matched entry goes last, when nothing else is left to drop: a three-page entry of which
    # the prompt shares one page leaves 2 pages free; the request needs 5 - 1, so the entry is
    # dropped, the match with it, and the request takes the whole pool
    cb.drop_cache()
    pe = ids(384, 7)
    cb.submit(pe + [1], 1)
    cb.run()
    assert [e.ids for e in cb.cache] == [pe] and len(fb.free) == 2
    rid = cb.submit(pe[:128] + ids(420, 8), 90)         # pages(638) = 5
    cb.run()
    assert cb.prefix_hits == 2 and cb.requests[rid].matched == 0 and len(cb.requests[rid].tokens) == 90
    # the cap: never more than prefix_cache_pages held by the cache alone
    small = FakeBatch(1, 1024, 8)
    cs = ContinuousBatcher(FakeEngine(small), slots=1, max_ctx=1024, prefix_cache_pages=2)
    for s in range(4):
        cs.submit(ids(128, 20 + s) + [1], 1)
        cs.run()
        assert cs._cache_only_pages() <= 2
    assert [e.ids for e in cs.cache] == [ids(128, 22), ids(128, 23)]


def test_matched_entry_survives_a_flush_that_trims_the_cache():
    """One admission pass with a cache at its cap (2 pages, held by entry A): a whole prompt that
    finishes at its first token waits in the pending run, then a request matching A arrives.  The
    pending run is prefilled, saved and released first — its page is then the cache's alone, the
    cap is exceeded and the least recently used entry goes.  That is A: the lookup that follows
    finds no match and the request prefills whole; a load on the dropped entry would be an error.
    With room under the cap the same pass keeps A and loads it."""
    for cap, want in [(2, [("prefill", 0, 129), ("save_prefix", 0, 128), ("release", 0), ("prefill", 0, 296)]),
                      (3, [("prefill", 0, 129), ("save_prefix", 0, 128), ("release", 0), ("load_prefix", 0, 256),
                           ("append", 0, 40, 256)])]:
        fb = FakeBatch(2, 1024, 12)
        cb = ContinuousBatcher(FakeEngine(fb), slots=2, max_ctx=1024, prefix_cache_pages=cap)
        a = ids(256, 1)
        cb.submit(a + [7], 1)
        cb.run()
        assert [e.ids for e in cb.cache] == [a]
        n0 = len(fb.calls)
        cb.submit(ids(128, 2) + [2], 1)
        rid = cb.submit(a + ids(40, 3), 5)
        cb.run()
        new = [c for c in fb.calls[n0:] if c[0] != "decode"]
        assert new[:len(want)] == want, (cap, new)
        r = cb.requests[rid]
        assert len(r.tokens) == 5 and r.matched == (256 if cap == 3 else 0)
        assert r.pages == cb._pages(296 + 5) - r.matched // T
        assert cb.prefix_hits == (1 if cap == 3 else 0)
        assert cb._cache_only_pages() <= cap
        cb.drop_cache()
        assert len(fb.free) == 11 and not any(fb.refs)


def test_batcher_chunked_prefill_with_a_match():
    """prefill_chunk applies to the remainder: a 600-id prompt with 256 cached goes in pieces of
    128 from 256 on, one per step, and is saved (512 ids) after its last piece."""
    fb = FakeBatch(2, 1024, 12)
    cb = ContinuousBatcher(FakeEngine(fb), slots=2, max_ctx=1024, prefill_chunk=128, prefix_cache_pages=8)
    base = ids(256, 1)
    cb.submit(base + [7], 2)
    cb.run()
    assert ("save_prefix", 0, 256) in fb.calls
    n0 = len(fb.calls)
    cb.submit(base + ids(344, 5), 3)
    cb.run()
    new = [c for c in fb.calls[n0:] if c[0] != "decode"]
    assert new == [("load_prefix", 0, 256), ("append", 0, 128, 256), ("append", 0, 128, 384),
                   ("append", 0, 88, 512), ("save_prefix", 0, 512), ("release", 0)]
    assert cb.prefix_tokens_reused == 256


def test_batcher_without_cache_makes_todays_calls():
    """prefix_cache_pages=0: the calls, in order, that the batcher made before the cache existed —
    page_stats once at construction, the grouped prefills, one decode per step, a release per
    finished request — and none of the new ones."""

    class Recorder(FakeBatch):
        def __getattribute__(self, name):
            v = object.__getattribute__(self, name)
            if callable(v) and not name.startswith("_"):
                object.__getattribute__(self, "names").append(name)
            return v

    fb = Recorder.__new__(Recorder)
    object.__setattr__(fb, "names", [])
    FakeBatch.__init__(fb, 4, 512, 64)
    cb = ContinuousBatcher(FakeEngine(fb), slots=4, max_ctx=512)
    for n, new in [(16, 2), (16, 2), (9, 1), (200, 3)]:
        cb.submit(list(range(n)), new)
    cb.run()
    assert fb.names == ["page_stats",
                        "prefill_batch", "prefill", "prefill", "release", "decode_step", "release", "release",
                        "decode_step", "release"]
    assert [c for c in fb.calls if c[0] != "decode"] == [
        ("prefill_batch", 0, 2), ("prefill", 2, 9), ("prefill", 3, 200), ("release", 2), ("release", 0),
        ("release", 1), ("release", 3)]
    assert cb.budget == 63 and cb.prefix_hits == 0 and not cb.cache
