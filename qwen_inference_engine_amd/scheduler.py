"""Multi-sequence serving loop over a paged batch.

The reference drives ONE sequence (iengine.cu:226-456; a second sequence is commented out
at iengine.cu:309-322, 369-373, 448-452) through ``llm()`` and grows a linked page list
per sequence (iengine.cu:73-109).  Here requests share the B slots of one ``Batch`` with
a paged KV cache: a waiting request is admitted into a free slot when the page pool can
hold its worst case (prompt + max_new_tokens), prefilled there while the other slots keep
decoding (requests admitted together with equal prompt lengths into consecutive slots
prefill in one ``qie_prefill_batch`` pass), and retired at its stop token / token budget, which returns its pages
(``qie_batch_release``).  Every step is one fixed-B decode step over all slots (idle
slots run on the scratch page and their outputs are dropped), so the hipGraph captured
for the batch is replayed unchanged.

With ``prefix_cache_pages`` the batcher keeps the page-aligned prefixes of the prompts it has
seen on shared KV pages (``Batch.save_prefix``) and starts a request that begins like one of them
from those pages (``Batch.load_prefix`` + ``append`` of the remainder) instead of prefilling the
same ids again.

Sampling is per request: ``submit(..., sampling=SlotSampling(...))`` sets that request's entry on
its slot (``Batch.set_sampling``) when it takes the slot — before its first prefill, append or
prefix load — and clears it when the request finishes; a request without one samples under the
batcher's ``sampling`` (``qie_sampling``, per step).  ``penalize_prompt=False`` starts the
penalty window behind the prompt.  Slot rows are independent, so a request's tokens do not
depend on what the other slots hold.

With ``drafter`` the step speculates for the whole batch: every emitting slot
proposes up to ``draft_tokens`` ids and one ``Batch.verify_batch`` call — up to 8 slots and 16
rows, dealt by ``deal_verify_rows`` — takes the decode step's place; a step without any draft is
the plain decode step.
"""
from __future__ import annotations

import collections
import dataclasses
from typing import Deque, Dict, List, Optional, Sequence

from .engine import GREEDY, Batch, Engine, Sampling, SlotSampling


@dataclasses.dataclass
class Request:
    rid: int
    prompt: List[int]
    max_new_tokens: int
    stop_ids: tuple = ()
    tokens: List[int] = dataclasses.field(default_factory=list)
    logits: list = dataclasses.field(default_factory=list)   # per token, when keep_logits
    logprobs: List[float] = dataclasses.field(default_factory=list)   # per token, when keep_logprobs
    slot: int = -1
    pages: int = 0
    done: bool = False
    chunks: list = dataclasses.field(default_factory=list)   # (offset, length) prompt pieces still to prefill
    matched: int = 0          # prompt ids taken from the prefix cache (a multiple of page_tokens)
    sampling: Optional[SlotSampling] = None   # the request's own entry (None: the batcher's sampling)


def prefill_runs(admitted: Sequence[Request]) -> List[List[Request]]:
    """Split requests (in admission order) into runs that one qie_prefill_batch call can
    take: consecutive slots, equal prompt lengths."""
    runs: List[List[Request]] = []
    for r in admitted:
        prev = runs[-1][-1] if runs else None
        if prev is not None and r.slot == prev.slot + 1 and len(r.prompt) == len(prev.prompt):
            runs[-1].append(r)
        else:
            runs.append([r])
    return runs


def ragged_segments(segments: Sequence[tuple]) -> List[tuple]:
    """Batch.prefill_ragged's argument check: (seq, ids) or (seq, ids, pos0) items -> a list of
    (seq, ids, pos0) with ids a list of ints and pos0 = 0 where omitted.  ValueError for an empty
    list, an empty ids, a malformed item or slots that are not strictly increasing."""
    out: List[tuple] = []
    for item in segments:
        if len(item) not in (2, 3):
            raise ValueError("prefill_ragged: a segment is (seq, ids) or (seq, ids, pos0)")
        seq, ids = int(item[0]), [int(t) for t in item[1]]
        pos0 = int(item[2] or 0) if len(item) == 3 else 0
        if not ids:
            raise ValueError(f"prefill_ragged: segment of slot {seq} has no ids")
        if out and seq <= out[-1][0]:
            raise ValueError("prefill_ragged: slots must be strictly increasing")
        out.append((seq, ids, pos0))
    if not out:
        raise ValueError("prefill_ragged: needs one or more segments")
    return out


def ragged_group(pieces: Sequence[tuple]) -> List[tuple]:
    """Prompt pieces (request, offset, length) that would be prefilled back to back -> the
    segments of the one Batch.prefill_ragged call that replaces those calls: (slot, ids, pos0) in
    slot order; a piece at offset 0 starts its sequence, a later one extends it at its offset."""
    return sorted(((r.slot, r.prompt[off:off + n], off) for r, off, n in pieces), key=lambda s: s[0])


VERIFY_MAX_ROWS = 16   # QIE_VERIFY_MAX_ROWS: rows of one verify step
VERIFY_MAX_SEGS = 8    # QIE_RAGGED_MAX_SEGS: slots of one verify step


def draft_cap(draft_tokens: int, max_new_tokens: int, emitted: int, pos: int, max_ctx: int) -> int:
    """How many drafts a slot may propose: min(draft_tokens, max_new_tokens - emitted - 1, context
    room), never negative.  A verify step of k drafts emits at most k + 1 tokens and writes K/V
    rows pos .. pos + k, so the request never over-emits and its writes stay inside the pages
    promised at admission (prompt + max_new_tokens); room: pos + k + 1 < max_ctx."""
    return max(0, min(int(draft_tokens), max_new_tokens - emitted - 1, max_ctx - pos - 2))


def deal_verify_rows(proposed: Sequence[tuple], max_rows: int = VERIFY_MAX_ROWS,
                     max_segs: int = VERIFY_MAX_SEGS) -> List[tuple]:
    """The table of one batcher step's Batch.verify_batch call.  proposed: (slot, ids) of every
    slot that emits this step, in slot order, ids already capped (draft_cap); at most max_segs of
    them (a batch has no more slots: ValueError).  Returns a list of (slot, draft): every slot has
    its one row, and the max_rows - (segments) spare rows are dealt one at a time in slot order,
    round-robin, among the slots that still have proposed ids left.  [] when no slot proposed
    anything: the step is then the plain decode step."""
    group = list(proposed)
    if len(group) > max_segs:
        raise ValueError(f"deal_verify_rows: {len(group)} slots, a verify step takes {max_segs}")
    if not any(ids for _, ids in group):
        return []
    take = [0] * len(group)
    spare = max_rows - len(group)
    while spare > 0:
        dealt = False
        for i, (_, ids) in enumerate(group):
            if spare > 0 and take[i] < len(ids):
                take[i] += 1
                spare -= 1
                dealt = True
        if not dealt:
            break
    return [(slot, list(ids[:take[i]])) for i, (slot, ids) in enumerate(group)]


def prefill_chunks(n: int, chunk: Optional[int]) -> List[tuple]:
    """(offset, length) pieces in which a prompt of n ids is prefilled: the whole prompt when
    chunk is None, else pieces of `chunk` ids with a shorter last one.  The first piece starts
    the sequence (qie_prefill), every later one extends it at its offset (qie_prefill_append)."""
    if n < 1:
        raise ValueError("prefill_chunks: empty prompt")
    if chunk is None:
        return [(0, n)]
    if chunk < 1:
        raise ValueError("prefill_chunks: chunk must be >= 1")
    return [(off, min(chunk, n - off)) for off in range(0, n, chunk)]


def score_pieces(ids: Sequence[int], chunk: Optional[int] = None, pos0: int = 0) -> List[tuple]:
    """(position, piece ids, piece targets) calls in which Batch.score scores `ids` laid at
    positions pos0 .. pos0+n-1: the pieces of prefill_chunks, row i of the text targeting
    ids[i + 1] — so the last row of a middle piece targets the next piece's first id — and the
    text's last row targeting nothing (-1)."""
    ids = [int(t) for t in ids]
    if pos0 < 0:
        raise ValueError("score_pieces: pos0 must be >= 0")
    targets = ids[1:] + [-1]
    return [(pos0 + off, ids[off:off + n], targets[off:off + n]) for off, n in prefill_chunks(len(ids), chunk)]


def longest_prefix_match(prompt: Sequence[int], cached: Sequence[Sequence[int]], page_tokens: int) -> tuple:
    """(n, index): the longest page-aligned prefix of `prompt` that one of the id lists in
    `cached` begins with — n ids, a multiple of page_tokens — and which list (the first of
    equally long matches); (0, -1) without one.  n is capped at
    ((len(prompt) - 1) // page_tokens) * page_tokens, so at least one id is left to append."""
    cap = ((len(prompt) - 1) // page_tokens) * page_tokens if len(prompt) else 0
    best, idx = 0, -1
    for i, ids in enumerate(cached):
        lim = min(cap, (len(ids) // page_tokens) * page_tokens)
        n = 0
        while n < lim and prompt[n] == ids[n]:
            n += 1
        n = (n // page_tokens) * page_tokens
        if n > best:
            best, idx = n, i
    return best, idx


@dataclasses.dataclass
class CacheEntry:
    prefix: object            # engine.Prefix
    ids: List[int]
    pages: List[int]          # the pool pages it references
    used: int = 0             # the batcher's clock at its last save / hit (least recently used goes first)


class ContinuousBatcher:
    def __init__(self, engine: Engine, slots: int = 8, max_ctx: Optional[int] = None, page_tokens: int = 128,
                 n_pages: int = 0, sampling: Sampling = GREEDY, keep_logits: bool = False,
                 prefill_chunk: Optional[int] = None, keep_logprobs: bool = False, prefix_cache_pages: int = 0,
                 ragged_prefill: bool = False, drafter=None, draft_tokens: int = 4):
        # drafter: speculative decoding for the whole batch.  An object with
        # propose(history, k) (NgramDrafter) shared by all requests, or — for drafters that keep
        # state — a factory called once per request.  Each step every emitting slot proposes up
        # to draft_tokens ids (draft_cap) and ONE Batch.verify_batch call (deal_verify_rows)
        # replaces the decode step; a step in which no slot proposes anything is the plain decode
        # step.  None: exactly the calls made without it.  Greedy streams are token for token
        # those of plain decode steps from the same logits.  On a use_graph engine a step is
        # captured per table (which slots, how many drafts each): a table the bounded cache has
        # not seen pays a capture first ("first call": 0.5 - 0.9 ms on
        # Qwen2-7B; the hit rate of a real request mix has not been measured).
        self.drafter = drafter
        self.draft_tokens = int(draft_tokens)
        if drafter is not None and not 0 <= self.draft_tokens <= VERIFY_MAX_ROWS - 1:
            raise ValueError(f"draft_tokens must be in [0, {VERIFY_MAX_ROWS - 1}]")
        self._drafters: Dict[int, object] = {}   # per request, when `drafter` is a factory
        # verify_calls, drafted (ids handed to verify_batch), accepted (drafts the model agreed
        # with), emitted (every token the batcher emitted, on any path)
        self.stats: Dict[str, int] = dict(verify_calls=0, drafted=0, accepted=0, emitted=0)
        # ragged_prefill: wherever several prefill / append calls would follow each other with
        # nothing in between (an admitted group, a flush of whole prompts, the chunks advanced in
        # one step), ONE Batch.prefill_ragged call over the group instead — one pass over the
        # weights.  A group of one stays the plain call.  False: exactly the calls made without it.
        self.ragged_prefill = bool(ragged_prefill)
        # prefix_cache_pages > 0: prompts' page-aligned prefixes stay cached on shared KV pages
        # (Batch.save_prefix) and a later prompt that begins alike loads them instead of
        # prefilling them again; at most that many pages are held by the cache alone.  0: off,
        # the batcher makes exactly the calls it made without the cache.
        self.prefix_cache_pages = int(prefix_cache_pages)
        self.cache: List[CacheEntry] = []
        self.prefix_hits = 0
        self.prefix_tokens_reused = 0
        self._clock = 0
        # prefill_chunk: a prompt longer than this takes its first chunk at admission and one
        # more chunk per step() (qie_prefill_append), so an admission stalls the live slots for
        # one chunk's prefill at a time; its first token is emitted after the last chunk
        self.prefill_chunk = prefill_chunk
        self.batch: Batch = engine.batch(slots, max_ctx, page_tokens=page_tokens, n_pages=n_pages)
        self.keep_logits = keep_logits          # copy each token's logit row (tests / diagnostics)
        # each emitted token's log-probability into Request.logprobs (Batch.logprobs: one float
        # per slot comes back, no [B][V] host copy)
        self.keep_logprobs = keep_logprobs
        self.max_ctx = self.batch.max_ctx
        self.sampling = sampling
        free, _, self.page_tokens = self.batch.page_stats()
        self.budget = free                      # pages not promised to an admitted request
        self.waiting: Deque[Request] = collections.deque()
        self.slots: List[Optional[Request]] = [None] * slots
        self.requests: Dict[int, Request] = {}
        self._next = 0

    def _pages(self, n_tokens: int) -> int:
        return -(-n_tokens // self.page_tokens)

    def submit(self, prompt: Sequence[int], max_new_tokens: int, stop_ids: Sequence[int] = (),
               sampling: Optional[SlotSampling] = None, penalize_prompt: bool = True) -> int:
        n = len(prompt)
        if n < 1 or max_new_tokens < 1 or n + max_new_tokens > self.max_ctx - 1:
            raise ValueError(f"request of {n} + {max_new_tokens} tokens does not fit max_ctx {self.max_ctx}")
        if self._pages(n + max_new_tokens) > self.budget + sum(r.pages for r in self.slots if r):
            raise ValueError("request larger than the whole page pool")
        r = Request(self._next, [int(t) for t in prompt], int(max_new_tokens), tuple(int(s) for s in stop_ids))
        if sampling is not None:   # penalize_prompt=False: the penalties see generated tokens only
            r.sampling = sampling if penalize_prompt else dataclasses.replace(sampling, penalty_start=n)
        self._next += 1
        self.requests[r.rid] = r
        self.waiting.append(r)
        return r.rid

    def _take_slot(self, r: Request) -> None:
        """The request's own entry goes onto its slot before anything of it is prefilled."""
        if r.sampling is not None:
            self.batch.set_sampling(r.slot, r.sampling)

    def _finish(self, r: Request) -> None:
        r.done = True
        self._drafters.pop(r.rid, None)
        if r.sampling is not None:
            self.batch.set_sampling(r.slot, None)
        self.batch.release(r.slot)
        self.slots[r.slot] = None
        self.budget += r.pages
        r.slot = -1
        if self.prefix_cache_pages > 0:
            self._trim_cache()   # pages the finished request shared with the cache are now the cache's alone

    def _logprobs(self, toks: Dict[int, int]):
        """Log-probability of toks[slot] under each of those slots' current logits (None when
        not kept); read before anything overwrites the rows."""
        if not self.keep_logprobs or not toks:
            return None
        return self.batch.logprobs([toks.get(i, -1) for i in range(len(self.slots))])

    def _emit(self, r: Request, tok: int, out: list, logits=None, lps=None) -> None:
        row = lp = None
        if self.keep_logits:
            row = (self.batch.logits() if logits is None else logits)[r.slot]
        if self.keep_logprobs:
            lp = (self._logprobs({r.slot: tok}) if lps is None else lps)[r.slot]
        self._emit_row(r, tok, out, row, lp)

    def _emit_row(self, r: Request, tok: int, out: list, row, lp) -> None:
        """The token with its logits row / log-probability (None where not kept); a stop id or
        the token budget ends the request at this token."""
        r.tokens.append(tok)
        if self.keep_logits:
            r.logits.append(row.copy())
        if self.keep_logprobs:
            r.logprobs.append(float(lp))
        out.append((r.rid, tok))
        self.stats["emitted"] += 1
        if len(r.tokens) >= r.max_new_tokens or tok in r.stop_ids:
            self._finish(r)

    # ------------------------------------------------------------ prefix cache
    # Accounting with the cache on reads the pool itself: a request needs pages(prompt +
    # max_new_tokens) minus the pages it shares with its match (Request.pages), and is admitted
    # when that fits in the pool's free pages minus what the live requests have not drawn yet.
    # Nothing the batcher does writes into a shared page (a loaded slot appends and decodes from
    # its match's end, a page boundary; a slot is saved only once its whole prompt is cached), so
    # no call makes a private copy and every admitted request's pages are there when it draws them.
    def _room(self) -> int:
        free, per, _ = self.batch.page_stats()
        owed = sum(max(0, r.pages - (int(per[r.slot]) - r.matched // self.page_tokens)) for r in self.slots if r)
        return free - owed

    def _cache_only_pages(self) -> int:
        refs = self.batch.page_refs()
        holders = collections.Counter(p for e in self.cache for p in e.pages)
        return sum(1 for p, c in holders.items() if int(refs[p]) == c)

    def _evict(self, keep: Optional[CacheEntry] = None) -> bool:
        """Drops the least recently used entry (`keep` only when nothing else is left)."""
        if not self.cache:
            return False
        rest = [e for e in self.cache if e is not keep] or self.cache
        e = min(rest, key=lambda x: x.used)
        e.prefix.drop()
        self.cache.remove(e)
        return True

    def _trim_cache(self) -> None:
        while self.cache and self._cache_only_pages() > self.prefix_cache_pages:
            self._evict()

    def drop_cache(self) -> None:
        while self._evict():
            pass

    def _save(self, r: Request) -> None:
        """The request's whole prompt is cached: one handle for its page-aligned part, unless an
        entry already covers it."""
        n = (len(r.prompt) // self.page_tokens) * self.page_tokens
        if n == 0 or any(len(e.ids) >= n and e.ids[:n] == r.prompt[:n] for e in self.cache):
            return
        self._clock += 1
        pages = [int(p) for p in self.batch.block_table(r.slot, n // self.page_tokens)]
        self.cache.append(CacheEntry(self.batch.save_prefix(r.slot, n), r.prompt[:n], pages, self._clock))
        self._trim_cache()

    def _prefill_pieces(self, pieces: List[tuple]) -> Dict[int, int]:
        """ragged_prefill: the (request, offset, length) pieces in one pass; returns the token
        after each piece by request id.  One piece is the plain call."""
        if len(pieces) == 1:
            r, off, n = pieces[0]
            ids = r.prompt[off:off + n]
            if off:
                return {r.rid: self.batch.append(r.slot, ids, off, self.sampling)}
            return {r.rid: self.batch.prefill(r.slot, ids, self.sampling)}
        toks = self.batch.prefill_ragged(ragged_group(pieces), self.sampling)
        by_slot = {r.slot: r for r, _, _ in pieces}
        return {by_slot[slot].rid: tok for slot, tok in zip(sorted(by_slot), toks)}

    def _prefill_whole(self, whole: List[Request]) -> Dict[int, int]:
        """First tokens of whole prompts by request id: one ragged pass, or the runs
        prefill_runs groups them into."""
        if self.ragged_prefill:
            return self._prefill_pieces([(r, 0, len(r.prompt)) for r in whole])
        first: Dict[int, int] = {}
        for run in prefill_runs(whole):
            if len(run) == 1:
                first[run[0].rid] = self.batch.prefill(run[0].slot, run[0].prompt, self.sampling)
            else:
                toks = self.batch.prefill_batch(run[0].slot, [r.prompt for r in run], self.sampling)
                first.update((r.rid, t) for r, t in zip(run, toks))
        return first

    def _flush_whole(self, whole: List[Request], out: list) -> None:
        """Prefills the admitted whole prompts without a match (grouped as prefill_runs groups
        them), saves them and emits their first tokens in admission order."""
        if not whole:
            return
        first = self._prefill_whole(whole)
        lg = self.batch.logits() if self.keep_logits else None
        lps = self._logprobs({r.slot: first[r.rid] for r in whole})
        for r in whole:
            self._save(r)
        for r in whole:
            self._emit(r, first[r.rid], out, lg, lps)
        whole.clear()

    def _admit_cached(self, out: list) -> None:
        T = self.page_tokens
        whole: List[Request] = []   # admitted, no match, not chunked: prefilled together at the next flush
        while self.waiting:
            r = self.waiting[0]
            free_slot = next((i for i, s in enumerate(self.slots) if s is None), None)
            if free_slot is None:
                break
            # a request admitted just before may hold this one's prefix: cache it first
            if whole and longest_prefix_match(r.prompt, [w.prompt for w in whole], T)[0] > 0:
                self._flush_whole(whole, out)
                continue   # (a request that finished at its first token freed a slot)
            total = self._pages(len(r.prompt) + r.max_new_tokens)
            n, idx = longest_prefix_match(r.prompt, [e.ids for e in self.cache], T)
            entry = self.cache[idx] if n else None
            # Only a whole prompt without a match may wait in `whole`.  Anything else prefills now,
            # and the pending run goes first — BEFORE this request is accounted: the flush saves
            # entries and may finish requests, and either can trim the cache, the matched entry
            # included.  So flush and look the request up again; from the lookup below to
            # load_prefix nothing then touches the cache but the eviction loop, which keeps `entry`.
            if whole and (n or len(prefill_chunks(len(r.prompt), self.prefill_chunk)) > 1):
                self._flush_whole(whole, out)
                continue
            # (_room counts the requests of `whole` too: they hold their slots and have drawn nothing)
            while total - n // T > self._room() and self._evict(keep=entry):
                if entry is not None and entry not in self.cache:
                    n, entry = 0, None
            need = total - n // T
            if need > self._room():
                break                           # FIFO: later requests wait behind the head
            self.waiting.popleft()
            r.slot, r.pages, r.matched = free_slot, need, n
            self.budget -= need
            self.slots[free_slot] = r
            self._take_slot(r)
            if n:
                self._clock += 1
                entry.used = self._clock
                self.prefix_hits += 1
                self.prefix_tokens_reused += n
            pieces = [(n + off, m) for off, m in prefill_chunks(len(r.prompt) - n, self.prefill_chunk)]
            if not n and len(pieces) == 1:
                whole.append(r)
                continue
            assert not whole and (entry is None or entry in self.cache)
            # pieces that follow a match are singletons; the first piece of an unmatched chunked
            # prompt starts the sequence
            off, m = pieces[0]
            if n:
                self.batch.load_prefix(entry.prefix, r.slot, r.prompt[n], n)
                tok = self.batch.append(r.slot, r.prompt[off:off + m], off, self.sampling)
            else:
                tok = self.batch.prefill(r.slot, r.prompt[:m], self.sampling)
            r.chunks = pieces[1:]
            if not r.chunks:
                self._save(r)
                self._emit(r, tok, out)
        self._flush_whole(whole, out)

    def _admit(self, out: list) -> None:
        if self.prefix_cache_pages > 0:
            return self._admit_cached(out)
        admitted: List[Request] = []
        while self.waiting:
            r = self.waiting[0]
            need = self._pages(len(r.prompt) + r.max_new_tokens)
            free_slot = next((i for i, s in enumerate(self.slots) if s is None), None)
            if free_slot is None or need > self.budget:
                break                           # FIFO: later requests wait behind the head
            self.waiting.popleft()
            r.slot, r.pages = free_slot, need
            self.budget -= need
            self.slots[free_slot] = r
            self._take_slot(r)
            admitted.append(r)
        # equal-length prompts landing in consecutive slots prefill in one pass
        # (qie_prefill_batch); tokens are emitted in admission order afterwards
        # (ragged_prefill: the first pieces and the whole prompts in one pass)
        first: Dict[int, int] = {}
        whole: List[Request] = []
        started: List[tuple] = []
        for r in admitted:
            pieces = prefill_chunks(len(r.prompt), self.prefill_chunk)
            if len(pieces) > 1:   # chunked: the first piece now, its token is not the request's
                if self.ragged_prefill:
                    started.append((r, 0, pieces[0][1]))
                else:
                    self.batch.prefill(r.slot, r.prompt[:pieces[0][1]], self.sampling)
                r.chunks = pieces[1:]
            else:
                whole.append(r)
        if self.ragged_prefill and started:
            first = self._prefill_pieces(started + [(r, 0, len(r.prompt)) for r in whole])
        elif whole:
            first = self._prefill_whole(whole)
        lg = self.batch.logits() if self.keep_logits and whole else None
        lps = self._logprobs({r.slot: first[r.rid] for r in whole})
        for r in whole:
            self._emit(r, first[r.rid], out, lg, lps)

    def _advance_chunks(self, out: list, fresh: set) -> None:
        """One more prompt piece for every slot still in chunked prefill (not the requests
        admitted in this step: they took their piece at admission).  pos0 is explicit: the
        decode step that ran since the last piece wrote one row at the slot's position, and this
        piece overwrites it."""
        due = [r for r in self.slots if r is not None and r.chunks and r.rid not in fresh]
        toks: Dict[int, int] = {}
        if self.ragged_prefill and due:   # every piece of this step in one pass
            toks = self._prefill_pieces([(r,) + r.chunks.pop(0) for r in due])
        for r in due:
            if self.ragged_prefill:
                tok = toks[r.rid]
            else:
                off, n = r.chunks.pop(0)
                tok = self.batch.append(r.slot, r.prompt[off:off + n], off, self.sampling)
            if not r.chunks:
                if self.prefix_cache_pages > 0:
                    self._save(r)
                self._emit(r, tok, out)

    def _propose(self, r: Request) -> List[int]:
        """The request's capped proposal for this step (ids the model lacks cut it short)."""
        pos = len(r.prompt) + len(r.tokens) - 1   # the pending token's position
        k = draft_cap(self.draft_tokens, r.max_new_tokens, len(r.tokens), pos, self.max_ctx)
        if k <= 0:
            return []
        d = self.drafter
        if isinstance(d, type) or not hasattr(d, "propose"):   # a factory (a class is one): one drafter per request
            d = self._drafters.get(r.rid)
            if d is None:
                d = self._drafters[r.rid] = self.drafter()
        vocab = self.batch.e.spec.vocab
        ids: List[int] = []
        for t in list(d.propose(r.prompt + r.tokens, k))[:k]:
            if not 0 <= int(t) < vocab:
                break
            ids.append(int(t))
        return ids

    def _verify_step(self, out: list) -> bool:
        """The step's tokens through Batch.verify_batch when some slot has a draft (False: none
        has, the caller runs the plain decode step).  Slots in chunked prefill are not in the
        table and do not advance.  Tokens are emitted in slot order, each slot's in order; a
        request that ends inside its accepted tokens is released there, so nothing is rewound."""
        emit = [r for r in self.slots if r is not None and not r.done and not r.chunks]
        table = deal_verify_rows([(r.slot, self._propose(r)) for r in emit])
        if not table:
            return False
        got = self.batch.verify_batch(table, self.sampling)
        self.stats["verify_calls"] += 1
        self.stats["drafted"] += sum(len(d) for _, d in table)
        self.stats["accepted"] += sum(len(ids) - 1 for ids in got)
        lg = self.batch.verify_logits() if self.keep_logits else None
        lps = None
        if self.keep_logprobs:   # row0[z] + i holds segment z's token i; the other rows are skipped
            want: List[int] = []
            for (_, d), ids in zip(table, got):
                want += list(ids) + [-1] * (len(d) + 1 - len(ids))
            lps = self.batch.verify_logprobs(want)
        row0 = 0
        for (slot, d), ids in zip(table, got):
            r = self.slots[slot]
            for i, tok in enumerate(ids):
                self._emit_row(r, int(tok), out, None if lg is None else lg[row0 + i],
                               None if lps is None else lps[row0 + i])
                if r.done:
                    break
            row0 += len(d) + 1
        return True

    def step(self) -> List[tuple]:
        """Admit what fits, then one decode step for every slot (with a drafter: one verify step
        over the emitting slots when any of them has a draft); returns the (request id, token)
        pairs produced, in slot order."""
        out: List[tuple] = []
        before = {r.rid for r in self.slots if r is not None}
        self._admit(out)
        self._advance_chunks(out, {r.rid for r in self.slots if r is not None} - before)
        if any(s is not None for s in self.slots):
            if self.drafter is not None and self._verify_step(out):
                return out
            live = list(self.slots)
            ids = self.batch.decode_step(self.sampling)
            lg = self.batch.logits() if self.keep_logits else None
            # a slot still in chunked prefill decodes too (fixed-B step); its output is dropped
            emit = [(i, r) for i, r in enumerate(live) if r is not None and not r.done and not r.chunks]
            lps = self._logprobs({i: int(ids[i]) for i, _ in emit})
            for i, r in emit:
                self._emit(r, int(ids[i]), out, lg, lps)
        return out

    def idle(self) -> bool:
        return not self.waiting and all(s is None for s in self.slots)

    def run(self) -> Dict[int, List[int]]:
        while not self.idle():
            self.step()
        return {rid: r.tokens for rid, r in self.requests.items()}

    def close(self) -> None:
        self.batch.close()
