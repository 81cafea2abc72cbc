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

One sampling configuration per batcher (``qie_sampling`` is per step); slot rows are
independent, so a request's tokens do not depend on what the other slots hold.
"""
from __future__ import annotations

import collections
import dataclasses
from typing import Deque, Dict, List, Optional, Sequence

from .engine import GREEDY, Batch, Engine, Sampling


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


class ContinuousBatcher:
    def __init__(self, engine: Engine, slots: int = 8, max_ctx: Optional[int] = None, page_tokens: int = 128,
                 n_pages: int = 0, sampling: Sampling = GREEDY, keep_logits: bool = False,
                 prefill_chunk: Optional[int] = None, keep_logprobs: bool = False):
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

    def submit(self, prompt: Sequence[int], max_new_tokens: int, stop_ids: Sequence[int] = ()) -> int:
        n = len(prompt)
        if n < 1 or max_new_tokens < 1 or n + max_new_tokens > self.max_ctx - 1:
            raise ValueError(f"request of {n} + {max_new_tokens} tokens does not fit max_ctx {self.max_ctx}")
        if self._pages(n + max_new_tokens) > self.budget + sum(r.pages for r in self.slots if r):
            raise ValueError("request larger than the whole page pool")
        r = Request(self._next, [int(t) for t in prompt], int(max_new_tokens), tuple(int(s) for s in stop_ids))
        self._next += 1
        self.requests[r.rid] = r
        self.waiting.append(r)
        return r.rid

    def _finish(self, r: Request) -> None:
        r.done = True
        self.batch.release(r.slot)
        self.slots[r.slot] = None
        self.budget += r.pages
        r.slot = -1

    def _logprobs(self, toks: Dict[int, int]):
        """Log-probability of toks[slot] under each of those slots' current logits (None when
        not kept); read before anything overwrites the rows."""
        if not self.keep_logprobs or not toks:
            return None
        return self.batch.logprobs([toks.get(i, -1) for i in range(len(self.slots))])

    def _emit(self, r: Request, tok: int, out: list, logits=None, lps=None) -> None:
        r.tokens.append(tok)
        if self.keep_logits:
            r.logits.append((self.batch.logits() if logits is None else logits)[r.slot].copy())
        if self.keep_logprobs:
            r.logprobs.append(float((self._logprobs({r.slot: tok}) if lps is None else lps)[r.slot]))
        out.append((r.rid, tok))
        if len(r.tokens) >= r.max_new_tokens or tok in r.stop_ids:
            self._finish(r)

    def _admit(self, out: list) -> None:
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
            admitted.append(r)
        # equal-length prompts landing in consecutive slots prefill in one pass
        # (qie_prefill_batch); tokens are emitted in admission order afterwards
        first: Dict[int, int] = {}
        whole: List[Request] = []
        for r in admitted:
            pieces = prefill_chunks(len(r.prompt), self.prefill_chunk)
            if len(pieces) > 1:   # chunked: the first piece now, its token is not the request's
                self.batch.prefill(r.slot, r.prompt[:pieces[0][1]], self.sampling)
                r.chunks = pieces[1:]
            else:
                whole.append(r)
        for run in prefill_runs(whole):
            if len(run) == 1:
                first[run[0].rid] = self.batch.prefill(run[0].slot, run[0].prompt, self.sampling)
            else:
                toks = self.batch.prefill_batch(run[0].slot, [r.prompt for r in run], self.sampling)
                first.update((r.rid, t) for r, t in zip(run, toks))
        lg = self.batch.logits() if self.keep_logits and whole else None
        lps = self._logprobs({r.slot: first[r.rid] for r in whole})
        for r in whole:
            self._emit(r, first[r.rid], out, lg, lps)

    def _advance_chunks(self, out: list, fresh: set) -> None:
        """One more prompt piece for every slot still in chunked prefill (not the requests
        admitted in this step: they took their piece at admission).  pos0 is explicit: the
        decode step that ran since the last piece wrote one row at the slot's position, and this
        piece overwrites it."""
        for r in self.slots:
            if r is None or not r.chunks or r.rid in fresh:
                continue
            off, n = r.chunks.pop(0)
            tok = self.batch.append(r.slot, r.prompt[off:off + n], off, self.sampling)
            if not r.chunks:
                self._emit(r, tok, out)

    def step(self) -> List[tuple]:
        """Admit what fits, then one decode step for every slot; returns the (request id,
        token) pairs produced, in slot order."""
        out: List[tuple] = []
        before = {r.rid for r in self.slots if r is not None}
        self._admit(out)
        self._advance_chunks(out, {r.rid for r in self.slots if r is not None} - before)
        if any(s is not None for s in self.slots):
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
