"""Speculative decoding over ``Batch.verify`` (qie_verify).

A drafter guesses the next k tokens; one verify pass over the target's weights scores the
pending token and all k guesses, and the target keeps its own choices up to the first guess
it disagrees with.  The emitted stream is the target's own (greedy: token for token what
plain decode steps would pick from the same logits), so a drafter only changes how many
tokens a weight pass yields, never which.

Drafters implement ``propose(history, k) -> list of at most k ids``, where ``history`` is
every token so far (prompt and generated, the last one being the pending current token):

* ``NgramDrafter``: prompt-lookup — continue the most recent earlier occurrence of the
  history's longest recent suffix.  Pure Python, no model.
* ``ModelDrafter``: greedy steps of a second, smaller ``Engine`` / ``Batch`` kept in step
  with the target's accepted history.

``SpeculativeDecoder`` drives one sequence.  For many requests at once hand a drafter to
``ContinuousBatcher(drafter=...)``: it verifies every slot's drafts in one ``Batch.verify_batch``
pass per step; a ``ModelDrafter`` shared across slots is not supported there.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

from . import _lib
from .engine import GREEDY, Sampling

MAX_DRAFT = _lib.QIE_VERIFY_MAX_ROWS - 1


class NgramDrafter:
    """Finds the longest suffix of `history` (n from max_ngram down to min_ngram tokens) that
    also occurred earlier in it and proposes the tokens that followed its most recent earlier
    occurrence.  Deterministic; [] when no suffix recurs."""

    def __init__(self, max_ngram: int = 3, min_ngram: int = 1):
        if not 1 <= min_ngram <= max_ngram:
            raise ValueError("NgramDrafter: need 1 <= min_ngram <= max_ngram")
        self.max_ngram, self.min_ngram = max_ngram, min_ngram

    def propose(self, history: Sequence[int], k: int) -> List[int]:
        h = list(history)
        if k <= 0:
            return []
        for n in range(self.max_ngram, self.min_ngram - 1, -1):
            if len(h) <= n:
                continue
            suffix = h[-n:]
            for i in range(len(h) - n - 1, -1, -1):   # most recent earlier occurrence first
                if h[i:i + n] == suffix:
                    return h[i + n:i + n + k]
        return []


class ModelDrafter:
    """Proposes k greedy decode steps of a draft model (slot `seq` of `draft_batch`, a batch of
    a second Engine, e.g. Qwen2-0.5B for a 7B target; use a batch of one slot, since a decode
    step advances every slot).  The draft sequence follows the target's accepted history:
    tokens it has not seen are appended (``Batch.append``), rejected guesses are rewound
    (``Batch.set_position``).  Vocabularies may differ: a proposal is cut before the first id
    outside `target_vocab` (SpeculativeDecoder sets it), and a history token outside the
    draft's vocabulary raises ValueError."""

    def __init__(self, draft_batch, seq: int = 0, target_vocab=None):
        self.b, self.seq = draft_batch, seq
        self.target_vocab = target_vocab
        self.vocab = draft_batch.e.spec.vocab
        self._seen: List[int] = []   # tokens the draft sequence was fed, the last one pending
        self._kv = 0                 # K/V rows [0, _kv) of the draft cache hold _seen[:_kv]

    def propose(self, history: Sequence[int], k: int) -> List[int]:
        h = [int(t) for t in history]
        if not h:
            return []
        bad = [t for t in h if not 0 <= t < self.vocab]
        if bad:
            raise ValueError(f"ModelDrafter: token {bad[0]} is outside the draft model's vocabulary ({self.vocab})")
        n = len(h)
        k = min(k, self.b.max_ctx - n - 1)   # the draft sequence must stay below its max_ctx
        if k <= 0:
            return []
        common = 0
        for a, c in zip(self._seen, h):
            if a != c:
                break
            common += 1
        keep = min(common, self._kv, n - 1)   # cached rows that still belong to this history
        if keep == 0:
            if n > 1:
                self.b.prefill(self.seq, h[:n - 1])
        elif keep < n - 1:
            self.b.append(self.seq, h[keep:n - 1], pos0=keep)
        self.b.set_position(self.seq, n - 1, h[-1])   # the pending token (rewinds past rejected guesses)
        out = [int(self.b.decode_step()[self.seq]) for _ in range(k)]
        self._seen = h + out
        self._kv = n - 1 + k
        if self.target_vocab is not None:
            for i, t in enumerate(out):
                if t >= self.target_vocab:
                    return out[:i]
        return out


class SpeculativeDecoder:
    """generate(): prefill, then propose / verify until max_new tokens or a stop id.

    `k` drafts per verify call (at most 15).  ``stats`` after a run: ``verify_calls``,
    ``drafted`` (ids handed to verify), ``accepted`` (drafts the target agreed with) and
    ``emitted`` (tokens returned, the prefill's first token included)."""

    def __init__(self, batch, drafter, seq: int = 0, k: int = 4):
        if not 0 <= k <= MAX_DRAFT:
            raise ValueError(f"SpeculativeDecoder: k must be in [0, {MAX_DRAFT}]")
        self.b, self.drafter, self.seq, self.k = batch, drafter, seq, k
        self.stats: Dict[str, int] = dict(verify_calls=0, drafted=0, accepted=0, emitted=0)
        if getattr(drafter, "target_vocab", 0) is None:
            drafter.target_vocab = batch.e.spec.vocab

    def generate(self, prompt: Sequence[int], max_new: int, sampling: Sampling = GREEDY,
                 stop_ids: Sequence[int] = ()) -> List[int]:
        self.stats = dict(verify_calls=0, drafted=0, accepted=0, emitted=0)
        if max_new <= 0:
            return []
        stop = set(int(t) for t in stop_ids)
        vocab = self.b.e.spec.vocab
        history = [int(t) for t in prompt]
        tok = int(self.b.prefill(self.seq, history, sampling))
        out = [tok]
        history.append(tok)
        while len(out) < max_new and tok not in stop:
            pos = len(history) - 1                       # position of the pending token
            room = self.b.max_ctx - pos - 2              # drafts the context still takes
            if room < 0:
                break
            k = min(self.k, max_new - len(out) - 1, room)
            draft = [int(t) for t in self.drafter.propose(history, k)][:k] if k > 0 else []
            for i, t in enumerate(draft):                # never hand the target an id it lacks
                if not 0 <= t < vocab:
                    draft = draft[:i]
                    break
            ids = self.b.verify(self.seq, draft, sampling)
            self.stats["verify_calls"] += 1
            self.stats["drafted"] += len(draft)
            self.stats["accepted"] += len(ids) - 1
            for i, t in enumerate(ids):
                out.append(t)
                history.append(t)
                tok = t
                if t in stop:
                    if i + 1 < len(ids):                 # the batch ran ahead of the stop: rewind onto it
                        self.b.set_position(self.seq, pos + i + 1, t)
                    break
        self.stats["emitted"] = len(out)
        return out
