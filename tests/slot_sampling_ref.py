"""The per-slot sampling contract (include/qie/qie_ops.h, qie_sample_rows) restated in numpy
float32, operation by operation; selection and the draw are the CPU oracle's on the processed
bf16 row (oracle.argmax / oracle.sample), so nothing here shares code with the kernels.

    v = f32(l[j])
    if c[j] > 0:
        v = (v > 0) ? v / repetition_penalty : v * repetition_penalty      (skipped when == 1)
        t = frequency_penalty * (float)c[j];  t = presence_penalty + t;  v = v - t
    if j is biased:  v = v + bias
    l'[j] = bf16_rne(v)            (an element with c[j] == 0 and no bias keeps its bits)

Entries are qwen_inference_engine_amd.SlotSampling objects."""
import collections

import numpy as np

F = np.float32
U64 = (1 << 64) - 1


def neutral(e) -> bool:
    return e.repetition_penalty == 1.0 and e.presence_penalty == 0.0 and e.frequency_penalty == 0.0


def window_ids(e, hist, q, tail=()):
    """The window of a row whose input token sits at position q: the ids at positions [lo, q] of
    the history row `hist` (its length is max_ctx), the last len(tail) of them replaced by
    `tail` (a verify row's drafts).  Positions at or past max_ctx are not read."""
    lo = max(int(e.penalty_start), q + 1 - int(e.penalty_last_n) if e.penalty_last_n > 0 else 0, 0)
    n = len(tail)
    hh = min(q - n, len(hist) - 1)
    ids = [int(hist[p]) for p in range(lo, hh + 1)]
    t0 = max(0, lo - (q - n + 1))
    return ids + [int(t) for t in tail[t0:]]


def process(oracle, row, e, ids):
    """The processed bf16 row l' of the bf16 row `row` (uint16 bits) under entry e and window ids."""
    row = np.ascontiguousarray(row, np.uint16)
    V = row.size
    f = oracle.bf16_to_f32(row)
    touched = {}
    with np.errstate(all="ignore"):
        if not neutral(e):   # with the three penalties neutral the window is not walked
            for j, c in collections.Counter(i for i in ids if 0 <= i < V).items():
                v = F(f[j])
                if F(e.repetition_penalty) != F(1.0):
                    v = F(v / F(e.repetition_penalty)) if v > 0 else F(v * F(e.repetition_penalty))
                t = F(F(e.frequency_penalty) * F(c))
                t = F(F(e.presence_penalty) + t)
                touched[j] = F(v - t)
        for j, bias in e.bias.items():
            if 0 <= j < V:
                touched[j] = F(F(touched.get(j, f[j])) + F(bias))
    out = row.copy()
    for j, v in touched.items():
        out[j] = oracle.f32_to_bf16(np.array([v], F))[0]
    return out


def min_p_keep(oracle, lp, e):
    """(kept, margin): how many of the k = min(top_k, 256, V) sorted candidates min-p keeps (a
    prefix: the weights are non-increasing), and the smallest relative distance of any weight
    from min_p (inf without min-p) — a choice is only as sure as that margin is above the
    difference between two expf implementations."""
    k = min(int(e.top_k), 256, lp.size)
    if not (0.0 < e.min_p <= 1.0):
        return k, float("inf")
    _, val = oracle.topk(lp, k)
    if val.size == 0:
        return k, float("inf")
    with np.errstate(all="ignore"):
        v = (val.astype(F) / F(e.temperature)).astype(F)
        w = np.exp((v - v.max()).astype(F)).astype(F)
    kept = 1
    while kept < w.size and w[kept] >= F(e.min_p):
        kept += 1
    if w.size < 2:   # entry 0 stays whatever its weight
        return kept, float("inf")
    margin = float(np.min(np.abs(w[1:].astype(np.float64) - float(F(e.min_p))) / float(F(e.min_p))))
    return kept, margin


def choose(oracle, row, e, ids, step):
    """(chosen id, min-p margin) of a row under entry e, window ids and step counter `step`."""
    lp = process(oracle, row, e, ids)
    if e.top_k <= 1 or not (e.temperature > 0):
        return oracle.argmax(lp), float("inf")
    kept, margin = min_p_keep(oracle, lp, e)
    return oracle.sample(lp, kept, e.temperature, e.top_p, (int(e.seed) + int(step)) & U64), margin
