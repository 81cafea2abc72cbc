#!/usr/bin/env python3
"""What scoring a prompt costs over prefilling it: Qwen2-7B widths at full depth,
synthetic weights, n = 2,048 ids, bf16 weights and again weight_fp8.  Three calls:

  (a) qie_prefill            the layers + the last-row head (the baseline);
  (b) qie_score              the same + the default scoring head (bf16: the fused qie_score_rows;
                             weight_fp8 has no fused head, so (b) runs the general path as well);
  (c) qie_score with QIE_SCORE_UNFUSED   the <= 16-row head launches + qie_logprob_rows.

tools/verify_bench.py's method: every call ends in a stream synchronise (its ids come back to the
host), so a host clock around one call is its time.  ITERS calls per kind after WARM warm-up
calls, their median taken; the whole table REPS times with the kinds alternating; per cell the
median and the min / max over the repetitions.  head_added = score - prefill; the statement to
check is fused head_added < unfused head_added.

  tools/score_bench.py                      the table -> profiles/score_head.json
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qwen_inference_engine_amd as Q  # noqa: E402
from qwen_inference_engine_amd import spec as S, weights as W  # noqa: E402

N, MAX_CTX = 2048, 2048 + 32
ITERS, WARM, REPS = 5, 2, 3
OUT = os.path.join(ROOT, "profiles", "score_head.json")
KINDS = ("prefill", "score", "score_unfused")


def timed(eng, fn, n):
    out = []
    for _ in range(n):
        eng.sync()                               # the clock starts on an idle stream
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def table(fp8, n_layers, n):
    spec = S.QWEN2_7B if n_layers is None else S.QWEN2_7B.replace(n_layers=n_layers)
    eng = Q.Engine(spec, max_ctx=MAX_CTX, weight_fp8=fp8).init_synthetic(W.SynthParams(seed=0))
    b = eng.batch(1, MAX_CTX)
    ids = [int(t) for t in np.random.default_rng(3).integers(0, spec.vocab, n)]
    targets = ids[1:] + [-1]
    fns = {"prefill": lambda: b.prefill(0, ids),
           "score": lambda: b.score_rows(0, ids, targets),
           "score_unfused": lambda: b.score_rows(0, ids, targets, unfused=True)}
    cells = collections.defaultdict(list)
    for rep in range(REPS + 1):                  # repetition 0 warms every kind (scratch, LDS limits) and is dropped
        for kind in KINDS:
            ms = timed(eng, fns[kind], WARM if rep == 0 else ITERS)
            if rep:
                cells[kind].append(ms)
    r = {"n": n}
    for kind in KINDS:
        v = cells[kind]
        r[kind + "_ms"] = round(statistics.median(v), 4)
        r[kind + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    r["head_added_ms"] = round(r["score_ms"] - r["prefill_ms"], 4)
    r["head_added_unfused_ms"] = round(r["score_unfused_ms"] - r["prefill_ms"], 4)
    r["default_path"] = "general (no fused fp8 head)" if fp8 else "fused"
    spread = max(r[k + "_ms_min_max"][1] - r[k + "_ms_min_max"][0] for k in KINDS)
    r["fused_adds_less_than_unfused"] = bool(r["head_added_ms"] < r["head_added_unfused_ms"])
    r["...by_more_than_spread"] = bool(r["head_added_unfused_ms"] - r["head_added_ms"] > spread)
    # the same text scores the same either way (a sanity line, not a parity test)
    lp_f, _, _ = b.score_rows(0, ids, targets)
    lp_u, _, _ = b.score_rows(0, ids, targets, unfused=True)
    r["max_abs_dlogprob_default_vs_unfused"] = float(np.abs(lp_f.astype(np.float64) - lp_u).max())
    r["perplexity"] = float(np.exp(-lp_f[:-1].astype(np.float64).mean()))
    print(json.dumps(r), flush=True)
    b.close()
    eng.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than Qwen2-7B's 28 (rehearsal)")
    ap.add_argument("--rows", type=int, default=N)
    args = ap.parse_args()
    doc = {"model": "Qwen2-7B widths, %s layers, synthetic weights" % (args.layers or 28),
           "method": "host clock around calls that end in a stream synchronise; median of %d calls after %d warm-up "
                     "calls, %d alternated repetitions (median, [min, max])" % (ITERS, WARM, REPS),
           "bf16": table(False, args.layers, args.rows), "weight_fp8": table(True, args.layers, args.rows)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
