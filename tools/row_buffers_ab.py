#!/usr/bin/env python3
"""What the engine's host paths cost with one library (QIE_LIB selects it): run it in alternating
processes for two builds and compare (profiles/row_buffers.json).  Qwen2-7B widths at full depth,
bf16, synthetic weights.  One JSON line:

  create_ms    qie_batch_create to return at B = 8, max_ctx = 4,096 (each of 5 on a fresh batch)
  prefill_ms   qie_prefill of 2,048 ids (the prefill rows: the GEMM operands of every layer)
  score_ms     qie_score of the same ids (the fused scoring head)
  verify_ms    one qie_verify with 7 drafts at position about 2,048 (captured step)
  step_us      graph decode step, 64 steps per sample

--page-tokens T measures the same figures on paged batches (pages of T tokens): the page pool's
reservation is then on every call's host path.

Host clock around calls that end in a stream synchronise; per figure the median of its calls after
warm-up calls (tools/score_bench.py's method)."""
import argparse
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

N, MAX_CTX = 2048, 4096


def ms(eng, fn, n, warm):
    out = []
    for i in range(warm + n):
        eng.sync()
        t0 = time.perf_counter()
        fn()
        if i >= warm:
            out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than Qwen2-7B's 28 (rehearsal)")
    ap.add_argument("--page-tokens", type=int, default=None,
                    help="every batch paged with pages of this many tokens (default: contiguous)")
    args = ap.parse_args()
    spec = S.QWEN2_7B if args.layers is None else S.QWEN2_7B.replace(n_layers=args.layers)
    eng = Q.Engine(spec, max_ctx=MAX_CTX).init_synthetic(W.SynthParams(seed=0))
    r = {"lib": os.environ.get("QIE_LIB", "default"), "page_tokens": args.page_tokens}
    made = []
    r["create_ms"] = ms(eng, lambda: made.append(eng.batch(8, MAX_CTX, page_tokens=args.page_tokens)), 5, 1)
    for b in made:
        b.close()
    b = eng.batch(1, MAX_CTX, page_tokens=args.page_tokens)
    ids = [int(t) for t in np.random.default_rng(3).integers(0, spec.vocab, N)]
    r["prefill_ms"] = ms(eng, lambda: b.prefill(0, ids), 7, 2)
    r["score_ms"] = ms(eng, lambda: b.score_rows(0, ids, ids[1:] + [-1]), 5, 2)
    b.prefill(0, ids)
    draft = ids[:7]
    r["verify_ms"] = ms(eng, lambda: b.verify(0, draft), 20, 3)
    r["step_us"] = round(ms(eng, lambda: b.decode(64, want_ids=False), 5, 1) * 1e3 / 64, 3)
    print(json.dumps(r), flush=True)
    b.close()
    eng.close()


if __name__ == "__main__":
    main()
