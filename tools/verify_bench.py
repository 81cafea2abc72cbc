#!/usr/bin/env python3
"""What an M-row speculative verify step costs: Qwen2-7B widths at full depth,
synthetic weights, context 2,048, bf16 weights and again weight_fp8.  For M in {1, 2, 4, 8, 16}:

  (a) qie_verify with M - 1 drafts (the captured step);
  (b) qie_prefill_append of M rows (what the engine could do before qie_verify: the baseline);
  (c) one qie_decode_step.

Every call ends in a stream synchronise (its ids come back to the host), so a host clock
around one call is its time; the sequence is put back to the same position before each call
(outside the timed window).  ITERS calls per (M, kind) after WARM warm-up calls, their median
taken; the whole table REPS times with the kinds alternating; per cell the median and the
min / max over the repetitions.  break_even = t_verify(M) / t_decode: the emitted tokens per
call above which verifying beats decoding.

  tools/verify_bench.py                      the table -> profiles/verify_step.json
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- \\
      python tools/verify_bench.py --trace-step      (a run of its own: the M = 8 step, traced)
  tools/verify_bench.py --merge-trace DIR/run_kernel_trace.csv    per-layer kernel times -> the JSON
"""
import argparse
import collections
import csv
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

CTX, MAX_CTX = 2048 - 16, 2048 + 32     # the rows of every call end at or below position 2,048
MS = (1, 2, 4, 8, 16)
ITERS, WARM, REPS = 20, 3, 3
OUT = os.path.join(ROOT, "profiles", "verify_step.json")


def make(fp8, n_layers=None):
    spec = S.QWEN2_7B if n_layers is None else S.QWEN2_7B.replace(n_layers=n_layers)
    eng = Q.Engine(spec, max_ctx=MAX_CTX, weight_fp8=fp8).init_synthetic(W.SynthParams(seed=0))
    b = eng.batch(1, MAX_CTX)
    ids = [int(t) for t in np.random.default_rng(3).integers(0, spec.vocab, CTX + 32)]
    tok = b.prefill(0, ids[:CTX])
    return eng, b, ids, tok


def timed(b, tok, fn, n):
    """Median ms of n calls of fn(), each from position CTX with current token tok."""
    out = []
    for _ in range(n):
        b.set_position(0, CTX, tok)          # synchronises: the clock starts on an idle stream
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def table(fp8, n_layers):
    eng, b, ids, tok = make(fp8, n_layers)
    cells = collections.defaultdict(list)
    for rep in range(REPS + 1):               # repetition 0 warms every shape (captures, scratch) and is dropped
        n = WARM if rep == 0 else ITERS
        for M in MS:
            draft = ids[CTX:CTX + M - 1]
            kinds = {"verify": lambda: b.verify(0, draft),
                     "append": lambda: b.append(0, ids[CTX:CTX + M], pos0=CTX),
                     "decode": lambda: b.decode_step()}
            for kind, fn in kinds.items():
                ms = timed(b, tok, fn, n)
                if rep:
                    cells[(M, kind)].append(ms)
    rows = []
    for M in MS:
        r = {"M": M}
        for kind in ("verify", "append", "decode"):
            v = cells[(M, kind)]
            r[kind + "_ms"] = round(statistics.median(v), 4)
            r[kind + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        spread = max(r[k + "_ms_min_max"][1] - r[k + "_ms_min_max"][0] for k in ("verify", "append"))
        r["break_even_tokens_per_call"] = round(r["verify_ms"] / r["decode_ms"], 3)
        r["append_over_verify"] = round(r["append_ms"] / r["verify_ms"], 3)
        r["verify_faster_than_append_by_more_than_spread"] = bool(r["append_ms"] - r["verify_ms"] > spread)
        rows.append(r)
        print(json.dumps(r), flush=True)
    b.close()
    eng.close()
    return rows


def trace_step():
    """The M = 8 verify step a few times (bf16), for a kernel trace taken around this process."""
    eng, b, ids, tok = make(False)
    for _ in range(6):
        b.set_position(0, CTX, tok)
        b.verify(0, ids[CTX:CTX + 7])
    eng.sync()


def short(name):
    return name.split("(")[0].replace("void ", "").replace("qie::", "")


def merge_trace(path, out):
    """Per-layer kernel durations of the traced M = 8 steps (layers 1 .. L-1 of every step but
    the first, which captured): the launches between verify_rows_kernel and
    verify_commit_kernel, cut into layers at each qkv_post_kernel."""
    t = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    names = [short(r["Kernel_Name"]) for r in t]
    dur = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in t]
    starts = [i for i, n in enumerate(names) if n == "verify_rows_kernel"]
    ends = [i for i, n in enumerate(names) if n == "verify_commit_kernel"]
    per_pos = collections.defaultdict(list)
    head = collections.defaultdict(list)
    order = []
    for a, e in list(zip(starts, ends))[1:]:
        seg = list(range(a + 1, e))
        qp = [k for k, i in enumerate(seg) if names[i].startswith("qkv_post_kernel")]
        if len(qp) < 3:
            continue
        per_layer, pre = qp[1] - qp[0], qp[0]
        for l in range(1, len(qp)):
            for k in range(per_layer):
                i = seg[qp[l] - pre + k]
                per_pos[(k, names[i])].append(dur[i])
                if (k, names[i]) not in order:
                    order.append((k, names[i]))
        for i in seg[qp[-1] - pre + per_layer:] + [e]:
            head[names[i]].append(dur[i])
    layer = [{"launch": k, "kernel": n, "avg_us": round(statistics.mean(per_pos[(k, n)]), 2),
              "median_us": round(statistics.median(per_pos[(k, n)]), 2), "samples": len(per_pos[(k, n)])}
             for k, n in sorted(order)]
    glue = [r for r in layer if r["kernel"].startswith(("qkv_post_kernel", "attn_extend_kernel", "attn_combine_kernel"))]
    rep = {"source": "rocprofv3 --kernel-trace --stats of tools/verify_bench.py --trace-step (Qwen2-7B bf16, M = 8, "
                     "context %d); kernel durations only" % CTX,
           "per_layer": layer, "per_layer_sum_us": round(sum(r["avg_us"] for r in layer), 2),
           "qkv_post_extend_combine_us": round(sum(r["avg_us"] for r in glue), 2),
           "head_and_commit": {n: round(statistics.mean(v), 2) for n, v in head.items()}}
    doc = json.load(open(out)) if os.path.exists(out) else {}
    doc["trace_m8"] = rep
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(rep, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than Qwen2-7B's 28 (rehearsal)")
    ap.add_argument("--trace-step", action="store_true")
    ap.add_argument("--merge-trace", default=None)
    args = ap.parse_args()
    if args.trace_step:
        return trace_step()
    if args.merge_trace:
        return merge_trace(args.merge_trace, args.out)
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc.update({"model": "Qwen2-7B widths, %s layers, synthetic weights" % (args.layers or 28), "context": CTX,
                "method": "host clock around calls that end in a stream synchronise; median of %d calls after %d "
                          "warm-up calls, %d alternated repetitions (median, [min, max])" % (ITERS, WARM, REPS),
                "bf16": table(False, args.layers), "weight_fp8": table(True, args.layers)})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
