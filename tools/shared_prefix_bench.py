#!/usr/bin/env python3
"""Decode mode 0 against mode 2 (the shared-prefix decode attention) on a paged
batch of 8 slots, Qwen2-7B geometry, synthetic weights.

Per shared length n (2k, 8k, 32k) two batches' worth of state on ONE batch, one after the other:
  shared    slot 0 holds n tokens, slots 1-7 are forks of it at n (all of its pages shared);
  control   eight unrelated sequences of n tokens (no page shared: mode 2 pays for its empty
            prefix roles and its second launch).
The slots are positioned, not prefilled: the K/V rows are whatever the pool holds, which the time of
a launch does not depend on.  Modes 0 and 2 alternate in one process; every sample repositions
the slots at n, then takes
  attn_us     qie_batch_time_kernel(5): the mean of `--iters` attention launches of the current mode
              that cycle through the layers (a launch never re-reads the layer the last one left
              in cache; at n = 2k the shared state's whole K/V, 0.12 GB, stays below the 256 MiB
              Infinity Cache all the same, the control's 0.94 GB does not);
  tok_s       `--steps` graph decode steps under a host clock ending in a synchronise (15 GB of
              weights stream between two attention launches of one layer).
Reported: the median and min .. max of `--repeats` samples.

    python tools/shared_prefix_bench.py --out profiles/shared_prefix_decode.json
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import qwen_inference_engine_amd as Q  # noqa: E402
from qwen_inference_engine_amd import spec as S, weights as W  # noqa: E402

B = 8


def stat(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 2), "min": round(v[0], 2), "max": round(v[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", type=int, nargs="+", default=[2048, 8192, 32768])
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=56)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    max_ctx = max(a.lengths) + 128
    eng = Q.Engine(S.QWEN2_7B, max_ctx=max_ctx).init_synthetic(W.SynthParams(seed=0))
    rows = []
    for n in a.lengths:
        for kind in ("shared", "control"):
            b = eng.batch(B, max_ctx, page_tokens=128)

            def place():
                for m in range(B):
                    if kind == "shared" and m > 0:
                        b.fork(0, m, n)
                    else:
                        b.set_position(m, n, 17 + m)

            samples = {0: ([], []), 2: ([], [])}
            table = None
            for rep in range(a.repeats + 1):               # sample 0: warm-up (graph captures), dropped
                for mode in (0, 2):
                    b.set_decode_mode(mode)
                    place()
                    if mode == 2:
                        table = b.shared_prefix()
                    b.decode(1, want_ids=False)            # the switch re-captures the graph: not timed
                    eng.sync()
                    t0 = time.perf_counter()
                    b.decode(a.steps, want_ids=False)
                    eng.sync()
                    tok = B * a.steps / (time.perf_counter() - t0)
                    us, _ = b.time_kernel(5, a.iters)
                    if rep:
                        samples[mode][0].append(us)
                        samples[mode][1].append(tok)
            row = {"n": n, "kind": kind, "batch": B, "share_table": table,
                   "mode0": {"attn_us": stat(samples[0][0]), "tok_s": stat(samples[0][1])},
                   "mode2": {"attn_us": stat(samples[2][0]), "tok_s": stat(samples[2][1])}}
            row["attn_speedup"] = round(row["mode0"]["attn_us"]["median"] / row["mode2"]["attn_us"]["median"], 3)
            row["tok_s_ratio"] = round(row["mode2"]["tok_s"]["median"] / row["mode0"]["tok_s"]["median"], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
            b.close()
    doc = {"what": "decode mode 0 vs mode 2 (shared-prefix decode attention), Qwen2-7B geometry, B = 8, paged",
           "iters": a.iters, "steps": a.steps, "repeats": a.repeats, "rows": rows}
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
