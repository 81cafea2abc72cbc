#!/usr/bin/env python3
"""What a batched verify step costs: Qwen2-7B widths at full depth, synthetic
weights, B = 8 slots at context 2,032, bf16 weights and again weight_fp8.

  (a) Batch.verify_batch with 8 x 1, 4 x 3 and 2 x 7 drafts (16 rows each) and 8 x 0 (8 rows);
  (b) one B = 8 decode_step;
  (c) the same drafts as sequential Batch.verify calls, one per segment.

The protocol is tools/verify_bench.py's (§16.3): every call ends in a stream synchronise, so a
host clock around it is its time; the slots are put back to the same position before each call
(outside the timed window); ITERS calls per cell after WARM warm-up calls, their median taken; the
whole table REPS times with the kinds alternating; per cell the median and the min / max over the
repetitions.  ratio_to_decode = (a) / (b); break_even_accepted_per_slot = (a) / (b) - 1: a verify
step emits 1 + accepted tokens per live slot where a decode step emits 1, so speculation pays
above that many accepted drafts per slot and step.  sequential_over_batched = (c) / (a).

first_call_ms is the FIRST call of a table on the batch: with use_graph it captures and
instantiates the step before running it, which is what a table the cache has not seen costs.

One process; every GPU step (a model build, a table repetition) runs under its own time limit,
kept by a watchdog thread (it ends the process with status 124 even while the main thread waits
inside a HIP call, where a signal handler would not run), and the run stops at the first failure.

  tools/verify_batch_bench.py            the tables -> profiles/verify_batch.json
  tools/verify_batch_bench.py --bench-vs-parent DIR
        bench.py of the tree DIR (a checkout of the parent commit, built) and of this tree,
        alternating, REPS_AB times each for the headline and for --batch 8 --fp8, every run a
        child process under its own time limit -> "bench_vs_parent" of the same JSON
"""
import argparse
import collections
import json
import os
import statistics
import subprocess
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qwen_inference_engine_amd as Q  # noqa: E402
from qwen_inference_engine_amd import spec as S, weights as W  # noqa: E402

B = 8
CTX, MAX_CTX = 2048 - 16, 2048 + 32
TABLES = {"8x1": (8, 1), "4x3": (4, 3), "2x7": (2, 7), "8x0": (8, 0)}   # segments x drafts
ITERS, WARM, REPS = 20, 3, 3
OUT = os.path.join(ROOT, "profiles", "verify_batch.json")


REPS_AB = 2


class step_limit:
    """A time limit around one GPU step of this process: past it a watchdog thread ends the
    process (status 124).  A thread, not SIGALRM: Python runs signal handlers between bytecodes
    only, so one would not fire while the main thread is blocked in a synchronising HIP call."""

    def __init__(self, seconds, what):
        self.seconds, self.what = seconds, what

    def _expired(self):
        sys.stderr.write("verify_batch_bench: %s exceeded its %d s limit\n" % (self.what, self.seconds))
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, self._expired)
        self.timer.daemon = True
        self.timer.start()

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


def make(fp8, n_layers, ctx):
    spec = S.QWEN2_7B if n_layers is None else S.QWEN2_7B.replace(n_layers=n_layers)
    eng = Q.Engine(spec, max_ctx=ctx + 48, weight_fp8=fp8).init_synthetic(W.SynthParams(seed=0))
    b = eng.batch(B, ctx + 48)
    r = np.random.default_rng(3)
    ids = [[int(t) for t in r.integers(0, spec.vocab, ctx + 32)] for _ in range(B)]
    toks = b.prefill_batch(0, [p[:ctx] for p in ids])
    return eng, b, ids, toks


def timed(b, toks, slots, fn, n, ctx):
    """Median ms of n calls of fn(), each with `slots` back at position ctx."""
    out = []
    for _ in range(n):
        for s in slots:
            b.set_position(s, ctx, toks[s])      # synchronises: the clock starts on an idle stream
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def tables(fp8, n_layers, ctx):
    with step_limit(300, "model build and prefill"):
        eng, b, ids, toks = make(fp8, n_layers, ctx)
    cells = collections.defaultdict(list)
    first = {}
    everyone = list(range(B))
    for rep in range(REPS + 1):                  # repetition 0 warms every shape (captures) and is dropped
        n = WARM if rep == 0 else ITERS
        with step_limit(240, "table repetition %d" % rep):
            for name, (segs, k) in TABLES.items():
                tab = [(s, ids[s][ctx:ctx + k]) for s in range(segs)]

                def batched():
                    b.verify_batch(tab)

                def sequential():
                    for s, d in tab:
                        b.verify(s, d)

                if rep == 0:                     # the table's first call on this batch: capture + run
                    first[name] = timed(b, toks, [s for s, _ in tab], batched, 1, ctx)
                for kind, fn in (("batched", batched), ("sequential", sequential)):
                    ms = timed(b, toks, [s for s, _ in tab], fn, n, ctx)
                    if rep:
                        cells[(name, kind)].append(ms)
            ms = timed(b, toks, everyone, lambda: b.decode_step(), n, ctx)
            if rep:
                cells[("decode", "decode")].append(ms)
    dec = cells[("decode", "decode")]
    rows = [{"kind": "decode_step B=8", "ms": round(statistics.median(dec), 4),
             "ms_min_max": [round(min(dec), 4), round(max(dec), 4)]}]
    print(json.dumps(rows[0]), flush=True)
    for name, (segs, k) in TABLES.items():
        r = {"table": name, "segments": segs, "drafts_per_segment": k, "rows": segs * (k + 1)}
        for kind in ("batched", "sequential"):
            v = cells[(name, kind)]
            r[kind + "_ms"] = round(statistics.median(v), 4)
            r[kind + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
        r["first_call_ms"] = round(first[name], 4)
        r["ratio_to_decode"] = round(r["batched_ms"] / rows[0]["ms"], 3)
        r["break_even_accepted_per_slot"] = round(r["batched_ms"] / rows[0]["ms"] - 1, 3)
        r["sequential_over_batched"] = round(r["sequential_ms"] / r["batched_ms"], 3)
        rows.append(r)
        print(json.dumps(r), flush=True)
    b.close()
    eng.close()
    return rows


def bench_vs_parent(parent):
    """bench.py of `parent` and of this tree, alternating; every run a fresh child process under
    its own time limit; stops at the first failure."""
    runs = []
    for extra in ([], ["--batch", "8", "--fp8"]):
        for _ in range(REPS_AB):
            for label, tree in (("parent", os.path.abspath(parent)), ("new", ROOT)):
                cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "255", "--warmup", "16"] + extra
                p = subprocess.run(cmd, cwd=tree, capture_output=True, text=True, timeout=240)
                if p.returncode != 0:
                    sys.stderr.write(p.stderr[-2000:])
                    raise SystemExit("bench.py failed in %s (status %d)" % (tree, p.returncode))
                x = json.loads(p.stdout.strip().splitlines()[-1])
                runs.append({"tree": label, "args": " ".join(cmd[1:]), "tokens_per_s": x["value"],
                             "ms_per_step": x["ms_per_step"], "prefill_tok_s": x["prefill_tok_s"]})
                print(json.dumps(runs[-1]), flush=True)
    return {"method": "tools/verify_batch_bench.py --bench-vs-parent: bench.py of the parent commit's tree and of "
                      "this tree, alternating, one box, one session", "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than Qwen2-7B's 28 (rehearsal)")
    ap.add_argument("--ctx", type=int, default=CTX)
    ap.add_argument("--only", choices=["bf16", "weight_fp8"], default=None)
    ap.add_argument("--bench-vs-parent", metavar="DIR", default=None)
    args = ap.parse_args()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.bench_vs_parent:
        doc["bench_vs_parent"] = bench_vs_parent(args.bench_vs_parent)
        with open(args.out, "w") as f:
            json.dump(doc, f, indent=1)
        return
    doc.update({"model": "Qwen2-7B widths, %s layers, synthetic weights, B = %d" % (args.layers or 28, B),
                "context": args.ctx,
                "method": "host clock around calls that end in a stream synchronise; median of %d calls after %d "
                          "warm-up calls, %d alternated repetitions (median, [min, max])" % (ITERS, WARM, REPS)})
    for kind in ("bf16", "weight_fp8"):
        if args.only in (None, kind):
            doc[kind] = tables(kind == "weight_fp8", args.layers, args.ctx)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
