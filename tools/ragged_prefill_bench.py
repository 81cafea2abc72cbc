#!/usr/bin/env python3
"""qie_prefill_ragged against the single calls it replaces (the shipped library, one GPU,
Qwen2-7B with synthetic weights):
  (a) eight fresh prompts of lengths 37, 150, 64, 300, 512, 90, 210, 128: one ragged call
      against the eight qie_prefill calls;
  (b) four appends of 128 rows at prefixes 1024, 1500, 200, 3000: one ragged call against the
      four qie_prefill_append calls;
  (c) the attention launch alone for one fresh 2,048-row segment: qie_attention_ragged against
      qie_attention (Qwen2-7B heads, seeded inputs, no engine).
The single calls are unchanged code and serve as the baseline, timed in the same process,
alternating with the ragged call.  (a), (b): a host clock around calls that return the sampled
ids (they end in a device synchronise), REPS repetitions after a warm-up of both forms, medians.
(c): device events around ITERS launches.  Writes the JSON report to --out (default
profiles/ragged_prefill.json)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gpu_util as G  # noqa: E402
import qwen_inference_engine_amd as Q  # noqa: E402
from extend_attn_bench import Events  # noqa: E402
from qwen_inference_engine_amd import _lib, spec as S, weights as W  # noqa: E402
from qwen_inference_engine_amd._lib import KvCacheC, RowSegsC  # noqa: E402

FRESH = (37, 150, 64, 300, 512, 90, 210, 128)
APPEND_ROWS, PREFIXES = 128, (1024, 1500, 200, 3000)
MAX_CTX = 4096
REPS, WARM = 9, 2
ATT_ROWS, ATT_ITERS, ATT_WARM, ATT_REPS = 2048, 100, 10, 3


def ms(lib, fn):
    G.check(lib.qie_synchronize())
    t0 = time.perf_counter()
    fn()   # returns after the sampled ids are on the host
    return (time.perf_counter() - t0) * 1e3


def compare(lib, name, ragged, single):
    """Alternates the two forms REPS times after WARM rounds of both; medians."""
    r_ms, s_ms = [], []
    for i in range(WARM + REPS):
        for fn, acc in ((ragged, r_ms), (single, s_ms)):
            t = ms(lib, fn)
            if i >= WARM:
                acc.append(t)
    r, s = float(np.median(r_ms)), float(np.median(s_ms))
    row = {"case": name, "ragged_ms": round(r, 3), "single_calls_ms": round(s, 3), "single_over_ragged": round(s / r, 3),
           "ragged_ms_all": [round(x, 3) for x in r_ms], "single_calls_ms_all": [round(x, 3) for x in s_ms]}
    print(json.dumps(row), flush=True)
    return row


def engine_cases(report, layers):
    lib = _lib.load()
    spec = S.QWEN2_7B if layers is None else S.QWEN2_7B.replace(n_layers=layers)
    eng = Q.Engine(spec, max_ctx=MAX_CTX).init_synthetic(W.SynthParams(seed=0))
    rng = np.random.default_rng(3)
    ids = lambda n: [int(t) for t in rng.integers(0, spec.vocab, n)]
    report["model"] = f"Qwen2-7B widths, {spec.n_layers} layers, synthetic bf16 weights"

    # (a) eight fresh prompts
    b = eng.batch(8, MAX_CTX)
    prompts = [ids(n) for n in FRESH]
    segs = [(s, p) for s, p in enumerate(prompts)]
    toks = {}

    def ragged_a():
        toks["ragged"] = b.prefill_ragged(segs)

    def single_a():
        toks["single"] = [b.prefill(s, p) for s, p in enumerate(prompts)]

    row = compare(lib, "a: 8 fresh prompts " + str(FRESH), ragged_a, single_a)
    row["rows"] = sum(FRESH)
    row["tokens_equal"] = sum(int(x == y) for x, y in zip(toks["ragged"], toks["single"]))   # of 8 (near-ties may flip)
    report["fresh"] = row
    b.close()

    # (b) four appends of 128 rows over cached prefixes
    b = eng.batch(4, MAX_CTX)
    heads = [ids(n) for n in PREFIXES]
    tails = [ids(APPEND_ROWS) for _ in PREFIXES]
    for s, h in enumerate(heads):
        b.prefill(s, h)
    segs_b = [(s, t, len(h)) for s, (h, t) in enumerate(zip(heads, tails))]

    def ragged_b():
        toks["ragged"] = b.prefill_ragged(segs_b)

    def single_b():
        toks["single"] = [b.append(s, t, len(h)) for s, (h, t) in enumerate(zip(heads, tails))]

    row = compare(lib, f"b: 4 appends of {APPEND_ROWS} rows at prefixes {PREFIXES}", ragged_b, single_b)
    row["rows"] = APPEND_ROWS * len(PREFIXES)
    row["tokens_equal"] = sum(int(x == y) for x, y in zip(toks["ragged"], toks["single"]))
    report["append"] = row
    b.close()
    eng.close()


def attention_case(report):
    """(c): one fresh segment of ATT_ROWS rows, the two attention launches alone."""
    lib = _lib.load()
    ev = Events()
    nq, nkv, hd = 28, 4, 128
    rnd = lambda shape, seed: G.to_bf16(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))
    kc, vc = G.dev(rnd((1, 1, nkv, MAX_CTX, hd), 1)), G.dev(rnd((1, 1, nkv, MAX_CTX, hd), 2))
    c = KvCacheC()
    c.k, c.v, c.seq_stride = G.p(kc), G.p(vc), nkv * MAX_CTX * hd
    c.n_layers, c.n_kv_heads, c.head_dim, c.max_ctx = 1, nkv, hd, MAX_CTX
    n = ATT_ROWS
    q, pos = G.dev(rnd((n, nq * hd), 3)), G.dev(np.arange(n, dtype=np.int32))
    t = RowSegsC()
    t.n = 1
    for z in range(1, _lib.QIE_RAGGED_MAX_SEGS + 1):
        t.row0[z] = n
    ws_r = G.zeros_bytes(lib.qie_attention_extend_workspace_bytes(n, nq, hd, MAX_CTX))
    ws_p = G.zeros_bytes(lib.qie_attention_workspace_bytes(n, nq, hd, MAX_CTX))
    out_r, out_p = G.zeros_bf16(n, nq * hd), G.zeros_bf16(n, nq * hd)
    rag = lambda: G.check(lib.qie_attention_ragged(G.p(q), G.p(pos), C.byref(t), C.byref(c), 0, nq, G.p(out_r),
                                                   G.p(ws_r), None))
    pre = lambda: G.check(lib.qie_attention(G.p(q), n, G.p(pos), n, C.byref(c), 0, nq, G.p(out_p), G.p(ws_p), None))
    for fn in (rag, pre):
        for _ in range(ATT_WARM):
            fn()
    G.check(lib.qie_synchronize())
    r_us, p_us = [], []
    for _ in range(ATT_REPS):
        r_us.append(ev.time(rag, ATT_ITERS))
        p_us.append(ev.time(pre, ATT_ITERS))
    d = np.abs(G.bf(G.host_bf16(out_r)) - G.bf(G.host_bf16(out_p)))
    r, p = float(np.median(r_us)), float(np.median(p_us))
    row = {"case": f"c: attention alone, one fresh segment of {n} rows (28 / 4 heads, hd 128, max_ctx {MAX_CTX})",
           "ragged_us": round(r, 2), "prefill_attention_us": round(p, 2), "ragged_over_prefill": round(r / p, 3),
           "ragged_us_all": [round(x, 2) for x in r_us], "prefill_attention_us_all": [round(x, 2) for x in p_us],
           "split_tokens": lib.qie_attention_extend_split_tokens(n, MAX_CTX), "max_abs_diff_of_outputs": float(d.max())}
    print(json.dumps(row), flush=True)
    report["attention"] = row
    G.release_all()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ragged_prefill.json"))
    ap.add_argument("--layers", type=int, default=None, help="layers of the Qwen2-7B widths (default: all 28)")
    args = ap.parse_args()
    report = {"reps": REPS, "warm": WARM, "timing": "host clock around calls that return the ids; medians"}
    attention_case(report)
    engine_cases(report, args.layers)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
