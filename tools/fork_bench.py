#!/usr/bin/env python3
"""What sharing KV pages buys, at Qwen2-7B geometry with synthetic weights.

  copy   qie_kv_copy alone: 28 layers x 4 kv heads x head_dim 128, 1 / 128 / 2048 rows, contiguous
         (sequences of one allocation at ctx 2048) and paged (sequences of one pool, page_tokens
         128).  Yardstick: one qie_memcpy_d2d (hipMemcpyAsync device to device) of the same total
         bytes as a single block, which the kernel cannot beat.  Each timing is ITERS back-to-back
         launches on one stream between two host clocks after a synchronise, the whole REPS times
         with the kinds alternating; the median per launch, min and max over the repetitions.
         Launch i works on source / destination pair i % PAIRS, for the kernel and the yardstick
         alike: at 2048 rows the PAIRS pairs are 940 MB, several times the 256 MiB Infinity
         Cache, so that line is an HBM figure; the smaller cases stay cache-resident.  GB/s counts
         bytes read + bytes written.
  fork   Batch.fork at position 2032: paged (15 pages shared, a 112-row tail copied) and
         contiguous (all 2032 rows copied), against the prefill of the same ids — the only way to
         a second such sequence without a fork.  Host clock around one call (each ends in a
         stream synchronise), the median of 5.
  ttft   a 2048-id prompt whose first 1920 ids are cached: load_prefix + append of 128 ids, against
         the plain prefill of all 2048.

  tools/fork_bench.py [--layers N] [--out profiles/kv_fork.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qwen_inference_engine_amd as Q  # noqa: E402
from qwen_inference_engine_amd import _lib, spec as S, weights as W  # noqa: E402

L, NKV, HD, T, CTX = 28, 4, 128, 128, 2048
ITERS, WARM, REPS = 20, 4, 5
PAIRS = 4          # source / destination pairs a timing rotates through


def _malloc(lib, n):
    p = C.c_void_p()
    _lib.check(lib.qie_malloc(C.byref(p), n), "qie_malloc")
    _lib.check(lib.qie_memset(p, 1, n), "qie_memset")
    return p


def _timed(lib, fn, iters):
    _lib.check(lib.qie_synchronize(), "sync")
    t0 = time.perf_counter()
    for i in range(iters):
        fn(i % PAIRS)
    _lib.check(lib.qie_synchronize(), "sync")
    return (time.perf_counter() - t0) / iters * 1e6


def _cell(vals, nbytes):
    med = statistics.median(vals)
    return {"us": round(med, 2), "us_min": round(min(vals), 2), "us_max": round(max(vals), 2),
            "gb_s": round(2 * nbytes / med / 1e3, 1)}


def copy_table(lib):
    run = L * NKV * HD                       # elements per token, K or V
    seq_bytes = run * CTX * 2
    mp = CTX // T
    nseq = 2 * PAIRS                         # pair j: sequence 2j -> sequence 2j + 1
    kc, vc = _malloc(lib, nseq * seq_bytes), _malloc(lib, nseq * seq_bytes)    # contiguous
    n_pages = nseq * mp + 1
    kp, vp = _malloc(lib, n_pages * run * T * 2), _malloc(lib, n_pages * run * T * 2)
    table = np.random.default_rng(0).permutation(np.arange(1, n_pages)).astype(np.int32)
    dt = _malloc(lib, table.nbytes)
    _lib.check(lib.qie_memcpy_h2d(dt, table.ctypes.data, table.nbytes), "h2d")
    src = [_malloc(lib, 2 * seq_bytes) for _ in range(PAIRS)]                  # the yardstick's blocks
    dst = [_malloc(lib, 2 * seq_bytes) for _ in range(PAIRS)]
    cc = _lib.KvCacheC()
    cc.k, cc.v, cc.seq_stride = kc.value, vc.value, run * CTX
    cc.n_layers, cc.n_kv_heads, cc.head_dim, cc.max_ctx = L, NKV, HD, CTX
    pc = _lib.KvCacheC()
    pc.k, pc.v, pc.seq_stride = kp.value, vp.value, run * T
    pc.n_layers, pc.n_kv_heads, pc.head_dim, pc.max_ctx = L, NKV, HD, CTX
    pc.block_table, pc.page_tokens, pc.max_pages = dt.value, T, mp
    rows_out = []
    for rows in (1, 128, 2048):
        nbytes = 2 * run * rows * 2          # K and V
        kinds = {
            "contiguous": lambda j: _lib.check(
                lib.qie_kv_copy(C.byref(cc), 2 * j, C.byref(cc), 2 * j + 1, 0, rows, None), "copy"),
            "paged": lambda j: _lib.check(
                lib.qie_kv_copy(C.byref(pc), 2 * j, C.byref(pc), 2 * j + 1, 0, rows, None), "copy"),
            "memcpy": lambda j: _lib.check(lib.qie_memcpy_d2d(dst[j], src[j], nbytes, None), "d2d"),
        }
        vals = {k: [] for k in kinds}
        for rep in range(REPS + 1):          # repetition 0 warms up and is dropped
            for k, fn in kinds.items():
                us = _timed(lib, fn, WARM if rep == 0 else ITERS)
                if rep:
                    vals[k].append(us)
        r = {"rows": rows, "bytes_each_way": nbytes}
        r.update({k: _cell(v, nbytes) for k, v in vals.items()})
        for k in ("contiguous", "paged"):
            r[k]["of_memcpy"] = round(r["memcpy"]["us"] / r[k]["us"], 3)
        rows_out.append(r)
        print(json.dumps(r), flush=True)
    for p in [kc, vc, kp, vp, dt] + src + dst:
        lib.qie_free(p)
    return rows_out


def _ms(fn, n=5):
    out = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return {"ms": round(statistics.median(out), 3), "ms_min": round(min(out), 3), "ms_max": round(max(out), 3)}


def engine_tables(n_layers):
    spec = S.QWEN2_7B if n_layers is None else S.QWEN2_7B.replace(n_layers=n_layers)
    max_ctx = CTX + 64
    eng = Q.Engine(spec, max_ctx=max_ctx).init_synthetic(W.SynthParams(seed=0))
    ids = [int(t) for t in np.random.default_rng(3).integers(0, spec.vocab, CTX)]
    out = {"n_layers": spec.n_layers}
    for form, kw in (("paged", dict(page_tokens=T)), ("contiguous", {})):
        b = eng.batch(2, max_ctx, **kw)
        b.prefill(0, ids[:CTX - 16])         # warm: scratch, plans
        pre = _ms(lambda: b.prefill(0, ids[:CTX - 16]))
        fork = _ms(lambda: b.fork(0, 1))     # every call ends in a stream synchronise
        out[f"fork_{form}"] = {"position": CTX - 16, "fork": fork, "prefill": pre}
        print(json.dumps({form: out[f"fork_{form}"]}), flush=True)
        if form == "paged":
            b.prefill(0, ids[:1920] + [1])
            pf = b.save_prefix(0, 1920)
            b.release(0)

            def reuse():
                b.load_prefix(pf, 1, ids[1920], 1920)
                return b.append(1, ids[1920:], pos0=1920)

            tok_r = reuse()
            tok_p = b.prefill(0, ids)
            out["ttft"] = {"prompt": CTX, "cached": 1920, "load_append": _ms(reuse), "prefill": _ms(lambda: b.prefill(0, ids)),
                           "same_first_token": tok_r == tok_p}
            print(json.dumps({"ttft": out["ttft"]}), flush=True)
            pf.drop()
        b.close()
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--layers", type=int, default=None, help="engine tables at fewer layers (default: all 28)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_fork.json"))
    ap.add_argument("--copy-only", action="store_true")
    a = ap.parse_args()
    lib = _lib.load()
    res = {"geometry": {"layers": L, "kv_heads": NKV, "head_dim": HD, "page_tokens": T, "ctx": CTX},
           "method": {"iters": ITERS, "warm": WARM, "reps": REPS, "pairs": PAIRS}, "copy": copy_table(lib)}
    if not a.copy_only:
        res["engine"] = engine_tables(a.layers)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
