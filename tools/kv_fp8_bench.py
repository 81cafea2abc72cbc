#!/usr/bin/env python3
"""Decode attention on a bf16 KV cache against the fp8 KV cache (qie_attention_decode /
qie_attention_decode_fp8), operator tier, Qwen2-7B head shapes (28 q heads, 4 kv heads, hd 128).

Per point (context, batch): both kernels run in one process, alternating, over a 28-layer cache
whose layers are visited in turn (as a decode step does: no launch re-reads the keys the previous
one left in L2 / MALL).  A sample is a host clock around at least `--launches` launches and at least
`--sample-ms` of them on one stream, ending in a stream synchronise; the figure is microseconds per
launch.  Reports the median and the
min .. max of `--repeats` samples of each kernel, and the K/V bytes a launch reads.

    python tools/kv_fp8_bench.py --out profiles/kv_fp8.json
    QIE_LIB=.../lib/dev/libqie.so python tools/kv_fp8_bench.py --step-ab      # 128- against 256-key steps
    python tools/kv_fp8_bench.py --extend --out profiles/kv_fp8_extend.json   # appends: the split-context attention
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qwen_inference_engine_amd import _lib  # noqa: E402

NQ, NKV, HD, LAYERS = 28, 4, 128, 28


def engines(a):
    """The two engines (bf16 KV, fp8 KV; synthetic Qwen2-7B weights), one after the other: decode tok/s
    at every (context, batch) point — all slots set to the context, `--steps` graph steps under a host
    clock ending in a synchronise, `--repeats` samples — prefill tok/s at 2,048 tokens (for the fp8
    engine this includes the staging pass), and kv_bytes of the batch."""
    import qwen_inference_engine_amd as Q
    from qwen_inference_engine_amd import spec as S, weights as W
    out = {}
    max_ctx = max(a.ctx) + a.steps + 64
    for name, kv8 in (("bf16", False), ("fp8", True)):
        eng = Q.Engine(S.QWEN2_7B, max_ctx=max_ctx, kv_fp8=kv8).init_synthetic(W.SynthParams(seed=0))
        rows = []
        for B in a.batch:
            b = eng.batch(B, max_ctx)
            for ctx in a.ctx:
                samples = []
                for i in range(a.repeats + 1):           # sample 0: warm-up (graph capture), dropped below
                    for s_ in range(B):
                        b.set_position(s_, ctx, 17 + s_)
                    eng.sync()
                    t0 = time.perf_counter()
                    b.decode(a.steps, want_ids=False)
                    eng.sync()
                    samples.append(B * a.steps / (time.perf_counter() - t0))
                samples = sorted(samples[1:])
                rows.append({"ctx": ctx, "batch": B, "decode_tok_s": {"median": round(samples[len(samples) // 2], 1),
                             "min": round(samples[0], 1), "max": round(samples[-1], 1)}})
                print(name, json.dumps(rows[-1]), flush=True)
            kvb = b.kv_bytes()
            b.close()
        b = eng.batch(1, max_ctx)
        ids = [int(t) for t in np.random.default_rng(1).integers(0, 1000, 2048)]
        b.prefill(0, ids)
        pf = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            b.prefill(0, ids)
            eng.sync()
            pf.append(2048 / (time.perf_counter() - t0))
        pf.sort()
        out[name] = {"decode": rows, "prefill_2048_tok_s": {"median": round(pf[len(pf) // 2]), "min": round(pf[0]),
                     "max": round(pf[-1])}, "kv_bytes_batch8": kvb, "max_ctx": max_ctx}
        print(name, json.dumps({k: v for k, v in out[name].items() if k != "decode"}), flush=True)
        b.close()
        eng.close()
    return out


def bench_points(q, st, a, shape, variants):
    """Times `variants` — (name, fp8 cache?, QIE_DEC_KS value or None) — alternating, at every
    (context, batch) point of head shape `shape` = (q heads, kv heads, head_dim, layers)."""
    NQ, NKV, HD, LAYERS = shape
    chk = _lib.check

    def dmalloc(n):
        p = C.c_void_p()
        chk(q.qie_malloc(C.byref(p), n), "qie_malloc")
        return p.value

    def upload(arr):
        arr = np.ascontiguousarray(arr)
        p = dmalloc(arr.nbytes)
        chk(q.qie_memcpy_h2d(p, arr.ctypes.data, arr.nbytes), "h2d")
        return p

    results = []
    for ctx in a.ctx:
        maxc = ctx + 128
        cs = np.empty((maxc, HD // 2), np.float32)
        sn = np.empty_like(cs)
        fp = C.POINTER(C.c_float)
        chk(q.qie_rope_table_host(cs.ctypes.data_as(fp), sn.ctypes.data_as(fp), maxc, HD, 1e6, 0), "rope")
        dcs, dsn = upload(cs), upload(sn)
        for B in a.batch:
            per_seq = LAYERS * NKV * maxc * HD          # elements per sequence
            bufs = []
            c16 = _lib.KvCacheC()
            c8 = _lib.KvCacheFp8C()
            for c, esz in ((c16, 2), (c8.c, 1)):
                if esz == 2 and not any(not v[1] for v in variants):
                    continue                            # no bf16 variant: no bf16 cache
                n = B * per_seq * esz
                c.k, c.v = dmalloc(n), dmalloc(n)
                bufs += [c.k, c.v]
                for p in (c.k, c.v):                    # 0x38: e4m3 1.0; 0x3838: a small finite bf16
                    chk(q.qie_memset(p, 0x38, n), "memset")
                c.seq_stride, c.n_layers, c.n_kv_heads, c.head_dim, c.max_ctx = per_seq, LAYERS, NKV, HD, maxc
            ne = B * LAYERS * NKV * maxc
            c8.k_exps, c8.v_exps, c8.exp_stride = dmalloc(ne), dmalloc(ne), LAYERS * NKV * maxc
            bufs += [c8.k_exps, c8.v_exps]
            for p in (c8.k_exps, c8.v_exps):
                chk(q.qie_memset(p, 127, ne), "memset")
            rng = np.random.default_rng(ctx + B)
            qkv = (rng.standard_normal((B, (NQ + 2 * NKV) * HD)).astype(np.float32) * 0.05)
            qkv = ((qkv.view(np.uint32) + 0x8000) >> 16).astype(np.uint16)
            dqkv, dpos = upload(qkv), upload(np.full(B, ctx - 1, np.int32))
            wsn = q.qie_attention_decode_workspace_bytes(B, NQ, NKV, HD, maxc)
            ws = [dmalloc(wsn) for _ in variants]
            for w in ws:
                chk(q.qie_memset(w, 0, wsn), "memset")
            out = dmalloc(B * NQ * HD * 2)
            bufs += [dqkv, dpos, out] + ws

            def run(vi, n):
                _, fp8, ks = variants[vi]
                if ks is None:
                    os.environ.pop("QIE_DEC_KS", None)
                else:
                    os.environ["QIE_DEC_KS"] = str(ks)  # read per launch by the development build
                fn = q.qie_attention_decode_fp8 if fp8 else q.qie_attention_decode
                cache = C.byref(c8) if fp8 else C.byref(c16)
                t0 = time.perf_counter()
                for i in range(n):
                    chk(fn(dqkv, B, dpos, None, None, dcs, dsn, NQ, cache, i % LAYERS, 1e-6, _lib.QIE_ATTN_PREROPED,
                           out, ws[vi], st), "launch")
                chk(q.qie_stream_synchronize(st), "sync")
                return (time.perf_counter() - t0) / n * 1e6

            samples = [[] for _ in variants]
            est = max((run(vi, LAYERS), run(vi, 4 * LAYERS))[1] for vi in range(len(variants)))   # warm-up
            # a sample lasts at least --sample-ms under the host clock, whatever the launch takes
            launches = max(a.launches, int(a.sample_ms * 1e3 / est)) // LAYERS * LAYERS
            for _ in range(a.repeats):
                for vi in range(len(variants)):         # alternating, same process
                    samples[vi].append(run(vi, launches))
            row = {"ctx": ctx, "batch": B, "launches_per_sample": launches}
            for vi, (name, fp8, ks) in enumerate(variants):
                s = sorted(samples[vi])
                row[name + "_us"] = {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}
                if ks is None:
                    row[name + "_kv_bytes_read"] = B * NKV * ctx * (HD * (1 if fp8 else 2) + fp8) * 2
            a_, b_ = variants[0][0], variants[1][0]
            row[f"{b_}_over_{a_}"] = round(row[b_ + "_us"]["median"] / row[a_ + "_us"]["median"], 3)
            print(json.dumps(row), flush=True)
            results.append(row)
            for p in bufs:
                chk(q.qie_free(p), "free")
        for p in (dcs, dsn):
            chk(q.qie_free(p), "free")
    os.environ.pop("QIE_DEC_KS", None)
    return results


def extend_points(q, st, a):
    """--extend: M new rows over a prefix, us per call, three variants alternating in one process:
    qie_attention_extend on a bf16 cache; qie_kv_dequantize_fp8 of the prefix into a one-layer staging
    cache followed by qie_attention_extend on it (what an fp8-KV append ran per layer before
    qie_attention_extend_fp8); qie_attention_extend_fp8 on the codes."""
    chk = _lib.check

    def dmalloc(n, fill):
        p = C.c_void_p()
        chk(q.qie_malloc(C.byref(p), n), "qie_malloc")
        chk(q.qie_memset(p.value, fill, n), "memset")
        return p.value

    results = []
    for ctx in a.ctx:
        for M in a.rows:
            maxc = ctx + M + 128
            per_seq = LAYERS * NKV * maxc * HD
            c16, stg, c8 = _lib.KvCacheC(), _lib.KvCacheC(), _lib.KvCacheFp8C()
            for c, n, layers in ((c16, per_seq * 2, LAYERS), (stg, per_seq // LAYERS * 2, 1), (c8.c, per_seq, LAYERS)):
                c.k, c.v = dmalloc(n, 0x38), dmalloc(n, 0x38)
                c.seq_stride, c.n_layers, c.n_kv_heads, c.head_dim, c.max_ctx = per_seq // LAYERS * layers, layers, NKV, HD, maxc
            ne = LAYERS * NKV * maxc
            c8.k_exps, c8.v_exps, c8.exp_stride = dmalloc(ne, 127), dmalloc(ne, 127), ne
            qh = np.random.default_rng(ctx + M).standard_normal((M, NQ * HD)).astype(np.float32) * 0.05
            qh = ((qh.view(np.uint32) + 0x8000) >> 16).astype(np.uint16)
            pos = np.arange(ctx, ctx + M, dtype=np.int32)
            dq, dpos = dmalloc(qh.nbytes, 0), dmalloc(pos.nbytes, 0)
            chk(q.qie_memcpy_h2d(dq, qh.ctypes.data, qh.nbytes), "h2d")
            chk(q.qie_memcpy_h2d(dpos, pos.ctypes.data, pos.nbytes), "h2d")
            ws = dmalloc(max(16, q.qie_attention_extend_workspace_bytes(M, NQ, HD, maxc)), 0)
            out = dmalloc(M * NQ * HD * 2, 0)
            bufs = [c16.k, c16.v, stg.k, stg.v, c8.c.k, c8.c.v, c8.k_exps, c8.v_exps, dq, dpos, ws, out]

            def run(name, n):
                t0 = time.perf_counter()
                for i in range(n):
                    l = i % LAYERS
                    if name == "bf16":
                        chk(q.qie_attention_extend(dq, M, dpos, M, C.byref(c16), l, NQ, out, ws, st), name)
                    elif name == "expand_then_bf16":
                        chk(q.qie_kv_dequantize_fp8(C.byref(c8), 0, l, 0, ctx, C.byref(stg), 0, 0, st), name)
                        chk(q.qie_attention_extend(dq, M, dpos, M, C.byref(stg), 0, NQ, out, ws, st), name)
                    else:
                        chk(q.qie_attention_extend_fp8(dq, M, dpos, M, C.byref(c8), l, NQ, out, ws, st), name)
                chk(q.qie_stream_synchronize(st), "sync")
                return (time.perf_counter() - t0) / n * 1e6

            names = ("bf16", "expand_then_bf16", "fp8")
            est = max((run(nm, LAYERS), run(nm, LAYERS))[1] for nm in names)   # warm-up
            calls = max(LAYERS, int(a.sample_ms * 1e3 / est) // LAYERS * LAYERS)
            samples = {nm: [] for nm in names}
            for _ in range(a.repeats):
                for nm in names:                          # alternating, same process
                    samples[nm].append(run(nm, calls))
            row = {"prefix": ctx, "rows": M, "calls_per_sample": calls}
            for nm in names:
                s = sorted(samples[nm])
                row[nm + "_us"] = {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}
            row["fp8_over_expand_then_bf16"] = round(row["fp8_us"]["median"] / row["expand_then_bf16_us"]["median"], 3)
            row["fp8_over_bf16"] = round(row["fp8_us"]["median"] / row["bf16_us"]["median"], 3)
            print(json.dumps(row), flush=True)
            results.append(row)
            for p in bufs:
                chk(q.qie_free(p), "free")
    return results


def extend_engine(a):
    """--extend --engines: Batch.prefill(chunk=512) of 8k and 32k tokens on a kv_fp8 engine, tok/s.
    Run once per library (QIE_LIB selects another build) to compare two commits."""
    import qwen_inference_engine_amd as Q
    from qwen_inference_engine_amd import spec as S, weights as W
    eng = Q.Engine(S.QWEN2_7B, max_ctx=32768 + 64, kv_fp8=True).init_synthetic(W.SynthParams(seed=0))
    rows = []
    for n in (8192, 32768):
        ids = [int(t) for t in np.random.default_rng(1).integers(0, 1000, n)]
        b = eng.batch(1, 32768 + 64)
        tok = []
        for i in range(a.repeats + 1):                    # sample 0: warm-up, dropped
            eng.sync()
            t0 = time.perf_counter()
            b.prefill(0, ids, chunk=512)
            eng.sync()
            tok.append(n / (time.perf_counter() - t0))
        tok = sorted(tok[1:])
        rows.append({"tokens": n, "chunk": 512, "tok_s": {"median": round(tok[len(tok) // 2]), "min": round(tok[0]),
                                                          "max": round(tok[-1])}})
        print(json.dumps(rows[-1]), flush=True)
        b.close()
    eng.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--extend", action="store_true", help="the split-context attention over a prefix: bf16 cache, "
                    "expand + bf16 on staging, and qie_attention_extend_fp8 (profiles/kv_fp8_extend.json)")
    ap.add_argument("--rows", type=int, nargs="+", default=[16, 512], help="--extend: new rows per call")
    ap.add_argument("--ctx", type=int, nargs="+", default=[2048, 8192, 32768])
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--launches", type=int, default=280, help="launches per sample at the least")
    ap.add_argument("--sample-ms", type=float, default=100.0, help="a sample lasts this long at the least")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--steps", type=int, default=64, help="decode steps per engine sample")
    ap.add_argument("--engines", action="store_true", help="also the two engines: decode / prefill tok/s, kv_bytes")
    ap.add_argument("--step-ab", action="store_true",
                    help="only the fp8 form's 128-key against 256-key steps (QIE_DEC_KS: needs the development "
                         "build, QIE_LIB=.../lib/dev/libqie.so), at hd 128 and hd 64")
    ap.add_argument("--out", default="profiles/kv_fp8.json")
    a = ap.parse_args()
    q = _lib.load()
    st = C.c_void_p()
    _lib.check(q.qie_stream_create(C.byref(st)), "stream")
    doc = {}
    if os.path.exists(a.out):                           # the sections this run does not measure are kept
        with open(a.out) as f:
            doc = json.load(f)
    if a.extend:
        doc["what"] = ("M new rows over a prefix, us per call, Qwen2-7B heads (28 / 4 x 128), 28 layers visited in turn: "
                       "qie_attention_extend on a bf16 cache; qie_kv_dequantize_fp8 of the prefix + qie_attention_extend "
                       "on staging; qie_attention_extend_fp8")
        doc["points"] = extend_points(q, st, a)
        if a.engines:
            doc["engine_chunked_prefill"] = extend_engine(a)
    elif a.step_ab:
        assert os.environ.get("QIE_LIB"), "--step-ab needs the development build (make DEV=1; QIE_LIB)"
        ab = [("fp8_ks128", 1, 128), ("fp8_ks256", 1, 256)]
        doc["step_ab"] = {
            "what": "qie_attention_decode_fp8 us per launch with 128-key against 256-key block steps "
                    "(development build, QIE_DEC_KS), alternating in one process, pre-rotated form",
            "hd128_28q_4kv": bench_points(q, st, a, (NQ, NKV, HD, LAYERS), ab),
            "hd64_14q_2kv": bench_points(q, st, a, (14, 2, 64, 24), ab)}
    else:
        doc["what"] = ("decode attention us per launch, bf16 KV cache vs fp8 KV cache, operator tier, "
                       "Qwen2-7B heads (28 / 4 x 128), 28 layers visited in turn, pre-rotated form")
        doc["points"] = bench_points(q, st, a, (NQ, NKV, HD, LAYERS), [("bf16", 0, None), ("fp8", 1, None)])
        if a.engines:
            doc["engines"] = engines(a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
