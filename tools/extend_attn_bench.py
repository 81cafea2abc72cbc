#!/usr/bin/env python3
"""qie_attention_extend against qie_attention on "n new rows over a cached prefix" (the
shipped library, seeded inputs, no engine): Qwen2-7B heads (28 / 4, hd 128), the shapes an
append meets, contiguous and paged-128.  Both operators get the same q, cache and pos array
— qie_attention with offset positions is what an append would have had to call without the
new kernel — and both outputs are checked against the CPU oracle on a 4-row sample.  Timing:
device events around ITERS launches after a warm-up, the two operators alternating in one
process, the whole table REPS times.  One end-to-end line: Qwen2-7B widths, 2 layers,
synthetic weights — prefill(8,192) against prefill(8,064) + append(128).
Writes the JSON report to --out (default profiles/extend_attention.json)."""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import gpu_util as G  # noqa: E402
import oracle as O  # noqa: E402
import qwen_inference_engine_amd as Q  # noqa: E402
from qwen_inference_engine_amd import _lib, spec as S, weights as W  # noqa: E402
from qwen_inference_engine_amd._lib import KvCacheC  # noqa: E402

NQ, NKV, HD, MAXC, T = 28, 4, 128, 8192, 128
SHAPES = [(8, 8184), (16, 8176), (128, 8064), (512, 7680), (128, 1024)]   # (new rows, prefix)
ITERS, WARM, REPS = 200, 20, 3
BAR = 2 ** -6   # tests/test_gpu_extend.py's


def rnd(shape, seed):
    a = np.random.default_rng(seed).standard_normal(shape).astype(np.float32)
    return O.f32_to_bf16(a)


class Events:
    """hipEvents of the runtime libqie runs on (elapsed ms between two records on stream 0)."""

    def __init__(self):
        try:
            self.hip = C.CDLL("libamdhip64.so")
        except OSError:
            self.hip = C.CDLL(os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so"))
        self.a, self.b = C.c_void_p(), C.c_void_p()
        for e in (self.a, self.b):
            assert self.hip.hipEventCreate(C.byref(e)) == 0

    def time(self, fn, iters):
        assert self.hip.hipEventRecord(self.a, None) == 0
        for _ in range(iters):
            fn()
        assert self.hip.hipEventRecord(self.b, None) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        ms = C.c_float()
        assert self.hip.hipEventElapsedTime(C.byref(ms), self.a, self.b) == 0
        return ms.value * 1e3 / iters   # us per launch


def caches(kc_h, vc_h):
    """{layout: descriptor} of one sequence's cache [1][1][NKV][MAXC][HD]; the keep-alive list."""
    keep = []
    c = KvCacheC()
    kc, vc = G.dev(kc_h), G.dev(vc_h)
    c.k, c.v, c.seq_stride = G.p(kc), G.p(vc), NKV * MAXC * HD
    c.n_layers, c.n_kv_heads, c.head_dim, c.max_ctx = 1, NKV, HD, MAXC
    mp = MAXC // T
    table = np.random.default_rng(5).permutation(np.arange(1, mp + 1)).astype(np.int32)
    pools = []
    for h in (kc_h, vc_h):
        pool = rnd((mp + 1, 1, NKV, T, HD), 77)   # page 0: garbage
        for j in range(mp):
            pool[table[j], 0] = h[0, 0, :, j * T:(j + 1) * T]
        pools.append(G.dev(pool))
    dt = G.dev(table)
    p = KvCacheC()
    p.k, p.v, p.seq_stride = G.p(pools[0]), G.p(pools[1]), NKV * T * HD
    p.n_layers, p.n_kv_heads, p.head_dim, p.max_ctx = 1, NKV, HD, MAXC
    p.block_table, p.page_tokens, p.max_pages = G.p(dt), T, mp
    keep += [kc, vc, dt] + pools
    return {"contiguous": c, "paged128": p}, keep


def operator_table(report):
    lib = _lib.load()
    ev = Events()
    kc_h, vc_h = rnd((1, 1, NKV, MAXC, HD), 1), rnd((1, 1, NKV, MAXC, HD), 2)
    descs, keep = caches(kc_h, vc_h)
    kv_bytes = lambda ctx: 2 * NKV * ctx * HD * 2   # K and V of one layer, read once
    rows = []
    for rep in range(REPS):
        for n, pre in SHAPES:
            q_h = rnd((n, NQ * HD), 100 + n)
            pos_h = np.arange(pre, pre + n, dtype=np.int32)
            q, pos = G.dev(q_h), G.dev(pos_h)
            sample = sorted({0, n // 3, (2 * n) // 3, n - 1})
            want = None
            for layout, c in descs.items():
                ws_e = G.zeros_bytes(lib.qie_attention_extend_workspace_bytes(n, NQ, HD, MAXC))
                ws_o = G.zeros_bytes(lib.qie_attention_workspace_bytes(n, NQ, HD, MAXC))
                out_e, out_o = G.zeros_bf16(n, NQ * HD), G.zeros_bf16(n, NQ * HD)
                ext = lambda: G.check(lib.qie_attention_extend(G.p(q), n, G.p(pos), n, C.byref(c), 0, NQ, G.p(out_e),
                                                               G.p(ws_e), None))
                old = lambda: G.check(lib.qie_attention(G.p(q), n, G.p(pos), n, C.byref(c), 0, NQ, G.p(out_o),
                                                        G.p(ws_o), None))
                for fn in (ext, old):
                    for _ in range(WARM):
                        fn()
                G.check(lib.qie_synchronize())
                us_e = ev.time(ext, ITERS)
                us_o = ev.time(old, ITERS)
                row = {"rep": rep, "rows": n, "prefix": pre, "layout": layout, "extend_us": round(us_e, 2),
                       "attention_us": round(us_o, 2), "speedup": round(us_o / us_e, 2),
                       "kv_bytes": kv_bytes(pre + n), "extend_TBps": round(kv_bytes(pre + n) / us_e / 1e6, 3)}
                if rep == 0:   # outputs against the oracle, 4 rows
                    if want is None:
                        want = {r: O.attention(q_h[r:r + 1], kc_h[0, 0, :, :pos_h[r] + 1], vc_h[0, 0, :, :pos_h[r] + 1],
                                               NQ, NKV, HD, True, int(pos_h[r]))[0] for r in sample}
                    ge, go = G.host_bf16(out_e), G.host_bf16(out_o)
                    row["extend_max_abs_err"] = float(max(np.abs(G.bf(ge[r]) - G.bf(want[r])).max() for r in sample))
                    row["attention_max_abs_err"] = float(max(np.abs(G.bf(go[r]) - G.bf(want[r])).max() for r in sample))
                    row["extend_ok"] = bool(row["extend_max_abs_err"] <= BAR)
                    row["attention_ok"] = bool(row["attention_max_abs_err"] <= BAR)
                rows.append(row)
                print(json.dumps(row), flush=True)
    report["operator"] = rows
    report["split_tokens"] = {str(n): lib.qie_attention_extend_split_tokens(n, MAXC) for n, _ in SHAPES}
    del keep
    G.release_all()


def end_to_end(report):
    """prefill(8,192) against prefill(8,064) + append(128): the append alone vs a full re-prefill."""
    spec = S.QWEN2_7B.replace(n_layers=2)
    eng = Q.Engine(spec, max_ctx=8320).init_synthetic(W.SynthParams(seed=0))
    ids = [int(t) for t in np.random.default_rng(3).integers(0, spec.vocab, 8192)]
    b = eng.batch(1, 8320)
    lib = _lib.load()

    def ms(fn):
        G.check(lib.qie_synchronize())
        t0 = time.perf_counter()
        fn()   # returns after the sampled id is on the host
        return (time.perf_counter() - t0) * 1e3

    b.prefill(0, ids)           # warm-up (scratch allocation)
    b.prefill(0, ids[:8064])
    b.append(0, ids[8064:])
    full, app = [], []
    for _ in range(5):
        full.append(ms(lambda: b.prefill(0, ids)))
        b.prefill(0, ids[:8064])
        app.append(ms(lambda: b.append(0, ids[8064:], 8064)))
    f, a = float(np.median(full)), float(np.median(app))
    report["end_to_end"] = {"model": "Qwen2-7B widths, 2 layers, synthetic", "prefill_8192_ms": round(f, 3),
                            "append_128_over_8064_ms": round(a, 3), "ratio": round(f / a, 2),
                            "prefill_8192_ms_all": [round(x, 3) for x in full],
                            "append_ms_all": [round(x, 3) for x in app]}
    print(json.dumps(report["end_to_end"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "extend_attention.json"))
    ap.add_argument("--skip-e2e", action="store_true")
    args = ap.parse_args()
    report = {"heads": {"nq": NQ, "nkv": NKV, "hd": HD}, "max_ctx": MAXC, "iters": ITERS, "reps": REPS}
    operator_table(report)
    if not args.skip_e2e:
        end_to_end(report)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    bad = [r for r in report["operator"] if r.get("extend_ok") is False]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
