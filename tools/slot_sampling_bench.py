#!/usr/bin/env python3
"""What per-slot sampling entries cost -> profiles/slot_sampling.json.

1. The operator alone, V = 152,064, M = 1 and 8, k = 50, T = 0.7: qie_sample (the baseline),
   qie_sample_rows with neutral entries, and with penalty windows of 512, 4,096 and 32,768 ids
   (random ids of the vocabulary, all three penalties on).  Each kind is captured as a hipGraph
   of INNER back-to-back calls and timed with hipEvents around REPLAYS replays, after a warm-up
   replay; the kinds alternate over REPS repetitions; per kind the median and [min, max] of the
   per-call microseconds.
2. A Qwen2-7B-shaped, B = 8, fp8-weight, paged (128-token pages) decode step — BASELINE config 4's
   step, at a context of 4,200 so that a 4,096-id window exists — sampled through the call's
   qie_sampling (k = 50, T = 0.7: the path without entries) and through entries with the same
   values plus penalties over the last 4,096 ids.  hipEvents on the engine's stream around STEPS
   replays of the captured step, every window from the same positions; alternated, REPS times.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qwen_inference_engine_amd as Q  # noqa: E402
from qwen_inference_engine_amd import _lib, spec as S, weights as W  # noqa: E402

OUT = os.path.join(ROOT, "profiles", "slot_sampling.json")
V = 152064
INNER, REPLAYS, REPS = 20, 50, 5
STEPS = 40
CTX = 4200


class Hip:
    """The few HIP runtime calls the timing needs (the runtime libqie itself links)."""

    def __init__(self):
        path = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamdhip64.so")
        self.h = C.CDLL(path if os.path.exists(path) else "libamdhip64.so")
        for name, args in [("hipEventCreate", [C.POINTER(C.c_void_p)]), ("hipEventRecord", [C.c_void_p, C.c_void_p]),
                           ("hipEventSynchronize", [C.c_void_p]), ("hipEventDestroy", [C.c_void_p]),
                           ("hipEventElapsedTime", [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]),
                           ("hipStreamBeginCapture", [C.c_void_p, C.c_int]),
                           ("hipStreamEndCapture", [C.c_void_p, C.POINTER(C.c_void_p)]),
                           ("hipGraphInstantiate", [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
                           ("hipGraphLaunch", [C.c_void_p, C.c_void_p]), ("hipGraphDestroy", [C.c_void_p]),
                           ("hipGraphExecDestroy", [C.c_void_p]), ("hipStreamSynchronize", [C.c_void_p])]:
            fn = getattr(self.h, name)
            fn.argtypes, fn.restype = args, C.c_int

    def ok(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: hip error {rc}")

    def events(self):
        a, b = C.c_void_p(), C.c_void_p()
        self.ok(self.h.hipEventCreate(C.byref(a)), "hipEventCreate")
        self.ok(self.h.hipEventCreate(C.byref(b)), "hipEventCreate")
        return a, b

    def elapsed_ms(self, stream, run):
        """Milliseconds of what run() enqueues on `stream`, between two events."""
        a, b = self.events()
        self.ok(self.h.hipEventRecord(a, stream), "hipEventRecord")
        run()
        self.ok(self.h.hipEventRecord(b, stream), "hipEventRecord")
        self.ok(self.h.hipEventSynchronize(b), "hipEventSynchronize")
        ms = C.c_float()
        self.ok(self.h.hipEventElapsedTime(C.byref(ms), a, b), "hipEventElapsedTime")
        self.h.hipEventDestroy(a)
        self.h.hipEventDestroy(b)
        return ms.value

    def capture(self, stream, enqueue):
        g, ex = C.c_void_p(), C.c_void_p()
        self.ok(self.h.hipStreamBeginCapture(stream, 1), "hipStreamBeginCapture")   # thread-local mode
        enqueue()
        self.ok(self.h.hipStreamEndCapture(stream, C.byref(g)), "hipStreamEndCapture")
        self.ok(self.h.hipGraphInstantiate(C.byref(ex), g, None, None, 0), "hipGraphInstantiate")
        self.h.hipGraphDestroy(g)
        return ex


def summary(v):
    return {"median": round(statistics.median(v), 2), "min_max": [round(min(v), 2), round(max(v), 2)]}


# ---------------------------------------------------------------------------------- 1. the operator
def dmem(lib, keep, a):
    a = np.ascontiguousarray(a)
    p = C.c_void_p()
    _lib.check(lib.qie_malloc(C.byref(p), max(a.nbytes, 16)), "qie_malloc")
    _lib.check(lib.qie_memcpy_h2d(p, a.ctypes.data, a.nbytes), "h2d")
    keep.append(p)
    return p


def op_table(lib, hip, M):
    r = np.random.default_rng(M)
    keep = []
    st = C.c_void_p()
    _lib.check(lib.qie_stream_create(C.byref(st)), "stream")
    lg = (r.standard_normal((M, V)) * 3).astype(np.float32).view(np.uint32)
    lg = ((lg + 0x7FFF + ((lg >> 16) & 1)) >> 16).astype(np.uint16)
    max_ctx = 32768
    d_lg = dmem(lib, keep, lg)
    d_hist = dmem(lib, keep, r.integers(0, V, (M, max_ctx)).astype(np.int32))
    d_q = dmem(lib, keep, np.full(M, max_ctx - 1, np.int32))
    d_step = dmem(lib, keep, np.arange(M, dtype=np.int32))
    d_ids = dmem(lib, keep, np.zeros(M, np.int32))
    d_ws = dmem(lib, keep, np.zeros(int(lib.qie_sample_workspace_bytes(M, V)), np.uint8))
    d_ws2 = dmem(lib, keep, np.zeros(int(lib.qie_sample_rows_workspace_bytes(M, V)), np.uint8))
    smp = Q.Sampling(top_k=50, temperature=0.7, seed=1234).to_c()

    def table_of(window):
        e = Q.SlotSampling(top_k=50, temperature=0.7, seed=1234)
        if window:
            e = Q.SlotSampling(top_k=50, temperature=0.7, seed=1234, repetition_penalty=1.1, presence_penalty=0.2,
                               frequency_penalty=0.1, penalty_last_n=window)
        arr = (_lib.SlotSamplingC * M)(*[e.to_c() for _ in range(M)])
        return dmem(lib, keep, np.frombuffer(bytes(arr), np.uint8).copy())

    def rows_call(tab):
        a = _lib.SampleRowsArgsC()
        a.logits, a.M, a.V, a.ld = d_lg, M, V, V
        a.table, a.slot0, a.slot_stride = tab, 0, 1
        a.hist, a.hist_stride, a.q_dev, a.step_dev, a.out_ids, a.ws = d_hist, max_ctx, d_q, d_step, d_ids, d_ws2
        return lambda: _lib.check(lib.qie_sample_rows(C.byref(a), st), "qie_sample_rows")

    calls = {"qie_sample": lambda: _lib.check(lib.qie_sample(d_lg, M, V, V, C.byref(smp), d_step, d_ids, d_ws, st),
                                              "qie_sample"),
             "rows_neutral": rows_call(table_of(0))}
    for w in (512, 4096, 32768):
        calls[f"rows_window_{w}"] = rows_call(table_of(w))
    graphs = {}
    for name, call in calls.items():
        call()                                    # outside a capture first: LDS limits, code objects
        hip.ok(hip.h.hipStreamSynchronize(st), "sync")
        graphs[name] = hip.capture(st, lambda: [call() for _ in range(INNER)])
        hip.ok(hip.h.hipGraphLaunch(graphs[name], st), "warm-up replay")
    hip.ok(hip.h.hipStreamSynchronize(st), "sync")
    cells = {name: [] for name in calls}
    for _ in range(REPS):
        for name, ex in graphs.items():
            ms = hip.elapsed_ms(st, lambda: [hip.ok(hip.h.hipGraphLaunch(ex, st), "replay") for _ in range(REPLAYS)])
            cells[name].append(ms * 1e3 / (INNER * REPLAYS))
    for ex in graphs.values():
        hip.h.hipGraphExecDestroy(ex)
    for p in keep:
        lib.qie_free(p)
    lib.qie_stream_destroy(st)
    out = {name: summary(v) for name, v in cells.items()}
    print(json.dumps({"M": M, **out}), flush=True)
    return out


# ------------------------------------------------------------------------------- 2. the decode step
def step_table(hip, n_layers):
    spec = S.QWEN2_7B if n_layers is None else S.QWEN2_7B.replace(n_layers=n_layers)
    B, max_ctx = 8, CTX + 256
    eng = Q.Engine(spec, max_ctx=max_ctx, weight_fp8=True).init_synthetic(W.SynthParams(seed=0))
    b = eng.batch(B, max_ctx, page_tokens=128)
    smp = Q.Sampling(top_k=50, temperature=0.7, seed=1234)
    r = np.random.default_rng(5)
    toks = []
    for s in range(B):
        ids = [int(t) for t in r.integers(0, spec.vocab, CTX)]
        b.prefill(s, ids, smp, chunk=1024)
        toks.append(ids[-1])
    entry = Q.SlotSampling(top_k=50, temperature=0.7, seed=1234, repetition_penalty=1.1, presence_penalty=0.2,
                           frequency_penalty=0.1, penalty_last_n=4096)
    st = eng.stream

    def window(entries):
        for s in range(B):
            b.set_sampling(s, entry if entries else None)
            b.set_position(s, CTX - 1, toks[s])   # every window decodes from the same positions
        b.decode(4, smp, want_ids=False)           # (re-)captures the step, warm
        eng.sync()
        ms = hip.elapsed_ms(st, lambda: _lib.check(eng.lib.qie_decode(b.h, STEPS, C.byref(smp.to_c()), None), "qie_decode"))
        return ms * 1e3 / STEPS

    cells = {"call_sampling": [], "entries_window_4096": []}
    for rep in range(REPS + 1):                    # repetition 0 is dropped
        for name, entries in (("call_sampling", False), ("entries_window_4096", True)):
            us = window(entries)
            if rep:
                cells[name].append(us)
    b.close()
    eng.close()
    out = {name: summary(v) for name, v in cells.items()}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--layers", type=int, default=None, help="fewer layers than Qwen2-7B's 28 (rehearsal)")
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    lib = _lib.load()
    hip = Hip()
    doc = {"operator": {"V": V, "k": 50, "temperature": 0.7, "unit": "us per call",
                        "method": "hipEvents around %d replays of a hipGraph of %d back-to-back calls; %d alternated "
                                  "repetitions: median, [min, max]" % (REPLAYS, INNER, REPS),
                        "M1": op_table(lib, hip, 1), "M8": op_table(lib, hip, 8)}}
    if not args.skip_step:
        doc["decode_step"] = {"model": "Qwen2-7B widths, %s layers, fp8 weights, B = 8, paged KV (128-token pages), "
                                       "context %d, k = 50, T = 0.7" % (args.layers or 28, CTX),
                              "unit": "us per step",
                              "method": "hipEvents on the engine's stream around %d replays of the captured step; %d "
                                        "alternated repetitions after one dropped: median, [min, max]" % (STEPS, REPS),
                              **step_table(hip, args.layers)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


if __name__ == "__main__":
    main()
