#!/usr/bin/env python3
"""Dev build (QIE_LIB=.../dev/libqie.so, QIE_GRAPH_DUMP=1): print every node of the decode
graph (kernel grid / block / dynamic LDS) for GD_MODEL, after a GD_P-token prefill of each of
GD_BATCH sequences (default 1); GD_FP8=1 fp8 weights, GD_PAGE_TOKENS=N a paged KV cache.

GD_NORMALIZE=file: instead of running a model, rewrite a captured dump (stderr of a run) with
every kernel address replaced by the index of its first occurrence, so that the dumps of two
builds compare equal exactly when their launch geometries do."""
import os
import re
import sys

if os.environ.get("GD_NORMALIZE"):
    seen = {}
    for line in open(os.environ["GD_NORMALIZE"]):
        if not line.startswith("graph"):
            continue
        print(re.sub(r"kernel (0x[0-9a-f]+)", lambda m: "kernel #%d" % seen.setdefault(m.group(1), len(seen)),
                     line.rstrip()))
    sys.exit(0)

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qwen_inference_engine_amd as Q  # noqa: E402
from qwen_inference_engine_amd import spec as S, weights as W  # noqa: E402

spec = S.PRESETS[os.environ.get("GD_MODEL", "Qwen2-0.5B")]
P = int(os.environ.get("GD_P", "128"))
B = int(os.environ.get("GD_BATCH", "1"))
PT = int(os.environ.get("GD_PAGE_TOKENS", "0"))
eng = Q.Engine(spec, max_ctx=P + 64, weight_fp8=os.environ.get("GD_FP8", "0") == "1").init_synthetic(
    W.SynthParams(seed=0))
b = eng.batch(B, P + 64, page_tokens=PT or None)
for i in range(B):
    b.prefill(i, [int(t) for t in np.random.default_rng(1 + i).integers(0, spec.vocab, P)])
print(b.decode(2).tolist())
