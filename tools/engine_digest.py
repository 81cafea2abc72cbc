#!/usr/bin/env python3
"""The engine's outputs per host path (tools/gemm_digest.py compares two LIBRARIES kernel by
kernel; this does it for engine.hip's orchestration): run it once per build, selected by QIE_LIB,
and diff the two outputs — a host-only change to the engine must reproduce every line.  One JSON
line per case: the generated ids and a SHA-256 of every step's logits (qie_batch_logits;
qie_verify_logits for a verify step).

Cases (tests/test_gpu_engine.py's tiny CONFIGS, synthetic weights, fixed seeds):
  * bf16 prefill (P = 5: split attention at <= 8 rows; P = 40: MFMA flash attention) + 4 decode
    steps, graph and eager, B = 1 and B = 2 (the pre-normed rows);
  * qie_prefill_batch: 3 prompts into slots 1-3 of 4, contiguous and paged (128-token pages);
  * qie_prefill_append: (P0, n) = (5, 37) and (40, 9);
  * qie_verify: 0, 7 and 15 drafts, greedy and top-k sampled, graph and eager, each step twice
    (capture, then replay);
  * fp8 weights, on a CONFIGS model (its widths keep the plain layout: fp8_t16 off) and on a tiny
    model whose widths take the 16-row tiled layout (K = 896 / 2,048: the batched-decode kernel
    reads every projection): P = 5 (fp8 codes), P = 23 (tiled: the dequantised copy), P = 300
    (>= 256 rows: the dequantised copy), 4 decode steps at B = 8 (the batched-decode kernel's
    fused norm where it applies), verify with 7 drafts;
  * prefill_fp8: tests/test_gpu_fp8_mx.py's test_engine_prefill_fp8_batched_tiny configuration;
  * comm_always at world size 1 (the exchange form of the row-parallel projections, the
    gathered head): prefill, 4 decode steps, verify with 7 drafts, greedy and sampled; scoring;
  * qie_batch_debug_step: a hash of the residual snapshots;
  * qie_score, fused and QIE_SCORE_UNFUSED, from position 0 and as an append (hashes of the
    log-probabilities and the greedy ids); qie_batch_logprobs;
  * release, then a new prefill of the slot; set_position;
  * the prefill rows growing on one batch: P = 5, 40, 5, then an append;
  * decode mode 1 (the persistent step), 4 steps;
  * paged batches whose slots share pages (3 slots, max_ctx 512, 128-token pages, prompts of about
    300 ids; after every call the block tables, page counts, free pages and positions, and a hash
    of the K/V rows where a copy happened): a fork at n == p and at n < p with a partial tail + 2
    decode steps; the fork rewound by set_position into a shared page + a step; an append at a
    pos0 inside a shared page; a verify with 7 drafts from a position rewound below the fork
    point; save_prefix / load_prefix / append of the remainder / drop; prefill_batch over two
    slots that share pages with each other; source and fork both rewound into the same shared
    page + a step; in a pool with no free page the refused set_position, append, verify, fork,
    prefill, prefill_batch, reserve and decode calls (the return code from the exception's text),
    then a step; reserve on a paged slot."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import qwen_inference_engine_amd as Q  # noqa: E402
from qwen_inference_engine_amd import spec as S, weights as W  # noqa: E402

CONFIGS = {
    "qwen2-bias-hd64": S.tiny("t-q2", n_layers=3, hidden=256, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512,
                              vocab=1000, bias=True),
    "qwen3-qknorm-hd128": S.tiny("t-q3", n_layers=2, hidden=512, n_heads=8, n_kv_heads=2, head_dim=128, ffn=768,
                                 vocab=1536, bias=False, qk_norm=True),
    "tied-g7": S.tiny("t-tied", n_layers=2, hidden=448, n_heads=7, n_kv_heads=1, head_dim=64, ffn=640,
                      vocab=777 * 2, tie=True, bias=True),
}
TILED = S.tiny("t-t16", n_layers=2, hidden=896, n_heads=14, n_kv_heads=2, head_dim=64, ffn=2048, vocab=1024, bias=True)
MX = S.tiny("t-mx", n_layers=2, hidden=256, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, vocab=1024, bias=True)
PERSIST = S.tiny("t-q3-128", n_layers=3, hidden=1024, n_heads=8, n_kv_heads=2, head_dim=128, ffn=2048, vocab=4096,
                 bias=False, qk_norm=True)
SYN = W.SynthParams(seed=11, w_scale=0.08, norm_scale=0.25, bias_scale=0.05)
SAMPLED = Q.Sampling(top_k=40, temperature=0.8, top_p=0.9, seed=99)


def ids(spec, seed, n):
    return [int(t) for t in np.random.default_rng(seed).integers(0, spec.vocab, n)]


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


class Case:
    """Collects what one case generates; prints it as one line."""

    def __init__(self, name):
        self.rec = {"case": name, "ids": [], "logits": []}

    def took(self, toks, b, rows=None):
        """rows: the slots whose logits this step wrote (default: all of the batch)"""
        self.rec["ids"].append([int(t) for t in np.atleast_1d(toks)])
        self.rec["logits"].append(sha(b.logits()[rows if rows is not None else slice(None)]))

    def decode(self, b, n, smp=Q.GREEDY, rows=None):
        for _ in range(n):
            self.took(b.decode_step(smp), b, rows)

    def verify(self, b, seq, draft, smp):
        self.rec["ids"].append(b.verify(seq, draft, smp))
        self.rec["logits"].append(sha(b.verify_logits()))

    def done(self, b=None):
        print(json.dumps(self.rec), flush=True)
        if b is not None:
            b.close()


def drafts(b_twin, spec, n, smp):
    """n drafts for a sequence in the twin batch's state: its own next tokens, one of them wrong."""
    if n == 0:
        return []
    d = [int(b_twin.decode_step(smp)[0]) for _ in range(n)]
    d[n // 2] = (d[n // 2] + 1) % spec.vocab
    return d


def verify_cases(tag, eng, spec, counts, samplings, P=12):
    for n in counts:
        for sn, smp in samplings:
            c = Case(f"{tag}_verify{n}_{sn}")
            b, twin = eng.batch(1, eng.max_ctx), eng.batch(1, eng.max_ctx)
            prompt = ids(spec, 31, P)
            c.took(b.prefill(0, prompt, smp), b)
            twin.prefill(0, prompt, smp)
            d = drafts(twin, spec, n, smp)
            c.verify(b, 0, d, smp)                                  # captures (graph engines)
            c.verify(b, 0, ids(spec, 32, n), smp)                   # replays; junk drafts
            c.took(b.decode_step(smp), b)
            twin.close()
            c.done(b)


def score_cases(tag, eng, spec, unfused_forms):
    """qie_score from position 0 (P = 40: the prefill rows grow past the scoring rows' first
    size) and as an append: the log-probabilities and the greedy ids of every row."""
    for unfused in unfused_forms:
        c = Case(f"{tag}_score_{'unfused' if unfused else 'fused'}")
        b = eng.batch(1, eng.max_ctx)
        text = ids(spec, 60, 40 + 21)
        lp, gr, nxt = b.score(0, text[:40], unfused=unfused)
        c.took(nxt, b)
        lp2, gr2, nxt = b.score(0, text[40:], pos0=40, unfused=unfused)
        c.took(nxt, b)
        c.rec["logprobs"] = [sha(lp), sha(lp2)]
        c.rec["greedy"] = [sha(gr), sha(gr2)]
        c.decode(b, 2)
        c.done(b)


class PagedCase(Case):
    """A case on a paged batch of 3 slots (tests/test_gpu_fork.py's: max_ctx 512, 128-token pages):
    after every call the record gains every slot's block table, the page counts, the free-page
    count and the positions."""

    def __init__(self, name, eng, n_pages=0):
        super().__init__(name)
        self.b = eng.batch(3, 512, page_tokens=128, n_pages=n_pages)
        self.rec.update(pages=[], rc=[], rows=[])

    def state(self):
        b = self.b
        self.rec["pages"].append({"tables": [b.block_table(s, 4).tolist() for s in range(3)],
                                  "refs": b.page_refs().tolist(), "free": int(b.page_stats()[0]),
                                  "pos": b.positions().tolist()})

    def call(self, fn, *a, **kw):
        """A call that returns nothing to hash (fork, set_position, reserve, ...)."""
        out = fn(*a, **kw)
        self.state()
        return out

    def tok(self, fn, *a, rows=None, **kw):
        """A call that returns ids and writes logits (prefill, append, prefill_batch)."""
        self.took(fn(*a, **kw), self.b, rows)
        self.state()

    def step(self, n=1, rows=None):
        for _ in range(n):
            self.decode(self.b, 1, rows=rows)
            self.state()

    def refused(self, fn, *a, **kw):
        """A call the pool must refuse: the return code, from the exception's text."""
        try:
            fn(*a, **kw)
            self.rec["rc"].append(0)
        except Q._lib.QieError as e:
            self.rec["rc"].append(int(str(e).split("rc=")[1].split(")")[0]))
        self.state()

    def kv(self, seq, n):
        """K/V rows [0, n) of a slot, every layer: where a copy happened."""
        self.rec["rows"].append(sha(np.concatenate([np.stack(self.b.kv_rows(seq, l, n)).ravel()
                                                    for l in range(self.b.e.spec.n_layers)])))

    def done(self):
        super().done(self.b)


def paged_cases(eng, spec):
    """Forks, copy-on-write and prefix handles: every writer's reservation on shared pages."""
    prompt = ids(spec, 101, 297)

    def forked(name, n_pages=0, at=None):
        """Slot 0 at position 300 (prefill of 297 + 3 steps), forked into slot 2."""
        c = PagedCase(name, eng, n_pages)
        c.tok(c.b.prefill, 0, prompt, rows=slice(0, 1))
        c.step(3, rows=slice(0, 1))
        c.call(c.b.fork, 0, 2, at)
        return c

    for at in (None, 200):   # n == p, and n < p with a partial tail
        c = forked(f"paged_fork_at_{at or 'p'}", at=at)
        c.kv(2, at or 300)
        c.step(2)
        c.done()
    c = forked("paged_fork_rewound_set_position")
    c.call(c.b.set_position, 2, 200, 5)
    c.kv(2, 200)
    c.step()
    c.done()
    c = forked("paged_append_into_shared_page")
    c.tok(c.b.append, 2, ids(spec, 102, 20), 130, rows=slice(2, 3))
    c.kv(2, 150)
    c.kv(0, 300)
    c.step()
    c.done()
    c = forked("paged_verify_below_fork_point")
    c.call(c.b.set_position, 2, 125, 5)                         # page 0 private; rows 125..132 reach shared page 1
    c.kv(2, 125)
    c.verify(c.b, 2, ids(spec, 103, 7), Q.GREEDY)
    c.state()
    c.step()
    c.done()
    c = forked("paged_prefix_save_load_append_drop")
    hist = c.b.history(0, 300).tolist()
    pf = c.call(c.b.save_prefix, 0, 256)
    c.call(c.b.release, 0)
    c.call(c.b.load_prefix, pf, 1, hist[128], 128)
    c.tok(c.b.append, 1, hist[128:300] + ids(spec, 104, 17), 128, rows=slice(1, 2))
    c.kv(1, 317)
    c.call(pf.drop)
    c.step()
    c.done()
    # slots 1 and 2 share two pages with each other (and with slot 0), then both start new prompts;
    # in a full pool the same call is refused (the shared pages count as returned by neither)
    for n_pages in (0, 5):
        c = forked(f"paged_prefill_batch_over_sharing_slots_{n_pages or 'roomy'}", n_pages)
        c.call(c.b.fork, 0, 1, 256)
        if n_pages:
            c.refused(c.b.prefill_batch, 1, [ids(spec, 108, 200), ids(spec, 109, 200)])
            c.refused(c.b.decode_step)                          # slot 1 at 256 needs a third page
        else:
            c.tok(c.b.prefill_batch, 1, [ids(spec, 108, 200), ids(spec, 109, 200)], rows=slice(1, 3))
            c.step(2)
        c.kv(0, 300)
        c.done()
    c = forked("paged_both_rewound_into_one_page", at=256)
    c.call(c.b.set_position, 0, 130, 5)
    c.call(c.b.set_position, 2, 130, 6)
    c.step()
    c.kv(0, 131)
    c.kv(2, 131)
    c.done()
    # a pool with no free page (scratch + 3 for the source + the fork's tail page): every refusal,
    # then a decode step
    c = forked("paged_refusals_in_a_full_pool", n_pages=5)
    c.refused(c.b.set_position, 2, 200, 5)
    c.refused(c.b.append, 2, ids(spec, 110, 20), 130)
    tok300 = int(c.b.history(0, 301)[300])
    c.call(c.b.set_position, 0, 380, 5)                         # within slot 0's own third page
    c.refused(c.b.verify, 0, ids(spec, 111, 7))                 # rows 380..387 need a fourth
    c.call(c.b.set_position, 0, 300, tok300)
    c.refused(c.b.fork, 0, 1, 300)
    c.refused(c.b.prefill, 1, ids(spec, 112, 10))
    c.refused(c.b.prefill_batch, 1, [ids(spec, 113, 140), ids(spec, 114, 140)])
    c.refused(c.b.reserve, 1, 10)
    c.refused(c.b.set_position, 1, 10, 5)
    c.refused(c.b.decode, 100)
    c.step()
    c.done()
    c = PagedCase("paged_reserve", eng)
    c.call(c.b.reserve, 1, 300)
    c.tok(c.b.prefill, 0, ids(spec, 115, 40), rows=slice(0, 1))
    c.call(c.b.reserve, 0, 129)
    c.call(c.b.reserve, 1, 100)
    c.step()
    c.done()


def main():
    # bf16: prefill + decode, prefill_batch, append, verify, debug step
    for name, spec in CONFIGS.items():
        for graph in (True, False):
            g = "graph" if graph else "eager"
            eng = Q.Engine(spec, max_ctx=128, use_graph=graph).init_synthetic(SYN)
            for P in (5, 40):
                for B in (1, 2):
                    c = Case(f"bf16_{name}_{g}_P{P}_B{B}")
                    b = eng.batch(B, 128)
                    for i in range(B):
                        c.took(b.prefill(i, ids(spec, 1 + i, P)), b, slice(0, i + 1))
                    c.decode(b, 4)
                    c.done(b)
            verify_cases(f"bf16_{name}_{g}", eng, spec, (0, 7, 15), (("greedy", Q.GREEDY), ("sampled", SAMPLED)))
            if graph:
                for paged in (False, True):
                    for L in (5, 40):
                        c = Case(f"bf16_{name}_prefill_batch_L{L}_{'paged' if paged else 'contig'}")
                        b = eng.batch(4, 128, page_tokens=128 if paged else None)
                        c.took(b.prefill_batch(1, [ids(spec, 10 + i, L) for i in range(3)]), b, slice(1, 4))
                        c.decode(b, 2, rows=slice(1, 4))
                        c.done(b)
                    for P0, n in ((5, 37), (40, 9)):
                        c = Case(f"bf16_{name}_append_{P0}_{n}_{'paged' if paged else 'contig'}")
                        b = eng.batch(1, 128, page_tokens=128 if paged else None)
                        c.took(b.prefill(0, ids(spec, 20, P0)), b)
                        c.took(b.append(0, ids(spec, 21, n), P0), b)
                        c.decode(b, 2)
                        c.done(b)
                c = Case(f"bf16_{name}_debug_step")
                b = eng.batch(2, 128)
                for i in range(2):
                    c.took(b.prefill(i, ids(spec, 1 + i, 9)), b, slice(0, i + 1))
                toks, xs = b.debug_step()
                c.took(toks, b)
                c.rec["residuals"] = sha(xs)
                c.done(b)
            eng.close()
    # fp8 weights: plain layout (a CONFIGS model) and the tiled layout
    for tag, spec in (("fp8_plain", CONFIGS["qwen2-bias-hd64"]), ("fp8_tiled", TILED)):
        eng = Q.Engine(spec, max_ctx=384, weight_fp8=True).init_synthetic(SYN)
        for P in (5, 23, 300):
            c = Case(f"{tag}_P{P}")
            b = eng.batch(1, 384)
            c.took(b.prefill(0, ids(spec, 40, P)), b)
            c.decode(b, 4)
            c.done(b)
        c = Case(f"{tag}_B8")
        b = eng.batch(8, 384)
        for i in range(8):
            c.took(b.prefill(i, ids(spec, 50 + i, 5)), b, slice(0, i + 1))
        c.decode(b, 4)
        c.done(b)
        verify_cases(tag, eng, spec, (7,), (("greedy", Q.GREEDY),))
        eng.close()
    # prefill_fp8
    eng = Q.Engine(MX, max_ctx=96, weight_fp8=True, prefill_fp8=True).init_synthetic(SYN)
    c = Case("prefill_fp8_batched")
    b = eng.batch(4, 96)
    c.took(b.prefill_batch(0, [ids(MX, 50 + i, 70) for i in range(4)]), b)
    c.decode(b, 6)
    c.done(b)
    eng.close()
    # the exchange path at world size 1
    spec = CONFIGS["qwen2-bias-hd64"]
    comm = Q.Comm.rccl(Q.Comm.unique_id(), 1, 0, 0)
    for graph in (True, False):
        g = "graph" if graph else "eager"
        eng = Q.Engine(spec, max_ctx=128, use_graph=graph, comm=comm, comm_always=True).init_synthetic(SYN)
        for sn, smp in (("greedy", Q.GREEDY), ("sampled", SAMPLED)):
            for P in (5, 40):
                c = Case(f"comm_{g}_{sn}_P{P}")
                b = eng.batch(2, 128)
                for i in range(2):
                    c.took(b.prefill(i, ids(spec, 1 + i, P), smp), b, slice(0, i + 1))
                c.decode(b, 4, smp)
                c.done(b)
            verify_cases(f"comm_{g}", eng, spec, (7,), ((sn, smp),))
        if graph:
            score_cases("comm", eng, spec, (True,))   # the exchange form always scores unfused
        eng.close()
    comm.close()
    # scoring, qie_batch_logprobs, slot reuse, scratch growth (bf16, graph)
    eng = Q.Engine(spec, max_ctx=128).init_synthetic(SYN)
    score_cases("bf16", eng, spec, (False, True))
    c = Case("bf16_logprobs_B2")
    b = eng.batch(2, 128)
    for i in range(2):
        c.took(b.prefill(i, ids(spec, 1 + i, 9)), b, slice(0, i + 1))
    c.rec["logprobs"] = [sha(b.logprobs(ids(spec, 80, 2))), sha(b.logprobs([-1, 3]))]
    c.done(b)
    c = Case("bf16_release_reprefill_set_position")
    b = eng.batch(2, 128)
    for i in range(2):
        c.took(b.prefill(i, ids(spec, 1 + i, 9)), b, slice(0, i + 1))
    c.decode(b, 2)
    b.release(0)
    c.took(b.prefill(0, ids(spec, 81, 40)), b)
    c.decode(b, 2)
    b.set_position(1, 4, 17)   # rewind slot 1 to position 4 with token 17 pending
    c.decode(b, 2)
    c.done(b)
    c = Case("bf16_scratch_growth")   # the prefill rows made, regrown, reused, then an append
    b = eng.batch(1, 128)
    for i, P in enumerate((5, 40, 5)):
        c.took(b.prefill(0, ids(spec, 82 + i, P)), b)
    c.took(b.append(0, ids(spec, 85, 50), 5), b)
    c.decode(b, 2)
    c.done(b)
    eng.close()
    # paged batches whose slots share pages (tests/test_gpu_fork.py's model and geometry)
    eng = Q.Engine(spec, max_ctx=512).init_synthetic(SYN)
    paged_cases(eng, spec)
    eng.close()
    # decode mode 1: the persistent step (tests/test_gpu_persist.py's qk-norm model)
    eng = Q.Engine(PERSIST, max_ctx=64).init_synthetic(SYN)
    c = Case("bf16_persistent_step")
    b = eng.batch(1, 64)
    b.set_decode_mode(1)
    c.took(b.prefill(0, ids(PERSIST, 90, 20)), b)
    c.decode(b, 4)
    c.done(b)
    eng.close()


if __name__ == "__main__":
    main()
