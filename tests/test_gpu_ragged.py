"""GPU: qie_prefill_ragged — prompts and appends of any lengths in one pass — against the CPU
oracle and against the single calls it replaces.

Numerics: the bars of test_gpu_append.py (logits within logit_tol of the oracle's, every token
the oracle's arg-max or a near-tie, flips <= parity.max_flips).  Logits are not compared with the
single calls' bit for bit: the GEMM kernels are picked by the total row count.  Everything that
is an integer — positions, history, pages — is compared exactly; bit-exact checks compare two
runs of the same kernels."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as G
from parity import max_flips
from test_gpu_append import _check_logits, _ids, _rc
from test_gpu_engine import CONFIGS, SYN

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib, spec as S, weights as W

pytestmark = pytest.mark.gpu

SPEC = CONFIGS["qwen2-bias-hd64"]


def _follow_all(oracle, b, om, lg, tok, n_steps, what=""):
    """_follow of test_gpu_append.py for several slots at once: om / lg / tok are dicts by slot
    (each slot its own oracle model, fed the engine's own tokens).  Returns (flips, decisions)."""
    got = b.logits()
    flips = sum(_check_logits(oracle, got[s], lg[s], tok[s], f"{what} slot {s} first") for s in om)
    tok = dict(tok)
    for t in range(n_steps):
        want = {s: om[s].forward([tok[s]]) for s in om}
        ids = b.decode_step()
        got = b.logits()
        for s in om:
            tok[s] = ids[s]
            flips += _check_logits(oracle, got[s], want[s], tok[s], f"{what} slot {s} step {t}")
    return flips, len(om) * (n_steps + 1)


def _mixed(oracle, eng, hw, spec, max_ctx, paged, what):
    """Slot 3 is prefilled with 40 ids; then ONE ragged call: slot 0 fresh 5 ids, slot 1 fresh 37
    ids, slot 3 appends 9 ids at 40; slot 2 stays idle.  Each of the three against its own oracle."""
    b = eng.batch(4, max_ctx, page_tokens=128 if paged else None)
    p0, p1, p3 = _ids(1, 5, spec), _ids(2, 37, spec), _ids(3, 49, spec)
    b.prefill(3, p3[:40])
    toks = b.prefill_ragged([(0, p0), (1, p1, 0), (3, p3[40:], 40)])
    assert [int(p) for p in b.positions()] == [5, 37, 0, 49]
    om, lg, tok = {}, {}, {}
    for s, pr, t in ((0, p0, toks[0]), (1, p1, toks[1]), (3, p3, toks[2])):
        hist = b.history(s, len(pr) + 1)
        assert list(hist[:-1]) == pr and int(hist[-1]) == t, f"{what}: history of slot {s}"
        om[s] = oracle.Model(hw, max_ctx)
        lg[s], tok[s] = om[s].forward(pr, 0), t
    flips, n = _follow_all(oracle, b, om, lg, tok, 3, what)
    assert flips <= max_flips(n)
    assert [int(p) for p in b.positions()][:2] == [8, 40] and int(b.positions()[3]) == 52
    b.close()


@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_ragged_matches_oracle(oracle, name, paged):
    spec = CONFIGS[name]
    eng = Q.Engine(spec, max_ctx=160).init_synthetic(SYN)
    _mixed(oracle, eng, W.HostWeights.synthetic(spec, SYN), spec, 160, paged, f"{name} paged {paged}")


def test_ragged_several_splits(oracle):
    """max_ctx 640 takes two 512-key splits at 40 rows: slot 0 appends 30 ids at 500, crossing
    key 512, beside a fresh 10-id prompt in slot 1."""
    spec = CONFIGS["tied-g7"]
    assert _lib.load().qie_attention_extend_workspace_bytes(40, spec.n_heads, spec.head_dim, 640) > 0
    eng = Q.Engine(spec, max_ctx=640).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(spec, SYN)
    b = eng.batch(2, 640)
    p0, p1 = _ids(5, 530, spec), _ids(6, 10, spec)
    b.prefill(0, p0[:500])
    toks = b.prefill_ragged([(0, p0[500:], 500), (1, p1)])
    assert [int(p) for p in b.positions()] == [530, 10]
    assert list(b.history(0, 531)) == p0 + [toks[0]] and list(b.history(1, 11)) == p1 + [toks[1]]
    om = {0: oracle.Model(hw, 640), 1: oracle.Model(hw, 640)}
    lg = {0: om[0].forward(p0, 0), 1: om[1].forward(p1, 0)}
    flips, n = _follow_all(oracle, b, om, lg, {0: toks[0], 1: toks[1]}, 3, "several splits")
    assert flips <= max_flips(n)


def _state(b):
    free, per, _ = b.page_stats()
    return [int(p) for p in b.positions()], int(free), [int(x) for x in per]


def test_ragged_state_equals_single_calls():
    """Two paged batches of one engine: the ragged call and the equivalent prefill / append
    sequence leave equal positions, history rows over the prompt ids, free pages, pages per slot
    and — one segment appends into a page it shares with a fork — holder counts.  (Which pool
    page a slot took depends on the order pages were returned and taken, so the counts are
    compared as a sorted list.)"""
    eng = Q.Engine(SPEC, max_ctx=512).init_synthetic(SYN)
    head, tail = _ids(11, 200), _ids(12, 70)       # the append rewinds to 100: rows 100 .. 169, pages 0 and 1
    pa, pc, old = _ids(13, 130), _ids(14, 9), _ids(15, 300)
    out = []
    for ragged in (True, False):
        b = eng.batch(4, 512, page_tokens=128, n_pages=14)
        b.prefill(1, head)
        b.fork(1, 2)                               # slot 2 shares page 0 (rows 0 .. 127) with slot 1
        b.prefill(0, old)                          # a live slot the fresh segment restarts (3 pages -> 2)
        shared = int((b.page_refs() > 1).sum())
        assert shared >= 1
        if ragged:
            b.prefill_ragged([(0, pa), (1, tail, 100), (3, pc)])
        else:
            b.prefill(0, pa)
            b.append(1, tail, 100)
            b.prefill(3, pc)
        hist = [list(b.history(s, n)) for s, n in ((0, 130), (1, 170), (3, 9))]
        assert hist == [pa, head[:100] + tail, pc]
        assert int((b.page_refs() > 1).sum()) == shared - 1   # the writer left the shared page to the fork
        out.append((_state(b), hist, sorted(int(r) for r in b.page_refs()), list(b.history(2, 200))))
        b.close()
    assert out[0] == out[1]
    assert out[0][0][0] == [130, 170, 200, 9] and out[0][0][2] == [2, 2, 2, 1]


def test_ragged_append_into_shared_page_leaves_the_fork_alone(oracle):
    """The append segment writes into a page a fork shares: the fork's rows stay what they were
    (it decodes like a twin that never saw the ragged call), and the writer follows the oracle."""
    eng = Q.Engine(SPEC, max_ctx=384).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(SPEC, SYN)
    head, tail, fresh = _ids(21, 150), _ids(22, 20), _ids(23, 7)
    runs = []
    for ragged in (True, False):
        b = eng.batch(3, 384, page_tokens=128)
        b.prefill(0, head)
        b.fork(0, 1, 140)                          # shares page 0, copies rows 128 .. 139
        if ragged:                                 # slot 0 rewinds into the shared page: a private copy first
            toks = b.prefill_ragged([(0, tail, 100), (2, fresh)])
            om = oracle.Model(hw, 384)
            lg = om.forward(head[:100] + tail, 0)
            assert _check_logits(oracle, b.logits()[0], lg, toks[0], "writer") <= 1
        runs.append([(b.decode_step()[1], b.logits()[1].copy()) for _ in range(3)])
        b.close()
    for (t1, l1), (t2, l2) in zip(*runs):
        assert t1 == t2 and np.array_equal(l1, l2)


def test_ragged_segment_isolated_bitwise():
    """Two ragged calls with the same segment A in the same rows and the same total row count,
    the other segment's ids different: A's logits row and its next 2 decode steps are equal bit
    for bit (rows meet nowhere: the GEMMs, the norms and the attention are per row)."""
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)
    a = _ids(31, 23)
    runs = []
    for seed in (32, 33):
        b = eng.batch(2, 128)
        toks = b.prefill_ragged([(0, a), (1, _ids(seed, 40))])
        got = [(toks[0], b.logits()[0].copy())]
        for _ in range(2):
            got.append((b.decode_step()[0], b.logits()[0].copy()))
        runs.append((got, toks[1]))
        b.close()
    for (t1, l1), (t2, l2) in zip(runs[0][0], runs[1][0]):
        assert t1 == t2 and np.array_equal(l1, l2)


def _raw(b, segs, ids, want_ids=True):
    """qie_prefill_ragged itself (Batch.prefill_ragged refuses some malformed calls on its own)."""
    arr = (_lib.PrefillSegC * max(len(segs), 1))(*[_lib.PrefillSegC(*s) for s in segs])
    flat = (C.c_int32 * max(len(ids), 1))(*ids)
    out = (C.c_int32 * 8)()
    sc = Q.GREEDY.to_c()
    return b.lib.qie_prefill_ragged(b.h, arr, len(segs), flat, C.byref(sc), out if want_ids else None)


def _snapshot(b, paged):
    return (_state(b), [int(r) for r in b.page_refs()]) if paged else [int(p) for p in b.positions()]


BAD = {
    "no_segments": ([], 0),
    "more_segments_than_slots": ([(0, 2, 0), (1, 2, 0), (2, 2, 0), (3, 2, 0)], 8),
    "slot_out_of_range": ([(0, 2, 0), (3, 2, 0)], 4),
    "negative_slot": ([(-1, 2, 0)], 2),
    "slots_repeated": ([(1, 2, 0), (1, 2, 0)], 4),
    "slots_decreasing": ([(2, 2, 0), (1, 2, 0)], 4),
    "empty_segment": ([(0, 2, 10), (2, 0, 0)], 2),
    "negative_pos0": ([(2, 2, -1)], 2),
    "reaches_max_ctx": ([(0, 54, 10)], 54),
    "fresh_reaches_max_ctx": ([(2, 64, 0)], 64),
    "id_out_of_range": ([(0, 2, 10), (2, 2, 0)], 4),
    "append_on_idle_slot": ([(0, 2, 10), (2, 2, 5)], 4),
    "append_on_released_slot": ([(1, 2, 3)], 2),
    "pos0_past_position": ([(0, 2, 11), (2, 2, 0)], 4),
}


@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("case", list(BAD))
def test_ragged_bad_arguments_change_nothing(case, paged):
    """-22 before anything is launched: positions and pages as before, and the live slot's next
    decode step equals, bit for bit, that of a twin batch that never made the call."""
    eng = Q.Engine(SPEC, max_ctx=64).init_synthetic(SYN)
    prompt = _ids(61, 10)

    def start():
        x = eng.batch(3, 64, page_tokens=128 if paged else None)
        x.prefill(0, prompt)
        x.prefill(1, prompt)
        x.release(1)
        return x

    twin = start()
    want = (twin.decode_step(), twin.logits())
    b = start()
    before = _snapshot(b, paged)
    segs, n_ids = BAD[case]
    ids = _ids(62, n_ids)
    if case == "id_out_of_range":
        ids[-1] = SPEC.vocab
    assert _raw(b, segs, ids) == -22, case
    assert _snapshot(b, paged) == before
    assert b.decode_step()[0] == want[0][0] and np.array_equal(b.logits()[0], want[1][0])


def test_ragged_refused_on_prefill_fp8_engine():
    spec = S.tiny("t-mx", n_layers=2, hidden=256, n_heads=4, n_kv_heads=2, head_dim=64, ffn=512, vocab=1024,
                  bias=True)
    eng = Q.Engine(spec, max_ctx=128, weight_fp8=True, prefill_fp8=True).init_synthetic(SYN)
    b = eng.batch(2, 128)
    b.prefill(0, _ids(51, 16, spec))
    with pytest.raises(_lib.QieError) as ex:
        b.prefill_ragged([(0, _ids(52, 8, spec), 16), (1, _ids(53, 5, spec))])
    assert "rc=-22" in _rc(ex) and "prefill_fp8" in _rc(ex)
    assert [int(p) for p in b.positions()] == [16, 0]


def test_ragged_pool_one_page_short_changes_nothing():
    """The segments need 1 + 1 + 1 fresh pages, the pool has 2 free: -28, nothing launched, the
    pool and the live slot as before; with one page more the same call succeeds."""
    eng = Q.Engine(SPEC, max_ctx=256).init_synthetic(SYN)
    prompt, tail = _ids(71, 120), _ids(72, 20)     # the append's rows 120 .. 139 need a second page
    call = [(0, tail, 120), (1, _ids(73, 30)), (2, _ids(74, 9))]

    def start(n_pages):
        x = eng.batch(3, 256, page_tokens=128, n_pages=n_pages)
        x.prefill(0, prompt)
        return x

    twin = start(4)
    want = (twin.decode_step(), twin.logits())
    b = start(4)                                   # scratch page + slot 0's page + 2 free
    before = _snapshot(b, True)
    with pytest.raises(_lib.QieError) as ex:
        b.prefill_ragged(call)
    assert "rc=-28" in _rc(ex)
    assert _snapshot(b, True) == before
    assert b.decode_step()[0] == want[0][0] and np.array_equal(b.logits()[0], want[1][0])
    ok = start(5)
    ok.prefill_ragged(call)
    assert _state(ok) == ([140, 30, 9], 0, [2, 1, 1])


def test_ragged_honours_slot_sampling():
    """A segment whose slot bans the token the plain call returns gets another token; the other
    segments' tokens are unchanged."""
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)
    call = [(0, _ids(81, 12)), (1, _ids(82, 30)), (2, _ids(83, 7))]
    b = eng.batch(3, 128)
    plain = b.prefill_ragged(call)
    b2 = eng.batch(3, 128)
    b2.set_sampling(1, Q.SlotSampling(bias={plain[1]: float("-inf")}))
    got = b2.prefill_ragged(call)
    assert got[1] != plain[1] and got[0] == plain[0] and got[2] == plain[2]
    lg = G.bf(b2.logits()[1]).astype(np.float64)
    lg[plain[1]] = -np.inf
    assert G.bf(b2.logits()[1])[got[1]] == lg.max()   # the best token that is left


@pytest.mark.parametrize("mode", ["weight_fp8", "comm_always"])
def test_ragged_fp8_weights_and_comm(oracle, mode):
    """The two other routes of the shared layer loop, as test_append_fp8_weights_and_comm."""
    hw = W.HostWeights.synthetic(SPEC, SYN)
    comm = None
    if mode == "weight_fp8":
        eng = Q.Engine(SPEC, max_ctx=160, weight_fp8=True).init_synthetic(SYN)
        hw = hw.fp8_dequantized()
    else:
        comm = Q.Comm.rccl(Q.Comm.unique_id(), 1, 0, 0)
        eng = Q.Engine(SPEC, max_ctx=160, comm=comm, comm_always=True).init_synthetic(SYN)
    try:
        _mixed(oracle, eng, hw, SPEC, 160, False, mode)
    finally:
        # nothing of the communicator may outlive the test (see test_gpu_append.py)
        eng.close()
        if comm is not None:
            comm.close()


def test_batcher_ragged_prefill_matches_oracle(oracle):
    """Five requests of prompt lengths 9, 70, 33, 33, 120 through 4 slots with 32-token chunks and
    ragged_prefill: admitted groups, whole prompts and advancing chunks go in ragged passes; every
    request's tokens and logits follow the oracle."""
    from qwen_inference_engine_amd.scheduler import ContinuousBatcher
    eng = Q.Engine(SPEC, max_ctx=256).init_synthetic(SYN)
    hw = W.HostWeights.synthetic(SPEC, SYN)
    cb = ContinuousBatcher(eng, slots=4, max_ctx=256, page_tokens=128, keep_logits=True, prefill_chunk=32,
                           ragged_prefill=True)
    calls = []
    real = cb.batch.prefill_ragged
    cb.batch.prefill_ragged = lambda segs, sampling=Q.GREEDY: (calls.append(len(segs)), real(segs, sampling))[1]
    prompts = [_ids(500 + i, n) for i, n in enumerate((9, 70, 33, 33, 120))]
    rids = [cb.submit(p, 5 + i) for i, p in enumerate(prompts)]
    cb.run()
    assert calls and calls[0] == 4 and max(calls) <= 4
    flips = n_tok = 0
    for rid, pr in zip(rids, prompts):
        r = cb.requests[rid]
        assert len(r.tokens) == len(r.logits) == 5 + rid
        om = oracle.Model(hw, 256)
        lg = om.forward(pr, 0)
        for t, (tok, got) in enumerate(zip(r.tokens, r.logits)):
            flips += _check_logits(oracle, got, lg, tok, f"request {rid} token {t}")
            if t + 1 < len(r.tokens):
                lg = om.forward([tok])
        n_tok += len(r.tokens)
    assert flips <= max_flips(n_tok)
