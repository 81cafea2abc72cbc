"""GPU: scoring — qie_logprob_rows, the fused qie_score_rows, qie_score / qie_batch_logprobs and
their Python tier (Batch.score, Batch.logprobs, ContinuousBatcher(keep_logprobs=True)).

Bars:
* log-probabilities on GIVEN logits against float64: 1e-4 absolute.  The kernels sum at most 256
  terms sequentially per partial and merge at most ceil(V / 256) partials, a relative sum error
  <= (255 + 594) * 2^-24 ~ 5e-5 even at V = 152,064, plus a few ulps of expf / logf.
* where the logits themselves come from a different fp32 summation order (a GEMM, the whole
  model), the logits' own bar D enters twice: log-sum-exp is 1-Lipschitz in the sup norm and the
  target logit adds one more D, so |dlogprob| <= 2 D + 1e-4.  D is the bar the existing tests
  give the same logits (G.assert_sum_close for a linear layer, test_gpu_engine.logit_tol for the
  model).
* greedy ids: the oracle's arg-max (reference tie rule), exactly on exact inputs, else a near-tie
  within D.
* state after qie_score against the plain prefill / append: bit for bit.
"""
import numpy as np
import pytest

import gpu_util as G
from conftest import rng
from parity import max_flips
from test_gpu_engine import CONFIGS, SYN, logit_tol, make_pair
from test_gpu_ops import _abs_scale, rand_bf16

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib
from qwen_inference_engine_amd.scheduler import ContinuousBatcher

pytestmark = pytest.mark.gpu

SPEC = CONFIGS["qwen2-bias-hd64"]
ABS = 1e-4


def _ids(seed, n, spec=SPEC):
    return [int(t) for t in rng(seed).integers(0, spec.vocab, n)]


def _logsoftmax64(l):
    """float64 log-softmax of float logit rows [..., V]."""
    l = np.asarray(l, np.float64)
    m = l.max(axis=-1, keepdims=True)
    return l - (m + np.log(np.exp(l - m).sum(axis=-1, keepdims=True)))


def _want_logprobs(l, targets):
    ls = _logsoftmax64(l)
    t = np.asarray(targets)
    return np.where(t >= 0, ls[np.arange(len(t)), np.maximum(t, 0)], 0.0)


# ------------------------------------------------------------------------------- operators
def _score_rows(qlib, x, w, targets, M, K, V, want_ids=True):
    """One qie_score_rows launch into fresh buffers (the workspace deliberately not zeroed:
    0xff bytes are NaNs and huge keys).  Returns (rc, logprobs, ids)."""
    lp = G.dev(np.full(max(M, 1), np.nan, np.float32))
    ids = G.dev(np.full(max(M, 1), -7, np.int32))
    nb = max(int(qlib.qie_score_rows_workspace_bytes(M, V)), 16)
    ws = G.dev(np.full(nb, 0xff, np.uint8))
    rc = qlib.qie_score_rows(G.p(x), K, G.p(w), M, K, V, G.p(targets), G.p(lp), G.p(ids) if want_ids else None,
                             G.p(ws), None)
    if rc == 0:
        G.check(qlib.qie_synchronize())
    return rc, G.host(lp), G.host(ids)


def _logprob_rows(qlib, logits, targets, M, V, ld):
    lp = G.dev(np.full(M, np.nan, np.float32))
    ids = G.dev(np.full(M, -7, np.int32))
    G.check(qlib.qie_logprob_rows(G.p(logits), M, V, ld, G.p(targets), G.p(lp), G.p(ids), None), "qie_logprob_rows")
    G.check(qlib.qie_synchronize())
    return G.host(lp), G.host(ids)


def _exact_case(M, K, V, seed):
    """x, W in {0, +-1/4} (one block of rows scaled 32x): every logit is a small multiple of 1/16
    (of 2 in the scaled rows), exact in bf16 and in every fp32 summation order.  Returns (x bits,
    W bits, exact logits float64 [M][V], targets)."""
    r = rng(seed)
    xi = r.integers(-1, 2, (M, K)).astype(np.int64)
    wi = r.integers(-1, 2, (V, K)).astype(np.int64)
    n = xi @ wi.T
    assert np.abs(n).max() <= 127, "the draw left the range in which every logit is a bf16"
    big = slice(M // 3, M // 3 + max(1, M // 8))
    xs = xi.astype(np.float32) * 0.25
    xs[big] *= 32.0
    l = n.astype(np.float64) / 16.0
    l[big] *= 32.0
    t = r.integers(0, V, M).astype(np.int32)
    fixed = [V - 1, 0, V - 3, -1]   # the last valid column, column 0, one of the ragged tile, none
    for i, v in enumerate(fixed[:M]):
        t[i * 7 if M > 4 else i] = v
    return G.to_bf16(xs), G.to_bf16(wi.astype(np.float32) * 0.25), l, t


EXACT_SHAPES = [(257, 256, 1000), (3, 448, 1554), (1, 256, 256)]


@pytest.mark.parametrize("M,K,V", EXACT_SHAPES)
def test_score_rows_exact_inputs(oracle, qlib, M, K, V):
    """Two row tiles with the minimum 4 k-tiles and a ragged last column tile; 7 k-tiles; one
    exact tile.  ids bit for bit, logprobs within 1e-4 of float64, -1 rows exactly 0, and two
    launches into fresh buffers bit-equal."""
    x, w, l, t = _exact_case(M, K, V, seed=M + V)
    lbits = G.to_bf16(l.astype(np.float32))
    assert np.array_equal(G.bf(lbits).astype(np.float64), l)
    want_ids = np.array([oracle.argmax(lbits[m]) for m in range(M)], np.int32)
    ties = sum(int((l[m] == l[m].max()).sum() > 1) for m in range(M))
    want = _want_logprobs(l, t)
    dx, dw, dt = G.dev(x), G.dev(w), G.dev(t)
    rc, lp, ids = _score_rows(qlib, dx, dw, dt, M, K, V)
    assert rc == 0, qlib.qie_last_error()
    err = np.abs(lp.astype(np.float64) - want)
    print(f"score_rows exact M={M} K={K} V={V}: max |dlogprob| {err.max():.3e}, rows with a tied maximum {ties}")
    assert np.array_equal(ids, want_ids)
    assert err.max() <= ABS
    assert (lp[t < 0] == 0.0).all() and (t < 0).any() == (M >= 4)
    rc2, lp2, ids2 = _score_rows(qlib, dx, dw, dt, M, K, V)
    assert rc2 == 0 and np.array_equal(lp.view(np.uint32), lp2.view(np.uint32)) and np.array_equal(ids, ids2)
    # ids_dev may be NULL
    rc3, lp3, _ = _score_rows(qlib, dx, dw, dt, M, K, V, want_ids=False)
    assert rc3 == 0 and np.array_equal(lp.view(np.uint32), lp3.view(np.uint32))


@pytest.mark.parametrize("M,K,V", EXACT_SHAPES)
@pytest.mark.parametrize("pad", [0, 3])
def test_logprob_rows_exact_inputs(oracle, qlib, M, K, V, pad):
    """The same logits, materialised by numpy (pad 3: an odd row stride, the unvectorised loads)."""
    _, _, l, t = _exact_case(M, K, V, seed=M + V)
    ld = V + pad
    rows = np.zeros((M, ld), np.uint16)
    rows[:, :V] = G.to_bf16(l.astype(np.float32))
    rows[:, V:] = 0x7F80   # +inf past V: read by nothing
    want_ids = np.array([oracle.argmax(rows[m, :V]) for m in range(M)], np.int32)
    dl, dt = G.dev(rows), G.dev(t)
    lp, ids = _logprob_rows(qlib, dl, dt, M, V, ld)
    err = np.abs(lp.astype(np.float64) - _want_logprobs(l, t))
    print(f"logprob_rows exact M={M} V={V} ld={ld}: max |dlogprob| {err.max():.3e}")
    assert np.array_equal(ids, want_ids)
    assert err.max() <= ABS
    assert (lp[t < 0] == 0.0).all()
    lp2, ids2 = _logprob_rows(qlib, dl, dt, M, V, ld)
    assert np.array_equal(lp.view(np.uint32), lp2.view(np.uint32)) and np.array_equal(ids, ids2)


def test_logprob_rows_full_vocabulary(oracle, qlib):
    M, V = 3, 152064
    rows = rand_bf16(oracle, (M, V), 3.0, seed=77)
    t = np.array([0, V - 1, -1], np.int32)
    lp, ids = _logprob_rows(qlib, G.dev(rows), G.dev(t), M, V, V)
    err = np.abs(lp.astype(np.float64) - _want_logprobs(G.bf(rows), t))
    print(f"logprob_rows V={V}: max |dlogprob| {err.max():.3e}")
    assert err.max() <= ABS and lp[2] == 0.0
    assert list(ids) == [oracle.argmax(rows[m]) for m in range(M)]


def test_score_rows_random_inputs(oracle, qlib):
    """Against oracle.matmul -> float64 log-softmax: the GEMM's summation order differs, so each
    logit may move by what G.assert_sum_close grants a linear layer on these inputs (D_row: the
    row's largest such tolerance); 2 D_row + 1e-4 on the log-probability, a near-tie within D_row
    on the id."""
    M, K, V = 300, 896, 5000
    x = rand_bf16(oracle, (M, K), seed=M)
    w = rand_bf16(oracle, (V, K), 0.05, seed=10)
    want = oracle.matmul(x, w)
    wl = G.bf(want).astype(np.float64)
    D = np.maximum(np.abs(wl) * 2.0 ** -7, 1e-5 * _abs_scale(oracle, x, w)).max(axis=1)
    t = rng(5).integers(0, V, M).astype(np.int32)
    t[::17] = -1
    rc, lp, ids = _score_rows(qlib, G.dev(x), G.dev(w), G.dev(t), M, K, V)
    assert rc == 0, qlib.qie_last_error()
    err = np.abs(lp.astype(np.float64) - _want_logprobs(wl, t))
    print(f"score_rows random: max |dlogprob| {err.max():.3e}, smallest bar {(2 * D + ABS).min():.3e}, "
          f"worst err / bar {(err / (2 * D + ABS)).max():.3f}")
    assert (err <= 2 * D + ABS).all()
    flips = 0
    for m in range(M):
        a = oracle.argmax(want[m])
        if ids[m] != a:
            assert 0 <= ids[m] < V and abs(wl[m, a] - wl[m, ids[m]]) <= D[m], f"row {m}: {ids[m]} vs {a}"
            flips += 1
    print(f"score_rows random: {flips} near-tie ids of {M}")


@pytest.mark.parametrize("M,K,V", [(4, 96, 512), (4, 320 - 32, 512), (0, 256, 512), (4, 256, 0)])
def test_score_rows_argument_checks(qlib, M, K, V):
    x, w = G.zeros_bf16(8, 512), G.zeros_bf16(512, 512)
    rc, _, _ = _score_rows(qlib, x, w, G.dev(np.zeros(8, np.int32)), M, K, V)
    assert rc == -22


# ---------------------------------------------------------------------------------- engine
def _oracle_rows(om, prompt, pos0=0):
    """Teacher-forced oracle logits of every row of `prompt` laid at pos0 ..: [n][V] bf16 bits."""
    rows = [om.forward(prompt[:1], pos0)]
    for t in prompt[1:]:
        rows.append(om.forward([t]))
    return rows


def _check_against_rows(oracle, lp, gr, rows, prompt, what):
    """Every log-probability within 2 logit_tol + 1e-4 of the float64 log-softmax of the oracle's
    row, every greedy id its arg-max or a near-tie within logit_tol.  Returns the flips."""
    n, flips, worst = len(prompt), 0, 0.0
    assert len(lp) == n - 1 and len(gr) == n
    for i, lg in enumerate(rows):
        l64 = G.bf(lg).astype(np.float64)
        tol = logit_tol(lg)
        if i + 1 < n:
            want = _logsoftmax64(l64)[prompt[i + 1]]
            worst = max(worst, abs(float(lp[i]) - want) / (2 * tol + ABS))
            assert abs(float(lp[i]) - want) <= 2 * tol + ABS, \
                f"{what} row {i}: logprob {lp[i]} vs {want} (bar {2 * tol + ABS})"
        a = oracle.argmax(lg)
        if int(gr[i]) != a:
            assert 0 <= gr[i] < len(lg) and abs(l64[a] - l64[int(gr[i])]) <= tol, f"{what} row {i}: id {gr[i]} vs {a}"
            flips += 1
    print(f"{what}: worst |dlogprob| / bar {worst:.3f}, {flips} near-tie ids")
    return flips


@pytest.mark.parametrize("num", ["ref", "hf"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_score_matches_oracle(oracle, name, num):
    spec = CONFIGS[name].with_numerics(num)
    eng, hw, om = make_pair(spec, oracle)
    prompt = _ids(45, 45, spec)
    b = eng.batch(1, 128)
    lp, gr, nxt = b.score(0, prompt)
    rows = _oracle_rows(om, prompt)
    flips = _check_against_rows(oracle, lp, gr, rows, prompt, f"{name}/{num}")
    assert flips <= max_flips(len(prompt))
    assert nxt == int(gr[-1])   # greedy: the sampled token is the last row's arg-max
    assert lp.dtype == np.float32 and gr.dtype == np.int32


def _state(b, n, seq=0):
    L = b.e.spec.n_layers
    return (b.logits().copy(), b.positions().copy(), b.history(seq, n + 1).copy(),
            [b.kv_rows(seq, l, n) for l in range(L)])


def _assert_same_state(a, c, what):
    assert np.array_equal(a[0], c[0]), f"{what}: logits"
    assert np.array_equal(a[1], c[1]), f"{what}: positions"
    assert np.array_equal(a[2], c[2]), f"{what}: history"
    for l, (ka, kc) in enumerate(zip(a[3], c[3])):
        assert np.array_equal(ka[0], kc[0]) and np.array_equal(ka[1], kc[1]), f"{what}: K/V rows of layer {l}"


@pytest.mark.parametrize("unfused", [False, True])
def test_score_leaves_the_state_of_a_prefill(unfused):
    eng = Q.Engine(SPEC, max_ctx=128).init_synthetic(SYN)
    prompt = _ids(7, 45)
    b1, b2 = eng.batch(1, 128), eng.batch(1, 128)
    _, _, t1 = b1.score(0, prompt, unfused=unfused)
    t2 = b2.prefill(0, prompt)
    assert t1 == t2
    _assert_same_state(_state(b1, len(prompt)), _state(b2, len(prompt)), "score vs prefill")
    d1, d2 = b1.decode(4), b2.decode(4)
    assert np.array_equal(d1, d2) and np.array_equal(b1.logits(), b2.logits())


@pytest.mark.parametrize("paged", [False, True])
def test_score_at_a_position_leaves_the_state_of_an_append(paged):
    """P0 = 100 cached rows, then 45 scored ones: the paged batch takes its second page."""
    eng = Q.Engine(SPEC, max_ctx=256).init_synthetic(SYN)
    P0, head, tail = 100, _ids(8, 100), _ids(9, 45)
    pt = 128 if paged else None
    b1, b2 = eng.batch(1, 256, page_tokens=pt), eng.batch(1, 256, page_tokens=pt)
    for b in (b1, b2):
        b.prefill(0, head)
    lp, gr, t1 = b1.score(0, tail, pos0=P0)
    t2 = b2.append(0, tail, P0)
    assert t1 == t2 and len(lp) == len(tail) - 1 and len(gr) == len(tail)
    n = P0 + len(tail)
    _assert_same_state(_state(b1, n), _state(b2, n), "score(pos0) vs append")
    if paged:
        assert b1.page_stats()[0] == b2.page_stats()[0] and list(b1.page_stats()[1]) == [2]
    d1, d2 = b1.decode(4), b2.decode(4)
    assert np.array_equal(d1, d2) and np.array_equal(b1.logits(), b2.logits())


@pytest.fixture(scope="module")
def base(oracle):
    """One engine, its oracle rows for one prompt, and the fused score of it (shared, read-only)."""
    eng, hw, om = make_pair(SPEC, oracle)
    prompt = _ids(45, 45)
    rows = _oracle_rows(om, prompt)
    b = eng.batch(1, 128)
    lp, gr, nxt = b.score(0, prompt)
    return dict(eng=eng, hw=hw, prompt=prompt, rows=rows, lp=lp, gr=gr, nxt=nxt)


def _bars(rows):
    return np.array([2 * logit_tol(lg) + ABS for lg in rows[:-1]])


def test_unfused_path_agrees_and_its_last_row_is_the_batch_logits(oracle, base):
    eng, prompt = base["eng"], base["prompt"]
    b = eng.batch(1, 128)
    lp_u, gr_u, nxt_u = b.score(0, prompt, unfused=True)
    d = np.abs(lp_u.astype(np.float64) - base["lp"].astype(np.float64))
    print(f"unfused vs fused: worst |dlogprob| / bar {(d / _bars(base['rows'])).max():.3f}")
    assert (d <= _bars(base["rows"])).all() and nxt_u == base["nxt"]
    _check_against_rows(oracle, lp_u, gr_u, base["rows"], prompt, "unfused")
    # row n - 1, targeted at the token the prefill itself picks: exactly Batch.logprobs of it
    lp_r, gr_r, nxt_r = b.score_rows(0, prompt, prompt[1:] + [nxt_u], unfused=True)
    assert nxt_r == nxt_u and int(gr_r[-1]) == nxt_u
    assert np.array_equal(lp_r[:-1].view(np.uint32), lp_u.view(np.uint32))
    assert lp_r[-1] == b.logprobs([nxt_u])[0] and lp_r[-1] < 0.0
    # and that value is the float64 log-softmax of the row qie_batch_logits returns
    want = _logsoftmax64(G.bf(b.logits()[0]))[nxt_u]
    assert abs(float(lp_r[-1]) - want) <= ABS
    assert b.logprobs([-1])[0] == 0.0


def test_score_fp8_weights(oracle, base):
    """The general path taken by itself: an fp8 head has no fused form.  The oracle runs the
    dequantised model, as the fp8 engine tests do."""
    eng = Q.Engine(SPEC, max_ctx=128, weight_fp8=True).init_synthetic(SYN)
    om = oracle.Model(base["hw"].fp8_dequantized(), 128)
    prompt = base["prompt"]
    lp, gr, _ = eng.batch(1, 128).score(0, prompt)
    flips = _check_against_rows(oracle, lp, gr, _oracle_rows(om, prompt), prompt, "weight_fp8")
    assert flips <= max_flips(len(prompt))


def test_score_on_the_exchange_path_equals_unfused(base):
    """comm_always at world 1: the head's rows go through the gather; bit for bit the plain
    engine's unfused result."""
    prompt = base["prompt"]
    lp_u, gr_u, nxt_u = base["eng"].batch(1, 128).score(0, prompt, unfused=True)
    comm = Q.Comm.rccl(Q.Comm.unique_id(), 1, 0, 0)
    eng = Q.Engine(SPEC, max_ctx=128, comm=comm, comm_always=True).init_synthetic(SYN)
    b = eng.batch(1, 128)
    lp, gr, nxt = b.score(0, prompt)
    assert nxt == nxt_u and np.array_equal(gr, gr_u) and np.array_equal(lp.view(np.uint32), lp_u.view(np.uint32))
    assert b.logprobs([nxt])[0] == base["eng"].batch(1, 128).score_rows(
        0, prompt, prompt[1:] + [nxt], unfused=True)[0][-1]
    b.close()
    eng.close()
    comm.close()


def test_score_in_chunks(base):
    eng, prompt = base["eng"], base["prompt"]
    b = eng.batch(1, 128)
    lp, gr, nxt = b.score(0, prompt, chunk=16)
    assert len(lp) == 44 and len(gr) == 45
    d = np.abs(lp.astype(np.float64) - base["lp"].astype(np.float64))
    print(f"chunked vs whole: worst |dlogprob| / bar {(d / _bars(base['rows'])).max():.3f}")
    assert (d <= _bars(base["rows"])).all()
    assert int(b.positions()[0]) == 45 and list(b.history(0, 45)) == prompt
    ppl = b.perplexity(0, prompt)
    assert ppl == float(np.exp(-base["lp"].astype(np.float64).mean()))


def test_batcher_keeps_logprobs(base):
    """Admission tokens (whole prompts), a chunk-completion token (the 20-id prompt in chunks of
    8) and decode-step tokens, each against the float64 log-softmax of its kept logit row."""
    cb = ContinuousBatcher(base["eng"], slots=2, max_ctx=128, page_tokens=128, keep_logprobs=True, keep_logits=True,
                           prefill_chunk=8)
    prompts = [_ids(300, 5), _ids(301, 20), _ids(302, 7)]
    rids = [cb.submit(p, 4 + i) for i, p in enumerate(prompts)]
    cb.run()
    worst = 0.0
    for rid in rids:
        r = cb.requests[rid]
        assert len(r.logprobs) == len(r.tokens) == len(r.logits) > 0
        for tok, lp, lg in zip(r.tokens, r.logprobs, r.logits):
            want = _logsoftmax64(G.bf(lg))[tok]
            worst = max(worst, abs(lp - want))
            assert abs(lp - want) <= ABS and lp <= 0.0
    print(f"batcher logprobs: worst |d| {worst:.3e}")
    cb.close()


def test_score_errors_leave_the_sequence_alone(base):
    eng, prompt = base["eng"], base["prompt"]
    V = SPEC.vocab
    b = eng.batch(2, 128)
    t0 = b.prefill(0, prompt[:20])
    before = _state(b, 20)
    with pytest.raises(_lib.QieError, match=r"rc=-22"):   # a target equal to V
        b.score_rows(0, prompt[:10], prompt[1:10] + [V])
    with pytest.raises(_lib.QieError, match=r"rc=-22"):   # ... in an append
        b.score_rows(0, prompt[:10], [V] * 10, pos0=5)
    with pytest.raises(_lib.QieError, match=r"rc=-22"):   # an idle slot
        b.score(1, prompt[:10], pos0=3)
    with pytest.raises(_lib.QieError, match=r"rc=-22"):   # pos0 past the position
        b.score(0, prompt[:10], pos0=21)
    _assert_same_state(_state(b, 20), before, "after refused calls")
    b2 = eng.batch(2, 128)
    assert b2.prefill(0, prompt[:20]) == t0
    assert b.decode_step()[0] == b2.decode_step()[0] and np.array_equal(b.logits()[0], b2.logits()[0])
    # pool exhausted: one page beside the scratch page, the append needs a second one
    pb = Q.Engine(SPEC, max_ctx=256).init_synthetic(SYN).batch(1, 256, page_tokens=128, n_pages=2)
    head = _ids(3, 100)
    pb.prefill(0, head)
    with pytest.raises(_lib.QieError, match=r"rc=-28") as e_score:
        pb.score(0, _ids(4, 60), pos0=100)
    with pytest.raises(_lib.QieError, match=r"rc=-28") as e_app:
        pb.append(0, _ids(4, 60), 100)
    assert int(pb.positions()[0]) == 100 and pb.page_stats()[0] == 0
    assert str(e_score.value).replace("qie_score", "X") == str(e_app.value).replace("qie_prefill_append", "X")
