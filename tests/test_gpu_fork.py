"""GPU: sequences that share KV pages — qie_kv_copy, qie_batch_fork, copy-on-write
in the writers, prefix handles and the batcher's prefix cache.

A fork changes where rows live and who holds them, never the arithmetic: every check that
compares a fork with its source, or with a batch that never forked, is BIT-EXACT (the same
kernels on the same rows).  Only a branch that diverges from its source is new computation; it is
held to the oracle under test_gpu_append.py's bar (logit_tol, the near-tie rule, max_flips)."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as G
from conftest import rng
from parity import max_flips
from test_gpu_engine import CONFIGS, SYN, logit_tol

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib, weights as W
from qwen_inference_engine_amd._lib import KvCacheC, SamplingC

pytestmark = pytest.mark.gpu

SPEC = CONFIGS["qwen2-bias-hd64"]
T = 128
_ENGINES = {}


def engine(name="qwen2-bias-hd64", max_ctx=512):
    if (name, max_ctx) not in _ENGINES:
        _ENGINES[name, max_ctx] = Q.Engine(CONFIGS[name], max_ctx=max_ctx).init_synthetic(SYN)
    return _ENGINES[name, max_ctx]


def _ids(seed, n, spec=SPEC):
    return [int(t) for t in rng(seed).integers(0, spec.vocab, n)]


def _rows(b, seq, n):
    L = b.e.spec.n_layers
    return [b.kv_rows(seq, l, n) for l in range(L)]


def _rows_equal(a, b):
    return all(np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) for x, y in zip(a, b))


def _state(b):
    """Everything a failed call must leave alone (paged: tables, counts and the free list too)."""
    st = {"pos": b.positions().tolist()}
    if b.paged:
        free, per, _ = b.page_stats()
        st.update(free=free, per=per.tolist(), refs=b.page_refs().tolist(),
                  tables=[b.block_table(s, b.max_ctx // T).tolist() for s in range(b.B)])
    return st


# ------------------------------------------------------------------ 1. qie_kv_copy
def _rand(shape, seed):
    return rng(seed).integers(0, 1 << 16, size=shape, dtype=np.uint16)


COPIES = [(0, 1), (0, 127), (0, 128), (0, 129), (128, 1), (130, 170), (299, 1)]


@pytest.mark.parametrize("hd,nkv", [(64, 1), (64, 2), (128, 2)])
def test_kv_copy_paged_equals_numpy(qlib, hd, nkv):
    """Two sequences of one garbage-filled pool with shuffled tables: the destination's rows equal
    the source's, every other byte of the pool (scratch page 0 included) is unchanged."""
    L, maxc = 2, 300
    mp = (maxc + T - 1) // T
    n_pages = 2 * mp + 1
    table = rng(hd + nkv).permutation(np.arange(1, n_pages)).astype(np.int32).reshape(2, mp)
    dt = G.dev(table)
    for i, (pos0, n) in enumerate(COPIES):
        kp, vp = _rand((n_pages, L, nkv, T, hd), 10 + i), _rand((n_pages, L, nkv, T, hd), 50 + i)
        dk, dv = G.dev(kp), G.dev(vp)
        c = KvCacheC()
        c.k, c.v, c.seq_stride = G.p(dk), G.p(dv), L * nkv * T * hd
        c.n_layers, c.n_kv_heads, c.head_dim, c.max_ctx = L, nkv, hd, maxc
        c.block_table, c.page_tokens, c.max_pages = G.p(dt), T, mp
        G.check(qlib.qie_kv_copy(C.byref(c), 0, C.byref(c), 1, pos0, n, None))
        G.check(qlib.qie_synchronize())
        for pool, dev in ((kp, dk), (vp, dv)):
            want = pool.copy()
            for t in range(pos0, pos0 + n):
                want[table[1, t // T], :, :, t % T] = pool[table[0, t // T], :, :, t % T]
            assert np.array_equal(G.host_bf16(dev).reshape(pool.shape), want), (pos0, n)


@pytest.mark.parametrize("hd,nkv", [(64, 1), (64, 2), (128, 2)])
def test_kv_copy_contiguous_equals_numpy(qlib, hd, nkv):
    """Two sequences of one allocation [2][L][nkv][300][hd], in both directions."""
    L, maxc = 2, 300
    for i, (pos0, n) in enumerate(COPIES):
        kc, vc = _rand((2, L, nkv, maxc, hd), 100 + i), _rand((2, L, nkv, maxc, hd), 150 + i)
        dk, dv = G.dev(kc), G.dev(vc)
        c = KvCacheC()
        c.k, c.v, c.seq_stride = G.p(dk), G.p(dv), L * nkv * maxc * hd
        c.n_layers, c.n_kv_heads, c.head_dim, c.max_ctx = L, nkv, hd, maxc
        src, dst = i % 2, 1 - i % 2
        G.check(qlib.qie_kv_copy(C.byref(c), src, C.byref(c), dst, pos0, n, None))
        G.check(qlib.qie_synchronize())
        for h, dev in ((kc, dk), (vc, dv)):
            want = h.copy()
            want[dst, :, :, pos0:pos0 + n] = h[src, :, :, pos0:pos0 + n]
            assert np.array_equal(G.host_bf16(dev).reshape(h.shape), want), (pos0, n)


def test_kv_copy_refuses_bad_calls(qlib):
    L, nkv, hd, maxc = 2, 2, 64, 300
    mp = 3
    buf = G.zeros_bf16(7 * L * nkv * T * hd)
    dt = G.dev(np.arange(1, 7, dtype=np.int32).reshape(2, mp))

    def cache(paged, hd_=hd, L_=L):
        c = KvCacheC()
        c.k = c.v = G.p(buf)
        c.n_layers, c.n_kv_heads, c.head_dim, c.max_ctx = L_, nkv, hd_, maxc
        if paged:
            c.seq_stride, c.block_table, c.page_tokens, c.max_pages = L * nkv * T * hd, G.p(dt), T, mp
        else:
            c.seq_stride = L * nkv * maxc * hd
        return c

    pg, ct = cache(True), cache(False)
    call = lambda a, sa, b_, sb, p0, n: qlib.qie_kv_copy(C.byref(a), sa, C.byref(b_), sb, p0, n, None)
    assert call(pg, 0, ct, 1, 0, 1) == -22 and call(ct, 0, pg, 1, 0, 1) == -22     # a mixed pair
    assert call(pg, 1, pg, 1, 0, 1) == -22 and call(ct, 0, ct, 0, 0, 1) == -22     # the same sequence
    assert call(pg, 0, pg, 1, 300, 1) == -22 and call(ct, 0, ct, 1, 200, 101) == -22   # past max_ctx
    assert call(ct, 0, ct, 1, -1, 1) == -22 and call(ct, 0, ct, 1, 0, -1) == -22
    assert call(ct, 0, cache(False, hd_=128), 1, 0, 1) == -22                       # geometry
    assert call(pg, 0, cache(True, L_=1), 1, 0, 1) == -22
    assert call(pg, 0, pg, 1, 5, 0) == 0                                           # nothing to copy
    G.check(qlib.qie_synchronize())
    assert not G.host_bf16(buf).any()


# ------------------------------------------------------------------ 2. a fork continues as its source
@pytest.mark.parametrize("paged", [True, False], ids=["paged", "contig"])
@pytest.mark.parametrize("pos", [127, 128, 129, 300])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_fork_continues_as_its_source(name, pos, paged):
    """Prefill slot 0, 3 decode steps, fork 0 -> 2 at the current position, 6 more steps: every
    id, every logit row and every K/V row of slot 2 equals slot 0's.  Control: the same prompt in
    two slots by prefill_batch (no fork) gives equal rows — what unshared slots produce."""
    spec = CONFIGS[name]
    eng = engine(name)
    kw = dict(page_tokens=T) if paged else {}
    prompt = _ids(pos, pos - 3, spec)
    ctl = eng.batch(3, 512, **kw)
    ctl.prefill_batch(0, [prompt, prompt])
    for _ in range(9):
        ids = ctl.decode_step()
        lg = ctl.logits()
        assert ids[0] == ids[1] and np.array_equal(lg[0], lg[1]), "control: two unshared slots differ"
    assert _rows_equal(_rows(ctl, 0, pos + 6), _rows(ctl, 1, pos + 6))
    ctl.close()
    b = eng.batch(3, 512, **kw)
    b.prefill(0, prompt)
    b.decode(3)
    assert int(b.positions()[0]) == pos
    b.fork(0, 2)
    assert b.positions().tolist()[2] == pos
    assert np.array_equal(b.history(2, pos + 1), b.history(0, pos + 1))
    lg = b.logits()
    assert np.array_equal(lg[2], lg[0])
    for _ in range(6):
        ids = b.decode_step()
        lg = b.logits()
        assert ids[2] == ids[0] and np.array_equal(lg[2], lg[0])
    assert _rows_equal(_rows(b, 2, pos + 6), _rows(b, 0, pos + 6))
    b.close()


# ------------------------------------------------------------------ 3. page accounting
def _forked(n_pages=0, pos=300, B=3, steps=3):
    eng = engine()
    prompt = _ids(31, pos - steps)
    b = eng.batch(B, 512, page_tokens=T, n_pages=n_pages)
    b.prefill(0, prompt)
    b.decode(steps)
    return eng, prompt, b


def test_fork_page_accounting():
    eng, prompt, b = _forked()
    ctl = eng.batch(3, 512, page_tokens=T)          # never forks
    ctl.prefill(0, prompt)
    ctl.decode(3)
    want = ctl.decode(100)[:, 0].tolist()
    free0 = b.page_stats()[0]
    b.fork(0, 2)
    t0, t2 = b.block_table(0, 3), b.block_table(2, 3)
    assert t0[0] == t2[0] and t0[1] == t2[1] and t0[2] != t2[2] and t2[2] != 0
    free, per, _ = b.page_stats()
    assert free == free0 - 1 and per.tolist() == [3, 0, 3]
    refs = b.page_refs()
    assert refs[t0[0]] == 2 and refs[t0[1]] == 2 and refs[t0[2]] == 1 and refs[t2[2]] == 1 and refs[0] == 0
    assert int(refs.sum()) == 6
    b.release(0)                                    # its private page returns, the shared ones stay
    assert b.page_stats()[0] == free + 1
    refs = b.page_refs()
    assert refs[t0[0]] == 1 and refs[t0[1]] == 1 and refs[t0[2]] == 0
    assert b.decode(100)[:, 2].tolist() == want     # crosses into a fourth page at 384
    b.release(2)
    assert b.page_stats()[0] == b.n_pages - 1 and not b.page_refs().any()


# ------------------------------------------------------------------ 4. copy-on-write
@pytest.mark.parametrize("who", ["fork", "source"])
@pytest.mark.parametrize("how", ["set_position", "append"])
def test_rewind_into_a_shared_page_copies_it(who, how):
    """After a fork at 300 one holder rewinds into shared page 1 (set_position to 200 and a
    decode step, or an append at 130): it gets a private page holding the rows below its write,
    the other holder's rows [0, 300) and page are untouched, the old page's count is back to 1."""
    eng, prompt, b = _forked()
    b.fork(0, 2)
    me, other = (2, 0) if who == "fork" else (0, 2)
    snap_other, snap_me = _rows(b, other, 300), _rows(b, me, 300)
    old = b.block_table(me, 3)
    free = b.page_stats()[0]
    lo = 200 if how == "set_position" else 130
    if how == "set_position":
        b.set_position(me, 200, 5)
        b.decode_step()
    else:
        b.append(me, _ids(41, 20), pos0=130)
    new = b.block_table(me, 3)
    assert new[0] == old[0] and new[1] != old[1] and new[1] != 0 and new[2] == old[2]
    assert b.block_table(other, 3).tolist()[:2] == old.tolist()[:2]
    refs = b.page_refs()
    assert refs[old[1]] == 1 and refs[new[1]] == 1 and refs[old[0]] == 2
    assert b.page_stats()[0] == free - 1
    assert _rows_equal(_rows(b, other, 300), snap_other)
    assert _rows_equal(_rows(b, me, lo), [[k[:, :lo], v[:, :lo]] for k, v in snap_me])
    mine = _rows(b, me, lo + 1)
    assert not all(np.array_equal(m[0][:, lo], s[0][:, lo]) for m, s in zip(mine, snap_me)), "nothing was written"
    b.close()


@pytest.mark.parametrize("how", ["set_position", "append"])
def test_rewind_without_a_page_fails_and_changes_nothing(how):
    """A pool with no page left: the rewinding call returns -28; tables, counts, positions and
    the next decode step are those of a batch on which it was never made."""
    out = []
    for attempt in (False, True):
        eng, prompt, b = _forked(n_pages=5)         # scratch + 4: three for the source, one for the tail
        b.fork(0, 2)
        assert b.page_stats()[0] == 0
        if attempt:
            before = _state(b)
            with pytest.raises(_lib.QieError, match=r"rc=-28"):
                if how == "set_position":
                    b.set_position(2, 200, 5)
                else:
                    b.append(2, _ids(41, 20), pos0=130)
            assert _state(b) == before
            b.set_position(2, 299, 5)               # the tail page is the fork's own: no page needed
            b.set_position(2, 300, int(b.history(0, 301)[300]))
        ids = b.decode_step()
        out.append((ids[0], ids[2], b.logits()[[0, 2]].copy()))
        b.close()
    assert out[0][:2] == out[1][:2] and np.array_equal(out[0][2], out[1][2])


def test_both_holders_rewind_into_one_shared_page():
    """Fork at 256 with a prefix handle as third holder of the two pages, then source AND fork
    rewind to 130 and one decode step writes row 130 of both: each ends with a page of its own at
    index 1 whose rows [128, 130) are the pre-fork rows bit for bit, and the handle's page — the
    old one — is untouched (a slot loaded from it reads the pre-fork rows [0, 256))."""
    eng, prompt, b = _forked()
    pf = b.save_prefix(0, 256)
    b.fork(0, 2, 256)
    snap = _rows(b, 0, 256)
    old = b.block_table(0, 2).tolist()
    assert b.block_table(2, 2).tolist() == old and b.page_refs()[old].tolist() == [3, 3]
    free = b.page_stats()[0]
    b.set_position(0, 130, 5)
    b.set_position(2, 130, 6)
    b.decode_step()
    t0, t2 = b.block_table(0, 2).tolist(), b.block_table(2, 2).tolist()
    assert t0[0] == t2[0] == old[0] and len({t0[1], t2[1], old[1], 0}) == 4
    refs = b.page_refs()
    assert refs[[old[0], old[1], t0[1], t2[1]]].tolist() == [3, 1, 1, 1] and b.page_stats()[0] == free - 2
    for s in (0, 2):
        assert _rows_equal(_rows(b, s, 130), [[k[:, :130], v[:, :130]] for k, v in snap]), s
    r0, r2 = _rows(b, 0, 131), _rows(b, 2, 131)
    assert not all(np.array_equal(x[0][:, 130], y[0][:, 130]) for x, y in zip(r0, r2)), "row 130: different tokens"
    b.load_prefix(pf, 1, 7, 256)
    assert b.block_table(1, 2).tolist() == old
    assert _rows_equal(_rows(b, 1, 256), snap)
    pf.drop()
    b.close()


# ------------------------------------------------------------------ 5. a fork that diverges
@pytest.mark.parametrize("paged", [True, False], ids=["paged", "contig"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_diverging_fork_follows_the_oracle(oracle, name, paged):
    spec = CONFIGS[name]
    eng = engine(name)
    om = oracle.Model(W.HostWeights.synthetic(spec, SYN), 512)
    kw = dict(page_tokens=T) if paged else {}
    prompt, branch = _ids(51, 200, spec), _ids(52, 30, spec)
    ctl = eng.batch(3, 512, **kw)
    ctl.prefill(0, prompt)
    want = [(ctl.decode_step()[0], ctl.logits()[0].copy()) for _ in range(10)]
    ctl.close()
    b = eng.batch(3, 512, **kw)
    b.prefill(0, prompt)
    b.decode(2)
    b.fork(0, 1, 150)
    assert int(b.positions()[1]) == 150 and int(b.history(1, 151)[150]) == prompt[150]
    tok = b.append(1, branch, pos0=150)
    # the branch: prefix + branch against the oracle, under test_gpu_append.py's bar
    from test_gpu_append import _check_logits
    lg = om.forward(prompt[:150] + branch, 0)
    flips = _check_logits(oracle, b.logits()[1], lg, tok, f"{name} branch first")
    got = []
    for t in range(8):
        lg = om.forward([tok])
        ids = b.decode_step()
        got.append((ids[0], b.logits()[0].copy()))
        tok = ids[1]
        flips += _check_logits(oracle, b.logits()[1], lg, tok, f"{name} branch step {t}")
    assert flips <= max_flips(9)
    # the source: bit-identical to the batch that never forked
    for (i, l), (wi, wl) in zip(got, want[2:]):
        assert i == wi and np.array_equal(l, wl)
    b.close()


# ------------------------------------------------------------------ 6. errors, all-or-nothing
@pytest.mark.parametrize("paged", [True, False], ids=["paged", "contig"])
def test_fork_errors_change_nothing(paged):
    eng = engine()
    prompt = _ids(61, 297)
    runs = []
    for attempt in (False, True):
        b = eng.batch(3, 512, **(dict(page_tokens=T, n_pages=4) if paged else {}))   # scratch + 3: none free
        b.prefill(0, prompt)
        b.decode(3)
        if attempt:
            before = _state(b)
            for args in [(1, 2, 1), (0, 0, 10), (0, 2, 0), (0, 2, 301), (0, 3, 10), (-1, 2, 10)]:
                with pytest.raises(_lib.QieError, match=r"rc=-22"):
                    b.fork(*args)
            if paged:
                with pytest.raises(_lib.QieError, match=r"rc=-28"):
                    b.fork(0, 2, 300)               # no page for the 44-row tail
                with pytest.raises(_lib.QieError, match=r"rc=-22"):
                    b.save_prefix(0, 100)
            else:
                with pytest.raises(_lib.QieError, match=r"rc=-22"):
                    b.save_prefix(0, 256)           # prefix handles need a paged batch
                with pytest.raises(_lib.QieError, match=r"rc=-22"):
                    b.page_refs()
            assert _state(b) == before
        ids = b.decode_step()
        runs.append((ids[0], b.logits()[0].copy(), b.positions().tolist()))
        if attempt and paged:
            b.fork(0, 2, 256)                       # whole pages need no page: fits the full pool
            assert b.page_stats()[0] == 0 and b.page_stats()[1].tolist() == [3, 0, 2]
        b.close()
    assert runs[0][0] == runs[1][0] and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]


# ------------------------------------------------------------------ 7. sampling
def test_fork_step_offset_moves_the_sampler(qlib):
    eng = engine()
    smp = Q.Sampling(top_k=8, temperature=1.0, seed=4321)
    b = eng.batch(3, 512, page_tokens=T)
    b.prefill(0, _ids(71, 140), smp)
    b.decode(4, smp)                                # the source's counter: 1 (prefill) + 4
    b.fork(0, 1, step_offset=0)
    b.fork(0, 2, step_offset=1000)
    first = b.decode_step(smp)
    assert first[1] == first[0]
    lg = b.logits()
    assert np.array_equal(lg[2], lg[0])             # same input, same logits; only the draw differs
    V = SPEC.vocab
    dl, step = G.dev(lg[2:3]), G.dev(np.array([5 + 1000], np.int32))
    ids, ws = G.zeros((1,), np.int32), G.zeros_bytes(qlib.qie_sample_workspace_bytes(1, V))
    s = SamplingC()
    s.top_k, s.temperature, s.top_p, s.seed = 8, 1.0, 1.0, 4321
    G.check(qlib.qie_sample(G.p(dl), 1, V, V, C.byref(s), G.p(step), G.p(ids), G.p(ws), None))
    G.check(qlib.qie_synchronize())
    assert int(G.host(ids)[0]) == first[2]
    step0 = G.dev(np.array([5], np.int32))
    G.check(qlib.qie_sample(G.p(dl), 1, V, V, C.byref(s), G.p(step0), G.p(ids), G.p(ws), None))
    G.check(qlib.qie_synchronize())
    assert int(G.host(ids)[0]) == first[0]
    for _ in range(5):                              # offset 0 keeps drawing the source's tokens
        nxt = b.decode_step(smp)
        assert nxt[1] == nxt[0]
    b.close()


# ------------------------------------------------------------------ 8. prefix handles
@pytest.mark.parametrize("n", [256, 128])
def test_prefix_load_equals_fork(n):
    """Save 256 of a 300-token sequence and release the slot: the pages stay with count 1.  A load
    (whole, or truncated to 128) + append of the remaining ids equals, bit for bit, a fork at the
    same length + the same append taken before the release."""
    eng, prompt, b = _forked()
    full = b.history(0, 300).tolist()
    rest = full[n:300] + _ids(81, 17)
    free0 = b.page_stats()[0]
    b.fork(0, 1, n)
    tok_f = b.append(1, rest, pos0=n)
    lg_f, rows_f = b.logits()[1].copy(), _rows(b, 1, n + len(rest))
    dec_f = [b.decode_step()[1] for _ in range(3)]
    b.release(1)
    pf = b.save_prefix(0, 256)
    assert pf.n_tokens == 256 and pf.ids == full[:256]
    assert b.page_stats()[0] == free0               # a save takes no page
    pages = b.block_table(0, 2).tolist()
    assert b.page_refs()[pages].tolist() == [2, 2]
    b.release(0)
    assert b.page_refs()[pages].tolist() == [1, 1] and b.page_stats()[0] == b.n_pages - 1 - 2
    b.load_prefix(pf, 2, rest[0], n)
    assert int(b.positions()[2]) == n and b.history(2, n).tolist() == full[:n]
    assert b.block_table(2, n // T).tolist() == pages[:n // T]
    tok_l = b.append(2, rest, pos0=n)
    assert tok_l == tok_f and np.array_equal(b.logits()[2], lg_f)
    assert _rows_equal(_rows(b, 2, n + len(rest)), rows_f)
    assert [b.decode_step()[2] for _ in range(3)] == dec_f
    with pytest.raises(_lib.QieError, match=r"rc=-22"):
        b.load_prefix(pf, 1, 5, 100)
    with pytest.raises(_lib.QieError, match=r"rc=-22"):
        b.load_prefix(pf, 1, 5, 384)
    b.release(2)
    assert b.page_refs()[pages].tolist() == [1, 1]
    pf.drop()
    assert b.page_stats()[0] == b.n_pages - 1 and not b.page_refs().any()
    b.close()


# ------------------------------------------------------------------ 9. the batcher's prefix cache
def test_batcher_prefix_cache_matches_oracle(oracle):
    """Three requests, the second and third beginning with the first's first 256 ids, the third
    submitted after the first finished, on a pool of 5 usable pages: when the third (3 pages)
    arrives, the second and the cache hold 3, so it fits only because 2 of its pages are shared.
    Tokens and logits follow the oracle under test_batcher_batched_admission_matches_oracle's
    bar; no call returns -28 (one would raise)."""
    from qwen_inference_engine_amd.scheduler import ContinuousBatcher
    eng = engine()
    hw = W.HostWeights.synthetic(SPEC, SYN)
    cb = ContinuousBatcher(eng, slots=2, max_ctx=512, page_tokens=T, n_pages=6, keep_logits=True,
                           prefix_cache_pages=4)
    base = _ids(91, 256)
    prompts = [base + _ids(92, 44), base + _ids(93, 30), base + _ids(94, 100)]
    new = [12, 40, 20]
    rids = [cb.submit(prompts[0], new[0]), cb.submit(prompts[1], new[1])]
    while not cb.requests[rids[0]].done:
        cb.step()
    assert not cb.requests[rids[1]].done
    rids.append(cb.submit(prompts[2], new[2]))          # pages(376) = 3, two of them cached
    cb.run()
    assert cb.prefix_hits == 2 and cb.prefix_tokens_reused == 512
    flips = n_tok = 0
    for rid, pr in zip(rids, prompts):
        r = cb.requests[rid]
        assert len(r.tokens) == new[rid]
        om = oracle.Model(hw, 512)
        lg = om.forward(pr, 0)
        for t, (tok, got) in enumerate(zip(r.tokens, r.logits)):
            d = np.abs(G.bf(got).astype(np.float64) - G.bf(lg))
            assert d.max() <= logit_tol(lg), f"request {rid} token {t}: {d.max()}"
            want = oracle.argmax(lg)
            if tok != want:
                assert abs(float(G.bf(lg[want])) - float(G.bf(lg[tok]))) <= logit_tol(lg)
                flips += 1
            if t + 1 < len(r.tokens):
                lg = om.forward([tok])
        n_tok += len(r.tokens)
    assert flips <= max_flips(n_tok)
    assert cb.batch.page_stats()[0] == 5 - 2            # the cache holds the shared prefix
    cb.drop_cache()
    assert cb.batch.page_stats()[0] == 5 and not cb.batch.page_refs().any()
    cb.close()
