"""GPU: Engine(kv_fp8=True) — the fp8 KV cache through the engine: the rows it holds, bit-identity
between cache forms and replays, three routes to one state, and the calls it refuses."""
import ctypes as C

import numpy as np
import pytest

import gpu_util as G
from conftest import rng
from parity import max_flips, norm_rel
from test_gpu_engine import CONFIGS, SYN
from test_gpu_kv_fp8 import quantize_rows

import qwen_inference_engine_amd as Q
from qwen_inference_engine_amd import _lib, spec as S

pytestmark = pytest.mark.gpu
SPEC = CONFIGS["qwen2-bias-hd64"]
IDS = [int(t) for t in rng(5).integers(0, SPEC.vocab, 200)]


def engine(kv_fp8, spec=SPEC, max_ctx=256):
    return Q.Engine(spec, max_ctx=max_ctx, kv_fp8=kv_fp8).init_synthetic(SYN)


def forced_steps(b, ids, p0, n, seq=0):
    """n teacher-forced decode steps: position p0 + t gets token ids[p0 + t]; returns (tokens, logits)"""
    out = []
    for t in range(n):
        b.set_position(seq, p0 + t, ids[p0 + t])
        tok = b.decode_step()[seq]
        out.append((tok, b.logits()[seq].copy()))
    return out


def d2h(lib, ptr, shape, dtype):
    a = np.zeros(shape, dtype)
    _lib.check(lib.qie_memcpy_d2h(a.ctypes.data, ptr, a.nbytes), "d2h")
    return a


# ------------------------------------------------------------- 5. layer-0 rows
def test_layer0_rows_are_the_bf16_engines_rows_quantized(qlib):
    """Layer 0's K/V depend on ids and positions only, and both engines run the same projections."""
    e16, e8 = engine(False), engine(True)
    b16, b8 = e16.batch(1, 256), e8.batch(1, 256)
    for b in (b16, b8):
        b.prefill(0, IDS[:40])
        forced_steps(b, IDS, 40, 4)
    c = b8.kv_cache_fp8(0)
    nkv, hd, run = c.c.n_kv_heads, c.c.head_dim, c.c.max_ctx
    for which, (codes_p, exps_p) in enumerate(((c.c.k, c.k_exps), (c.c.v, c.v_exps))):
        codes = d2h(qlib, codes_p, (nkv, run, hd), np.uint8)[:, :44]      # layer 0 of slot 0
        exps = d2h(qlib, exps_p, (nkv, run), np.uint8)[:, :44]
        want_c, want_e = quantize_rows(qlib, b16.kv_rows(0, 0, 44)[which].reshape(nkv * 44, hd))
        assert np.array_equal(codes.reshape(-1, hd), want_c) and np.array_equal(exps.reshape(-1), want_e), which


# ------------------------------------------------------------- 6. bit-identity
def test_paged_contiguous_rewind_and_slots_bit_identical():
    e8 = engine(True)
    runs = []
    for pt in (None, 128):
        b = e8.batch(2, 256, page_tokens=pt)
        first = b.prefill(0, IDS[:120])
        runs.append((first, b.logits()[0].copy(), forced_steps(b, IDS, 120, 12)))      # across the page boundary
        again = forced_steps(b, IDS, 125, 7)                                            # rewind and re-decode
        assert all(t == u and np.array_equal(x, y) for (t, x), (u, y) in zip(runs[-1][2][5:], again)), pt
        # a second slot given the same prompt: the same token and logits, and slot 0's next step unmoved
        assert b.prefill(1, IDS[:120]) == first and np.array_equal(b.logits()[1], runs[-1][1])
        b.set_position(1, 120, IDS[120])
        b.set_position(0, 131, IDS[131])
        toks = b.decode_step()
        assert toks[0] == again[6][0] and np.array_equal(b.logits()[0], again[6][1])
        assert toks[1] == runs[-1][2][0][0] and np.array_equal(b.logits()[1], runs[-1][2][0][1])
    (f0, l0, s0), (f1, l1, s1) = runs
    assert f0 == f1 and np.array_equal(l0, l1)
    assert all(t == u and np.array_equal(x, y) for (t, x), (u, y) in zip(s0, s1))


# ------------------------------------------------- 7. three routes to one state
def route_logits(eng, lib=None):
    """(token, logits, rows) per route; rows (fp8 engine, `lib` given): the codes and the exponent of
    every K and V row of positions [0, P + n), all layers and kv heads, one row per line"""
    P, n = 70, 20
    out = []
    for route in range(3):
        b = eng.batch(1, 256)
        if route == 0:
            tok = b.prefill(0, IDS[:P + n])
        elif route == 1:
            b.prefill(0, IDS[:P])
            tok = b.append(0, IDS[P:P + n])
        else:
            b.prefill(0, IDS[:P])
            tok = forced_steps(b, IDS, P, n)[-1][0]
        logits, rows = b.logits()[0].copy(), None
        if lib:
            c = b.kv_cache_fp8(0)
            sh = (c.c.n_layers, c.c.n_kv_heads, c.c.max_ctx)
            rows = np.concatenate([np.concatenate([d2h(lib, cp, sh + (c.c.head_dim,), np.uint8)[:, :, :P + n],
                                                   d2h(lib, ep, sh + (1,), np.uint8)[:, :, :P + n]], -1)
                                   for cp, ep in ((c.c.k, c.k_exps), (c.c.v, c.v_exps))]).reshape(-1, c.c.head_dim + 1)
        out.append((tok, logits, rows))
        b.close()
    return out


MARGIN = 4   # 1 + 32 x 0.0889 = 3.84: the measured share of rows with differing codes, see below


def test_three_routes_reach_one_state(qlib):
    """prefill(P + n), prefill(P) + append(n), prefill(P) + n forced decode steps: same history, same
    position.  The routes' projection kernels differ, so K/V rows differ by a bf16 ulp (2^-8 relative)
    in places.  On the fp8 engine a row whose codes and exponent agree between the routes carries no
    difference at all, and a row whose codes differ carries elements moved by one e4m3 step (2^-3), 32
    bf16 ulps.  Were the whole bf16-KV spread s16 the K/V rows' doing (it is not: the routes' last
    projections and attention kernels differ too), a share f of differing rows would give at most
    s16 (1 - f) + 32 f s16 < s16 (1 + 32 f).  Bound: s16, measured here at the same seeds (the
    parent's behaviour), times MARGIN = 1 + 32 f rounded up, and never above 2^-5: an error of one
    e4m3 step in the logits is a broken read path, not rounding.
    Measured (MI355X): s16 6.707e-3, fp8 spread 6.717e-3, f = 96 of 1,080 rows (0.0889), so MARGIN 4 and
    a bound of 2.68e-2 (profiles/kv_fp8.json, three_routes)."""
    r16, r8 = route_logits(engine(False)), route_logits(engine(True), qlib)
    spread = lambda r: max(norm_rel(r[i][1], r[j][1]) for i in range(3) for j in range(i))
    s16, s8 = spread(r16), spread(r8)
    differs = np.zeros(len(r8[0][2]), bool)
    for i in range(3):
        for j in range(i):
            differs |= (r8[i][2] != r8[j][2]).any(1)
    bound = min(2.0 ** -5, MARGIN * s16)
    print(f"three-route spread: bf16-KV {s16:.3e}, fp8-KV {s8:.3e}, rows with differing codes "
          f"{differs.mean():.4f} of {len(differs)}, bound {bound:.3e}")
    assert s8 <= bound, (s8, bound)
    assert sum(r8[i][0] != r8[0][0] for i in (1, 2)) <= max_flips(3)


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_batch_alone_and_kv_bytes():
    e8 = engine(True)
    b = e8.batch(2, 256, page_tokens=128)
    b.prefill(0, IDS[:130])
    state = lambda: (b.positions().tolist(), b.page_stats()[0], list(b.page_stats()[1]))
    before = state()
    refused = [lambda: b.prefill_ragged([(1, IDS[:5])]), lambda: b.verify(0, IDS[:2]),
               lambda: b.verify_batch([(0, IDS[:2])]), lambda: b.fork(0, 1), lambda: b.save_prefix(0, 128),
               lambda: b.set_decode_mode(1), lambda: b.debug_step(), lambda: b.time_kernel(5),
               lambda: b.time_kernel(6), lambda: b.kv_cache(0)]
    for i, call in enumerate(refused):
        with pytest.raises(_lib.QieError, match=r"rc=-22.*fp8-KV"):
            call()
        assert state() == before, i
    ref = e8.batch(1, 256, page_tokens=128)
    ref.prefill(0, IDS[:130])
    assert b.decode_step()[0] == ref.decode_step()[0] and np.array_equal(b.logits()[0], ref.logits()[0])
    for bad in (dict(kv_fp8=2), dict(kv_fp8=True, weight_fp8=True, prefill_fp8=True)):
        with pytest.raises(_lib.QieError, match="kv_fp8"):
            Q.Engine(SPEC, max_ctx=64, **bad)
    from qwen_inference_engine_amd.scheduler import ContinuousBatcher
    for bad in (dict(ragged_prefill=True), dict(drafter=object()), dict(prefix_cache_pages=2)):
        with pytest.raises(ValueError, match="fp8-KV"):
            ContinuousBatcher(e8, slots=2, max_ctx=256, **bad)
    cb = ContinuousBatcher(e8, slots=2, max_ctx=256, prefill_chunk=48)
    rid = cb.submit(IDS[:100], 3)
    got = [t for _ in range(8) for r, t in cb.step() if r == rid]
    assert len(got) == 3
    # shape check at L = 24, hd = 128: codes + exponents + one staging layer < 0.6 of the bf16 cache
    big = S.tiny("t-kvb", n_layers=24, hidden=128, n_heads=2, n_kv_heads=1, head_dim=128, ffn=128, vocab=256)
    by = [Q.Engine(big, max_ctx=512, kv_fp8=k).init_synthetic(SYN).batch(2, 512).kv_bytes() for k in (False, True)]
    assert by[1] < 0.6 * by[0], by
