"""GPU: the four attention kernels key by key (cases, reference and rules: attn_cases.py).

Family 1 is exact (np.array_equal): needles and ramps make one key carry the whole softmax, so
a kernel that sees one key too many or too few — the row's own key, the new token's LDS row,
the last key of a split, a key on a tile / step / page boundary, a tile the causal mask was
skipped for — returns another key's V row, and traps (K = 2 x a query row, NaN, +Inf in every
cache row past the context) show any read the score select or the buffer bounds let through.
Family 2 compares random inputs of wide score range with the float64 reference under
|d| <= half a bf16 ulp + kappa * sum_t w_t |v_t|.  `out` is framed by a sentinel row on each
side; the extend workspace starts as 0xFF bytes, the decode workspace zeroed (its contract).
"""
import ctypes as C

import numpy as np
import pytest

import attn_cases as A
import gpu_util as G
from test_gpu_paged import Paged, _contig

from qwen_inference_engine_amd import _lib

pytestmark = pytest.mark.gpu

T = 128
SENTINEL = 0x4D4D
TRAPS = [None, "finite", "nan", "inf"]
KS = [(k, s) for k in A.KERNELS for s in A.SHAPES[k]]
KS_IDS = [f"{k}-{s[0]}-{s[1]}-{s[2]}" for k, s in KS]
KSF = [(k, s, f) for k, s in KS for f in (A.DECODE_FORMS if k == "decode" else (None,))]
KSF_IDS = [f"{k}-{s[0]}-{s[1]}-{s[2]}" + (f"-{f}" if f else "") for k, s, f in KSF]
KSW = [(k, s, f) for k, s in KS for f in (("ref", "pre") if k == "decode" else (None,))]
KSW_IDS = [f"{k}-{s[0]}-{s[1]}-{s[2]}" + (f"-{f}" if f else "") for k, s, f in KSW]


class Dev:
    """The device cache of a case, contiguous or paged (shuffled 128-token pages).  Paged, the
    pool holds one sequence more than the call uses — pages no table row of the call names —
    and with a trap that sequence, page 0 and the page tails past max_ctx hold the trap too."""

    def __init__(self, oracle, c, paged):
        Kh, Vh = (c.Kdev, c.Vdev) if c.kernel == "decode" else (c.K, c.V)
        self.c, self.paged, self.shape = c, paged, Kh.shape
        if not paged:
            self.kc, self.vc = G.dev(Kh), G.dev(Vh)
            self.desc = _contig(self.kc, self.vc, A.L, c.nkv, c.hd, c.maxc)
            return

        def fill(n, id0):   # [L][nkv][n][hd] of trap content
            kv = [A.trap_rows(c, n, g, 0, id0 + g * n) for g in range(c.nkv)]
            return [np.broadcast_to(np.stack([x[i] for x in kv])[None], (A.L, c.nkv, n, c.hd)) for i in (0, 1)]

        id0 = 4 * A.n_cache_rows(c)
        xk, xv = fill(c.maxc, id0) if c.trap else (Kh[0], Vh[0])
        pg = Paged(oracle, np.concatenate([Kh, xk[None]]), np.concatenate([Vh, xv[None]]), T, seed=7)
        if c.trap:
            pg.kp[0], pg.vp[0] = fill(T, id0 + c.nkv * c.maxc)
            n = c.maxc - (pg.mp - 1) * T
            if n < T:
                for b in range(c.B):
                    pg.kp[pg.table[b, -1], :, :, n:], pg.vp[pg.table[b, -1], :, :, n:] = fill(T - n, id0 + 2 * c.nkv * c.maxc)
        pg.dk, pg.dv = G.dev(pg.kp), G.dev(pg.vp)
        self.pg, self.desc = pg, pg.cache()

    def check_append(self):
        """Decode: the new K / V row is written (the existing rule against the oracle's rotated
        row), and no other element of the cache — or, paged, of the pool — changed."""
        c, layer = self.c, A.LAYER
        if self.paged:
            hk, hv = self.pg.gather(self.pg.dk)[:c.B], self.pg.gather(self.pg.dv)[:c.B]
        else:
            hk, hv = G.host_bf16(self.kc).reshape(self.shape), G.host_bf16(self.vc).reshape(self.shape)
        ek, ev = c.Kdev.copy(), c.Vdev.copy()
        for b in range(c.B):
            p = int(c.pos[b])
            if c.form == "pre":
                assert np.array_equal(hk[b, layer, :, p].reshape(-1), c.knew[b]), f"{c.name}: appended K row {b}"
            else:   # qk-norm sum order may flip one rounding; HF rounds twice (2 ulps)
                G.assert_bf16_close(hk[b, layer, :, p].reshape(-1), c.knew[b], 1 if c.num == "ref" else 2,
                                    0.9 if c.qkn else 1.0, f"{c.name}: appended K row {b}")
            assert np.array_equal(hv[b, layer, :, p].reshape(-1), c.vnew[b]), f"{c.name}: appended V row {b}"
            ek[b, layer, :, p], ev[b, layer, :, p] = hk[b, layer, :, p], hv[b, layer, :, p]
        assert np.array_equal(hk, ek) and np.array_equal(hv, ev), f"{c.name}: a cache row other than pos changed"
        if self.paged:
            pg = self.pg
            for pool, dev, h in ((pg.kp, pg.dk, hk), (pg.vp, pg.dv, hv)):
                want = pool.copy()
                for b in range(c.B):
                    p = int(c.pos[b])
                    want[pg.table[b, p // T], layer, :, p % T] = h[b, layer, :, p]
                assert np.array_equal(G.host_bf16(dev).reshape(pool.shape), want), f"{c.name}: the pool changed elsewhere"


def launch(qlib, oracle, c, paged):
    """Runs the case's operator; returns the outputs [M][nq*hd] of its calls (decode: two in a
    row on one workspace)."""
    d = Dev(oracle, c, paged)
    row = c.nq * c.hd
    out = G.dev(np.full((c.M + 2, row), SENTINEL, np.uint16))
    o, q, pos = G.p(out) + row * 2, G.dev(c.q), G.dev(c.pos)
    outs = []

    def take():
        got = G.host_bf16(out)
        assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), f"{c.name}: rows outside [0, M) were written"
        outs.append(got[1:-1].copy())

    if c.kernel in ("split", "prefill"):
        assert (c.rps >= 32 and c.M % c.rps == 0) == (c.kernel == "prefill")
        ws = G.zeros_bytes(qlib.qie_attention_workspace_bytes(c.M, c.nq, c.hd, c.maxc))
        G.check(qlib.qie_attention(G.p(q), c.M, G.p(pos), c.rps, C.byref(d.desc), A.LAYER, c.nq, o, G.p(ws), None), c.name)
        take()
    elif c.kernel == "extend":
        assert qlib.qie_attention_extend_split_tokens(c.M, c.maxc) == A.extend_split_tokens(c.M, c.maxc)
        nbytes = qlib.qie_attention_extend_workspace_bytes(c.M, c.nq, c.hd, c.maxc)
        assert nbytes > 0
        ws = G.zeros_bytes(nbytes)
        G.check(qlib.qie_memset(G.p(ws), 0xFF, nbytes))   # need not be initialised: NaNs in every partial slot
        G.check(qlib.qie_attention_extend(G.p(q), c.M, G.p(pos), c.rps, C.byref(d.desc), A.LAYER, c.nq, o, G.p(ws), None),
                c.name)
        take()
    else:
        ws = G.zeros_bytes(qlib.qie_attention_decode_workspace_bytes(c.B, c.nq, c.nkv, c.hd, c.maxc))
        qkv, cs, sn = G.dev(c.qkv), G.dev(c.cs), G.dev(c.sn)
        qn, kn = (G.dev(c.qn), G.dev(c.kn)) if c.qkn else (None, None)
        num = _lib.QIE_ATTN_PREROPED if c.form == "pre" else (0 if c.num == "ref" else 1)
        for rep in range(2):   # the second call finds the counters zeroed and the row already appended
            G.check(qlib.qie_attention_decode(G.p(qkv), c.B, G.p(pos), G.p(qn), G.p(kn), G.p(cs), G.p(sn), c.nq,
                                              C.byref(d.desc), A.LAYER, c.eps, num, o, G.p(ws), None), c.name)
            take()
            d.check_append()
        assert not G.host(ws)[:c.B * c.nkv * 4].any(), f"{c.name}: counters not left zeroed"
    G.release_all()
    return outs


def run_exact(qlib, oracle, kernel, shape, family, paged, trap, form):
    n = 0
    for c in A.cases(kernel, shape, family, trap=trap, oracle=oracle, form=form, sweeps=trap is None):
        for got in launch(qlib, oracle, c, paged):
            ok = A.accepted(c, got)
            assert ok.all(), (f"{int((~ok).sum())} of {ok.size} (row, head)s, paged {paged}: "
                              + A.describe(c, got, *np.argwhere(~ok)[0]))
        n += 1
    print(f"{kernel} {shape} {family} paged {paged} trap {trap} form {form}: {n} launches exact")


@pytest.mark.parametrize("trap", TRAPS, ids=lambda t: t or "plain")
@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("kernel,shape,form", KSF, ids=KSF_IDS)
def test_needles(oracle, qlib, kernel, shape, form, paged, trap):
    """Key 0, pos, pos - 1 and both sides of every tile / step / split edge are each the one key
    some (row, head) must return; without a trap also every key of a context (the full sweep)."""
    run_exact(qlib, oracle, kernel, shape, "needle", paged, trap, form)


@pytest.mark.parametrize("trap", TRAPS, ids=lambda t: t or "plain")
@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("up", [True, False], ids=["up", "down"])
@pytest.mark.parametrize("kernel,shape", KS, ids=KS_IDS)
def test_ramps(oracle, qlib, kernel, shape, up, paged, trap):
    """Ascending: every row returns V[pos] (the running max grows at every key, alpha underflows at
    every tile; rows of one 16-row group sit at different positions, which pins gmin).
    Descending: V[0] (later tiles, steps and splits weigh 0; the merge sees exp(ms - mn) = 0).
    Decode: the QIE_ATTN_PREROPED form only — RoPE would turn the ramp's two dimensions."""
    run_exact(qlib, oracle, kernel, shape, "ramp_up" if up else "ramp_down", paged, trap, "pre" if kernel == "decode" else None)


@pytest.mark.parametrize("s", A.WIDE_SCALES)
@pytest.mark.parametrize("paged", [False, True], ids=["contig", "paged"])
@pytest.mark.parametrize("kernel,shape,form", KSW, ids=KSW_IDS)
def test_wide_score_range(oracle, qlib, kernel, shape, form, paged, s):
    """q ~ N(0, s**2): scores span tens of nats and the running-max rescale does real work.
    Every element within half a bf16 ulp + kappa x the mass of the float64 reference."""
    k, worst = A.kappa(kernel), 0.0
    for c in A.cases(kernel, shape, "wide", oracle=oracle, form=form, s=s):
        ref = A.ref64(c)
        for got in launch(qlib, oracle, c, paged):
            x = A.excess(got, *ref)
            d = np.abs(A.f64(got) - ref[0])
            print(f"{c.name} paged {paged} form {form}: max |d| {np.nanmax(d):.3e}, worst excess {x.max():.3e} of the mass = "
                  f"{x.max() / k:.3f} of kappa 2**{np.log2(k):.2f}")
            worst = max(worst, x.max() / k)
            assert np.isfinite(A.f64(got)).all(), c.name
            m, e = np.unravel_index(np.argmax(x), x.shape)
            assert x.max() <= k, (f"{c.name}: row {m} (pos {int(c.pos[m])}) element {e}: got {A.f64(got)[m, e]!r} ref "
                                  f"{ref[0][m, e]!r} mass {ref[1][m, e]:.4f}; {int((x > k).sum())} of {x.size} elements over")
    print(f"F2 {kernel} {shape} form {form} paged {paged} s {s}: worst excess / kappa {worst:.3f}")
