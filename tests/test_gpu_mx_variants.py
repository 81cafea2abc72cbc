"""GPU parity: every form of gemm8mx_kernel (fp8 activations: 4 epilogues x plain / 16-row
tiled weights x 1..4 split-K parts), the protocol of tests/test_gpu_gemm_variants.py.

One test per (row of tests/mx_cases.py, input family); tests/test_mx_cases_cpu.py keeps the
table complete and the exact families sharp.  Per launch:
  * the library's own plan (qie_debug_linear_plan) must be the row's declaration, grid aside;
  * the operands are handed over as codes: x e4m3 codes and x_exps, each weight segment a blob
    built here (codes, tiled by qie_fp8_tile16 for T16 rows and compared with mx_cases.tile16,
    then the fp32 row scales) -- no quantiser between the inputs and the kernel;
  * x, x_exps, every weight blob and every bias are allocations of their own with NaN guards
    before and after (code 0x7F rows around x and in its ldx pad, 0xFF bytes -- a NaN e8m0
    exponent, a NaN code, a NaN scale -- around x_exps and around each blob, whose scales follow
    its codes by the format; bf16 NaN around a bias): any use of a guard or a pad poisons the
    output;
  * y has a sentinel row before and after its M rows and sentinel pad columns where ldy > N;
  * rows marked `twice` (split-K) run twice into fresh outputs, bit-equal.
F1 (scaled integers) and F2 (scaled needles) have one right answer each and are compared with it
bit for bit (mx_cases.accepted, the function the CPU mutant test uses).  F3 draws rand_bf16 data
through the quantisers (qie_quantize_rows_fp8, qie_quantize_fp8) and holds the result to the
oracle's matmul of the dequantised operands under tests/test_gpu_fp8_mx.py's bounds
(MX_ACC_REL of sum|a w|; SWIGLU as there: the epilogue on the kernel's own bf16 halves, the
halves under MX_ACC_REL), then runs test_gemm_random's two isolation launches: x row r* all NaN
codes, and the last weight row of a segment all NaN codes -- bit-equal to the clean launch
except row r* / column n*, which are all NaN.
test_quantisers_reproduce_the_cases feeds the F1 / F2 operands, as bf16, through the quantisers
and the tiler: what the engine would produce from these values is what the exact tests feed.
The last test interleaves this kernel's split forms with the bf16 kernels' on one fresh stream:
they share the split-K workspace and its ticket reset."""
import ctypes as C

import numpy as np
import pytest

import gemm_cases as GC
import gpu_util as G
import mx_cases as MC
from test_gpu_fp8_mx import MX_ACC_REL, _fp8w, _mx_linear, _quant_dev
from test_gpu_gemm_variants import _At, _exact as _gemm_exact, _guarded_bias, _guarded_fp8, _is_nan
from test_gpu_linear_variants import EPI, W_SCALE, _live_plan
from test_gpu_ops import _abs_scale, _linear_args, rand_bf16

from qwen_inference_engine_amd import _lib, weights as W

pytestmark = pytest.mark.gpu

IDS = [c.name for c in MC.CASES]
NO_SWIGLU = [c for c in MC.CASES if c.epi != "SWIGLU"]


def _guarded_codes(x, ld):
    """[M, K] codes -> its own allocation [M + 2, ld], NaN code 0x7F everywhere but x."""
    M, K = x.shape
    h = np.full((M + 2, ld), MC.NAN_CODE, np.uint8)
    h[1:M + 1, :K] = x
    return _At(G.dev(h), ld)


def _guarded_exps(ea):
    h = np.full(len(ea) + 32, 0xFF, np.uint8)
    h[16:16 + len(ea)] = ea
    return _At(G.dev(h), 16)


def _tile16_dev(qlib, codes, scales):
    """qie_fp8_tile16 of the plain blob (codes, scales) -> the tiled codes [rows, K]."""
    rows, K = codes.shape
    src = G.dev(np.concatenate([codes.reshape(-1), scales.view(np.uint8)]))
    dst = G.zeros((src.nbytes,), np.uint8)
    G.check(qlib.qie_fp8_tile16(G.p(src), rows, K, G.p(dst), None), "qie_fp8_tile16")
    out = G.host(dst)
    assert np.array_equal(out[rows * K:], scales.view(np.uint8)), "qie_fp8_tile16 changed the row scales"
    return out[:rows * K].reshape(rows, K)


class _Launch:
    """The device side of one row: guarded operands, and launches into fresh framed outputs."""

    def __init__(self, qlib, c, x, ea, ws, scales, bs, y0):
        """ws: plain codes per segment; scales: fp32 row scales per segment."""
        self.qlib, self.c, self.y0 = qlib, c, y0
        self.N, self.ldx, self.ldy = GC.n_cols(c), c.K + c.ldx_pad, y0.shape[1]
        self.rows = MC.segments(c)
        self.dx, self.de = _guarded_codes(x, self.ldx), _guarded_exps(ea)
        self.dws = [self._blob(w, s) for w, s in zip(ws, scales)]
        self.dbs = [_guarded_bias(b) for b in bs]

    def _blob(self, codes, scales):
        if MC.is_t16(self.c):
            tiled = _tile16_dev(self.qlib, codes, scales)
            assert np.array_equal(tiled, MC.tile16(codes)), f"{self.c.name}: qie_fp8_tile16 is not the documented layout"
            codes = tiled
        return _guarded_fp8(codes, scales)

    def with_nan_x_row(self, x, r):
        x = x.copy()
        x[r] = MC.NAN_CODE
        self.dx = _guarded_codes(x, self.ldx)

    def with_nan_weight_row(self, ws, scales, seg, r):
        w = ws[seg].copy()
        w[r] = MC.NAN_CODE
        self.dws[seg] = self._blob(w, scales[seg])

    def __call__(self, stream=None):
        c = self.c
        y = G.dev(self.y0)
        a = _linear_args(self.dx, list(zip(self.dws, self.rows)), self.dbs, c.M, c.K, self.N,
                         _At(y, self.ldy * self.y0.dtype.itemsize), EPI[c.epi], ldy=self.ldy, flags=c.flags, ldx=self.ldx)
        a.x_exps = self.de.ptr
        plan = _live_plan(self.qlib, a)
        assert plan.split(" grid=")[0] == c.plan, f"{c.name}: the library plans {plan}"
        G.check(self.qlib.qie_linear(C.byref(a), stream), "qie_linear act_fp8")
        return G.host(y)   # (synchronises the device)

    def frame_kept(self, y):
        outside = np.ones(self.y0.shape, bool)
        outside[1:self.c.M + 1, :self.N] = False
        assert np.array_equal(GC.bits(y)[outside], GC.bits(self.y0)[outside]), f"{self.c.name}: wrote outside y[:M, :N]"


def _scales(ss):
    return [np.ldexp(np.float32(1), s.astype(np.int32)).astype(np.float32) for s in ss]


def _exact(qlib, c, fam, stream=None):
    inp = MC.inputs(c, fam)
    run = _Launch(qlib, c, inp.x, inp.ea, inp.ws, _scales(inp.ss), inp.bs, inp.y0)
    y = run(stream)
    if c.twice:
        assert np.array_equal(GC.bits(y), GC.bits(run(stream))), f"{c.name}: two launches differ"
    ok, why = MC.accepted(c, y, inp.y0, MC.expected(c, fam, inp))
    print(f"{c.name} {fam}: {c.plan}: {'exact' if ok else why}")
    assert ok, why
    return y


@pytest.mark.parametrize("case", MC.CASES, ids=IDS)
def test_mx_integers(qlib, case):
    _exact(qlib, case, "F1")


@pytest.mark.parametrize("case", NO_SWIGLU, ids=[c.name for c in NO_SWIGLU])
def test_mx_needles(qlib, case):
    _exact(qlib, case, "F2")


@pytest.mark.parametrize("case", MC.CASES, ids=IDS)
def test_mx_random(oracle, qlib, case):
    c = case
    M, K, N, epi = c.M, c.K, GC.n_cols(c), c.epi
    idx = MC.CASES.index(c)
    seed = GC.seed_of(c, "F3") % 10000
    rows = MC.segments(c)
    xb = rand_bf16(oracle, (M, K), seed=seed)
    wb = [rand_bf16(oracle, (r, K), W_SCALE[epi], seed=seed + 10 + i) for i, r in enumerate(rows)]
    bs = [rand_bf16(oracle, (r,), 0.1, seed=seed + 20 + i) for i, r in enumerate(rows)] if c.bias else []
    res = rand_bf16(oracle, (M, N), seed=seed + 40) if epi == "RESIDUAL" else None
    # ---- through the quantisers; the kernel is fed what they wrote
    q, e = _quant_dev(qlib, xb)
    x, ea = G.host(q).reshape(M, K), G.host(e)[:M]
    dqx, e_or = oracle.quant_rows_fp8(xb)
    assert np.array_equal(ea.astype(np.int64) - 127, e_or)
    assert np.array_equal(np.ldexp(MC.e4m3_values()[x], ea.astype(np.int32)[:, None] - 127), GC.bf(dqx))   # (as values)
    dev_w = [_fp8w(qlib, w, False) for w in wb]
    ws = [G.host(d)[:r * K].reshape(r, K) for (d, _), r in zip(dev_w, rows)]
    scales = [G.host(d)[r * K:].view(np.float32).copy() for (d, _), r in zip(dev_w, rows)]
    dq = [v for _, v in dev_w]
    for w_, s_, v in zip(ws, scales, dq):
        assert np.array_equal(W.dequantize_fp8(w_, s_), v)
    y0 = GC.frame(c, res)
    run = _Launch(qlib, c, x, ea, ws, scales, bs, y0)

    y = run()
    run.frame_kept(y)
    if c.twice:
        assert np.array_equal(GC.bits(y), GC.bits(run())), f"{c.name}: two launches differ"
    got = GC.live(c, y)

    # ---- the bounds of tests/test_gpu_fp8_mx.py
    if epi == "STORE":
        want = np.concatenate([oracle.matmul(dqx, v, bs[i] if bs else None) for i, v in enumerate(dq)], axis=1)
        scale = np.concatenate([_abs_scale(oracle, dqx, v) for v in dq], axis=1)
        print(f"{c.name} F3: {c.plan}: max {G.ulp_diff(got, want).max()} ulps, exact {(got == want).mean():.4f}")
        G.assert_sum_close(got, want, scale, rel=MX_ACC_REL, what=c.name)
    elif epi == "RESIDUAL":
        acc = oracle.matmul(dqx, dq[0])
        want = oracle.resadd(res, acc)
        sc = _abs_scale(oracle, dqx, dq[0])
        err = np.abs(G.bf(got).astype(np.float64) - G.bf(want))
        tol = 2.0 ** -7 * (np.abs(G.bf(acc).astype(np.float64)) + np.abs(G.bf(want))) + MX_ACC_REL * sc
        print(f"{c.name} F3: {c.plan}: max {G.ulp_diff(got, want).max()} ulps, worst error / bound {(err / tol).max():.3f}")
        assert (err <= tol).all(), c.name
    elif epi == "F32":
        exact = oracle.bf16_to_f32(dqx).astype(np.float64) @ oracle.bf16_to_f32(dq[0]).astype(np.float64).T
        sc = _abs_scale(oracle, dqx, dq[0])
        print(f"{c.name} F3: {c.plan}: max error {np.abs(got - exact).max():.3e}, {(np.abs(got - exact) / sc).max():.2e} of sum|a*w|")
        assert (np.abs(got - exact) <= MX_ACC_REL * sc + 1e-6).all(), c.name
    else:   # the epilogue on the kernel's own halves: STORE launches of the same kernel and split
        halves = []
        for (d, _), v in zip(dev_w, dq):
            if MC.is_t16(c):
                t = G.zeros((d.nbytes,), np.uint8)
                G.check(qlib.qie_fp8_tile16(G.p(d), N, K, G.p(t), None))
                d = t
            yh = G.zeros_bf16(M, N)
            _mx_linear(qlib, q, e, [(d, N)], [None], M, K, N, yh, _lib.QIE_EPI_STORE, MC.is_t16(c))
            halves.append(G.host_bf16(yh))
            G.assert_sum_close(halves[-1], oracle.matmul(dqx, v), _abs_scale(oracle, dqx, v), rel=MX_ACC_REL,
                               what=f"{c.name} gate/up half")
        d = G.ulp_diff(got, oracle.silu_mul(halves[0], halves[1]))
        print(f"{c.name} F3: {c.plan}: max {d.max()} ulps of silu_mul of the halves, exact {(d == 0).mean():.4f}")
        assert d.max() <= 1 and (d == 0).mean() > 0.99, f"{c.name}: SWIGLU epilogue: max {d.max()} ulps"

    # ---- isolation: one x row of NaN codes; 255 is the last row of the first 256-row tile
    r = 255 if (M > 256 and idx % 2 == 0) else M - 1
    run.with_nan_x_row(x, r)
    yr = run()
    run.frame_kept(yr)
    other = np.ones((M, N), bool)
    other[r] = False
    assert _is_nan(GC.live(c, yr)[r]).all(), f"{c.name}: row {r} of x is NaN, row {r} of y is not"
    assert np.array_equal(GC.bits(GC.live(c, yr))[other], GC.bits(got)[other]), f"{c.name}: a NaN in x row {r} reached other rows"

    # ---- one weight row of NaN codes: the last row of a segment (SWIGLU: of the gate)
    run = _Launch(qlib, c, x, ea, ws, scales, bs, y0)
    seg = 0 if epi == "SWIGLU" else idx % len(rows)
    n = int(np.cumsum(rows)[seg]) - 1 if epi != "SWIGLU" else N - 1
    run.with_nan_weight_row(ws, scales, seg, rows[seg] - 1)
    yn = run()
    run.frame_kept(yn)
    other = np.ones((M, N), bool)
    other[:, n] = False
    assert _is_nan(GC.live(c, yn)[:, n]).all(), f"{c.name}: weight row {n} is NaN, column {n} of y is not"
    assert np.array_equal(GC.bits(GC.live(c, yn))[other], GC.bits(got)[other]), f"{c.name}: a NaN weight row {n} reached other columns"


def _plus_zero(codes):
    return np.where(codes == 0x80, 0, codes).astype(np.uint8)


# (the quantisers do not know the split count: the rows up to two parts)
QUANT = [(c, f) for c in MC.CASES for f in ("F1", "F2") if not (f == "F2" and c.epi == "SWIGLU") and c.K <= 2176]


@pytest.mark.parametrize("case,fam", QUANT, ids=[f"{c.name}-{f}" for c, f in QUANT])
def test_quantisers_reproduce_the_cases(qlib, case, fam):
    """The F1 / F2 operands as bf16 values through qie_quantize_rows_fp8, qie_quantize_fp8 and
    qie_fp8_tile16: where the quantiser's scale rule (the smallest power of two that brings the
    row's largest magnitude to <= 448) picks the exponent the case uses, the codes are the
    case's bit for bit; where it picks a smaller one (F1's small integers, a needle), or 2^0 for
    an all-zero row, the dequantised values are the case's, exactly.  Zero codes are compared
    without their sign: the weight quantiser (e4m3_encode) writes 0x00 for -0, the row quantiser
    (v_cvt_pk_fp8_f32) keeps 0x80."""
    c = case
    inp = MC.inputs(c, fam)
    t = MC.e4m3_values()
    xv = MC.x_values(inp)
    q, e = _quant_dev(qlib, GC.to_bf16(xv))
    codes, ea = G.host(q).reshape(c.M, c.K), G.host(e)[:c.M]
    same = ea == inp.ea
    assert np.array_equal(_plus_zero(codes[same]), _plus_zero(inp.x[same]))
    assert np.array_equal(np.ldexp(t[codes], ea.astype(np.int32)[:, None] - 127), xv)
    n_same = [int(same.sum())]
    for w, s in zip(inp.ws, inp.ss):
        wv = np.ldexp(t[w], s.astype(np.int32)[:, None])
        rows = len(w)
        d, _ = _fp8w(qlib, GC.to_bf16(wv), False)
        blob = G.host(d)
        wc, sc = blob[:rows * c.K].reshape(rows, c.K), blob[rows * c.K:].view(np.float32)
        assert (sc.view(np.uint32) & 0x7FFFFF == 0).all() and (sc > 0).all()   # powers of two
        same = sc == np.ldexp(np.float32(1), s.astype(np.int32))
        assert np.array_equal(_plus_zero(wc[same]), _plus_zero(w[same]))
        assert np.array_equal(t[wc] * sc[:, None], wv)
        n_same.append(int(same.sum()))
        if MC.is_t16(c):
            assert np.array_equal(_tile16_dev(qlib, w, sc.copy()), MC.tile16(w))
    print(f"{c.name} {fam}: rows with the case's own exponent: x {n_same[0]} of {c.M}, weights {n_same[1:]}")
    if fam == "F2":   # rows that hold a code of 256 or more quantise to themselves
        big = (np.abs(t[inp.x]) >= 256).any(axis=1)
        assert big.sum() > c.M // 4 and (ea == inp.ea)[big].all()


SEQUENCE = (("mx", "mx_split2_store"), ("bf16", "split4_f32"), ("mx", "mx16_split4_swiglu"), ("bf16", "sk_c2_residual"),
            ("mx", "mx_split3_f32"), ("mx", "mx16_k3_residual"))


def test_mx_workspace_sequence(qlib):
    """gemm8mx_kernel shares g8_workspace (one slab and ticket set per stream, reallocated when
    it grows) and the ticket reset with the bf16 kernels.  On a fresh stream: mx split 2 -> bf16
    gemm8 split 4 -> mx split 4 -> stream-K ranges -> mx split 3 -> unsplit mx, each exact (F1)
    and bit-equal to the same launch made alone on the default stream."""
    table = {"mx": ({c.name: c for c in MC.CASES}, _exact), "bf16": ({c.name: c for c in GC.CASES}, _gemm_exact)}
    alone = {n: table[k][1](qlib, table[k][0][n], "F1") for k, n in SEQUENCE}
    st = G.stream()
    for k, n in SEQUENCE:
        y = table[k][1](qlib, table[k][0][n], "F1", stream=st)
        assert np.array_equal(GC.bits(y), GC.bits(alone[n])), f"{n}: differs after the launches before it"
