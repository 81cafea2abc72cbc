"""CPU: the MXFP4 format and the fp4 planner (no GPU).

  * qie_quantize_fp4_host equals weights.quantize_mxfp4 -- the rule of include/qie/qie_ops.h
    written down in numpy, independent of the C quantiser -- bit for bit: all-zero blocks, blocks
    with one outlier, every tie of the e2m1 grid, block maxima just under and over 6 * 2^k, the
    lower and upper scale clamps, the largest finite bf16 (finite in, finite out);
  * every dequantised value is a bf16 (zero low half as an f32);
  * qie_fp4_weight_bytes;
  * the planner: every row of tests/fp4_cases.py plans to the form it declares; over a grid of
    M x K x N x epilogue x norm with the fp4 flags every Dec4 form reached is some row's, and every
    shape not taken is an error line -- never another kernel's plan.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fp4_cases as FC
import linear_cases as LC

from qwen_inference_engine_amd import _lib, weights as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen_inference_engine_amd", "csrc")


def bf16(a):
    """float32 values that are exactly bf16 -> their bits."""
    b = np.ascontiguousarray(a, np.float32).view(np.uint32)
    assert not (b & 0xFFFF).any()
    return (b >> 16).astype(np.uint16)


def trunc_bf16(a):
    """float32 values truncated to bf16 bits."""
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def host_quantize(qlib, w):
    rows, cols = w.shape
    out = np.empty(int(qlib.qie_fp4_weight_bytes(rows, cols)), np.uint8)
    w = np.ascontiguousarray(w)
    assert qlib.qie_quantize_fp4_host(w.ctypes.data, rows, cols, out.ctypes.data) == 0, qlib.qie_last_error()
    return out


def assert_same(qlib, w, what):
    codes, exps = W.quantize_mxfp4(w)
    got = host_quantize(qlib, w)
    want = W.pack_mxfp4(codes, exps)
    n = w.size // 2
    assert np.array_equal(got[n:], want[n:]), f"{what}: block exponents differ"
    assert np.array_equal(got[:n], want[:n]), f"{what}: codes differ"
    return codes, exps


def test_weight_bytes(qlib):
    for rows, cols in [(1, 32), (7, 64), (33, 896), (5, 18944), (3584, 3584)]:
        assert qlib.qie_fp4_weight_bytes(rows, cols) == rows * cols // 2 + rows * cols // 32


def test_host_quantiser_equals_the_written_rule_on_random_weights(qlib):
    r = np.random.default_rng(4)
    for rows, cols, scale in [(7, 64, 0.05), (33, 896, 0.02), (5, 18944, 0.3), (16, 128, 40.0)]:
        w = trunc_bf16(r.standard_normal((rows, cols)) * scale)
        w[0, :32] = 0                                   # an all-zero block: exponent 127, codes 0
        w[1 % rows, 5] = trunc_bf16(np.array([1e4]))[0]   # one outlier
        codes, exps = assert_same(qlib, w, f"{rows}x{cols}")
        assert exps[0, 0] == 127 and not codes[0, :32].any()
        # the outlier's block: its own value is 3, 4 or 6 (amax / s in (3, 6]), nearly all others 0
        blk = codes[1 % rows, :32] & 7
        assert blk[5] in (5, 6, 7) and (np.delete(blk, 5) == 0).mean() > 0.9
        dq = W.dequantize_mxfp4(codes, exps)            # asserts the zero low halves itself
        assert np.isfinite((dq.astype(np.uint32) << 16).view(np.float32)).all()


def test_ties_go_to_the_even_code_index(qlib):
    """One block per scale: the value 6 pins s = 1 * 2^k, the ties sit beside it."""
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0]
    want_idx = [0, 2, 2, 4, 4, 6, 6]      # values 0, 1, 1, 2, 2, 4, 4
    for k in (-20, -1, 0, 3, 60):
        row = np.zeros(32, np.float32)
        row[0] = 6.0
        row[1:8] = ties
        row[8:15] = [-t for t in ties]
        w = bf16(row * np.float32(2.0 ** k)).reshape(1, 32)
        w[0, 15:22] = w[0, 1:8] + 1      # the next bf16 above each tie: the upper neighbour
        w[0, 22:29] = w[0, 1:8] - 1      # the next bf16 below: the lower neighbour
        codes, exps = assert_same(qlib, w, f"ties 2^{k}")
        assert exps[0, 0] == 127 + k
        assert list(codes[0, 1:8]) == want_idx
        assert list(codes[0, 8:15]) == [0] + [i | 8 for i in want_idx[1:]]   # -0.25 -> code 0: no negative zero
        assert list(codes[0, 15:22]) == [1, 2, 3, 4, 5, 6, 7]
        assert list(codes[0, 22:29]) == [0, 1, 2, 3, 4, 5, 6]


def test_block_maximum_around_six_times_a_power_of_two(qlib):
    for k in (-100, -3, 0, 5, 100):
        for f, e_want in [(6.0, k), (6.0 - 2.0 ** -5, k), (6.0 + 2.0 ** -5, k + 1), (3.0, k - 1),
                          (3.0 + 2.0 ** -6, k), (4.0, k), (8.0, k + 1)]:   # (the bf16 neighbours of 6 and 3)
            row = np.full(32, 2.0 ** (k - 2), np.float32)
            row[17] = -f * 2.0 ** k
            w = bf16(row).reshape(1, 32)
            codes, exps = assert_same(qlib, w, f"amax {f} * 2^{k}")
            assert exps[0, 0] == 127 + e_want, (f, k, exps[0, 0])
            assert (codes[0, 17] & 7) in (5, 6, 7) and codes[0, 17] & 8   # amax / s in (3, 6]: 3, 4 or 6
            # nothing saturates: the dequantised maximum is within half a grid step of the input
            dq = (W.dequantize_mxfp4(codes, exps).astype(np.uint32) << 16).view(np.float32)[0, 17]
            assert abs(dq - row[17]) <= 2.0 ** (e_want + 0)


def test_lower_scale_clamp_and_largest_bf16(qlib):
    # amax = 2^-130 (a subnormal bf16): the scale stops at 2^-125, the value rounds to code 0
    tiny = np.zeros((1, 32), np.uint16)
    tiny[0, 3] = 0x0008          # 2^-130
    tiny[0, 4] = 0x8040          # -2^-127: 0.25 * 2^-125 -> a tie -> code 0
    tiny[0, 5] = 0x0060          # 1.5 * 2^-127 = 0.375 * 2^-125 -> code 1 (0.5 * 2^-125 = 2^-126, normal)
    codes, exps = assert_same(qlib, tiny, "lower clamp")
    assert exps[0, 0] == 2 and list(codes[0, 3:6]) == [0, 0, 1]
    dq = W.dequantize_mxfp4(codes, exps)
    assert dq[0, 5] == 0x0080    # the smallest normal bf16: every non-zero output is normal
    # scales at the clamp itself and one above
    for bits, e in [(0x0200, 2), (0x0240, 2), (0x0280, 3)]:   # 2^-123 = 4 s, 6 s at s = 2^-125; 8 * 2^-125
        w = np.zeros((1, 32), np.uint16)
        w[0, 31] = bits
        _, exps = assert_same(qlib, w, hex(bits))
        assert exps[0, 0] == e
    # finite in, finite out: block maxima above 6 * 2^125 = 1.5 * 2^127 keep s = 2^125 (e8m0 252) and
    # saturate at code 6 -- at s = 2^126 the largest finite bf16 would round to 4 * 2^126 = inf
    big = np.zeros((3, 32), np.uint16)
    big[0, 0] = 0x7F7F           # the largest finite bf16
    big[0, 1] = 0xFF7F           # and its negative
    big[0, 2] = 0x7F00           # 2^127 = 4 * 2^125
    big[1, 0] = 0x7F40           # 1.5 * 2^127 = 6 * 2^125: the last maximum below the clamp
    big[1, 1] = 0xFF00           # -2^127
    big[2, 0] = 0x7F41           # the next bf16 above 6 * 2^125: the first saturated maximum
    codes, exps = assert_same(qlib, big, "largest bf16")
    assert list(exps[:, 0]) == [252, 252, 252]
    assert list(codes[0, :3]) == [7, 7 | 8, 6] and list(codes[1, :2]) == [7, 6 | 8] and codes[2, 0] == 7
    dq = W.dequantize_mxfp4(codes, exps)
    assert list(dq[0, :3]) == [0x7F40, 0xFF40, 0x7F00] and list(dq[1, :2]) == [0x7F40, 0xFF00] and dq[2, 0] == 0x7F40
    # every finite bf16 pattern as a block maximum gives finite values only
    allb = np.arange(0x7F80, dtype=np.uint16)
    w = np.zeros((len(allb), 32), np.uint16)
    w[:, 9] = allb
    w[:, 10] = allb | 0x8000
    codes, exps = assert_same(qlib, w, "every finite bf16")
    f = (W.dequantize_mxfp4(codes, exps).astype(np.uint32) << 16).view(np.float32)
    assert np.isfinite(f).all() and (exps >= 2).all() and (exps <= 252).all()


def test_dequantised_values_are_bf16_for_every_code_and_exponent():
    codes = np.tile(np.arange(16, dtype=np.uint8), 2).reshape(1, 32)
    for e in (2, 3, 120, 127, 134, 250, 252):
        dq = W.dequantize_mxfp4(codes, np.array([[e]], np.uint8))   # asserts the zero low halves
        v = (dq.astype(np.uint32) << 16).view(np.float32)[0, :16]
        want = np.array([0, .5, 1, 1.5, 2, 3, 4, 6, -0.0, -.5, -1, -1.5, -2, -3, -4, -6], np.float64) * 2.0 ** (e - 127)
        assert np.array_equal(v.astype(np.float64), want)
        nz = v[v != 0]
        assert (np.abs(nz) >= 2.0 ** -126).all() and np.isfinite(nz).all()


def test_quantiser_argument_checks(qlib):
    w = np.zeros((2, 48), np.uint16)
    out = np.zeros(64, np.uint8)
    assert qlib.qie_quantize_fp4_host(w.ctypes.data, 2, 48, out.ctypes.data) == -22   # cols % 32


# ---------------------------------------------------------------------------- the planner
GRID_UNITS = list(range(1, 65)) + [136, 148, 231]
GRID_N = [16, 40, 72, 2048, 18944, 32768]


@pytest.fixture(scope="module")
def plan_dump():
    subprocess.run(["make", "-s", "-C", CSRC, "plan_dump"], check=True, timeout=300)
    exe = os.path.join(ROOT, "qwen_inference_engine_amd", "_build", "plan_dump")

    def run(lines):
        r = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.splitlines()
        assert len(out) == len(lines)
        return [l.split(": ", 1)[1] for l in out]
    return run


def test_case_names_unique():
    names = [c.name for c in FC.CASES + FC.MANY_TILES]
    assert len(names) == len(set(names))


def test_every_case_plans_to_its_declared_form(plan_dump):
    cases = FC.CASES + FC.MANY_TILES
    for fl in (0, FC.FP4_T16):   # the tiled layout takes the same form where its segments are whole tiles
        sel = [c for c in cases if fl == 0 or all(r % 16 == 0 for r in c.segs)]
        got = plan_dump([LC.dump_line(c.name, c.M, c.K, c.segs, c.epi, c.norm, c.flags | fl) for c in sel])
        bad = [f"{c.name}: declares {c.plan}, plans {g}" for c, g in zip(sel, got)
               if g != f"{c.plan} t16={1 if fl else 0}"]
        assert not bad, "\n".join(bad)


def test_library_export_words_the_plan_as_plan_dump(plan_dump, qlib):
    dummy = (C.c_uint16 * 8)()
    ptr = C.addressof(dummy)
    buf = C.create_string_buffer(512)
    cases = FC.CASES + FC.MANY_TILES
    want = plan_dump([LC.dump_line(c.name, c.M, c.K, c.segs, c.epi, c.norm, c.flags) for c in cases])
    for c, w in zip(cases, want):
        a = _lib.LinearArgsC()
        n = LC.n_cols(c)
        a.x = a.y = ptr
        a.M, a.K, a.N, a.ldx, a.ldy, a.flags = c.M, c.K, n, c.K, n, c.flags
        a.epilogue = LC.EPIS.index(c.epi)
        for i, r in enumerate((n, n) if c.epi == "SWIGLU" else c.segs):
            a.w[i], a.seg_rows[i] = ptr, r
        a.norm_w = ptr if c.norm else None
        assert qlib.qie_debug_linear_plan(C.byref(a), buf, len(buf)) == 0
        assert buf.value.decode() == w and FC.plan_key(w) == c.plan, (c.name, buf.value, w)


def test_every_reachable_form_has_a_case_and_nothing_is_routed_elsewhere(plan_dump):
    shapes = [(M, 128 * u, N, e, norm, fl)
              for M in range(1, 17) for u in GRID_UNITS for N in GRID_N for e in LC.EPIS for norm in (0, 1)
              for fl in (FC.FP4, FC.FP4 | FC.FP4_T16)]
    got = plan_dump([LC.dump_line("g", M, K, (N,), e, norm, fl) for M, K, N, e, norm, fl in shapes])
    reached, refused = {}, 0
    for (M, K, N, e, norm, fl), g in zip(shapes, got):
        k = FC.plan_key(g)
        if k is None:
            assert g.startswith("error "), f"fp4 flags routed to another kernel: M={M} K={K} N={N} {e}: {g}"
            # what is refused: split-K with a norm or SwiGLU; tiled weights with a ragged last tile
            assert (K > 8192 and (norm or e == "SWIGLU")) or (fl & FC.FP4_T16 and N % 16), (M, K, N, e, norm, fl, g)
            refused += 1
        else:
            reached[k] = reached.get(k, 0) + 1
    print(f"{len(reached)} Dec4 forms reached by {len(shapes)} shapes, {refused} refused")
    # units 1..64 unsplit: KU 2 x KS 1..4, KU 4 x KS 3..8, KU 8 x KS 5..8; 136 / 148 / 231 units: 9 / 10 / 15 parts
    assert len(reached) == 17
    declared = {c.plan for c in FC.CASES}
    missing = sorted(set(reached) - declared)
    assert not missing, "reachable Dec4 forms without a case in tests/fp4_cases.py:\n" + "\n".join(missing)
    # the model widths the kernel must take unsplit with a fused norm, and their O / down projections
    need = [LC.dump_line("m", 1, K, (64,), "STORE", 1, FC.FP4) for K in (896, 3584, 8192, 5120)] + \
           [LC.dump_line("m", 8, K, (64,), "RESIDUAL", 0, FC.FP4) for K in (18944, 29568, 17408, 4864)]
    assert plan_dump(need) == ["dec4 KU=2 KS=4 parts=1 t16=0", "dec4 KU=4 KS=7 parts=1 t16=0",
                               "dec4 KU=8 KS=8 parts=1 t16=0", "dec4 KU=8 KS=5 parts=1 t16=0",
                               "dec4 KU=2 KS=8 parts=10 t16=0", "dec4 KU=2 KS=8 parts=15 t16=0",
                               "dec4 KU=2 KS=8 parts=9 t16=0", "dec4 KU=8 KS=5 parts=1 t16=0"]


def test_refused_shapes_plan_to_an_error(plan_dump):
    got = plan_dump([LC.dump_line(name, M, K, (N,), epi, norm, fl) for name, M, K, N, epi, norm, fl, _ in FC.REFUSALS])
    for (name, *_), g in zip(FC.REFUSALS, got):
        assert g.startswith("error "), (name, g)


def test_flags_zero_and_fp8_plan_as_before(plan_dump):
    """The fp4 branch sits in front of plan_linear: without its flags nothing may change.  A few of
    tests/linear_cases.py's rows (that file's own test covers all of them) plus fp8 Dec8 shapes."""
    rows = [c for c in LC.CASES][::7]
    got = plan_dump([LC.dump_line(c.name, c.M, c.K, c.segs, c.epi, c.norm, c.flags) for c in rows])
    assert all(g.startswith(c.plan + " ") for c, g in zip(rows, got))
    dec8 = plan_dump([LC.dump_line("d", 8, 3584, (512,), "STORE", 1, LC.FP8),
                      LC.dump_line("d", 8, 18944, (512,), "RESIDUAL", 0, LC.FP8)])
    assert dec8 == ["dec8 KU=8 KS=7 parts=1", "dec8 KU=4 KS=8 parts=10"]
