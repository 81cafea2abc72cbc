"""The fp8-activation prefill GEMM (QIE_LINEAR_ACT_FP8), one op-level case per reachable form.

gemm8mx_kernel<EPI, T16> (csrc/k_gemm.hip) takes e4m3 codes with one e8m0 exponent per
activation row and one power-of-two scale per weight row, reads plain or 16-row tiled weights,
runs 1..4 split-K parts and ends in the four epilogues: 32 forms.  Every row of CASES is a small
shape, the plan it gets on 256 CUs worded as tools/plan_dump prints it up to the grid, and what
the GPU test feeds it -- the protocol of tests/gemm_cases.py, whose helpers this module uses.
tests/test_mx_cases_cpu.py checks the declarations, that no reachable form lacks a row and that
the exact families reject every mutant; tests/test_gpu_mx_variants.py runs every row.

Plain data and numpy helpers: no test, no fixture.

Shapes.  plan_gemm splits where 2 * tiles <= CUs into min(4, k-tiles // 8) parts, so K = 2,176
(17 k-tiles of 128 codes: 8 + 9), 3,200 (25: 8 + 8 + 9) and 4,224 (33: 8 + 8 + 8 + 9) are the
smallest K with 2, 3 and 4 uneven parts; unsplit K = 128 is one k-tile (prologue and drain
only), 384 three (both buffers and the tail), 1,024 eight (the longest unsplit).  M = 257 or
300 (the second row tile has 1 or 44 live rows), N ends inside a column tile; plain weights cut
their segments inside a 16-column fragment (200, 40, 24), tiled weights (whole 16-row tiles per
segment) off multiples of 64 (208, 48, 16).  "m5" rows are a single tile nearly all clamped
(the prefill_fp8 engine sends short prompts here), "noclamp" has M and N whole multiples of 256.

Operands are fed as codes (inputs()): x e4m3 codes [M, K] with exponents
ea[m] = 127 + (7 m) % 41 - 20 and weight row n = codes * 2^s[n], s[n] = (7 n) % 25 - 12.
7 d is no multiple of 41 or 25 for d = 1, 16, 64, 128, so no row or column agrees with its
neighbour at those distances: the byte maps of sa_pk / sb_pk (row 128 wm + 64 qa + 16 i + fr,
column 64 wn + 32 qb + 16 j + fr) and the clamped reads of ea and of the scales are pinned.
SWIGLU rows use ea[m] = 127 + (7 m) % 29 - 4, gate scales (7 n) % 9 + 4 and up scales
(7 n + 11) % 25 - 12 (the same property): the gate's combined exponent is >= 0, and the product
of gate and up stays a finite bf16 (exponents up to 2 * 24 + 24, sums below 2^17 each).

  F1  scaled integers, all four epilogues.  Codes are the integers of gemm_cases F1 ([-4, 4];
      SWIGLU x and gate side [1, 4]) as e4m3, so sum = 2^(ea[m] - 127 + s[n]) * integer with
      every k contributing.  Exact if the instruction adds 128 integer products to an integer
      accumulator without losing a bit: MEASURED, not assumed -- tools/mx_mfma_probe.hip
      (profiles/mx_mfma_probe_integers.txt) adds products in [-16, 16] to accumulator inputs of
      up to 2^L, with unit and with row / column scales: no wrong element of 6,144 for every
      L <= 23, 738 wrong at L = 24.  So L = EXACT_L = 23, and every row keeps
      range^2 * K < 2^23 (asserted; [-4, 4] holds it for every K here: 16 * 4,224 < 2^17).  The
      split-K merge adds such partial sums in fp32: integers below 2^24 times one power of two.
      STORE adds a bias per column: 2^s[n] * integer, and in every fourth column the bias that
      makes one element 257 / 259 times a power of two (both round-to-nearest-even ties occur in
      every row of the table, M = 5 included); RESIDUAL adds 2^e * [-8, 8] to bf16(acc);
      SWIGLU gates are >= 2^0 * K >= 128, where silu(g) rounds to g whatever the formula.
  F2  scaled needles (STORE without bias, RESIDUAL onto zeros, F32).  Weight row n holds one
      nonzero code (any of the 252 finite nonzero e4m3 codes, subnormals and both signs) at
      column perm(n) of K; x holds random codes over all 254 non-NaN values.  Then
      y[m, n] = c * v * 2^(ea[m] - 127 + s[n]): exact in fp32 (the product of two e4m3 values
      has at most 8 significant bits) and whatever the instruction's internal precision, one
      nonzero term per sum (the probe's "needles" line: 0 wrong of 4,096).  Needles sit at
      k = 0, K - 1, both sides of every split-K cut, of every 128-code k-tile edge and, as far
      as the columns reach, of every 32-code fragment edge (the 2g, 2g + 1 chunk pairs); one x
      row and one weight row are all zero.
  F3  random, through the quantisers (the GPU test holds it: it needs the oracle).

accepted() compares bit for bit after mapping -0 to +0 in the result and in the answer, the only
normalisation: a sum whose every product is zero is a zero whose sign depends on the signs of
the zero products and on the order they meet the +0 accumulator (and the split-K slabs), which
no reference fixes; every nonzero result has one right sign.

model() is the reference as one float32 product of the dequantised operands (exact on F1 / F2)
with MUTANTS: gemm_cases' ten (k-tile = 128 codes) and the ways this kernel can be subtly wrong.
"""
import collections
import functools
import re

import numpy as np

import gemm_cases as GC
from gemm_cases import C, EPIS, n_cols

FP8, T16, ACT_FP8 = 1, 16, 32   # QIE_LINEAR_*
PLAIN, TILED = FP8 | ACT_FP8, FP8 | T16 | ACT_FP8
BK = 128                        # codes per k-tile
EXACT_L = 23                    # profiles/mx_mfma_probe_integers.txt: "largest exact L: 23"
NAN_CODE = 0x7F


def mx(e, t16, n_mt, tiles, splitk=1):
    ws = f"slabs={tiles * splitk} tickets={tiles}" if splitk > 1 else "slabs=0 tickets=0"
    return f"gemm8mx_kernel<{e},{t16}> splitk={splitk} n_mt={n_mt} tiles={tiles} {ws}"


def _family(tag, t16, M, K, splitk=1, **kw):
    """One row per epilogue at (M, K): plain segments (200, 40, 24), tiled (208, 48, 16); SWIGLU
    264 / 272 outputs (528 / 544 weight rows: three column tiles); pads on every other row."""
    segs, I = ((208, 48, 16), 272) if t16 else ((200, 40, 24), 264)
    n_mt = -(-M // 256)
    rows = []
    for i, e in enumerate(EPIS):
        s = I if e in ("SWIGLU", "RESIDUAL") else (segs if e == "STORE" else sum(segs))
        tiles = n_mt * (3 if e == "SWIGLU" else 2)
        pads = dict(ldx_pad=16 * (1 + i % 3), ldy_pad=(3, 1, 5, 2)[i % 4]) if (i + t16 + splitk) % 2 == 0 else {}
        rows.append(C(f"{tag}_{e.lower()}", M, K, s, e, mx(e, t16, n_mt, tiles, splitk), flags=TILED if t16 else PLAIN,
                      bias=(e == "STORE"), twice=splitk > 1, **pads, **kw))
    return rows


CASES = tuple(
    r for t16, t in ((0, "mx_"), (1, "mx16_"))
    for r in (
        # unsplit: 1, 3 and 8 k-tiles
        _family(f"{t}k1", t16, 257, 128) + _family(f"{t}k3", t16, 300, 384) + _family(f"{t}k8", t16, 257, 1024)
        # split-K: 2, 3 and 4 uneven parts
        + _family(f"{t}split2", t16, 257, 2176, 2) + _family(f"{t}split3", t16, 300, 3200, 3)
        + _family(f"{t}split4", t16, 257, 4224, 4))
) + (
    # one tile nearly all clamped: 5 live rows
    C("mx_m5_store", 5, 384, (200, 40, 24), "STORE", mx("STORE", 0, 1, 2), flags=PLAIN, bias=True, ldy_pad=1),
    C("mx16_m5_swiglu", 5, 1024, 272, "SWIGLU", mx("SWIGLU", 1, 1, 3), flags=TILED, ldx_pad=16),
    # M and N whole multiples of 256: no clamped row or column anywhere
    C("mx_noclamp", 512, 384, (256, 128, 128), "STORE", mx("STORE", 0, 2, 4), flags=PLAIN, bias=True),
)

_FORM = re.compile(r"(gemm8mx_kernel<\w+,\d>) splitk=(\d+)")


def form_key(text):
    """gemm_cases.form_key's sibling: (instantiation, splitk) of a gemm8mx_kernel plan line,
    None for any other plan."""
    m = _FORM.match(text)
    return (m.group(1), int(m.group(2))) if m else None


def is_t16(c):
    return bool(c.flags & T16)


def split_of(c):
    return form_key(c.plan)[1]


def cut_tiles(c):
    """k-tile indices (128 codes each) where a split-K part begins: part p of s covers k-tiles
    [p nk / s, (p + 1) nk / s)."""
    nk, s = c.K // BK, split_of(c)
    return sorted({p * nk // s for p in range(1, s)})


# ---------------------------------------------------------------------------- exponents, scales
def x_exps(c):
    """e8m0 exponents of the M activation rows."""
    m = np.arange(c.M)
    return (127 + ((7 * m) % 29 - 4 if c.epi == "SWIGLU" else (7 * m) % 41 - 20)).astype(np.uint8)


def w_scale_exps(c):
    """log2 of the scale of every weight row, in segment order (SWIGLU: gate rows, then up rows)."""
    n = np.arange(n_cols(c))
    if c.epi == "SWIGLU":
        return np.concatenate([(7 * n) % 9 + 4, (7 * n + 11) % 25 - 12])
    return (7 * n) % 25 - 12


_TABLE = None


def e4m3_values():
    """float32 value of every e4m3 code (0x7F / 0xFF: NaN)."""
    global _TABLE
    if _TABLE is None:
        from qwen_inference_engine_amd.weights import e4m3_table
        _TABLE = e4m3_table()
    return _TABLE


def codes_of_ints(a):
    """The e4m3 codes of integers in [-16, 16]."""
    t = e4m3_values()
    lut = np.zeros(33, np.uint8)
    for v in range(-16, 17):
        hit = [k for k in range(256) if t[k] == v and not (v == 0 and k)]
        lut[v + 16] = hit[0]
    return lut[np.asarray(a, np.int64) + 16]


def tile16(codes):
    """[rows, K] codes -> the 16-row tiled layout of qie_ops.h (QIE_LINEAR_FP8_T16), as
    [rows, K] bytes: block (t, j) holds row 16 t + l % 16, columns 64 j + 16 (l / 16) + [0, 16)
    at bytes [16 l, 16 l + 16)."""
    rows, K = codes.shape
    return np.ascontiguousarray(codes.reshape(rows // 16, 16, K // 64, 4, 16).transpose(0, 2, 3, 1, 4)).reshape(rows, K)


# ---------------------------------------------------------------------------- inputs
Inputs = collections.namedtuple("Inputs", "x ea ws ss bs res y0")
"""x [M, K] e4m3 codes; ea [M] e8m0 exponents; ws: plain codes per segment (SWIGLU: gate, up);
ss: log2 of the row scales per segment; bs: bf16 bits per segment or []; res [M, N] bf16 bits or
None; y0: the framed output (gemm_cases.frame)."""


def segments(c):
    N = n_cols(c)
    return (N, N) if c.epi == "SWIGLU" else c.segs


def x_values(inp):
    """What the codes and exponents of x stand for, float32 (exact)."""
    return np.ldexp(e4m3_values()[inp.x], inp.ea.astype(np.int32)[:, None] - 127)


def w_values(inp):
    return np.ldexp(e4m3_values()[np.concatenate(inp.ws)], np.concatenate(inp.ss).astype(np.int32)[:, None])


def out_exps(c, inp):
    """ea[m] - 127 + s[n] per accumulator [M, weight rows]."""
    return (inp.ea.astype(np.int32)[:, None] - 127) + np.concatenate(inp.ss).astype(np.int32)[None, :]


def int_range(c):
    """F1's largest integer: the first of 4, 2, 1 with range^2 * K < 2^EXACT_L."""
    return next(r for r in (4, 2, 1) if r * r * c.K < (1 << EXACT_L))


def perm(c, cols):
    """F2: `cols` needle columns of K (gemm_cases.place_needles: all of the first list, of the
    32-code fragment edges as many as the columns reach)."""
    K = c.K
    want = [0, K - 1]
    for t in cut_tiles(c):
        want += [BK * t - 1, BK * t]
    want += [k for e in range(BK, K, BK) for k in (e - 1, e)]
    return GC.place_needles(c, cols, want, [k for e in range(32, K, 32) for k in (e - 1, e)])


def zero_rows(c):
    """F2's all-zero x row and all-zero weight row."""
    return min(c.M - 1, 19), 37


@functools.lru_cache(maxsize=8)
def inputs(c, fam):
    """The inputs of family "F1" / "F2" for row c (deterministic by name; treat as read-only)."""
    M, K, N = c.M, c.K, n_cols(c)
    r = np.random.default_rng(GC.seed_of(c, fam))
    sw = c.epi == "SWIGLU"
    rows = segments(c)
    ea, s_all = x_exps(c), w_scale_exps(c)
    ss = [s_all[o - n:o] for n, o in zip(rows, np.cumsum(rows))]
    bs, res = [], None
    if fam == "F1":
        R = int_range(c)
        assert R * R * K < (1 << EXACT_L)
        lo = 1 if sw else -R
        xi = r.integers(lo, R + 1, (M, K))
        wi = [r.integers(lo if (sw and i == 0) else -R, R + 1, (n, K)) for i, n in enumerate(rows)]
        x, ws = codes_of_ints(xi), [codes_of_ints(w) for w in wi]
        e = (ea.astype(np.int64)[:, None] - 127) + s_all[None, :]
        if c.epi == "STORE":
            # per column 2^s[n] * an integer of [-255, 255]; every fourth column: the bias that
            # makes element (m, n) +-257 or +-259 times 2^e[m, n] (a tie of either kind)
            acc = xi.astype(np.float64) @ np.concatenate(wi).astype(np.float64).T
            b = np.ldexp(r.integers(-255, 256, N).astype(np.float64), s_all)
            for j, n in enumerate(range(0, N, 4)):
                t = (257, 259)[j % 2] * np.where(acc[:, n] >= 0, 1, -1)
                ok = np.nonzero((t != acc[:, n]) & (np.abs(t - acc[:, n]) <= 255))[0]   # the bias is a bf16
                m = ok[(11 * j) % len(ok)]
                b[n] = np.ldexp(t[m] - acc[m, n], int(e[m, n]))
            b64, b = b, GC.to_bf16(b.astype(np.float32))
            assert np.array_equal(GC.bf(b).astype(np.float64), b64)
            bs = [b[o - n:o] for n, o in zip(rows, np.cumsum(rows))]
        if c.epi == "RESIDUAL":
            res = GC.to_bf16(np.ldexp(r.integers(-8, 9, (M, N)).astype(np.float32), e.astype(np.int32)))
    elif fam == "F2":
        assert not sw, "F2 has no SWIGLU form"
        x = r.integers(0, 254, (M, K)).astype(np.uint8)
        x = (x + (x >= 0x7F)).astype(np.uint8)            # 0x00 .. 0xFE without 0x7F
        mz, nz = zero_rows(c)
        x[mz] = 0
        needle = r.integers(0, 252, N).astype(np.uint8)   # 0x01 .. 0x7E, 0x81 .. 0xFE
        needle = (1 + needle + 2 * (needle >= 126)).astype(np.uint8)
        p = perm(c, N - 1)
        W = np.zeros((N, K), np.uint8)
        live = np.delete(np.arange(N), nz)
        W[live, p] = needle[live]
        ws = [W[o - n:o] for n, o in zip(rows, np.cumsum(rows))]
        if c.epi == "RESIDUAL":
            res = np.zeros((M, N), np.uint16)
    else:
        raise ValueError(fam)
    return Inputs(x, ea, ws, ss, bs, res, GC.frame(c, res))


def blob(c, codes, s):
    """A weight segment as the kernel reads it: codes (tiled for T16 rows), then the fp32 row
    scales 2^s."""
    q = tile16(codes) if is_t16(c) else codes
    return np.concatenate([q.reshape(-1), np.ldexp(np.float32(1), s.astype(np.int32)).astype(np.float32).view(np.uint8)])


# ---------------------------------------------------------------------------- the answers
def expected(c, fam, inp):
    """The one right live region [M, N] of F1 / F2, computed apart from model(): F1 a float64
    product of the integers, scaled; F2 the gathered needles."""
    t = e4m3_values()
    e = out_exps(c, inp)
    if fam == "F1":
        acc = t[inp.x].astype(np.float64) @ t[np.concatenate(inp.ws)].astype(np.float64).T
        assert np.abs(acc).max() < (1 << EXACT_L)
        return GC._finish(c, np.ldexp(acc, e).astype(np.float32), inp)
    W = np.concatenate(inp.ws)
    p = (W != 0).argmax(axis=1)
    prod = t[inp.x][:, p].astype(np.float64) * t[W[np.arange(len(p)), p]].astype(np.float64)[None, :]
    acc = np.ldexp(prod, e)
    assert np.array_equal(acc.astype(np.float32).astype(np.float64), acc)
    return GC._finish(c, acc.astype(np.float32), inp)


MX_MUTANTS = ("exp_row_16", "exp_row_64", "exp_row_clamped", "scale_col_16", "scale_prev_segment", "a_chunks_swapped",
              "t16_row_off_by_one", "a_exp_twice", "a_exp_dropped", "b_scale_twice", "b_scale_dropped")
MUTANTS = GC.MUTANTS + MX_MUTANTS


def model(c, inp, mut=None):
    """The framed output of row c on F1 / F2 inputs as one float32 product of the dequantised
    operands, with one way of being subtly wrong: gemm_cases.model's ten (the k-tile is 128
    codes, the cuts this kernel's), or
      exp_row_16 / exp_row_64  the rows of every second 16-row fragment / 64-row half take the
                          exponent of the row 16 / 64 above (a wrong byte of sa_pk);
      exp_row_clamped     the live rows of the last row tile take the exponent of row M - 1,
                          which the clamped rows read;
      scale_col_16        every second 16-column fragment takes the scales 16 columns before;
      scale_prev_segment  a segment's first row takes the scale of the previous segment's last;
      a_chunks_swapped    the two 16-byte chunks of every 32-code fragment of A exchanged;
      t16_row_off_by_one  tiled weights gathered one row off within their 16-row block;
      a_exp_twice / a_exp_dropped / b_scale_twice / b_scale_dropped
                          the scale exponent of one side applied twice / not at all."""
    assert mut is None or mut in MUTANTS, mut
    M, K = c.M, c.K
    ea = inp.ea.astype(np.int32) - 127
    s = np.concatenate(inp.ss).astype(np.int32)
    X, Wc = inp.x, np.concatenate(inp.ws)
    m, n = np.arange(M), np.arange(len(s))
    if mut == "exp_row_16":
        ea = np.where((m // 16) % 2 == 1, ea[np.maximum(m - 16, 0)], ea)
    elif mut == "exp_row_64":
        ea = np.where((m // 64) % 2 == 1, ea[np.maximum(m - 64, 0)], ea)
    elif mut == "exp_row_clamped":
        ea = np.where(m >= (M - 1) // 256 * 256, ea[M - 1], ea)
    elif mut == "scale_col_16":
        s = np.where((n // 16) % 2 == 1, s[np.maximum(n - 16, 0)], s)
    elif mut == "scale_prev_segment" and len(segments(c)) > 1:
        s = s.copy()
        s[segments(c)[0]] = s[segments(c)[0] - 1]
    elif mut == "a_chunks_swapped":
        X = X[:, np.arange(K) ^ 16]
    elif mut == "t16_row_off_by_one" and is_t16(c):
        Wc = Wc[(n & ~15) | ((n + 1) & 15)]
    elif mut in ("a_exp_twice", "a_exp_dropped"):
        ea = ea * (2 if mut == "a_exp_twice" else 0)
    elif mut in ("b_scale_twice", "b_scale_dropped"):
        s = s * (2 if mut == "b_scale_twice" else 0)
    t = e4m3_values()
    x = np.ldexp(t[X], ea[:, None])
    W = np.ldexp(t[Wc], s[:, None])
    cuts = cut_tiles(c)
    with np.errstate(over="ignore", invalid="ignore"):   # a doubled exponent may overflow a bf16: still rejected
        return GC.model_of(c, inp, x, W, BK, cuts[0] if cuts else None, mut)


def no_negative_zero(a):
    """-0 -> +0 (bf16 bits or float32)."""
    if a.dtype == np.float32:
        u = a.view(np.uint32).copy()
        u[u == 0x80000000] = 0
        return u.view(np.float32)
    a = a.copy()
    a[a == 0x8000] = 0
    return a


def accepted(c, y, y0, want):
    """gemm_cases.accepted (the frame untouched, the live region bit-equal to `want`) after -0
    -> +0 in the live region and in `want`: see the module docstring.  Returns (ok, words)."""
    M, N = c.M, n_cols(c)
    y = y.copy()
    y[1:M + 1, :N] = no_negative_zero(GC.live(c, y))
    return GC.accepted(c, y, y0, no_negative_zero(np.ascontiguousarray(want)))
