"""The prefill GEMMs (M > 16), one op-level case per kernel instantiation and split form.

plan_gemm() (csrc/gemm_plan.hpp) chooses among gemm_kernel, gemm_big_kernel, gemm8_kernel (1..4
split-K parts) and gemm8sk_kernel (stream-K) by shape and flag.  Every row of CASES is a small
shape, the plan that shape gets on 256 CUs with the shipped knobs, worded as tools/plan_dump
prints it up to the grid, and what the GPU test feeds it.  tests/test_gemm_cases_cpu.py checks
the declarations against plan_dump, that no reachable form lacks a row, and that the exact
families below reject every mutant of the reference; tests/test_gpu_gemm_variants.py runs every
row in three input families.  The fp8-activation kernel (gemm8mx_kernel) has its own table under
the same protocol: tests/mx_cases.py, tests/test_mx_cases_cpu.py, tests/test_gpu_mx_variants.py.

Plain data and numpy helpers: no test, no fixture.

Shapes: the smallest that reach the form, ragged on purpose: M = 257 or 300 (the second row tile
has 1 or 44 live rows, the rest re-read row M-1), N that ends inside a tile (columns past N
re-read weight row N-1), segment boundaries inside a 16-column fragment, K with a ragged last
k-tile where the kernel allows one.  One row ("noclamp") has M and N whole multiples of 256.

Input families (inputs(), expected()):
  F1  integers.  x and w are integers in [-4, 4] stored as bf16, so |sum| <= 16 K < 2^24 and
      every fp32 summation order gives the same integer: each epilogue has ONE right answer, and
      every k contributes to it.  STORE adds an integer bias (257 -> 256 and 259 -> 260: both
      ties of round-to-nearest-even occur); RESIDUAL adds a small integer residual to bf16(acc);
      SWIGLU has x and the gate weights in [1, 4], so every gate sum is >= K >= 32, where
      silu(g) rounds to g whatever the formula, and the answer is bf16(bf16(up) * bf16(gate)).
  F2  needles.  Weight row n is +-2^e (e in [-2, 2]) at column perm(n) and zero elsewhere, x is
      random finite bf16 bit patterns (2^-20 <= |x| < 2^21): y[m, n] = x[m, perm(n)] * 2^e bit for
      bit (STORE without bias, RESIDUAL onto zeros, F32; not SWIGLU).  perm() puts needles at k = 0,
      k = K-1, both sides of every split-K part and stream-K range cut and, as far as the
      columns reach, both sides of every k-tile edge; the rest are spread over all of K.
  F3  random, drawn as tests/test_gpu_ops.py draws (the GPU test holds it: it needs the oracle).

model() is the reference of F1 / F2 as one float32 product (exact on these inputs) with the
MUTANTS below, the usual ways such a kernel is subtly wrong; accepted() is the one acceptance
function of the GPU test and of the CPU mutant test.
"""
import collections
import re
import zlib

import numpy as np

FP8, TILE256, TILE128, STREAMK = 1, 2, 4, 8   # QIE_LINEAR_*
EPIS = ("STORE", "RESIDUAL", "SWIGLU", "F32")
NAN_BF16 = 0x7FC0

Case = collections.namedtuple("Case", "name M K segs epi plan flags ldx_pad ldy_pad bias twice")


def C(name, M, K, segs, epi, plan, flags=0, ldx_pad=0, ldy_pad=0, bias=False, twice=False):
    """segs: rows per weight segment (SWIGLU: (I,), gate and up have I rows each); ldx_pad (a
    multiple of 8) / ldy_pad (any): elements beyond K / N in a row of x / y; bias: F3 has one bias
    per segment (F1 STORE always has an integer bias); twice: split-K / stream-K -- two launches
    into fresh outputs must agree bit for bit."""
    segs = (segs,) if isinstance(segs, int) else tuple(segs)
    return Case(name, M, K, segs, epi, plan, flags, ldx_pad, ldy_pad, bias, twice)


def n_cols(c):
    return sum(c.segs)


# ---------------------------------------------------------------------------- plan wording
def generic(e, wt, gm, gn):
    return f"gemm_kernel<{e},{wt}> n_mt={gm} tiles={gm * gn} slabs=0 tickets=0"


def big(e, bn, n_mt, tiles):
    return f"gemm_big_kernel<{e},{bn}> n_mt={n_mt} tiles={tiles} slabs=0 tickets=0"


def g8(e, n_mt, tiles, splitk=1):
    ws = f"slabs={tiles * splitk} tickets={tiles}" if splitk > 1 else "slabs=0 tickets=0"
    return f"gemm8_kernel<{e}> splitk={splitk} n_mt={n_mt} tiles={tiles} {ws}"


def sk(e, dp, chunk, n_mt, tiles):
    return f"gemm8sk_kernel<{e}> dp_rounds={dp} chunk={chunk} n_mt={n_mt} tiles={tiles} slabs=512 tickets={tiles}"


def _pads(i):   # pads for a quarter of the rows of a family, every family gets some
    return dict(ldx_pad=8 * (1 + i % 3), ldy_pad=(3, 1, 5, 2)[i % 4])


def _four(tag, rows, **kw):
    """One row per epilogue: rows maps the epilogue to (M, K, segs, plan)."""
    return [C(f"{tag}_{e.lower()}", *rows[e][:3], e, rows[e][3], bias=(e == "STORE"), **kw, **(_pads(i) if i % 2 == 0 else {}))
            for i, e in enumerate(EPIS)]


CASES = (
    # ------------------------------------------------------------------ generic 128x128 kernel,
    # bf16 weights: K with a ragged last k-tile (72 = 64 + 8, 200 = 192 + 8, 40), 1 / 2 / 3 row
    # tiles, the last column tile partly filled
    _four("gen", {"STORE": (17, 72, (100, 20, 10), generic("STORE", 0, 1, 2)),
                  "RESIDUAL": (129, 72, 130, generic("RESIDUAL", 0, 2, 2)),
                  "SWIGLU": (255, 200, 136, generic("SWIGLU", 0, 2, 3)),
                  "F32": (300, 40, 200, generic("F32", 0, 3, 2))})
    # ------------------------------------------------------------------ generic kernel, fp8
    # weights decoded on the way into LDS (the quantiser takes K % 16 == 0: 208 = 192 + 16, 80)
    + _four("fp8", {"STORE": (129, 208, (200, 40, 24), generic("STORE", 1, 2, 3)),
                    "RESIDUAL": (129, 208, 130, generic("RESIDUAL", 1, 2, 2)),
                    "SWIGLU": (300, 896, 320, generic("SWIGLU", 1, 3, 5)),
                    "F32": (33, 80, 136, generic("F32", 1, 1, 2))}, flags=FP8)
    # ------------------------------------------------------------------ LDS-DMA ring kernel,
    # 256x128 tiles chosen by count (192 <= tiles <= 256): K = 896 is 28 ring k-tiles (too few
    # 256x256 tiles for gemm8 unsplit), K = 96 three: prologue and drain only
    + _four("big128", {"STORE": (257, 96, (12000, 100, 100), big("STORE", 128, 2, 192)),
                       "RESIDUAL": (257, 896, 12200, big("RESIDUAL", 128, 2, 192)),
                       "SWIGLU": (257, 96, 6100, big("SWIGLU", 128, 2, 192)),
                       "F32": (257, 96, 12200, big("F32", 128, 2, 192))})
    # ... 256x256 tiles chosen by count: one round (130 tiles, 128-column tiles would take two)
    # and a full chip (256); grids that are no multiple of 8 through the XCD remap
    + _four("big256", {"STORE": (257, 96, (16000, 200, 200), big("STORE", 256, 2, 130)),
                       "RESIDUAL": (257, 96, 16400, big("RESIDUAL", 256, 2, 130)),
                       "SWIGLU": (257, 96, 16356, big("SWIGLU", 256, 2, 256)),
                       "F32": (257, 96, 16400, big("F32", 256, 2, 130))})
    # ------------------------------------------------------------------ phase-interleaved
    # 256x256 kernel unsplit, by count: half a chip (128 tiles) and a full one (256); K = 256 is
    # its shortest pipeline, 4 k-tiles
    + _four("g8", {"STORE": (257, 256, (16000, 200, 128), g8("STORE", 2, 128)),
                   "RESIDUAL": (257, 256, 32712, g8("RESIDUAL", 2, 256)),
                   "SWIGLU": (257, 256, 8164, g8("SWIGLU", 2, 128)),
                   "F32": (257, 256, 16328, g8("F32", 2, 128))})
    # ... split-K: 2 uneven parts (129 k-tiles: 64 + 65), 3 parts (193: 64 + 64 + 65), 4 parts
    # (257: 64 + 64 + 64 + 65); 2 x 2 tiles, SwiGLU's 528 weight rows 2 x 3
    + [r for s, K in ((2, 8256), (3, 12352), (4, 16448))
       for r in _four(f"split{s}", {"STORE": (257, K, (200, 40, 24), g8("STORE", 2, 4, s)),
                                    "RESIDUAL": (257, K, 264, g8("RESIDUAL", 2, 4, s)),
                                    "SWIGLU": (257, K, 264, g8("SWIGLU", 2, 6, s)),
                                    "F32": (257, K, 264, g8("F32", 2, 4, s))}, twice=True)]
    # ------------------------------------------------------------------ stream-K.  One k-tile per
    # workgroup (the existing tests' form): 4 tiles of 14 k-tiles, 56 segments
    + _four("sk_c1", {"STORE": (300, 896, (200, 72, 48), sk("STORE", 0, 1, 2, 4)),
                      "RESIDUAL": (300, 896, 320, sk("RESIDUAL", 0, 1, 2, 4)),
                      "SWIGLU": (300, 896, 160, sk("SWIGLU", 0, 1, 2, 4)),
                      "F32": (300, 896, 320, sk("F32", 0, 1, 2, 4))}, flags=STREAMK, twice=True)
    # ranges of 2 k-tiles over 12 tiles of 35: every 18th range ends one tile and begins the
    # next (slab slot 0 and 1), tiles are summed from 18 or 19 segments, pipeline runs of 1 and 2
    + _four("sk_c2", {"STORE": (300, 2240, (1000, 300, 100), sk("STORE", 0, 2, 2, 12)),
                      "RESIDUAL": (300, 2240, 1400, sk("RESIDUAL", 0, 2, 2, 12)),
                      "SWIGLU": (300, 2240, 700, sk("SWIGLU", 0, 2, 2, 12)),
                      "F32": (300, 2240, 1400, sk("F32", 0, 2, 2, 12))}, flags=STREAMK, twice=True)
    # a whole-tile round of 256, then 144 tiles of 4 k-tiles in ranges of 3 (runs of 1, 2 and 3)
    + _four("sk_dp_c3", {"STORE": (257, 256, (51000, 60, 40), sk("STORE", 1, 3, 2, 400)),
                         "RESIDUAL": (257, 256, 51100, sk("RESIDUAL", 1, 3, 2, 400)),
                         "SWIGLU": (257, 256, 25550, sk("SWIGLU", 1, 3, 2, 400)),
                         "F32": (257, 256, 51100, sk("F32", 1, 3, 2, 400))}, flags=STREAMK, twice=True)
    # a whole-tile round, then 2 tiles in 8 ranges of one k-tile
    + _four("sk_dp_c1", {"STORE": (257, 256, (32000, 900, 100), sk("STORE", 1, 1, 2, 258)),
                         "RESIDUAL": (257, 256, 33000, sk("RESIDUAL", 1, 1, 2, 258)),
                         "SWIGLU": (257, 256, 16500, sk("SWIGLU", 1, 1, 2, 258)),
                         "F32": (257, 256, 33000, sk("F32", 1, 1, 2, 258))}, flags=STREAMK, twice=True)
    # ------------------------------------------------------------------ forced tiles, as
    # test_gemm_plan_cpu.py rows t256, t256_k96, t128 (streamk: sk_c1_residual above)
    + [C("t256", 300, 896, 320, "RESIDUAL", g8("RESIDUAL", 2, 4), flags=TILE256),
       C("t256_k96", 300, 96, 320, "RESIDUAL", big("RESIDUAL", 256, 2, 4), flags=TILE256, ldy_pad=1),
       C("t128", 300, 896, 320, "RESIDUAL", big("RESIDUAL", 128, 2, 6), flags=TILE128, ldx_pad=8),
       # M and N whole multiples of 256: no clamped row or column anywhere
       C("noclamp", 512, 256, (256, 128, 128), "STORE", g8("STORE", 2, 4), flags=TILE256, bias=True)]
)

# ---------------------------------------------------------------------------- plan_dump helpers
_FORM = re.compile(r"(gemm8sk_kernel<\w+>) dp_rounds=(\d+) chunk=(\d+)|(gemm8_kernel<\w+>) splitk=(\d+)|"
                   r"(gemm_big_kernel<\w+,\d+>|gemm_kernel<\w+,\d>)")


def form_key(text):
    """What the coverage rule counts of a plan line: (instantiation, splitk) for gemm8_kernel,
    (instantiation, dp_rounds > 0, chunk > 1) for stream-K, the instantiation otherwise; None for
    other plans (gemm8mx_kernel: mx_cases.form_key; the M <= 16 kernels: linear_cases)."""
    m = _FORM.match(text)
    if not m:
        return None
    if m.group(1):
        return (m.group(1), int(m.group(2)) > 0, int(m.group(3)) > 1)
    if m.group(4):
        return (m.group(4), int(m.group(5)))
    return (m.group(6),)


def dump_line(name, M, K, segs, epi, flags):
    n = sum(segs)
    seg = f"{n},{n},0" if epi == "SWIGLU" else ",".join(str(s) for s in (tuple(segs) + (0, 0))[:3])
    return f"{name} {M} {K} {n} {epi} 0 {flags} {seg} 1"


def k_tile(c):
    """Elements of K per pipeline step of the row's kernel."""
    return 32 if c.plan.startswith("gemm_big_kernel") else 64


def cut_tiles(c):
    """k-tile indices (of k_tile(c) elements) where a split-K part or a stream-K range begins
    inside a tile's K: the sums of both sides meet through the fp32 slabs."""
    nk = c.K // 64
    m = re.match(r"gemm8_kernel<\w+> splitk=(\d+)", c.plan)
    if m:
        s = int(m.group(1))
        return sorted({p * nk // s for p in range(1, s)})
    m = re.match(r"gemm8sk_kernel<\w+> dp_rounds=(\d+) chunk=(\d+) n_mt=\d+ tiles=(\d+)", c.plan)
    if m:
        dp, chunk, tiles = (int(v) for v in m.groups())
        units = (tiles - dp * 256) * nk
        return sorted({u % nk for u in range(0, units, chunk)} - {0})
    return []


# ---------------------------------------------------------------------------- bf16 helpers
def to_bf16(a):
    """fp32 -> bf16 bits, round to nearest even (finite values)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def trunc_bf16(a):
    return (np.ascontiguousarray(a, np.float32).view(np.uint32) >> 16).astype(np.uint16)


def bf(a):
    return (np.asarray(a, np.uint16).astype(np.uint32) << 16).view(np.float32)


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def sentinel(shape, dtype):
    """test_gpu_linear_variants._sentinel: values that no result equals by chance (fp32: quiet
    NaNs with a counting payload).  Imported on use: that module needs no GPU to import."""
    from test_gpu_linear_variants import _sentinel
    return _sentinel(shape, dtype)


# ---------------------------------------------------------------------------- inputs
Inputs = collections.namedtuple("Inputs", "x ws bs res y0")
"""x [M, K] bf16 bits; ws: bf16 bits per segment (SWIGLU: gate, up; fp8 rows: what the kernel must
see after dequantisation -- the GPU test quantises them and asserts that); bs: bf16 bits per
segment or []; res [M, N] bf16 bits or None; y0: the framed output, frame(c) with res in place."""


def seed_of(c, fam):
    return zlib.crc32(f"{c.name}/{fam}".encode()) % (1 << 31)


def frame(c, res=None):
    """The output buffer before a launch: [M + 2, ldy], a sentinel row before and after the M
    rows and sentinel pad columns; RESIDUAL: res in the live region."""
    ydt = np.float32 if c.epi == "F32" else np.uint16
    y0 = sentinel((c.M + 2, n_cols(c) + c.ldy_pad), ydt)
    if res is not None:
        y0[1:c.M + 1, :n_cols(c)] = res
    return y0


def live(c, y):
    return np.ascontiguousarray(y[1:c.M + 1, :n_cols(c)])


def perm(c):
    """F2: the column of K that holds weight row n's needle, for every n."""
    K, bk = c.K, k_tile(c)
    want = [0, K - 1]
    for t in cut_tiles(c):
        want += [64 * t - 1, 64 * t]
    return place_needles(c, n_cols(c), want, [k for e in range(bk, K, bk) for k in (e - 1, e)])


def place_needles(c, cols, want, edges):
    """`cols` needle positions in [0, K): every k of `want`, the k of `edges` (an even choice of
    them where the columns do not reach), the rest spread over all of K; in a random order."""
    K = c.K
    want = list(dict.fromkeys(want))
    edges = [k for k in dict.fromkeys(edges) if k not in want]
    if len(edges) > cols - len(want):   # fewer columns than edges: an even choice over all of K
        edges = [edges[i] for i in np.unique(np.linspace(0, len(edges) - 1, cols - len(want)).astype(np.int64))]
    want += edges
    assert len(want) <= cols, f"{c.name}: {cols} columns cannot hold the cuts' needles"
    r = np.random.default_rng(seed_of(c, "perm"))
    rest = cols - len(want)
    if rest > 0:   # one needle in each of `rest` equal stretches of K, at a random offset
        edges = np.linspace(0, K, rest + 1).astype(np.int64)
        want += [int(r.integers(lo, max(lo + 1, hi))) for lo, hi in zip(edges[:-1], edges[1:])]
    p = np.array(want, np.int64)
    return p[r.permutation(cols)]


def inputs(c, fam):
    """The inputs of family "F1" / "F2" for row c (deterministic by name)."""
    M, K, N = c.M, c.K, n_cols(c)
    r = np.random.default_rng(seed_of(c, fam))
    sw = c.epi == "SWIGLU"
    rows = (N, N) if sw else c.segs
    bs, res = [], None
    if fam == "F1":
        assert 16 * K < (1 << 24), "F1: |sum| <= 16 K must stay below 2^24"
        lo = 1 if sw else -4
        x = to_bf16(r.integers(lo, 5, (M, K)).astype(np.float32))
        ws = [to_bf16(r.integers(lo if (sw and i == 0) else -4, 5, (n, K)).astype(np.float32))
              for i, n in enumerate(rows)]
        if c.epi == "STORE":   # integer biases; every fourth one +-256, where acc + bias meets the ties 257, 259
            for n in rows:
                b = r.integers(-255, 256, n)
                b[::4] = 256 * r.choice([-1, 1], len(b[::4]))
                bs.append(to_bf16(b.astype(np.float32)))
        if c.epi == "RESIDUAL":
            res = to_bf16(r.integers(-8, 9, (M, N)).astype(np.float32))
    elif fam == "F2":
        assert not sw, "F2 has no SWIGLU form"
        x = (r.integers(0, 2, (M, K)) << 15 | r.integers(107, 148, (M, K)) << 7 | r.integers(0, 128, (M, K))).astype(np.uint16)
        p, sign, e = perm(c), r.choice([-1.0, 1.0], N), r.integers(-2, 3, N)
        W = np.zeros((N, K), np.float32)
        W[np.arange(N), p] = sign * 2.0 ** e
        W = to_bf16(W)
        ws = [W[o - n:o] for n, o in zip(rows, np.cumsum(rows))]
        if c.epi == "RESIDUAL":
            res = np.zeros((M, N), np.uint16)
    else:
        raise ValueError(fam)
    return Inputs(x, ws, bs, res, frame(c, res))


# ---------------------------------------------------------------------------- the answers
def _finish(c, acc, inp, rnd=to_bf16, inner=True, silu=False):
    """acc [M, cols] fp32 sums -> the live region, by the row's epilogue.  silu: SWIGLU with the
    fp32 formula of the kernel, g / (1 + exp(-g)) rounded to bf16 (model()); without, the closed
    form that holds from g = 17 upward, where 1 + exp(-g) is 1 in fp32 (expected())."""
    N = n_cols(c)
    if c.epi == "F32":
        return acc
    if c.epi == "SWIGLU":
        g = bf(rnd(acc[:, :N]))
        if silu:
            with np.errstate(over="ignore"):
                g = bf(rnd(g * (np.float32(1) / (np.float32(1) + np.exp(-g)))))
        return rnd(bf(rnd(acc[:, N:])) * g)
    if c.epi == "RESIDUAL":
        return rnd(bf(inp.res) + (bf(rnd(acc)) if inner else acc))
    return rnd(acc + bf(np.concatenate(inp.bs))[None, :]) if inp.bs else rnd(acc)


def expected(c, fam, inp):
    """The one right live region [M, N] of F1 / F2, computed apart from model(): F1 a float64
    product of the integers, F2 the gathered needles."""
    if fam == "F1":
        acc = (bf(inp.x).astype(np.float64) @ bf(np.concatenate(inp.ws)).astype(np.float64).T)
        assert np.abs(acc).max() < (1 << 24)
        return _finish(c, acc.astype(np.float32), inp)
    W = bf(np.concatenate(inp.ws))
    p = np.abs(W).argmax(axis=1)
    return _finish(c, bf(inp.x)[:, p] * W[np.arange(len(p)), p][None, :], inp)


MUTANTS = ("ktile_dropped", "ktile_twice", "part_off_by_one", "truncation", "residual_unrounded", "neighbour_bias",
           "weight_row_shift", "gate_up_swapped", "clamped_row_stored", "column_n_written")


def model(c, inp, mut=None):
    """The framed output of row c on F1 / F2 inputs as one float32 product (exact there: integer
    sums below 2^24, or one nonzero term per sum), with one way of being subtly wrong:
      ktile_dropped / ktile_twice   the middle k-tile left out / counted twice;
      part_off_by_one     the second split-K part (range) begins one k-tile late; unsplit, the
                          k loop ends one k-tile early;
      truncation          bf16 by truncation instead of round-to-nearest-even;
      residual_unrounded  RESIDUAL as bf16(res + acc);
      neighbour_bias      a segment's first column takes the previous segment's last bias;
      weight_row_shift    a segment's first column takes the weight row before it;
      gate_up_swapped     SWIGLU with the two segments exchanged;
      clamped_row_stored  row M (a re-read of row M-1) stored below the last row;
      column_n_written    column N (a re-read of weight row N-1) stored beside the last column."""
    assert mut is None or mut in MUTANTS, mut
    bk, cuts = k_tile(c), cut_tiles(c)
    return model_of(c, inp, bf(inp.x).copy(), bf(np.concatenate(inp.ws)).copy(), bk, cuts[0] * 64 // bk if cuts else None, mut)


def model_of(c, inp, x, W, bk, cut, mut):
    """model() on the float32 values x [M, K] and W [rows, K] (changed in place) of a kernel
    whose k-tile is bk elements and whose second part begins at k-tile `cut` (None: unsplit);
    a `mut` that is none of MUTANTS changes nothing here."""
    M, K, N = c.M, c.K, n_cols(c)
    nk = -(-K // bk)
    bs = [b.copy() for b in inp.bs]
    seg0 = c.segs[0] if len(c.segs) > 1 else None   # the first column of segment 1

    def tile(t):
        return slice(t * bk, min(K, (t + 1) * bk))
    if mut == "ktile_dropped":
        x[:, tile(nk // 2)] = 0
    elif mut == "ktile_twice":
        x[:, tile(nk // 2)] *= 2
    elif mut == "part_off_by_one":
        x[:, tile(cut if cut is not None else nk - 1)] = 0
    elif mut == "weight_row_shift" and seg0:
        W[seg0] = W[seg0 - 1]
    elif mut == "neighbour_bias" and seg0 and bs:
        bs[1][0] = bs[0][-1]
    elif mut == "gate_up_swapped" and c.epi == "SWIGLU":
        W = np.concatenate([W[N:], W[:N]])
    acc = x @ W.T
    out = _finish(c, acc, inp._replace(bs=bs), rnd=trunc_bf16 if mut == "truncation" else to_bf16,
                  inner=mut != "residual_unrounded", silu=True)
    y = inp.y0.copy()
    y[1:M + 1, :N] = out
    if mut == "clamped_row_stored":
        y[M + 1, :N] = out[M - 1]
    elif mut == "column_n_written":
        flat = y.reshape(-1)
        flat[np.arange(1, M + 1) * y.shape[1] + N] = out[:, N - 1]
    return y


def accepted(c, y, y0, want):
    """The acceptance of an exact case: the frame (sentinel rows and pad columns of y0) untouched
    bit for bit, and the live region bit-equal to `want`.  Returns (ok, words)."""
    M, N = c.M, n_cols(c)
    outside = np.ones(y0.shape, bool)
    outside[1:M + 1, :N] = False
    if not np.array_equal(bits(y)[outside], bits(y0)[outside]):
        return False, f"{c.name}: wrote outside y[:M, :N]"
    got = live(c, y)
    wrong = bits(got) != bits(np.ascontiguousarray(want))
    if wrong.any():
        m, n = np.argwhere(wrong)[0]
        return False, (f"{c.name}: {wrong.sum()} of {wrong.size} wrong, rows {np.unique(np.nonzero(wrong)[0])[:8]}, "
                       f"columns {np.unique(np.nonzero(wrong)[1])[:8]}; y[{m}, {n}] = {got[m, n]!r}, want {want[m, n]!r}")
    return True, ""
