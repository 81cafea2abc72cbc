"""CPU: tests/mx_cases.py against the planner (tools/plan_dump, no GPU) and against itself --
tests/test_gemm_cases_cpu.py's (a)-(d) for gemm8mx_kernel (fp8 activations).

(a) every row plans to the plan it declares (256 CUs, shipped knobs), and the library's
    qie_debug_linear_plan words it as plan_dump does;
(b) coverage: over a grid of shapes -- M 5 .. 8,192, the K of the rows plus the model widths, N
    as test_gemm_cases_cpu's grid, every epilogue, plain and 16-row tiled weights -- every
    distinct (kernel instantiation, splitk) is the declaration of some row, and those are all
    32: 4 epilogues x 2 layouts x 1..4 parts.  Besides: pads under both layouts and every split
    count, `twice` on every split row, one row without clamps, one M <= 16 row per layout, the
    uneven cuts the split rows are there for;
(c) the exact families check themselves: codes finite, F1 integers and sums below 2^EXACT_L (the
    instruction probe's measured bound), both round-to-nearest-even ties in every STORE row,
    every SwiGLU gate >= 32, row exponents and weight scales distinct at distances 1, 16, 64 and
    128, F2 needles on every required k, results normal (or zero) and finite;
(d) every mutant of the reference -- gemm_cases' ten and this kernel's own -- is rejected by at
    least one F1 or F2 case under the GPU test's acceptance function, and the unmutated model is
    accepted by every case."""
import ctypes as C

import numpy as np
import pytest

import gemm_cases as GC
import mx_cases as MC
from test_gemm_cases_cpu import GRID_M, GRID_N, plan_dump  # noqa: F401  (plan_dump: the fixture)

GRID_K = sorted({c.K for c in MC.CASES} | {896, 3584, 4864, 5120, 8192, 17408, 18944})
IDS = [c.name for c in MC.CASES]
NO_SWIGLU = [c for c in MC.CASES if c.epi != "SWIGLU"]
ALL_FORMS = {(f"gemm8mx_kernel<{e},{t}>", s) for e in GC.EPIS for t in (0, 1) for s in (1, 2, 3, 4)}


def _lines(cases):
    return [GC.dump_line(c.name, c.M, c.K, c.segs, c.epi, c.flags) for c in cases]


# ------------------------------------------------------------------------------------ (a)
def test_case_names_unique():
    names = [c.name for c in MC.CASES] + [c.name for c in GC.CASES]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)


def test_every_case_plans_to_its_declaration(plan_dump):
    got = plan_dump(_lines(MC.CASES))
    bad = [f"{c.name}: declares {c.plan}, plans {g}" for c, g in zip(MC.CASES, got) if g.split(" grid=")[0] != c.plan]
    assert not bad, "\n".join(bad)
    assert all(MC.form_key(c.plan) for c in MC.CASES)


def test_library_export_words_the_plan_as_plan_dump(plan_dump, qlib):
    from qwen_inference_engine_amd._lib import LinearArgsC
    dummy = (C.c_uint16 * 8)()
    ptr = C.addressof(dummy)
    buf = C.create_string_buffer(512)
    for c, w in zip(MC.CASES, plan_dump(_lines(MC.CASES))):
        a = LinearArgsC()
        n = GC.n_cols(c)
        a.x = a.y = a.x_exps = ptr
        a.M, a.K, a.N, a.ldx, a.ldy, a.flags = c.M, c.K, n, c.K + c.ldx_pad, n + c.ldy_pad, c.flags
        a.epilogue = GC.EPIS.index(c.epi)
        for i, r in enumerate(MC.segments(c)):
            a.w[i], a.seg_rows[i] = ptr, r
        assert qlib.qie_debug_linear_plan(C.byref(a), buf, len(buf)) == 0
        assert buf.value.decode() == w, (c.name, buf.value.decode(), w)


# ------------------------------------------------------------------------------------ (b)
def test_every_reachable_form_has_a_case(plan_dump):
    lines = [GC.dump_line("g", M, K, (N,), e, fl)
             for M in [5] + GRID_M for K in GRID_K for N in GRID_N for e in GC.EPIS for fl in (MC.PLAIN, MC.TILED)]
    reached = {}
    for line, g in zip(lines, plan_dump(lines)):
        k = MC.form_key(g)
        assert k and GC.form_key(g) is None, f"{line}: {g}"
        reached.setdefault(k, line)
    print(f"{len(reached)} distinct forms reached by {len(lines)} shapes")
    assert set(reached) == ALL_FORMS, sorted(ALL_FORMS ^ set(reached))
    declared = {MC.form_key(c.plan) for c in MC.CASES}
    missing = sorted(set(reached) - declared, key=str)
    assert not missing, "reachable forms without a case in tests/mx_cases.py:\n" + "\n".join(
        f"{k}  <-  {reached[k]}" for k in missing)
    assert declared == set(reached), sorted(declared - set(reached))


def test_table_rules():
    for t16 in (0, 1):
        lay = [c for c in MC.CASES if MC.is_t16(c) == bool(t16)]
        for s in (1, 2, 3, 4):
            cs = [c for c in lay if MC.split_of(c) == s]
            assert {c.epi for c in cs} == set(GC.EPIS), f"t16={t16} split {s}: not every epilogue"
            assert any(c.ldx_pad for c in cs) and any(c.ldy_pad for c in cs), f"t16={t16} split {s}: no row with pads"
        assert any(c.ldy_pad % 2 for c in lay)
        assert {c.K for c in lay if MC.split_of(c) == 1} >= {128, 384, 1024}   # 1, 3 and 8 k-tiles
        assert any(c.M <= 16 for c in lay), f"t16={t16}: no M <= 16 row"
        assert {c.M for c in lay} >= {257, 300}
    for c in MC.CASES:
        N = GC.n_cols(c)
        assert c.K % 128 == 0 and c.ldx_pad % 16 == 0, c.name   # check_mx
        assert c.M <= 512 and N * (2 if c.epi == "SWIGLU" else 1) <= 1100, c.name
        assert c.twice == (MC.split_of(c) > 1), f"{c.name}: twice is for the split rows"
        assert c.flags in (MC.PLAIN, MC.TILED)
        if MC.is_t16(c):
            assert all(r % 16 == 0 for r in MC.segments(c)), c.name
        elif len(c.segs) > 1:
            assert c.name == "mx_noclamp" or any(o % 16 for o in np.cumsum(c.segs)[:-1]), c.name
        if c.name != "mx_noclamp":
            assert N % 128, f"{c.name}: N ends on a tile edge"
    assert any(c.M % 256 == 0 and GC.n_cols(c) % 256 == 0 for c in MC.CASES)
    cuts = {c.name: MC.cut_tiles(c) for c in MC.CASES}
    assert cuts["mx_k8_store"] == [] and cuts["mx_split2_store"] == [8] and cuts["mx16_split3_f32"] == [8, 16]
    assert cuts["mx_split4_swiglu"] == [8, 16, 24] and {c.K // 128 for c in MC.CASES if c.twice} == {17, 25, 33}


# ------------------------------------------------------------------------------------ (c)
def _normal_or_zero(a):
    """Every element finite and no subnormal."""
    if a.dtype == np.float32:
        ex, rest = (a.view(np.uint32) >> 23) & 0xFF, a.view(np.uint32) & 0x7FFFFFFF
    else:
        ex, rest = (a >> 7) & 0xFF, a & 0x7FFF
    return bool(((ex != 0xFF) & ((ex != 0) | (rest == 0))).all())


def test_exponents_and_scales_differ_between_neighbours():
    for c in MC.CASES:
        ea = MC.x_exps(c).astype(np.int64)
        assert 127 - 20 <= ea.min() and ea.max() <= 127 + 24
        for s in np.split(MC.w_scale_exps(c), np.cumsum(MC.segments(c))[:-1]) if c.epi == "SWIGLU" else [MC.w_scale_exps(c)]:
            assert -12 <= s.min() and s.max() <= 12
            for d in (1, 16, 64, 128):
                assert (s[d:] != s[:-d]).all(), (c.name, d)
        for d in (1, 16, 64, 128):
            assert (ea[d:] != ea[:-d]).all(), (c.name, d)
        if c.epi == "SWIGLU":   # the gate's combined exponent is never negative
            assert (ea.min() - 127) + MC.w_scale_exps(c)[:GC.n_cols(c)].min() >= 0


@pytest.mark.parametrize("c", MC.CASES, ids=IDS)
def test_f1_is_exact_and_the_model_agrees(c, qlib):
    inp = MC.inputs(c, "F1")
    want = MC.expected(c, "F1", inp)   # asserts |integer sum| < 2^EXACT_L
    t = MC.e4m3_values()
    xi, wi = t[inp.x], t[np.concatenate(inp.ws)]
    R = MC.int_range(c)
    assert MC.EXACT_L == 23 and R * R * c.K < (1 << MC.EXACT_L)
    assert (xi == np.rint(xi)).all() and (wi == np.rint(wi)).all() and np.abs(xi).max() <= R and np.abs(wi).max() <= R
    assert (xi != 0).any(axis=1).all() and len(inp.ea) == c.M
    N = GC.n_cols(c)
    e = MC.out_exps(c, inp)
    acc = xi.astype(np.float64) @ wi.astype(np.float64).T
    if c.epi == "SWIGLU":
        assert np.ldexp(acc[:, :N], e[:, :N]).min() >= 32 and xi.min() >= 1 and wi[:N].min() >= 1 and wi[N:].min() < 0
    if c.epi == "STORE":   # both ties of round-to-nearest-even: ...0|1000... (down to even), ...1|1000... (up)
        u = (np.ldexp(acc, e).astype(np.float32) + GC.bf(np.concatenate(inp.bs))[None, :]).view(np.uint32)
        tie = (u & 0xFFFF) == 0x8000
        assert (tie & ((u >> 16) & 1 == 0)).any() and (tie & ((u >> 16) & 1 == 1)).any(), c.name
        assert np.array_equal(want[tie], ((u[tie] >> 16) + ((u[tie] >> 16) & 1)).astype(np.uint16))
    assert _normal_or_zero(want) and _normal_or_zero(np.ldexp(acc, e).astype(np.float32)), c.name
    ok, why = MC.accepted(c, MC.model(c, inp), inp.y0, want)
    assert ok, why


@pytest.mark.parametrize("c", NO_SWIGLU, ids=[c.name for c in NO_SWIGLU])
def test_f2_needles_and_the_model_agrees(c, qlib):
    inp = MC.inputs(c, "F2")
    K, N = c.K, GC.n_cols(c)
    W = np.concatenate(inp.ws)
    mz, nz = MC.zero_rows(c)
    assert not (inp.x & 0x7F == 0x7F).any() and not (W & 0x7F == 0x7F).any()   # no NaN code
    assert len(np.unique(inp.x)) == 254 or c.M * K < 254 * 40
    assert (inp.x & 0x78 == 0).any() and not inp.x[mz].any() and inp.x[np.arange(c.M) != mz].any(axis=1).all()
    assert np.array_equal((W != 0).sum(axis=1), np.arange(N) != nz)
    needles = W[W != 0]
    assert ((needles & 0x78) == 0).any() and (needles & 0x80).any() and (~needles & 0x80).any() and len(np.unique(needles)) > 100
    hit = set(np.nonzero(W)[1].tolist())
    must = {0, K - 1} | {k for e in range(128, K, 128) for k in (e - 1, e)}
    for t in MC.cut_tiles(c):
        must |= {128 * t - 1, 128 * t}
    assert must <= hit, f"{c.name}: no needle at {sorted(must - hit)}"
    frag = {k for e in range(32, K, 32) for k in (e - 1, e)}
    if len(frag | must) <= N - 1:
        assert frag <= hit, f"{c.name}: a fragment edge without a needle"
    assert len(frag & hit) >= min(len(frag), N - 1 - len(must)) - 1, c.name
    want = MC.expected(c, "F2", inp)   # asserts every product exact in fp32
    assert _normal_or_zero(want) and (GC.live(c, MC.model(c, inp))[mz] == 0).all()
    ok, why = MC.accepted(c, MC.model(c, inp), inp.y0, want)
    assert ok, why


def test_both_layouts_have_rows_with_every_fragment_edge_needled():
    done = {MC.is_t16(c) for c in NO_SWIGLU if 2 * (c.K // 32) <= GC.n_cols(c) - 1}
    assert done == {False, True}


def test_tile16_is_the_documented_layout():
    """mx_cases.tile16 against the sentence of qie_ops.h, element by element."""
    codes = np.arange(32 * 128, dtype=np.uint32).reshape(32, 128)
    t = MC.tile16(codes).reshape(-1)
    for tt, j, l, b in [(0, 0, 0, 0), (1, 1, 37, 5), (0, 1, 63, 15), (1, 0, 16, 0)]:
        assert t[(tt * 2 + j) * 1024 + 16 * l + b] == codes[16 * tt + l % 16, 64 * j + 16 * (l // 16) + b]


def test_accepted_is_bit_exact_but_for_the_sign_of_zero():
    c = MC.CASES[0]
    inp = MC.inputs(c, "F2")
    want = MC.expected(c, "F2", inp)
    y = MC.model(c, inp)
    live = y[1:c.M + 1, :GC.n_cols(c)]
    assert (live == 0).any()
    y2 = y.copy()
    y2[1:c.M + 1, :GC.n_cols(c)][live == 0] = 0x8000   # -0 for +0: accepted
    assert MC.accepted(c, y2, inp.y0, want)[0]
    m, n = np.argwhere(live != 0)[0]
    y2 = y.copy()
    y2[1 + m, n] ^= 1                                    # one ulp: rejected
    assert not MC.accepted(c, y2, inp.y0, want)[0]
    y2 = y.copy()
    y2[0, 0] ^= 1                                        # the frame: rejected
    assert not MC.accepted(c, y2, inp.y0, want)[0]


# ------------------------------------------------------------------------------------ (d)
def _cost(c):
    return c.M * c.K * (2 if c.epi == "SWIGLU" else 1) * GC.n_cols(c)


@pytest.mark.parametrize("mut", MC.MUTANTS)
def test_every_mutant_is_rejected(mut):
    """By the cheapest cases first; a mutant that a row cannot express (no second segment, no
    split, no tiled weights) equals the model there and is accepted."""
    rejected = []
    for c in sorted(MC.CASES, key=_cost):
        for fam in ("F1", "F2"):
            if fam == "F2" and c.epi == "SWIGLU":
                continue
            inp = MC.inputs(c, fam)
            ok, _ = MC.accepted(c, MC.model(c, inp, mut), inp.y0, MC.expected(c, fam, inp))
            if not ok:
                rejected.append(f"{c.name}/{fam}")
        if len(rejected) >= 3:
            break
    print(f"{mut}: rejected by {rejected}")
    assert rejected, f"no F1 / F2 case rejects the mutant {mut}"


def test_split_mutants_are_rejected_by_the_split_rows():
    for c in MC.CASES:
        if not MC.cut_tiles(c):
            continue
        for fam in ("F1", "F2"):
            if fam == "F2" and c.epi == "SWIGLU":
                continue
            inp = MC.inputs(c, fam)
            ok, _ = MC.accepted(c, MC.model(c, inp, "part_off_by_one"), inp.y0, MC.expected(c, fam, inp))
            assert not ok, (c.name, fam)


def test_scale_and_exponent_mutants_are_rejected_by_every_row_that_can_express_them():
    """The byte-map mutants on the rows they are about: every row with more than 16 / 64 rows or
    columns rejects them under F1."""
    for c in MC.CASES:
        inp = MC.inputs(c, "F1")
        want = MC.expected(c, "F1", inp)
        for mut in ("exp_row_16", "exp_row_64", "scale_col_16", "a_exp_dropped", "b_scale_twice"):
            if c.M <= 16 and mut.startswith("exp_row"):
                continue
            ok, _ = MC.accepted(c, MC.model(c, inp, mut), inp.y0, want)
            assert not ok, (c.name, mut)
