"""CPU: tests/gemm_cases.py against the planner (tools/plan_dump, no GPU) and against itself.

(a) every row plans to the plan it declares (256 CUs, shipped knobs);
(b) coverage: over a grid of shapes -- M 17 .. 8,192, the K values of the rows plus the model
    widths, N from 130 to 51,100 (SWIGLU: the same counts of weight rows), every epilogue, flags
    0 / FP8 / TILE256 / TILE128 / STREAMK -- every distinct (kernel instantiation, splitk), and for
    stream-K (kernel instantiation, dp_rounds > 0, chunk > 1), is the declaration of some row, so
    tests/test_gpu_gemm_variants.py runs it: a newly reachable form without a case fails here.
    Besides: every epilogue under every kernel template, every split count under at least two
    epilogues, pads in every family, `twice` on every split and stream-K row, one row without
    clamps;
(c) the exact families check themselves: F1 sums below 2^24, both round-to-nearest-even ties in
    the STORE data, every SwiGLU gate >= 32, fp8 dequantisation exact; F2 needles on k = 0,
    K - 1, both sides of every part / range cut and of every k-tile edge the columns can reach;
(d) every mutant of the reference is rejected by at least one F1 or F2 case under the GPU
    test's own acceptance function, and the unmutated model is accepted by every case.
fp8 activations (gemm8mx_kernel) have the same protocol in tests/mx_cases.py,
tests/test_mx_cases_cpu.py and tests/test_gpu_mx_variants.py.  Out of scope: the forms only
development knobs reach (QIE_GEMM8 = 1 / 3, QIE_GEMM_BIG, QIE_GEMM8_SK_GRID / _SK_MINK: compiled
out of the shipped library)."""
import os
import re
import subprocess

import numpy as np
import pytest

import gemm_cases as GC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen_inference_engine_amd", "csrc")

# The grid of (b).  K: the rows' own (ragged 72 / 200 / 208, the ring's 96, 4 k-tiles, 129 / 193 /
# 257 k-tiles) and the model widths; N: 130, around the 128- and 256-tile counts that switch kernels
# at 1, 2, 8 and 32 row tiles, the model widths, and the rows' own largest.
GRID_M = [17, 128, 255, 256, 257, 300, 512, 2048, 8192]
GRID_K = [40, 72, 80, 96, 200, 208, 256, 896, 2240, 3584, 4864, 5120, 8192, 8256, 12352, 16448, 17408, 18944]
GRID_N = [130, 264, 320, 896, 1400, 3584, 4608, 5120, 6100, 8164, 12200, 16328, 16400, 18944, 25550, 32712, 33000,
          51100]
GRID_FLAGS = [0, GC.FP8, GC.TILE256, GC.TILE128, GC.STREAMK]

FAMILIES = {"gemm_kernel<E,0>": "generic", "gemm_kernel<E,1>": "fp8", "gemm_big_kernel<E,128>": "big128",
            "gemm_big_kernel<E,256>": "big256", "gemm8_kernel<E>": "gemm8", "gemm8sk_kernel<E>": "streamk"}


def template(key):
    return re.sub(r"<\w+", "<E", key[0])


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


def _small(c):
    return c.M * c.K * (2 if c.epi == "SWIGLU" else 1) * GC.n_cols(c)


# ------------------------------------------------------------------------------------ (a)
def test_case_names_unique():
    names = [c.name for c in GC.CASES]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)


def test_every_case_plans_to_its_declaration(plan_dump):
    got = plan_dump([GC.dump_line(c.name, c.M, c.K, c.segs, c.epi, c.flags) for c in GC.CASES])
    bad = [f"{c.name}: declares {c.plan}, plans {g}" for c, g in zip(GC.CASES, got) if g.split(" grid=")[0] != c.plan]
    assert not bad, "\n".join(bad)
    assert all(GC.form_key(c.plan) for c in GC.CASES)


def test_library_export_words_the_plan_as_plan_dump(plan_dump, qlib):
    """qie_debug_linear_plan (asserted before every GPU launch) with no device plans for 256 CUs,
    in plan_dump's words, grid included; ldx and ldy pads do not move the plan."""
    import ctypes as C
    from qwen_inference_engine_amd._lib import LinearArgsC
    want = plan_dump([GC.dump_line(c.name, c.M, c.K, c.segs, c.epi, c.flags) for c in GC.CASES])
    dummy = (C.c_uint16 * 8)()
    ptr = C.addressof(dummy)
    buf = C.create_string_buffer(512)
    for c, w in zip(GC.CASES, want):
        a = LinearArgsC()
        n = GC.n_cols(c)
        a.x = a.y = ptr
        a.M, a.K, a.N, a.ldx, a.ldy, a.flags = c.M, c.K, n, c.K + c.ldx_pad, n + c.ldy_pad, c.flags
        a.epilogue = GC.EPIS.index(c.epi)
        for i, r in enumerate((n, n) if c.epi == "SWIGLU" else c.segs):
            a.w[i], a.seg_rows[i] = ptr, r
        assert qlib.qie_debug_linear_plan(C.byref(a), buf, len(buf)) == 0
        assert buf.value.decode() == w, (c.name, buf.value.decode(), w)


# ------------------------------------------------------------------------------------ (b)
def test_every_reachable_form_has_a_case(plan_dump):
    lines = [GC.dump_line("g", M, K, (N,), e, fl)
             for M in GRID_M for K in GRID_K for N in GRID_N for e in GC.EPIS for fl in GRID_FLAGS
             if not (fl == GC.FP8 and K % 16)]
    reached = {}
    for line, g in zip(lines, plan_dump(lines)):
        k = GC.form_key(g)
        assert k, f"{line}: {g}"
        reached.setdefault(k, line)
    print(f"{len(reached)} distinct forms reached by {len(lines)} shapes")
    # 4 epilogues x (generic, fp8, 256x128, 256x256, gemm8 at 1..4 parts, stream-K's 4 forms)
    assert len(reached) == 4 * (4 + 4 + 4), sorted(reached)
    declared = {GC.form_key(c.plan) for c in GC.CASES}
    missing = sorted(set(reached) - declared, key=str)
    assert not missing, "reachable forms without a case in tests/gemm_cases.py:\n" + "\n".join(
        f"{k}  <-  {reached[k]}" for k in missing)
    stale = sorted(declared - set(reached), key=str)
    assert not stale, f"declared forms the grid does not reach (widen the grid): {stale}"


def test_table_rules():
    keys = {c.name: GC.form_key(c.plan) for c in GC.CASES}
    by_template = {}
    for c in GC.CASES:
        by_template.setdefault(template(keys[c.name]), []).append(c)
    assert set(by_template) == set(FAMILIES)
    for t, cs in by_template.items():
        assert {c.epi for c in cs} == set(GC.EPIS), f"{t}: not every epilogue"
        assert any(c.ldx_pad for c in cs) and any(c.ldy_pad for c in cs), f"{t}: no row with pads"
        assert any(c.ldy_pad % 2 for c in cs), f"{t}: no odd ldy pad"
    for s in (1, 2, 3, 4):
        assert len({c.epi for c in GC.CASES if keys[c.name][0].startswith("gemm8_kernel") and keys[c.name][1] == s}) >= 2
    for c in GC.CASES:
        assert c.M > 16 and c.K % 8 == 0 and c.ldx_pad % 8 == 0
        split = GC.cut_tiles(c) or keys[c.name][0].startswith("gemm8sk")
        assert c.twice == bool(split), f"{c.name}: twice is for the split and stream-K rows"
        assert not (c.flags & GC.FP8) or c.K % 16 == 0
    assert any(c.M % 256 == 0 and GC.n_cols(c) % 256 == 0 and c.plan.startswith("gemm8_kernel") for c in GC.CASES)
    # the cuts the rows are there for: uneven parts, and ranges that cross tiles
    cuts = {c.name: GC.cut_tiles(c) for c in GC.CASES}
    assert cuts["split2_store"] == [64] and cuts["split3_f32"] == [64, 128] and cuts["split4_swiglu"] == [64, 128, 192]
    assert cuts["sk_c1_f32"] == list(range(1, 14)) and len(cuts["sk_c2_f32"]) == 34 and cuts["sk_dp_c3_f32"] == [1, 2, 3]


# ------------------------------------------------------------------------------------ (c)
@pytest.mark.parametrize("c", GC.CASES, ids=[c.name for c in GC.CASES])
def test_f1_is_exact_and_the_model_agrees(c, qlib):
    inp = GC.inputs(c, "F1")
    want = GC.expected(c, "F1", inp)   # asserts |sum| < 2^24
    x, W = GC.bf(inp.x), GC.bf(np.concatenate(inp.ws))
    assert (x == np.rint(x)).all() and (W == np.rint(W)).all() and np.abs(x).max() <= 4 and np.abs(W).max() <= 4
    N = GC.n_cols(c)
    if c.epi == "SWIGLU":
        gate = x.astype(np.float64) @ W[:N].astype(np.float64).T
        assert gate.min() >= 32 and x.min() >= 1 and W[:N].min() >= 1 and W[N:].min() < 0
    if c.epi == "STORE":   # both ties of round-to-nearest-even: 257 -> 256 (down to even), 259 -> 260 (up)
        v = np.abs(x.astype(np.float64) @ W.astype(np.float64).T + GC.bf(np.concatenate(inp.bs)).astype(np.float64))
        assert (v == 257).any() and (v == 259).any(), c.name
        assert (np.abs(GC.bf(want))[v == 257] == 256).all() and (np.abs(GC.bf(want))[v == 259] == 260).all()
    if c.flags & GC.FP8:   # what the kernel decodes is what the reference multiplies
        from qwen_inference_engine_amd import weights as Wt
        for w in inp.ws:
            assert np.array_equal(Wt.dequantize_fp8(*Wt.quantize_fp8(w)), w), c.name
    ok, why = GC.accepted(c, GC.model(c, inp), inp.y0, want)
    assert ok, why


@pytest.mark.parametrize("c", [c for c in GC.CASES if c.epi != "SWIGLU"],
                         ids=[c.name for c in GC.CASES if c.epi != "SWIGLU"])
def test_f2_needles_and_the_model_agrees(c, qlib):
    inp = GC.inputs(c, "F2")
    K, N, bk = c.K, GC.n_cols(c), GC.k_tile(c)
    W = GC.bf(np.concatenate(inp.ws))
    assert ((W != 0).sum(axis=1) == 1).all()
    vals = np.abs(W[W != 0])
    assert set(np.unique(vals)) <= {0.25, 0.5, 1.0, 2.0, 4.0} and (W < 0).any() and (W > 0).any()
    e = (inp.x >> 7) & 0xFF
    assert e.min() >= 107 and e.max() <= 147
    hit = set(np.nonzero(W)[1].tolist())
    assert {0, K - 1} <= hit
    for t in GC.cut_tiles(c):
        assert {64 * t - 1, 64 * t} <= hit, f"{c.name}: no needle beside the cut at k-tile {t}"
    edges = [k for e in range(bk, K, bk) for k in (e - 1, e)]
    if len(set(edges) | {0, K - 1}) <= N:
        assert set(edges) <= hit, f"{c.name}: a k-tile edge without a needle"
    tiles_hit = {k // bk for k in hit}   # fewer columns than edges: still no stretch of K without a needle
    assert len(tiles_hit) >= min(-(-K // bk), N) * 0.6, (c.name, len(tiles_hit))
    if c.flags & GC.FP8:
        from qwen_inference_engine_amd import weights as Wt
        for w in inp.ws:
            assert np.array_equal(Wt.dequantize_fp8(*Wt.quantize_fp8(w)), w), c.name
    want = GC.expected(c, "F2", inp)
    ok, why = GC.accepted(c, GC.model(c, inp), inp.y0, want)
    assert ok, why


def test_every_kernel_family_has_a_row_with_every_k_tile_edge_needled():
    done = set()
    for c in GC.CASES:
        if c.epi != "SWIGLU" and 2 * (-(-c.K // GC.k_tile(c))) <= GC.n_cols(c):
            done.add(template(GC.form_key(c.plan)))
    assert done == set(FAMILIES), set(FAMILIES) - done


# ------------------------------------------------------------------------------------ (d)
@pytest.mark.parametrize("mut", GC.MUTANTS)
def test_every_mutant_is_rejected(mut):
    """By the cheapest cases first; a mutant that a row cannot express (no second segment, no
    split) equals the model there and is accepted, which is why the table needs all its rows."""
    rejected = []
    for c in sorted(GC.CASES, key=_small):
        if _small(c) > 2e9 and rejected:
            break
        for fam in ("F1", "F2"):
            if fam == "F2" and c.epi == "SWIGLU":
                continue
            inp = GC.inputs(c, fam)
            ok, _ = GC.accepted(c, GC.model(c, inp, mut), inp.y0, GC.expected(c, fam, inp))
            if not ok:
                rejected.append(f"{c.name}/{fam}")
        if len(rejected) >= 3:
            break
    print(f"{mut}: rejected by {rejected}")
    assert rejected, f"no F1 / F2 case rejects the mutant {mut}"


def test_split_mutants_are_rejected_by_the_split_rows():
    """The k-range mutants on the rows they are about: every split-K and stream-K row with a cut
    rejects a part that begins one k-tile late, under F1 and (non-SWIGLU) F2."""
    for c in GC.CASES:
        if not GC.cut_tiles(c) or _small(c) > 6e8:
            continue
        for fam in ("F1", "F2"):
            if fam == "F2" and c.epi == "SWIGLU":
                continue
            inp = GC.inputs(c, fam)
            ok, _ = GC.accepted(c, GC.model(c, inp, "part_off_by_one"), inp.y0, GC.expected(c, fam, inp))
            assert not ok, (c.name, fam)
