"""CPU: tests/linear_cases.py against the planner (tools/plan_dump, no GPU).

(a) every row plans to the instantiation it declares (256 CUs, shipped knobs);
(b) every gemv_kernel / skinny_mfma_kernel instantiation (+ block bound + staged x) that a grid of
    shapes reaches is the declared instantiation of a row, so tests/test_gpu_linear_variants.py
    runs it against the oracle: a new reachable instantiation without a case fails here; the
    same for 200,000 seeded random shapes, in case the grid's hand-picked sizes miss a path;
(c) every QIE_GEMV_CASE the library compiles is reached by that grid or listed below with the
    development knob that reaches it.
Out of scope: the fp8 batched-decode kernel (Dec8 plans), 16-row tiled weights and fp8
activations, which have their own files (test_gpu_fp8.py, test_gpu_fp8_mx.py)."""
import os
import re
import subprocess

import pytest

import linear_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen_inference_engine_amd", "csrc")

# The grid of (b).  K: every prologue boundary from both sides (512-element wave-loads, XCH 2 /
# 5 / 10 at 4,096 / 10,240 / 20,480, the 96-KiB staging cap at 49,152) and the model widths;
# 80 and 49168 are multiples of 16 and not of 64 (fp8 rows on the MT 2 / 4 / 8 GEMV, x staged
# and, past the cap, not staged).
# N: around 4, 9 and 16 row tasks per CU, the skinny kernel's 512 column tiles and the
# vocabulary threshold.
GRID_K = [8, 64, 80, 128, 504, 512, 520, 896, 1000, 1024, 1032, 2048, 3584, 3592, 4096, 4104, 5120, 5128, 8192,
          10240, 10248, 17408, 18944, 20480, 20488, 24576, 32768, 49152, 49160, 49168, 65536]
GRID_N = [2, 16, 18, 130, 512, 1024, 2048, 2050, 2304, 2306, 3584, 4096, 4098, 4608, 5120, 8192, 8208, 16384,
          18944, 32768, 32784, 65536, 65538, 152064]

# QIE_GEMV_CASE(MT, XCH, WT, UO) entries no shape reaches with the shipped knobs: development
# A/B code ("Linear variants: the coverage rule").
DEV_ONLY_GEMV_CASES = {
    (1, 3, 0, 7): "QIE_GEMV_XREG=1 (XCH 3 below the vocabulary threshold, K of 7 wave-loads)",
}


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


@pytest.fixture(scope="module")
def grid_plans(plan_dump):
    lines = [LC.dump_line("g", M, K, (N,), e, norm, fl)
             for M in range(1, 17) for K in GRID_K for N in GRID_N for e in LC.EPIS for norm in (0, 1)
             for fl in (0, LC.FP8)]
    return plan_dump(lines)


def test_case_names_unique():
    names = [c.name for c in LC.CASES]
    assert len(names) == len(set(names)), sorted(n for n in names if names.count(n) > 1)


def test_every_case_plans_to_its_declared_instantiation(plan_dump):
    got = plan_dump([LC.dump_line(c.name, c.M, c.K, c.segs, c.epi, c.norm, c.flags) for c in LC.CASES])
    bad = [f"{c.name}: declares {c.plan}, plans {g}" for c, g in zip(LC.CASES, got)
           if not g.startswith(c.plan + " ")]
    assert not bad, "\n".join(bad)


def test_library_export_words_the_plan_as_plan_dump(plan_dump, qlib):
    """qie_debug_linear_plan (what the GPU test asserts before each launch) is plan_dump's line up
    to the grid, which the export leaves open ("grid=?") where it needs an occupancy query.  No
    device here: the library then plans for 256 CUs, as plan_dump does."""
    import ctypes as C
    from qwen_inference_engine_amd._lib import LinearArgsC
    want = plan_dump([LC.dump_line(c.name, c.M, c.K, c.segs, c.epi, c.norm, c.flags) for c in LC.CASES])
    dummy = (C.c_uint16 * 8)()
    ptr = C.addressof(dummy)
    buf = C.create_string_buffer(512)
    for c, w in zip(LC.CASES, want):
        a = LinearArgsC()
        n = LC.n_cols(c)
        a.x = a.y = ptr
        a.M, a.K, a.N, a.ldx, a.ldy, a.flags = c.M, c.K, n, c.K, n, c.flags
        a.epilogue = LC.EPIS.index(c.epi)
        for i, r in enumerate((n, n) if c.epi == "SWIGLU" else c.segs):
            a.w[i], a.seg_rows[i] = ptr, r
        a.norm_w = ptr if c.norm else None
        assert qlib.qie_debug_linear_plan(C.byref(a), buf, len(buf)) == 0
        got = buf.value.decode()
        assert got.split(" grid=")[0] == w.split(" grid=")[0] and LC.plan_key(got) == c.plan, (c.name, got, w)
    assert qlib.qie_debug_linear_plan(C.byref(a), buf, 4) == -22   # the line does not fit


def test_refusals_plan_to_an_error_or_the_gemm(plan_dump):
    """The refused shapes: plan_linear reports NormLds (error 2), or hands the rows to the GEMM,
    which takes no fused norm (the GPU test asserts qie_linear's error text)."""
    got = plan_dump([LC.dump_line(name, M, K, (N,), epi, 1, 0) for name, M, K, N, epi, _ in LC.REFUSALS])
    for (name, *_rest, words), g in zip(LC.REFUSALS, got):
        assert g == "error 2" if "needs M*K*2" in words else g.startswith("gemm_kernel<"), (name, g)


def test_every_reachable_instantiation_has_a_case(grid_plans):
    reached = {}
    for g in grid_plans:
        k = LC.plan_key(g)
        if k and not k.startswith("gemm_kernel") and " t16=1" not in g:
            reached[k] = reached.get(k, 0) + 1
    print(f"{len(reached)} distinct Gemv / Skinny instantiations reached by {len(grid_plans)} shapes")
    assert len(reached) >= 140
    declared = {c.plan for c in LC.CASES}
    missing = sorted(set(reached) - declared)
    assert not missing, "reachable instantiations without a case in tests/linear_cases.py:\n" + "\n".join(missing)


def test_random_shapes_reach_no_instantiation_without_a_case(plan_dump):
    """A second net under the grid, whose K and N are chosen by hand: 200,000 seeded random
    shapes (K in steps of 8, 16, 64 or 512 up to 66,000, N log-uniform up to 160,000) must plan
    to declared instantiations only."""
    import numpy as np
    r = np.random.default_rng(20)
    n = 200000
    M, step = r.integers(1, 17, n), np.array([8, 16, 64, 512])[r.integers(0, 4, n)]
    K = (r.integers(0, 66000, n) // step + 1) * step
    N = np.exp(r.uniform(0, np.log(160000), n)).astype(np.int64)
    epi, norm, fp8 = r.integers(0, 4, n), r.integers(0, 2, n), r.integers(0, 2, n)
    lines = [LC.dump_line("r", int(M[i]), int(K[i]), (int(N[i]),), LC.EPIS[epi[i]], int(norm[i]), int(fp8[i]))
             for i in range(n)]
    declared = {c.plan for c in LC.CASES}
    missing = {}
    for line, g in zip(lines, plan_dump(lines)):
        k = LC.plan_key(g)
        if k and not k.startswith("gemm_kernel") and k not in declared:
            missing.setdefault(k, line)
    assert not missing, "\n".join(f"{k}  <-  {l}" for k, l in sorted(missing.items()))


def test_every_compiled_gemv_case_is_reached_or_listed(grid_plans):
    text = open(os.path.join(CSRC, "k_gemv.hip")).read()
    compiled = {tuple(int(v) for v in m.groups())
                for m in re.finditer(r"^\s*QIE_GEMV_CASE\((\d+), (\d+), (\d+), (\d+)\);", text, flags=re.M)}
    assert len(compiled) >= 20
    # plan_dump prints U, the chunks in flight: UO, or 8 where UO is 0 (two rows per wave)
    compiled = {(mt, xch, wt, uo or 8) for mt, xch, wt, uo in compiled}
    reached = set()
    for g in grid_plans:
        m = re.match(r"gemv_kernel<(\d+),(\d+),(\w+),(\d+),(\d+),(\d+)>", g)
        if m:
            mt, rpw, _, u, xch, wt = m.groups()
            assert rpw in ("1", "2"), f"rows per wave {rpw} reached by shape: add cases for it ({g})"
            reached.add((int(mt), int(xch), int(wt), int(u)))
    assert reached <= compiled, sorted(reached - compiled)
    unlisted = sorted(compiled - reached - set(DEV_ONLY_GEMV_CASES))
    assert not unlisted, f"compiled, reached by no shape, and not listed as dev-only: {unlisted}"
    stale = sorted(set(DEV_ONLY_GEMV_CASES) & reached)
    assert not stale, f"listed as dev-only but reached by shape: {stale}"
