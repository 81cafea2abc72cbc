"""The M <= 16 linear layer, one op-level case per kernel instantiation its planner can pick.

plan_linear() (csrc/linear_plan.hpp) chooses among the gemv_kernel and skinny_mfma_kernel
instantiations by shape alone.  Every row below is a small shape, the instantiation that shape
plans to on 256 CUs with the shipped knobs, worded as tools/plan_dump prints it, and what the GPU
test feeds it.  tests/test_linear_variants_cpu.py checks the declared instantiations against
plan_dump and that no reachable Gemv / Skinny instantiation lacks a row;
tests/test_gpu_linear_variants.py runs every row against the CPU oracle.

Plain data and small helpers: no test, no fixture.

Shapes: the smallest that reaches the variant, with the tails a kernel can get wrong: K that ends
in a ragged 512-element wave-load (1000 = 512 + 488, 3080, 4104 ...), an odd N (the last two-row
task has one row), N just past a block-count step (2050 = 5 waves, 4600 = 9, 4095 = 16), segment
boundaries at odd rows.  Vocabulary rows (N >= 65,536) keep K <= 1,032.
"""
import collections
import re

FP8 = 1   # QIE_LINEAR_FP8

Case = collections.namedtuple(
    "Case", "name M K segs epi plan norm flags ldx_pad ldy_pad key_col0 bias twice")


def C(name, M, K, segs, epi, plan, norm=None, flags=0, ldx_pad=0, ldy_pad=0, key_col0=None, bias=False,
      twice=False):
    """segs: rows per weight segment (SWIGLU: (I,), gate and up have I rows each); norm: None /
    "ref" / "hf" fused RMSNorm; ldx_pad / ldy_pad: elements beyond K / N in a row of x / y;
    key_col0: None, or the column offset of fused arg-max keys; bias: one bias per segment;
    twice: several row tasks per wave -- two launches into fresh outputs must agree bit for bit."""
    segs = (segs,) if isinstance(segs, int) else tuple(segs)
    return Case(name, M, K, segs, epi, plan, norm, flags, ldx_pad, ldy_pad, key_col0, bias, twice)


def n_cols(c):
    return sum(c.segs)


EPIS = ("STORE", "RESIDUAL", "SWIGLU", "F32")
E3 = ("STORE", "RESIDUAL", "F32")

CASES = [
    # ------------------------------------------------------------------ one bf16 row, XCH 1:
    # x read beside the weights, one block per CU.  One row per wave (LB=1024, up to 16 waves):
    C("rpw1_res_16waves", 1, 512, 4095, "RESIDUAL", "gemv_kernel<1,1,RESIDUAL,8,1,0> LB=1024 xlds=0"),
    C("rpw1_store_16waves_keys", 1, 512, 4095, "STORE", "gemv_kernel<1,1,STORE,8,1,0> LB=1024 xlds=0", key_col0=0),
    C("rpw1_res_9waves_u7", 1, 3584, 2049, "RESIDUAL", "gemv_kernel<1,1,RESIDUAL,7,1,0> LB=1024 xlds=0"),
    C("rpw1_store_odd_segs", 1, 1000, (2001, 7, 43), "STORE", "gemv_kernel<1,1,STORE,8,1,0> LB=1024 xlds=0",
      bias=True, ldx_pad=8, ldy_pad=3),
    C("rpw1_store_u7", 1, 3080, 2050, "STORE", "gemv_kernel<1,1,STORE,7,1,0> LB=1024 xlds=0", ldx_pad=16),
    # two rows per wave (LB=576, 5..9 waves): K > 4,096, N > 4,096 or the F32 epilogue
    C("rpw2_res_5waves", 1, 4104, 2306, "RESIDUAL", "gemv_kernel<1,2,RESIDUAL,8,1,0> LB=576 xlds=0"),
    C("rpw2_res_9waves", 1, 10248, 4098, "RESIDUAL", "gemv_kernel<1,2,RESIDUAL,8,1,0> LB=576 xlds=0", ldy_pad=5),
    C("rpw2_store_9waves", 1, 520, (4001, 97), "STORE", "gemv_kernel<1,2,STORE,8,1,0> LB=576 xlds=0", bias=True),
    C("rpw2_f32_5waves", 1, 520, 2051, "F32", "gemv_kernel<1,2,F32,8,1,0> LB=576 xlds=0", ldy_pad=3),
    C("rpw2_res_u7", 1, 3080, 4099, "RESIDUAL", "gemv_kernel<1,2,RESIDUAL,7,1,0> LB=576 xlds=0"),
    C("rpw2_store_u7", 1, 3584, 4098, "STORE", "gemv_kernel<1,2,STORE,7,1,0> LB=576 xlds=0", key_col0=7),
    C("rpw2_f32_u7", 1, 3080, 2050, "F32", "gemv_kernel<1,2,F32,7,1,0> LB=576 xlds=0", ldx_pad=8),

    # ------------------------------------------------------------------ one bf16 row, x-first
    # prologue with a fused norm on one block per CU (LB=576, x staged, the norm's block
    # reduction over 5..9 waves instead of 4)
    C("lb576_norm_store_5waves", 1, 3592, (2001, 7, 42), "STORE", "gemv_kernel<1,2,STORE,8,2,0> LB=576 xlds=1",
      norm="ref", bias=True),
    C("lb576_norm_store_x5_9waves", 1, 4104, 4600, "STORE", "gemv_kernel<1,2,STORE,5,5,0> LB=576 xlds=1", norm="hf"),
    C("lb576_norm_store_u2", 1, 1000, 2051, "STORE", "gemv_kernel<1,2,STORE,2,2,0> LB=576 xlds=1", norm="hf",
      ldx_pad=8, key_col0=0),
    C("lb576_norm_store_u7", 1, 3080, 2050, "STORE", "gemv_kernel<1,2,STORE,7,2,0> LB=576 xlds=1", norm="ref"),
    C("lb576_norm_store_x5_u8", 1, 5128, 2050, "STORE", "gemv_kernel<1,2,STORE,8,5,0> LB=576 xlds=1", norm="ref"),
    C("lb576_norm_store_x0", 1, 10248, 2050, "STORE", "gemv_kernel<1,2,STORE,8,0,0> LB=576 xlds=1", norm="ref"),
] + [
    # the same six prologues under the RESIDUAL and F32 epilogues
    C(f"lb576_norm_{e.lower()}_{tag}", 1, K, N, e, f"gemv_kernel<1,2,{e},{uxch},0> LB=576 xlds=1", norm=num)
    for e in ("RESIDUAL", "F32")
    for tag, K, N, uxch, num in [("u2", 1000, 2051, "2,2", "ref"), ("u7", 3080, 2050, "7,2", "hf"),
                                 ("u8", 1032, 2306, "8,2", "ref"), ("x5_u5", 4104, 2050, "5,5", "ref"),
                                 ("x5_u8", 5128, 2050, "8,5", "hf"), ("x0", 10248, 2050, "8,0", "ref")]
] + [
    # ------------------------------------------------------------------ one bf16 row on 4-wave
    # blocks.  The normed QKV shape with two blocks per CU:
    C("bpc2_norm_store", 1, 3584, 3074, "STORE", "gemv_kernel<1,2,STORE,7,2,0> xlds=1", norm="ref", twice=True),
    # the prologue boundaries: XCH 2 ends at K = 4,096, XCH 5 (norm) at 10,240, XCH 10 (no norm)
    # at 20,480; past them the generic prologue, and past 48 Ki elements x is not staged
    C("k4096_norm", 1, 4096, 6, "STORE", "gemv_kernel<1,2,STORE,8,2,0> xlds=1", norm="ref"),
    C("k4104_norm", 1, 4104, 6, "STORE", "gemv_kernel<1,2,STORE,5,5,0> xlds=1", norm="ref", ldx_pad=8, ldy_pad=1),
    C("k4096", 1, 4096, 6, "STORE", "gemv_kernel<1,2,STORE,8,2,0> xlds=1"),
    C("k4104", 1, 4104, 6, "STORE", "gemv_kernel<1,2,STORE,5,10,0> xlds=1"),
    C("k10240_norm", 1, 10240, 6, "STORE", "gemv_kernel<1,2,STORE,8,5,0> xlds=1", norm="hf", ldx_pad=24,
      key_col0=3),
    C("k10248_norm", 1, 10248, 6, "STORE", "gemv_kernel<1,2,STORE,8,0,0> xlds=1", norm="ref"),
    C("k20480_res", 1, 20480, 6, "RESIDUAL", "gemv_kernel<1,2,RESIDUAL,8,10,0> xlds=1"),
    C("k20488_res", 1, 20488, 6, "RESIDUAL", "gemv_kernel<1,2,RESIDUAL,8,0,0> xlds=1"),
    C("k49160_store", 1, 49160, 6, "STORE", "gemv_kernel<1,2,STORE,8,0,0> xlds=0"),
] + [
    # every prologue x chunk count under every epilogue, no norm, 7 output columns (4 tasks, the
    # last of one row; SWIGLU: 7 gate/up pairs)
    C(f"m1_{e.lower()}_{tag}", 1, K, 7, e, f"gemv_kernel<1,2,{e},{uxch},0> xlds={xl}", ldx_pad=8 if e == "F32" else 0)
    for e in EPIS
    for tag, K, uxch, xl in [("x2_u2", 1000, "2,2", 1), ("x2_u7", 3080, "7,2", 1), ("x2_u8", 1032, "8,2", 1),
                             ("x10_u5", 4104, "5,10", 1), ("x10_u7", 10240, "7,10", 1), ("x10_u8", 5128, "8,10", 1),
                             ("x0", 20488, "8,0", 1), ("x0_nolds", 49160, "8,0", 0)]
] + [
    # the fused norm's XCH 5 under the epilogues the rows above leave (STORE: k4104_norm, k10240_norm)
    C(f"m1_norm_{e.lower()}_{tag}", 1, K, 7, e, f"gemv_kernel<1,2,{e},{uxch},0> xlds=1", norm=num)
    for e in ("RESIDUAL", "F32")
    for tag, K, uxch, num in [("x5_u5", 4104, "5,5", "hf"), ("x5_u8", 5128, "8,5", "ref")]
] + [
    # ------------------------------------------------------------------ vocabulary projection:
    # XCH 3, the per-wave sum of squares (N >= 65,536 with a fused norm)
    C("vocab_u2_keys", 1, 1000, 65538, "STORE", "gemv_kernel<1,2,STORE,2,3,0> xlds=1", norm="ref", key_col0=151,
      twice=True),
    C("vocab_u8_keys", 1, 1032, 65536, "STORE", "gemv_kernel<1,2,STORE,8,3,0> xlds=1", norm="hf", key_col0=65536,
      ldx_pad=8, ldy_pad=3, twice=True),
    C("vocab_u2_res", 1, 520, 65538, "RESIDUAL", "gemv_kernel<1,2,RESIDUAL,2,3,0> xlds=1", norm="ref", ldx_pad=16,
      ldy_pad=1, twice=True),
    C("vocab_u8_res", 1, 1032, 65536, "RESIDUAL", "gemv_kernel<1,2,RESIDUAL,8,3,0> xlds=1", norm="ref", twice=True),
    C("vocab_u2_f32", 1, 520, 65538, "F32", "gemv_kernel<1,2,F32,2,3,0> xlds=1", norm="hf", twice=True),
    C("vocab_u8_f32", 1, 1032, 65536, "F32", "gemv_kernel<1,2,F32,8,3,0> xlds=1", norm="ref", twice=True),

    # ------------------------------------------------------------------ gate/up with a fused norm:
    # XCH 4, the normalised x in registers (K <= 4,096), XCH 5 and the generic prologue above
    C("swiglu_norm_x4_u2_bpc3", 1, 1000, 4100, "SWIGLU", "gemv_kernel<1,2,SWIGLU,2,4,0> xlds=0", norm="ref",
      twice=True),
    C("swiglu_norm_x4_u8", 1, 3592, 24, "SWIGLU", "gemv_kernel<1,2,SWIGLU,8,4,0> xlds=0", norm="ref"),
    C("swiglu_norm_x4_u7", 1, 3584, 24, "SWIGLU", "gemv_kernel<1,2,SWIGLU,7,4,0> xlds=0", norm="hf", ldx_pad=8,
      ldy_pad=1),
    C("swiglu_norm_x5_u8", 1, 5128, 24, "SWIGLU", "gemv_kernel<1,2,SWIGLU,8,5,0> xlds=1", norm="ref"),
    C("swiglu_norm_x5_u5", 1, 4104, 25, "SWIGLU", "gemv_kernel<1,2,SWIGLU,5,5,0> xlds=1", norm="hf"),
    C("swiglu_norm_x0", 1, 10248, 7, "SWIGLU", "gemv_kernel<1,2,SWIGLU,8,0,0> xlds=1", norm="ref"),
] + [
    # ------------------------------------------------------------------ 2..8 bf16 rows the skinny
    # kernel does not take (K no multiple of 64): MT 2 / 4 / 8, x staged or (past 96 KiB) not
    C("m8_norm_store", 8, 72, 40, "STORE", "gemv_kernel<8,2,STORE,8,0,0> xlds=1", norm="ref", ldx_pad=8, ldy_pad=3),
    C("m3_nolds_store", 3, 20488, 2, "STORE", "gemv_kernel<4,2,STORE,8,0,0> xlds=0"),
    C("m5_nolds_store", 5, 10248, 2, "STORE", "gemv_kernel<8,2,STORE,8,0,0> xlds=0"),
    C("m2_nolds_store", 2, 49160, 3, "STORE", "gemv_kernel<2,2,STORE,8,0,0> xlds=0", bias=True),
] + [
    C(f"m{M}_{e.lower()}", M, 1000, 41, e, f"gemv_kernel<{mt},2,{e},8,0,0> xlds=1", norm=num, ldy_pad=pad)
    for e in EPIS
    for M, mt, num, pad in [(2, 2, None, 0), (4, 4, "hf", 3), (7, 8, None, 0)]
] + [
    C(f"m{M}_nolds_{e.lower()}", M, K, 3, e, f"gemv_kernel<{mt},2,{e},8,0,0> xlds=0")
    for e in ("RESIDUAL", "SWIGLU", "F32")
    for M, mt, K in [(2, 2, 49160), (4, 4, 12296), (8, 8, 6152)]
] + [
    # ------------------------------------------------------------------ fp8 weights on the GEMV
    # (K % 16 == 0; K no multiple of 64 keeps 2..8 rows off the MFMA kernels)
    C("fp8_m1_norm_store", 1, 80, 40, "STORE", "gemv_kernel<1,2,STORE,8,0,1> xlds=1", norm="ref", flags=FP8),
    C("fp8_m5_swiglu", 5, 80, 40, "SWIGLU", "gemv_kernel<8,2,SWIGLU,8,0,1> xlds=1", flags=FP8),
] + [
    C(f"fp8_m{M}_{e.lower()}", M, 1008, 41, e, f"gemv_kernel<{mt},2,{e},8,0,1> xlds=1", norm=num, flags=FP8,
      bias=(e == "STORE"))
    for e in EPIS
    for M, mt, num in [(1, 1, None), (2, 2, "ref"), (3, 4, None), (8, 8, "hf")]
] + [
    C(f"fp8_m1_nolds_{e.lower()}", 1, 49168, 3, e, f"gemv_kernel<1,2,{e},8,0,1> xlds=0", flags=FP8)
    for e in EPIS
] + [
    # 2..8 fp8 rows past 96 KiB: the codes decoded against x read from global, row by row
    C(f"fp8_m{M}_nolds_{e.lower()}", M, K, 3, e, f"gemv_kernel<{mt},2,{e},8,0,1> xlds=0", flags=FP8,
      bias=(e == "STORE"), ldx_pad=16 if M == 3 else 0)
    for e in EPIS
    for M, mt, K in [(2, 2, 49168), (3, 4, 16400), (8, 8, 6160)]
] + [
    # ------------------------------------------------------------------ bf16 skinny MFMA kernel
    # (2..16 rows, K % 64 == 0; four waves split K in 64-element units): XL 0 the A fragments from
    # L2, XL 1 the rows staged in LDS (a fused norm, or more than two column tiles per CU)
    C("sk_store_m16_k192", 16, 192, (23, 9, 8), "STORE", "skinny_mfma_kernel<STORE,0,0,4,0>", bias=True,
      ldx_pad=8, ldy_pad=3),   # 3 units: wave 3 has no K range
    C("sk_store_m13_keys", 13, 192, (23, 9, 8), "STORE", "skinny_mfma_kernel<STORE,0,0,4,0>", bias=True,
      key_col0=5),             # arg-max keys of rows past 4 (every lane group of the C tile), three column tiles
    C("sk_swiglu_norm_m16_k320", 16, 320, 40, "SWIGLU", "skinny_mfma_kernel<SWIGLU,0,1,4,0>", norm="ref"),
    C("sk_res_staged_514tiles", 5, 64, 8210, "RESIDUAL", "skinny_mfma_kernel<RESIDUAL,0,1,4,0>", twice=True),
    C("sk_swiglu_staged_514tiles", 5, 64, 8210, "SWIGLU", "skinny_mfma_kernel<SWIGLU,0,1,4,0>", twice=True),
    C("sk_f32_staged_514tiles", 13, 64, 8210, "F32", "skinny_mfma_kernel<F32,0,1,4,0>", ldy_pad=2, twice=True),
    C("sk_f32_m16", 16, 3904, 24, "F32", "skinny_mfma_kernel<F32,0,0,4,0>"),
    C("sk_store_norm_m3", 3, 128, (33, 7), "STORE", "skinny_mfma_kernel<STORE,0,1,4,0>", norm="hf", bias=True,
      key_col0=9, ldx_pad=8),
    C("sk_res_m2_k64", 2, 64, 24, "RESIDUAL", "skinny_mfma_kernel<RESIDUAL,0,0,4,0>", ldy_pad=5),
    C("sk_swiglu_m7_k192", 7, 192, 24, "SWIGLU", "skinny_mfma_kernel<SWIGLU,0,0,4,0>"),
    C("sk_f32_norm_m9_k320", 9, 320, 40, "F32", "skinny_mfma_kernel<F32,0,1,4,0>", norm="ref"),
    C("sk_res_norm_m16_k320", 16, 320, 41, "RESIDUAL", "skinny_mfma_kernel<RESIDUAL,0,1,4,0>", norm="ref"),
] + [
    # ------------------------------------------------------------------ fp8 skinny MFMA kernel
    # (what the batched-decode kernel leaves: K of no slice shape and too short to split): UO 7
    # where a wave's K range is 7 units (K = 1,600: 25 units, ranges of 7 / 7 / 7 / 4)
    C(f"sk8_{e.lower()}_{tag}", M, K, N, e, f"skinny_mfma_kernel<{e},1,{xl},4,{uo}>", norm=num, flags=FP8,
      bias=(e == "STORE"))
    for e in EPIS
    for tag, M, K, N, xl, uo, num in [("xl0", 3, 192, 40, 0, 0, None), ("xl0_u7", 16, 1600, 24, 0, 7, None),
                                      ("xl1_norm", 16, 320, 41, 1, 0, "ref"), ("xl1_u7_norm", 6, 1600, 24, 1, 7, "hf")]
] + [
    C("sk8_store_staged_514tiles", 9, 64, 8210, "STORE", "skinny_mfma_kernel<STORE,1,1,4,0>", flags=FP8, twice=True),
] + [
    # ------------------------------------------------------------------ 9..16 rows the skinny
    # kernel cannot take (K no multiple of 64): the tiled GEMM
    C(f"gemm_m12_{e.lower()}", 12, 72, (23, 9, 8) if e == "STORE" else 40, e, f"gemm_kernel<{e},0>",
      bias=(e == "STORE"), ldx_pad=8 if e == "RESIDUAL" else 0)
    for e in EPIS
]

# shapes qie_linear refuses (rc -22): (name, M, K, N, epilogue, words of the error)
REFUSALS = [
    ("norm_m1_k49160", 1, 49160, 6, "STORE", "fused RMSNorm needs M*K*2"),   # PlanError::NormLds
    ("norm_m8_k6152", 8, 6152, 6, "STORE", "fused RMSNorm needs M*K*2"),
    ("norm_m16_k3840", 16, 3840, 6, "STORE", "fused RMSNorm is GEMV-only"),  # x cannot be staged: the GEMM
]

# ---------------------------------------------------------------------------- plan_dump helpers
_KEY = re.compile(r"(gemv_kernel<[^>]*>(?: LB=\d+)? xlds=\d|skinny_mfma_kernel<[^>]*>|gemm_kernel<[^>]*>)")


def plan_key(text):
    """The instantiation (+ LB + xlds) at the start of a plan line, None for other plans."""
    m = _KEY.match(text)
    return m.group(1) if m else None


def dump_line(name, M, K, segs, epi, norm, flags):
    """One line of plan_dump input (resident blocks 1: the keys do not depend on the grid)."""
    n = sum(segs)
    seg = f"{n},{n},0" if epi == "SWIGLU" else ",".join(str(s) for s in (tuple(segs) + (0, 0))[:3])
    return f"{name} {M} {K} {n} {epi} {1 if norm else 0} {flags} {seg} 1"
