"""CPU: the launch plan of the M <= 16 linear layers (csrc/linear_plan.hpp), printed by a plain
host program (`make -C qwen_inference_engine_amd/csrc plan_dump`, no HIP, no GPU) and compared
with a table derived by hand from the launch code this plan replaced (k_gemv.hip's gemv() and
launch_gemv_t, k_decode_fp8.hip's dec8_applies), on 256 CUs, REF numerics.

Where the grid depends on the occupancy query (the `nb` column), the value is what that query
returned on an MI355X for the kernel named in the row, read off the grid of that launch in the
decode-graph dumps under profiles/ (linear_plan_graph_*.txt; tools/graph_dump.py).  Rows whose
grid does not depend on it pass nb = 1."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen_inference_engine_amd", "csrc")

FP8 = 1   # QIE_LINEAR_FP8

# (name, M, K, N, epilogue, norm, flags, seg rows, nb, knobs) -> expected line
ROWS = [
    # ---- Qwen2-7B, bf16, M = 1 (hidden 3,584, QKV 3,584 + 2 x 512, ffn 18,944, vocab 152,064)
    (("7b_qkv", 1, 3584, 4608, "STORE", 1, 0, "3584,512,512", 1, ""),
     "gemv_kernel<1,2,STORE,7,2,0> xlds=1 tasks=2304 bpc=2 grid=512 threads=256 lds=7232"),
    (("7b_o", 1, 3584, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, ""),
     "gemv_kernel<1,1,RESIDUAL,7,1,0> LB=1024 xlds=0 tasks=3584 bpc=-1 grid=256 threads=896 lds=64"),
    (("7b_gate_up", 1, 3584, 18944, "SWIGLU", 1, 0, "18944,18944,0", 1, ""),
     "gemv_kernel<1,2,SWIGLU,7,4,0> xlds=0 tasks=18944 bpc=6 grid=1536 threads=256 lds=64"),
    (("7b_down", 1, 18944, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, ""),
     "gemv_kernel<1,2,RESIDUAL,8,1,0> LB=576 xlds=0 tasks=1792 bpc=-1 grid=256 threads=448 lds=64"),
    (("7b_lm_head", 1, 3584, 152064, "STORE", 1, 0, "152064,0,0", 1, ""),
     "gemv_kernel<1,2,STORE,8,3,0> xlds=1 tasks=76032 bpc=2 grid=512 threads=256 lds=7232"),
    # ---- Qwen2-0.5B (hidden 896, QKV 896 + 2 x 128, ffn 4,864, vocab 151,936): every
    # occupancy-balanced grid below is one round (tasks <= 4 x 256 x nb for any nb >= 1)
    (("05b_qkv", 1, 896, 1152, "STORE", 1, 0, "896,128,128", 1, ""),
     "gemv_kernel<1,2,STORE,2,2,0> xlds=1 tasks=576 bpc=-1 grid=144 threads=256 lds=1856"),
    (("05b_o", 1, 896, 896, "RESIDUAL", 0, 0, "896,0,0", 1, ""),
     "gemv_kernel<1,2,RESIDUAL,2,2,0> xlds=1 tasks=448 bpc=-1 grid=112 threads=256 lds=1856"),
    (("05b_gate_up", 1, 896, 4864, "SWIGLU", 1, 0, "4864,4864,0", 1, ""),
     "gemv_kernel<1,2,SWIGLU,2,4,0> xlds=0 tasks=4864 bpc=3 grid=768 threads=256 lds=64"),
    (("05b_down", 1, 4864, 896, "RESIDUAL", 0, 0, "896,0,0", 1, ""),
     "gemv_kernel<1,2,RESIDUAL,5,10,0> xlds=1 tasks=448 bpc=-1 grid=112 threads=256 lds=9792"),
    (("05b_lm_head", 1, 896, 151936, "STORE", 1, 0, "151936,0,0", 1, ""),
     "gemv_kernel<1,2,STORE,2,3,0> xlds=1 tasks=75968 bpc=5 grid=1280 threads=256 lds=1856"),
    # ---- Qwen3-14B (hidden 5,120, QKV 5,120 + 2 x 1,024, ffn 17,408, vocab 151,936): more than
    # 9 row tasks per CU everywhere, so every grid comes from the occupancy query: nb = 3 blocks
    # per CU, from profiles/linear_plan_graph_qwen3_14b.txt (gate/up's full-residency grid is
    # 768 = 256 x 3; lm_head's 760 blocks are 25 rounds over 768 slots; O and down, one round
    # of 640 blocks, fit nb >= 3)
    (("14b_qkv", 1, 5120, 7168, "STORE", 1, 0, "5120,1024,1024", 3, ""),
     "gemv_kernel<1,2,STORE,5,5,0> xlds=1 tasks=3584 bpc=-1 grid=448 threads=256 lds=10304"),
    (("14b_o", 1, 5120, 5120, "RESIDUAL", 0, 0, "5120,0,0", 3, ""),
     "gemv_kernel<1,2,RESIDUAL,5,10,0> xlds=1 tasks=2560 bpc=-1 grid=640 threads=256 lds=10304"),
    (("14b_gate_up", 1, 5120, 17408, "SWIGLU", 1, 0, "17408,17408,0", 3, ""),
     "gemv_kernel<1,2,SWIGLU,5,5,0> xlds=1 tasks=17408 bpc=-2 grid=768 threads=256 lds=10304"),
    (("14b_down", 1, 17408, 5120, "RESIDUAL", 0, 0, "5120,0,0", 3, ""),
     "gemv_kernel<1,2,RESIDUAL,7,10,0> xlds=1 tasks=2560 bpc=-1 grid=640 threads=256 lds=34880"),
    (("14b_lm_head", 1, 5120, 151936, "STORE", 1, 0, "151936,0,0", 3, ""),
     "gemv_kernel<1,2,STORE,8,5,0> xlds=1 tasks=75968 bpc=-1 grid=760 threads=256 lds=10304"),
    # ---- fp8 weights (Qwen2-7B shapes): M = 1 the GEMV's fp8 form; M = 8 the batched-decode
    # kernel at K = 3,584 (7 waves x 8 units), split-K at K = 18,944 (296 units: 10 parts of
    # 8 waves x 4 units), the skinny kernel for the vocabulary (N > 32,768; rows normed before it;
    # nb = 2 at 60,544 B of LDS: the 512-block lm_head of profiles/linear_plan_graph_config4.txt)
    # (M = 1 on plain fp8 rows is in no engine's decode graph — engines tile their fp8 weights —
    # so the row has 1,024 row tasks: one round of the occupancy-balanced grid for any nb)
    (("fp8_m1", 1, 3584, 2048, "STORE", 1, FP8, "2048,0,0", 1, ""),
     "gemv_kernel<1,2,STORE,8,0,1> xlds=1 tasks=1024 bpc=-1 grid=256 threads=256 lds=7232"),
    (("fp8_m8_qkv", 8, 3584, 4608, "STORE", 1, FP8, "3584,512,512", 1, ""), "dec8 KU=8 KS=7 parts=1"),
    (("fp8_m8_down", 8, 18944, 3584, "RESIDUAL", 0, FP8, "3584,0,0", 1, ""), "dec8 KU=4 KS=8 parts=10"),
    (("fp8_m8_lm_head", 8, 3584, 152064, "STORE", 0, FP8, "152064,0,0", 2, ""),
     "skinny_mfma_kernel<STORE,1,1,4,7> t16=0 grid=512 threads=256 lds=60544"),
    # ---- the paths beside the main ones
    # 4 bf16 rows: the skinny kernel, 224 column tiles (< 256 CUs: the grid is the tile count)
    (("m4_o", 4, 3584, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, ""),
     "skinny_mfma_kernel<RESIDUAL,0,0,4,0> t16=0 grid=224 threads=256 lds=3072"),
    # 12 rows, K no multiple of 64: the tiled GEMM (gemm_plan.hpp; tests/test_gemm_plan_cpu.py) —
    # K no multiple of 32 either, so its generic 128x128 kernel, one row tile x 28 column tiles
    (("m12_k3592", 12, 3592, 3584, "STORE", 0, 0, "3584,0,0", 1, ""),
     "gemm_kernel<STORE,0> n_mt=1 tiles=28 slabs=0 tickets=0 grid=1x28 threads=256 lds=65536"),
    # a fused norm at K > 10,240: no x-first variant holds it (XCH 5 ends at 10,240, XCH 10 has
    # no norm), so the generic prologue — on the one-block-per-CU grid (9 row tasks per CU)
    (("k10248_norm", 1, 10248, 4608, "STORE", 1, 0, "4608,0,0", 1, ""),
     "gemv_kernel<1,2,STORE,8,0,0> LB=576 xlds=1 tasks=2304 bpc=-1 grid=256 threads=576 lds=20560"),
    # ---- two knobs through Knobs: Qwen2-7B's O projection without the one-block-per-CU layout,
    # capped at 16 blocks per CU (448 four-wave blocks; x staged by the x-first prologue)
    (("7b_o_knobs", 1, 3584, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, "balanced=0 blocks_per_cu=16"),
     "gemv_kernel<1,2,RESIDUAL,7,2,0> xlds=1 tasks=1792 bpc=16 grid=448 threads=256 lds=7232"),
]


def test_linear_plan_table():
    subprocess.run(["make", "-s", "-C", CSRC, "plan_dump"], check=True, timeout=300)
    exe = os.path.join(ROOT, "qwen_inference_engine_amd", "_build", "plan_dump")
    text = "".join(" ".join(str(v) for v in row) + "\n" for row, _ in ROWS)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    want = [f"{row[0]}: {line}" for row, line in ROWS]
    assert got == want, "\n".join(f"{g}\n   want {w}" for g, w in zip(got, want) if g != w)
