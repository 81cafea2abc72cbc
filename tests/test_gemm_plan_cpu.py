"""CPU: the launch plan of the prefill GEMMs (csrc/gemm_plan.hpp plan_gemm: M > 16, and every M
with fp8 activations), printed by the plain host program plan_dump and compared with a table
derived by hand from the launch code this plan replaced (k_gemm.hip's gemm(), gemm_mx(),
g8_splitk and launch_gemm8sk), on 256 CUs with the shipped knobs.

Notation: n_mt row tiles of 256 (128 for the generic kernel), t256 / t128 = n_mt x column tiles
of 256 / 128 weight rows (SwiGLU: gate and up rows, 2 N), nk = K / 64 k-tiles (K / 128 with fp8
activations).  LDS: 131,072 B for the 256x256 kernels, 98,304 B for 256x128, 65,536 B generic."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen_inference_engine_amd", "csrc")

FP8, TILE256, TILE128, STREAMK, T16, ACT8 = 1, 2, 4, 8, 16, 32
MX, MXT = FP8 | ACT8, FP8 | T16 | ACT8


def g8(epi, tiles, n_mt, splitk=1):
    ws = f"slabs={tiles * splitk} tickets={tiles}" if splitk > 1 else "slabs=0 tickets=0"
    return f"gemm8_kernel<{epi}> splitk={splitk} n_mt={n_mt} tiles={tiles} {ws} grid={tiles * splitk} threads=512 lds=131072"


def mx(epi, t16, tiles, n_mt, splitk=1):
    ws = f"slabs={tiles * splitk} tickets={tiles}" if splitk > 1 else "slabs=0 tickets=0"
    return (f"gemm8mx_kernel<{epi},{t16}> splitk={splitk} n_mt={n_mt} tiles={tiles} {ws} grid={tiles * splitk} "
            "threads=512 lds=131072")


def big(epi, bn, tiles, n_mt):
    return (f"gemm_big_kernel<{epi},{bn}> n_mt={n_mt} tiles={tiles} slabs=0 tickets=0 grid={tiles} threads=512 "
            f"lds={131072 if bn == 256 else 98304}")


def generic(epi, wt, gm, gn):
    return f"gemm_kernel<{epi},{wt}> n_mt={gm} tiles={gm * gn} slabs=0 tickets=0 grid={gm}x{gn} threads=256 lds=65536"


QKV7, GU7 = "3584,512,512", "18944,18944,0"
# (name, M, K, N, epilogue, norm, flags, seg rows, nb, knobs) -> expected line
ROWS = [
    # ---- Qwen2-7B at 2,048 rows (n_mt 8).  QKV: 18 column tiles, t256 144 < 256;
    # nk 56 < 64, so no split; 2 x 144 >= 256: gemm8 unsplit.  O: t256 112, no split, 224 < 256,
    # so not gemm8; t128 224 in [192, 256]: 256x128.  gate/up: 148 column tiles, 1,184 >= 256.
    # down: 112 tiles, nk 296: 2 parts of 148 make one round of half tiles (3 parts: two rounds
    # of thirds; 4 parts of 74: two rounds of quarters, no better than 2)
    (("7b_qkv", 2048, 3584, 4608, "STORE", 0, 0, QKV7, 1, ""), g8("STORE", 144, 8)),
    (("7b_o", 2048, 3584, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, ""), big("RESIDUAL", 128, 224, 8)),
    (("7b_gate_up", 2048, 3584, 18944, "SWIGLU", 0, 0, GU7, 1, ""), g8("SWIGLU", 1184, 8)),
    (("7b_down", 2048, 18944, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, ""), g8("RESIDUAL", 112, 8, 2)),
    # ---- the same at 8,192 rows (config 4; n_mt 32): every t256 >= 256, gemm8 on full-chip grids
    (("7b_qkv_8k", 8192, 3584, 4608, "STORE", 0, 0, QKV7, 1, ""), g8("STORE", 576, 32)),
    (("7b_o_8k", 8192, 3584, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, ""), g8("RESIDUAL", 448, 32)),
    (("7b_gate_up_8k", 8192, 3584, 18944, "SWIGLU", 0, 0, GU7, 1, ""), g8("SWIGLU", 4736, 32)),
    (("7b_down_8k", 8192, 18944, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, ""), g8("RESIDUAL", 448, 32)),
    # ---- Qwen2-0.5B at 128 rows: M < 256, nothing forced: the generic kernel, one row tile,
    # 128 columns (SwiGLU: 64 outputs) per tile
    (("05b_qkv", 128, 896, 1152, "STORE", 0, 0, "896,128,128", 1, ""), generic("STORE", 0, 1, 9)),
    (("05b_gate_up", 128, 896, 4864, "SWIGLU", 0, 0, "4864,4864,0", 1, ""), generic("SWIGLU", 0, 1, 76)),
    (("05b_down", 128, 4864, 896, "RESIDUAL", 0, 0, "896,0,0", 1, ""), generic("RESIDUAL", 0, 1, 7)),
    # ---- Qwen3-14B at 2,048 rows (hidden 5,120, QKV 7,168, ffn 17,408; nk 80 at K = 5,120: one
    # part only).  QKV 224 and O 160 tiles cover half the chip unsplit; gate/up 1,088; down 160
    # tiles, nk 272: 3 parts of 90 run two rounds of thirds (2 parts: two rounds of halves, 4
    # parts of 68: three rounds of quarters)
    (("14b_qkv", 2048, 5120, 7168, "STORE", 0, 0, "5120,1024,1024", 1, ""), g8("STORE", 224, 8)),
    (("14b_o", 2048, 5120, 5120, "RESIDUAL", 0, 0, "5120,0,0", 1, ""), g8("RESIDUAL", 160, 8)),
    (("14b_gate_up", 2048, 5120, 17408, "SWIGLU", 0, 0, "17408,17408,0", 1, ""), g8("SWIGLU", 1088, 8)),
    (("14b_down", 2048, 17408, 5120, "RESIDUAL", 0, 0, "5120,0,0", 1, ""), g8("RESIDUAL", 160, 8, 3)),
    # ---- the smallest shape that splits by default (tests/test_gpu_ops.py
    # test_linear_gemm8_splitk): 2 x 2 tiles (SwiGLU: 528 weight rows, 2 x 3), nk 128: 2 parts of
    # 64 k-tiles (3 parts would be 42 < 64)
    (("split_small", 257, 8192, 264, "STORE", 0, 0, "200,40,24", 1, ""), g8("STORE", 4, 2, 2)),
    (("split_small_sw", 257, 8192, 264, "SWIGLU", 0, 0, "264,264,0", 1, ""), g8("SWIGLU", 6, 2, 2)),
    # ---- fp8 weights with bf16 activations: the generic kernel's decoding form, 16 x 28 tiles
    (("fp8w_o", 2048, 3584, 3584, "RESIDUAL", 0, FP8, "3584,0,0", 1, ""), generic("RESIDUAL", 1, 16, 28)),
    # ---- K a multiple of 32 but not of 64: no gemm8; the LDS-DMA ring kernel by tile count
    (("k3616_gate_up", 2048, 3616, 18944, "SWIGLU", 0, 0, GU7, 1, ""), big("SWIGLU", 256, 1184, 8)),
    (("k3616_o", 2048, 3616, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, ""), big("RESIDUAL", 128, 224, 8)),
    # ---- K no multiple of 32: generic
    (("k3592_o", 2048, 3592, 3584, "STORE", 0, 0, "3584,0,0", 1, ""), generic("STORE", 0, 16, 28)),
    # ---- forced tiles on a small shape (300 x 320: n_mt 2, t256 4, t128 6).  TILE256 at K = 896
    # (14 k-tiles) is gemm8 unsplit, at K = 96 (no multiple of 64) the ring kernel; stream-K on
    # 256 workgroups: no whole-tile round, 4 x 14 = 56 units, one per range, slab [256][2]
    (("t256", 300, 896, 320, "RESIDUAL", 0, TILE256, "320,0,0", 1, ""), g8("RESIDUAL", 4, 2)),
    (("t256_k96", 300, 96, 320, "RESIDUAL", 0, TILE256, "320,0,0", 1, ""), big("RESIDUAL", 256, 4, 2)),
    (("t128", 300, 896, 320, "RESIDUAL", 0, TILE128, "320,0,0", 1, ""), big("RESIDUAL", 128, 6, 2)),
    (("streamk", 300, 896, 320, "RESIDUAL", 0, STREAMK, "320,0,0", 1, ""),
     "gemm8sk_kernel<RESIDUAL> dp_rounds=0 chunk=1 n_mt=2 tiles=4 slabs=512 tickets=4 grid=256 threads=512 lds=131072"),
    # ... and without a workspace: the ordinary chain, where 4 tiles fill nothing: generic, 3 x 3
    (("streamk_nows", 300, 896, 320, "RESIDUAL", 0, STREAMK, "320,0,0", 1, "allow_split=0"),
     generic("RESIDUAL", 0, 3, 3)),
    # ---- fp8 activations, Qwen2-7B at 2,048 rows, plain and tiled weights (nk = K / 128): QKV
    # 144 tiles are more than half the chip: unsplit; O 112 tiles, nk 28: 2 parts of 14 (3 parts
    # of 9: two rounds of thirds; 4 parts would be 7 < 8 k-tiles); down nk 148: 2 parts
    (("mx_qkv", 2048, 3584, 4608, "STORE", 0, MX, QKV7, 1, ""), mx("STORE", 0, 144, 8)),
    (("mx_o", 2048, 3584, 3584, "RESIDUAL", 0, MX, "3584,0,0", 1, ""), mx("RESIDUAL", 0, 112, 8, 2)),
    (("mx_gate_up", 2048, 3584, 18944, "SWIGLU", 0, MX, GU7, 1, ""), mx("SWIGLU", 0, 1184, 8)),
    (("mx_down", 2048, 18944, 3584, "RESIDUAL", 0, MX, "3584,0,0", 1, ""), mx("RESIDUAL", 0, 112, 8, 2)),
    (("mxt_qkv", 2048, 3584, 4608, "STORE", 0, MXT, QKV7, 1, ""), mx("STORE", 1, 144, 8)),
    (("mxt_o", 2048, 3584, 3584, "RESIDUAL", 0, MXT, "3584,0,0", 1, ""), mx("RESIDUAL", 1, 112, 8, 2)),
    (("mxt_gate_up", 2048, 3584, 18944, "SWIGLU", 0, MXT, GU7, 1, ""), mx("SWIGLU", 1, 1184, 8)),
    (("mxt_down", 2048, 18944, 3584, "RESIDUAL", 0, MXT, "3584,0,0", 1, ""), mx("RESIDUAL", 1, 112, 8, 2)),
    # 3 tiles, nk 28: 3 parts of 9 (one round of thirds); 8 rows (fp8 activations take this
    # kernel at every M): 14 tiles, 3 parts; no workspace: unsplit
    (("mx_256x768", 256, 3584, 768, "STORE", 0, MX, "768,0,0", 1, ""), mx("STORE", 0, 3, 1, 3)),
    (("mxt_m8_o", 8, 3584, 3584, "RESIDUAL", 0, MXT, "3584,0,0", 1, ""), mx("RESIDUAL", 1, 14, 1, 3)),
    (("mx_o_nows", 2048, 3584, 3584, "RESIDUAL", 0, MX, "3584,0,0", 1, "allow_split=0"), mx("RESIDUAL", 0, 112, 8)),
    # ---- no workspace for the down projection's split: the ring kernel's choices, 256x128
    (("7b_down_nows", 2048, 18944, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, "allow_split=0"),
     big("RESIDUAL", 128, 224, 8)),
    # ---- knobs: QIE_GEMM8 = 1 (full-chip grids only) leaves down to the ring kernel;
    # QIE_GEMM8_SK_MINK = 16 lets O (nk 56) split in 2 x 28 (3 x 18: two rounds of thirds);
    # QIE_MX_SPLITK_MAX = 1: no split; QIE_GEMM8 = 3: stream-K for gate/up, 4 whole rounds of
    # 256 tiles, the last 160 tiles' 8,960 units in 256 ranges of 35
    (("7b_down_g8_1", 2048, 18944, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, "gemm8=1"), big("RESIDUAL", 128, 224, 8)),
    (("7b_o_mink16", 2048, 3584, 3584, "RESIDUAL", 0, 0, "3584,0,0", 1, "sk_mink=16"), g8("RESIDUAL", 112, 8, 2)),
    (("mx_o_max1", 2048, 3584, 3584, "RESIDUAL", 0, MX, "3584,0,0", 1, "mx_splitk_max=1"), mx("RESIDUAL", 0, 112, 8)),
    (("7b_gate_up_g8_3", 2048, 3584, 18944, "SWIGLU", 0, 0, GU7, 1, "gemm8=3"),
     "gemm8sk_kernel<SWIGLU> dp_rounds=4 chunk=35 n_mt=8 tiles=1184 slabs=512 tickets=1184 grid=256 threads=512 lds=131072"),
]


def test_gemm_plan_table():
    subprocess.run(["make", "-s", "-C", CSRC, "plan_dump"], check=True, timeout=300)
    exe = os.path.join(ROOT, "qwen_inference_engine_amd", "_build", "plan_dump")
    text = "".join(" ".join(str(v) for v in row) + "\n" for row, _ in ROWS)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    want = [f"{row[0]}: {line}" for row, line in ROWS]
    assert got == want, "\n".join(f"{g}\n   want {w}" for g, w in zip(got, want) if g != w)
