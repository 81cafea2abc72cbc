"""plan_gemm's choices for the MXFP4 prefill GEMM (QIE_LINEAR_FP4 | _FP4_GEMM, M > 16) through
tools/plan_dump on 256 CUs; the fp4 flags without the new one still refuse M > 16 (PlanError 6) and
flags 0 plan at the same shapes what they planned."""
import os
import subprocess

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "qwen_inference_engine_amd", "csrc")
FP4, T16, GEMM = 64, 128, 256
T = "threads=512 lds=131072"
# (name, M, K, N, epilogue, flags, segs [knob], the plan line); Qwen2-7B at 2,048 rows: O / down 112 tiles -> 2 parts
ROWS = [
    ("m17", 17, 1024, 64, "STORE", FP4 | GEMM, "64,0,0", f"gemm4_kernel<STORE,0> splitk=1 n_mt=1 tiles=1 slabs=0 tickets=0 grid=1 {T}"),
    ("m17_t16", 17, 1024, 64, "STORE", FP4 | T16 | GEMM, "64,0,0", f"gemm4_kernel<STORE,1> splitk=1 n_mt=1 tiles=1 slabs=0 tickets=0 grid=1 {T}"),
    ("gateup", 2048, 3584, 18944, "SWIGLU", FP4 | T16 | GEMM, "18944,18944,0",
     f"gemm4_kernel<SWIGLU,1> splitk=1 n_mt=8 tiles=1184 slabs=0 tickets=0 grid=1184 {T}"),
    ("qkv", 2048, 3584, 4608, "STORE", FP4 | T16 | GEMM, "3584,512,512", f"gemm4_kernel<STORE,1> splitk=1 n_mt=8 tiles=144 slabs=0 tickets=0 grid=144 {T}"),
    ("o", 2048, 3584, 3584, "RESIDUAL", FP4 | T16 | GEMM, "3584,0,0", f"gemm4_kernel<RESIDUAL,1> splitk=2 n_mt=8 tiles=112 slabs=224 tickets=112 grid=224 {T}"),
    ("down", 2048, 18944, 3584, "RESIDUAL", FP4 | GEMM, "3584,0,0", f"gemm4_kernel<RESIDUAL,0> splitk=2 n_mt=8 tiles=112 slabs=224 tickets=112 grid=224 {T}"),
    ("down_no_ws", 2048, 18944, 3584, "RESIDUAL", FP4 | GEMM, "3584,0,0 allow_split=0",
     f"gemm4_kernel<RESIDUAL,0> splitk=1 n_mt=8 tiles=112 slabs=0 tickets=0 grid=112 {T}"),
    ("m16_flag", 16, 1024, 64, "STORE", FP4 | GEMM, "64,0,0", "dec4 KU=2 KS=4 parts=1 t16=0"),
    ("m17_noflag", 17, 1024, 64, "STORE", FP4, "64,0,0", "error 6"),
    ("m2048_noflag", 2048, 3584, 3584, "RESIDUAL", FP4 | T16, "3584,0,0", "error 6"),
    ("bf16_m17", 17, 1024, 64, "STORE", 0, "64,0,0", "gemm_kernel<STORE,0> n_mt=1 tiles=1 slabs=0 tickets=0 grid=1 threads=256 lds=65536"),
    ("bf16_o", 2048, 3584, 3584, "RESIDUAL", 0, "3584,0,0", "gemm_big_kernel<RESIDUAL,128> n_mt=8 tiles=224 slabs=0 tickets=0 grid=224 threads=512 lds=98304"),
    ("bf16_down", 2048, 18944, 3584, "RESIDUAL", 0, "3584,0,0", f"gemm8_kernel<RESIDUAL> splitk=2 n_mt=8 tiles=112 slabs=224 tickets=112 grid=224 {T}"),
]


@pytest.fixture(scope="module")
def plans():
    subprocess.check_call(["make", "-s", "-C", CSRC, "plan_dump"])
    text = "".join(f"{n} {M} {K} {N} {epi} 0 {fl} {segs.split()[0]} 1 {' '.join(segs.split()[1:])}\n"
                   for n, M, K, N, epi, fl, segs, _ in ROWS)
    out = subprocess.run([os.path.join(CSRC, "..", "_build", "plan_dump")], input=text, capture_output=True, text=True, check=True)
    return dict(line.split(": ", 1) for line in out.stdout.splitlines())


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_fp4_gemm_plan(plans, row):
    assert plans[row[0]] == row[-1]
