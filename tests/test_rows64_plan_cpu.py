"""CPU: the launch plan of the 17..64-row decode kernel (csrc/rows64_plan.hpp, QIE_LINEAR_ROWS64 =
512), printed by plan_dump on 256 CUs and compared with a table derived by hand from the rule:

  tiles = ceil(N / 16), col_blocks = ceil(tiles / 4), chunks = ceil(K / 256), MT = ceil(M / 16),
  NB = 2 for SWIGLU else 1;
  parts0 = max(1, min(512 / col_blocks, chunks / 2, 16, 8192 / (tiles * NB)));
  cpp = ceil(chunks / parts0), parts = ceil(chunks / cpp), grid = col_blocks * parts;
  lds = MT * 16 * 528; ws = tiles * parts * NB * MT * 1024 when parts >= 2, else 0.

Per shape (7B: hidden 3,584, QKV 4,608, ffn 18,944; 0.5B: 896, 1,152, 4,864) the min() terms are
written beside its row of SHAPES below.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen_inference_engine_amd", "csrc")

# name: (K, N, epilogue, seg rows, tiles, col_blocks, chunks, parts, cpp, grid, NB)
SHAPES = {
    "7b_qkv": (3584, 4608, "STORE", "3584,512,512", 288, 72, 14, 7, 2, 504, 1),           # min(7, 7, 16, 28)
    "7b_o": (3584, 3584, "RESIDUAL", "3584,0,0", 224, 56, 14, 7, 2, 392, 1),             # min(9, 7, 16, 36)
    "7b_gate_up": (3584, 18944, "SWIGLU", "18944,18944,0", 1184, 296, 14, 1, 14, 296, 2),  # min(1, 7, 16, 3)
    "7b_down": (18944, 3584, "RESIDUAL", "3584,0,0", 224, 56, 74, 9, 9, 504, 1),         # min(9, 37, 16, 36)
    "05b_qkv": (896, 1152, "STORE", "896,128,128", 72, 18, 4, 2, 2, 36, 1),              # min(28, 2, ..)
    "05b_o": (896, 896, "RESIDUAL", "896,0,0", 56, 14, 4, 2, 2, 28, 1),                  # min(36, 2, ..)
    "05b_gate_up": (896, 4864, "SWIGLU", "4864,4864,0", 304, 76, 4, 2, 2, 152, 2),       # min(6, 2, 16, 13)
    "05b_down": (4864, 896, "RESIDUAL", "896,0,0", 56, 14, 19, 7, 3, 98, 1),   # min(36, 9, 16, 146) = 9: cpp 3, parts 7
}


def _rows():
    for name, (K, N, epi, segs, tiles, cb, chunks, parts, cpp, grid, nb) in SHAPES.items():
        for M, mt in ((17, 2), (64, 4)):
            for flags, wt in ((512, 0), (512 + 1 + 16, 2)):   # bf16; QIE_LINEAR_FP8 | QIE_LINEAR_FP8_T16
                ws = tiles * parts * nb * mt * 1024 if parts >= 2 else 0
                yield (f"{name} {M} {K} {N} {epi} 0 {flags} {segs} 0",
                       f"{name}: rows64_kernel<{epi},{wt},{mt}> tiles={tiles} col_blocks={cb} chunks={chunks} "
                       f"parts={parts} cpp={cpp} grid={grid} threads=256 lds={mt * 16 * 528} ws={ws}")
    # without the flag the plan is what it was: the generic GEMM (tests/test_gemm_plan_cpu.py's wording)
    yield ("7b_qkv_noflag 64 3584 4608 STORE 0 0 3584,512,512 0",
           "7b_qkv_noflag: gemm_kernel<STORE,0> n_mt=1 tiles=36 slabs=0 tickets=0 grid=1x36 threads=256 lds=65536")
    # refusals print their error: 16 rows (Rows = 1), an MXFP4 flag (Flags = 2), a fused norm (Norm = 4)
    yield ("m16 16 3584 4608 STORE 0 512 3584,512,512 0", "m16: rows64 error 1")
    yield ("fp4 32 3584 4608 STORE 0 576 3584,512,512 0", "fp4: rows64 error 2")
    yield ("norm 32 3584 4608 STORE 1 512 3584,512,512 0", "norm: rows64 error 4")


ROWS = list(_rows())


@pytest.fixture(scope="module")
def dumped():
    subprocess.run(["make", "-s", "-C", CSRC, "plan_dump"], check=True, timeout=300)
    exe = os.path.join(ROOT, "qwen_inference_engine_amd", "_build", "plan_dump")
    r = subprocess.run([exe], input="".join(line + "\n" for line, _ in ROWS), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout.splitlines()


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[line.split()[0] + "_m" + line.split()[1] + "_f" + line.split()[6]
                                                     for line, _ in ROWS])
def test_rows64_plan(dumped, i):
    assert dumped[i] == ROWS[i][1]
