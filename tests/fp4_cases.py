"""The MXFP4 linear kernel (csrc/k_decode_fp4.hip), one op-level case per form its planner picks.

dec4_plan() (csrc/linear_plan.hpp) chooses the K slice shape by K alone: KU units of 128 columns
per wave (2 up to 8 units, 4 up to 32, 8 up to 64), KS = ceil(units / KU) waves, and split-K parts
of 8 waves x 2 units beyond 64 units.  Every row is the smallest K that reaches its (KU, KS, parts)
-- (KS - 1) * KU + 1 units, so the last wave's slice is ragged -- with the plan worded as
tools/plan_dump prints it.  tests/test_fp4_host.py checks the declarations against plan_dump and
that a grid of shapes reaches no undeclared form; tests/test_gpu_fp4.py runs every row against the
CPU oracle on the dequantised weights.

Rows reuse tests/linear_cases.py's Case tuple (segs, norm, pads, key_col0, bias, twice).  The
MANY_TILES rows hold more column tiles than resident blocks, so a block walks several tiles: the
per-tile hand-off (two tiles) and the deferred reduction (three and more; packed two tiles to a
slot at M <= 8).  Plain data and small helpers: no test, no fixture.
"""
import re

from linear_cases import C, EPIS

FP4 = 64        # QIE_LINEAR_FP4
FP4_T16 = 128   # QIE_LINEAR_FP4_T16


def plan(ku, ks, parts=1):
    return f"dec4 KU={ku} KS={ks} parts={parts}"


def _unsplit():
    rows = []
    i = 0
    for ku, ks_range in ((2, range(1, 5)), (4, range(3, 9)), (8, range(5, 9))):
        for ks in ks_range:
            units = (ks - 1) * ku + 1
            epi = EPIS[i % 4]
            M = (1, 2, 5, 8, 9, 13, 16)[i % 7]
            norm = (None, "ref", "hf")[i % 3]
            segs = {"STORE": (32, 16, 24), "RESIDUAL": 41, "SWIGLU": 40, "F32": 24}[epi]
            rows.append(C(f"ku{ku}_ks{ks}_{epi.lower()}_m{M}", M, 128 * units, segs, epi, plan(ku, ks), norm=norm,
                          flags=FP4, bias=(epi == "STORE"), key_col0=(7 if epi == "STORE" and i % 2 == 0 else None),
                          ldx_pad=8 if i % 2 else 0, ldy_pad=3 if i % 3 == 0 else 0))
            i += 1
    return rows


CASES = _unsplit() + [
    # whole slices (no ragged wave) at the widest block of each KU, every epilogue not met above
    C("ku2_ks4_full_swiglu_norm", 16, 1024, 40, "SWIGLU", plan(2, 4), norm="hf", flags=FP4),
    C("ku4_ks8_full_res", 7, 4096, 41, "RESIDUAL", plan(4, 8), flags=FP4),
    C("ku4_ks7_store_norm_keys", 8, 3584, (64, 16, 16), "STORE", plan(4, 7), norm="ref", flags=FP4, bias=True,
      key_col0=0),
    C("ku8_ks8_full_f32_norm", 3, 8192, 24, "F32", plan(8, 8), norm="ref", flags=FP4),
    C("ku8_ks5_swiglu_norm", 16, 5120, 40, "SWIGLU", plan(8, 5), norm="ref", flags=FP4),
    C("ku8_ks7_res_norm", 11, 6272, 41, "RESIDUAL", plan(8, 7), norm="hf", flags=FP4),
    # ------------------------------------------------------------------ split-K (no norm, one
    # segment): parts of 16 units; 65 units = 5 parts with a last part of ONE unit (seven of its
    # waves idle), 129 / 145 / 225 units the part counts of K = 17,408 / 18,944 / 29,568
    C("split5_res_ragged", 16, 8320, 41, "RESIDUAL", plan(2, 8, 5), flags=FP4, twice=True),
    C("split9_f32", 5, 16512, 24, "F32", plan(2, 8, 9), flags=FP4, twice=True),
    C("split10_store_bias_keys", 8, 18560, 40, "STORE", plan(2, 8, 10), flags=FP4, bias=True, key_col0=3, twice=True,
      ldy_pad=5),
    C("split15_res", 1, 28800, 24, "RESIDUAL", plan(2, 8, 15), flags=FP4, twice=True, ldx_pad=16),
]

# more column tiles than resident blocks (256 CUs: 768 four-wave blocks, 512 eight-wave ones)
MANY_TILES = [
    C("mt_ku4_swiglu_defer_m16", 16, 1152, 18944, "SWIGLU", plan(4, 3), norm="ref", flags=FP4, twice=True),
    C("mt_ku4_swiglu_defer_packed_m5", 5, 1152, 18944, "SWIGLU", plan(4, 3), norm="hf", flags=FP4, twice=True),
    C("mt_ku4_store_two_tiles_keys", 3, 1152, (8192, 256, 272), "STORE", plan(4, 3), flags=FP4, bias=True, key_col0=0,
      twice=True),
    C("mt_ku2_res_defer_m9", 9, 384, 32768, "RESIDUAL", plan(2, 2), flags=FP4, twice=True),
    C("mt_ku8_f32_two_tiles", 4, 4224, 8208, "F32", plan(8, 5), flags=FP4, twice=True),
    # split-K, 10 parts: 128 tiles on the 51 to 76 blocks each part gets, two or three tiles a block
    C("mt_split10_res_three_tiles", 8, 18560, 2048, "RESIDUAL", plan(2, 8, 10), flags=FP4, twice=True),
]

# shapes qie_linear refuses with fp4 flags (rc -22): (name, M, K, N, epilogue, norm, flags, words)
REFUSALS = [
    ("m17", 17, 1024, 64, "STORE", 0, FP4, "1 <= M <= 16"),
    ("m300", 300, 1024, 64, "STORE", 0, FP4, "1 <= M <= 16"),
    ("k192", 4, 192, 64, "STORE", 0, FP4, "K % 128 == 0"),
    ("k64", 1, 64, 64, "RESIDUAL", 0, FP4, "K % 128 == 0"),
    ("with_fp8", 4, 1024, 64, "STORE", 0, FP4 | 1, "combine"),
    ("with_fp8_t16", 4, 1024, 64, "STORE", 0, FP4 | 16, "combine"),
    ("with_act_fp8", 4, 1024, 64, "STORE", 0, FP4 | 32, "combine"),
    ("t16_alone", 4, 1024, 64, "STORE", 0, FP4_T16, "combine"),
    ("split_norm", 4, 8320, 64, "STORE", 1, FP4, "does not take"),
    ("split_swiglu", 4, 8320, 64, "SWIGLU", 0, FP4, "does not take"),
    ("n_vocab", 4, 1024, 32784, "STORE", 0, FP4, "does not take"),
    ("k_past_16_parts", 4, 128 * 257, 64, "RESIDUAL", 0, FP4, "does not take"),
    ("t16_ragged_n", 4, 1024, 40, "STORE", 0, FP4 | FP4_T16, "does not take"),
]

_KEY = re.compile(r"(dec4 KU=\d+ KS=\d+ parts=\d+)")


def plan_key(text):
    """The (KU, KS, parts) form at the start of a plan line, None for other plans and errors."""
    m = _KEY.match(text)
    return m.group(1) if m else None
