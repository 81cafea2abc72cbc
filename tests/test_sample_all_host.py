"""CPU: QIE_TOP_K_ALL is one value in the header, in _lib and in the contract's text."""
import os
import re

from qwen_inference_engine_amd import _lib

INC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "qie")


def test_top_k_all_is_exported_and_named_by_the_contract():
    types = open(os.path.join(INC, "qie_types.h")).read()
    m = re.search(r"#define\s+QIE_TOP_K_ALL\s+\((-?\d+)\)", types)
    assert m and int(m.group(1)) == _lib.QIE_TOP_K_ALL == -1
    ops = open(os.path.join(INC, "qie_ops.h")).read()
    contract = ops[ops.index("per-row sampling entries"):ops.index("typedef struct qie_sample_rows_args")]
    assert "top_k == QIE_TOP_K_ALL" in contract
