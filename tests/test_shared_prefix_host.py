"""CPU: the shared-prefix decode attention's symbols, binding and argument refusals (no GPU)."""
import ctypes as C
import subprocess

import pytest

from qwen_inference_engine_amd import _lib
from qwen_inference_engine_amd._lib import KvCacheC

OPS = ("qie_attention_decode_shared_workspace_bytes", "qie_attention_decode_shared", "qie_batch_shared_prefix")


def test_shared_prefix_symbols_exported_and_bound(qlib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(OPS) <= exported, sorted(set(OPS) - exported)
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    assert [len(bound[n]) for n in OPS] == [5, 16, 3]
    assert C.sizeof(_lib.PrefixShareC) == 8
    # 2 x nj partial slots of head_dim + 2 floats per (row, head): max_ctx 512 is 4 splits of 128 keys
    assert qlib.qie_attention_decode_shared_workspace_bytes(6, 8, 1, 64, 512) == 6 * 8 * 8 * 66 * 4
    assert qlib.qie_batch_shared_prefix(None, None, None) == -22


@pytest.mark.parametrize("case", ["null_share", "null_ws", "B0", "B9", "hd96", "group9", "layer"])
def test_shared_decode_refuses_before_any_hip_call(qlib, case):
    """Every pointer is a host dummy: a refusal that came after a launch would not return -22."""
    buf = (C.c_char * 64)()
    p = C.addressof(buf)
    c = KvCacheC()
    c.k, c.v, c.seq_stride = p, p, 2 * 1 * 512 * 64
    c.n_layers, c.n_kv_heads, c.head_dim, c.max_ctx = 2, 1, 96 if case == "hd96" else 64, 512
    B = {"B0": 0, "B9": 9}.get(case, 6)
    rc = qlib.qie_attention_decode_shared(p, B, p, None if case == "null_share" else p, None, None, p, p,
                                          9 if case == "group9" else 8, C.byref(c), 2 if case == "layer" else 1, 1e-6, 0,
                                          p, None if case == "null_ws" else p, None)
    assert rc == -22
