"""CPU: the fp8 KV cache's C ABI — the new ops are exported and bound, the descriptor structs of
the binding match include/qie/qie_ops.h, and the existing structs kept their sizes."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT
from qwen_inference_engine_amd import _lib

OPS = ("qie_qkv_post_fp8", "qie_attention_decode_fp8", "qie_kv_dequantize_fp8", "qie_kv_copy_fp8",
       "qie_batch_kv_cache_fp8", "qie_batch_kv_bytes")


def test_fp8_kv_ops_exported_and_bound(qlib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(OPS) <= exported, sorted(set(OPS) - exported)
    bound = {n: a for n, _, a in _lib.SIGNATURES}
    assert [len(bound[n]) for n in OPS] == [17, 15, 9, 7, 3, 2]
    # bad arguments are refused before any HIP call
    assert qlib.qie_kv_copy_fp8(None, 0, None, 1, 0, 1, None) == -22
    assert b"qie_kv_copy_fp8" in qlib.qie_last_error()


def test_kv_cache_structs_match_the_header():
    text = open(os.path.join(ROOT, "include", "qie", "qie_ops.h")).read()
    body = re.search(r"typedef struct qie_kv_cache_fp8 \{(.*?)\} qie_kv_cache_fp8;", text, flags=re.S).group(1)
    names = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [n for n, _ in _lib.KvCacheFp8C._fields_] == names == ["c", "k_exps", "v_exps", "exp_stride"]
    # qie_kv_cache is unchanged (compat.hpp and the tools declare it uninitialised); the fp8 form
    # wraps it and adds two pointers and one stride
    assert C.sizeof(_lib.KvCacheC) == 56 and C.sizeof(_lib.EngineOptsC) == 64
    assert _lib.KvCacheFp8C.c.offset == 0 and _lib.KvCacheFp8C.k_exps.offset == 56
    assert C.sizeof(_lib.KvCacheFp8C) == 56 + 24


def test_engine_opts_kv_fp8_takes_reserved_0():
    text = open(os.path.join(ROOT, "include", "qie", "qie_engine.h")).read()
    body = re.search(r"typedef struct qie_engine_opts \{(.*?)\} qie_engine_opts;", text, flags=re.S).group(1)
    names = re.findall(r"(\w+)(?:\[\d+\])?\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert [n for n, _ in _lib.EngineOptsC._fields_] == names and names[-2:] == ["kv_fp8", "reserved"]
    assert _lib.EngineOptsC.kv_fp8.offset == 48 and C.sizeof(_lib.EngineOptsC) == 64   # reserved[4] began at 48
