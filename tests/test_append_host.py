"""CPU: the host side of append prefill — the chunk planning of Batch.prefill(chunk=) and
ContinuousBatcher(prefill_chunk=), and the declaration / binding of qie_prefill_append."""
import os
import re

import pytest

from conftest import ROOT

from qwen_inference_engine_amd import _lib
from qwen_inference_engine_amd.scheduler import prefill_chunks


def test_prefill_chunks_pieces():
    assert prefill_chunks(100, None) == [(0, 100)]
    assert prefill_chunks(21, 32) == [(0, 21)]                      # below the chunk
    assert prefill_chunks(32, 32) == [(0, 32)]                      # at the chunk
    assert prefill_chunks(33, 32) == [(0, 32), (32, 1)]             # just above
    assert prefill_chunks(100, 32) == [(0, 32), (32, 32), (64, 32), (96, 4)]
    assert prefill_chunks(64, 32) == [(0, 32), (32, 32)]
    assert prefill_chunks(3, 1) == [(0, 1), (1, 1), (2, 1)]
    for n, c in [(1, 1), (7, 3), (4096, 512), (1000, 999)]:
        pieces = prefill_chunks(n, c)
        assert pieces[0][0] == 0 and sum(ln for _, ln in pieces) == n
        assert all(0 < ln <= c for _, ln in pieces)
        assert all(a[0] + a[1] == b[0] for a, b in zip(pieces, pieces[1:]))


def test_prefill_chunks_rejects_nonsense():
    for n, c in [(0, 8), (5, 0), (5, -1), (0, None)]:
        with pytest.raises(ValueError):
            prefill_chunks(n, c)


def test_prefill_append_declared_and_bound():
    text = open(os.path.join(ROOT, "include", "qie", "qie_engine.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\bint\s+qie_prefill_append\s*\(([^)]*)\)\s*;", text)
    assert m, "qie_engine.h does not declare qie_prefill_append"
    n_args = len([a for a in m.group(1).split(",") if a.strip()])
    bound = {n: args for n, _, args in _lib.SIGNATURES}
    assert "qie_prefill_append" in bound
    assert len(bound["qie_prefill_append"]) == n_args == 7
    # the operator underneath is declared and bound too
    ops = open(os.path.join(ROOT, "include", "qie", "qie_ops.h")).read()
    for name in ("qie_attention_extend", "qie_attention_extend_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, ops) and name in bound
