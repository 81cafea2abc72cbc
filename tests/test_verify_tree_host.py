"""CPU: the host side of tree verification — the new C functions are exported and
bound, qie_verify_tree refuses a null batch and a malformed tree before any HIP call, and
NgramDrafter.propose_tree builds a well-formed trie."""
import ctypes as C
import subprocess

import pytest

from qwen_inference_engine_amd import _lib
from qwen_inference_engine_amd.speculative import NgramDrafter

NEW = {"qie_verify_tree", "qie_qkv_post_tree", "qie_attention_extend_tree", "qie_kv_compact"}


def test_new_symbols_are_exported_and_bound(qlib):
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH]).decode()
    assert NEW <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert NEW <= {n for n, _, _ in _lib.SIGNATURES}
    assert C.sizeof(_lib.DraftTreeC) == 64


def _tree(n, parents=()):
    return _lib.DraftTreeC(n, (C.c_int32 * 15)(*parents))


@pytest.mark.parametrize("tree,word", [(_tree(2, [0, 1]), b"bad arguments"),      # well formed: the null batch
                                       (_tree(2, [0, 2]), b"malformed tree"),     # parent[i - 1] >= i
                                       (_tree(3, [0, -1, 0]), b"malformed tree"),
                                       (_tree(16), b"malformed tree"),
                                       (_tree(-1), b"malformed tree")])
def test_refused_without_a_gpu(qlib, tree, word):
    draft, out, n = (C.c_int32 * 16)(), (C.c_int32 * 16)(), C.c_int32(7)
    assert qlib.qie_verify_tree(None, 0, draft, C.byref(tree), None, out, C.byref(n)) == -22
    assert b"qie_verify_tree" in qlib.qie_last_error() and word in qlib.qie_last_error()
    assert n.value == 7


def test_propose_tree_merges_recent_continuations():
    #    ... 5 6 [1 2 3]   5 6 [1 2 4]   5 6 [9]   5 6 ?
    h = [5, 6, 1, 2, 3, 5, 6, 1, 2, 4, 5, 6, 9, 5, 6]
    d = NgramDrafter(max_ngram=2)
    assert d.propose_tree(h, 4, 1) == (d.propose(h, 4), [0, 1, 2]) == ([9, 5, 6], [0, 1, 2])   # width 1: propose()'s chain
    ids, parents = d.propose_tree(h, 8, 3)
    # most recent first: 9 5 6 (to the end of the history), then 1 2 4 5 ..., then 1 2 3 sharing 1 2
    assert ids[:3] == [9, 5, 6] and parents[:3] == [0, 1, 2]
    assert ids[3:] == [1, 2, 4, 5, 6][:5] and parents[3:] == [0, 4, 5, 6, 7]
    assert d.propose_tree([1, 2, 3], 4, 2) == ([], [])
