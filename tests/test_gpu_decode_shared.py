"""GPU: decode mode 2 (qie_batch_set_decode_mode(b, 2)) — the decode step with the
shared-prefix attention — against a twin batch built the same way that stays in mode 0: the share
table the engine derives, teacher-forced steps through forks, a release of the leader and a
copy-on-write, and what the switch refuses."""
import numpy as np
import pytest

import qwen_inference_engine_amd as Q
from conftest import rng
from parity import max_flips, norm_rel
from qwen_inference_engine_amd import _lib
from test_gpu_engine import CONFIGS, SYN

pytestmark = pytest.mark.gpu

T = 128


def build(eng, spec, mode):
    """Slot 0 prefilled with 300 ids, forked to 1 and 2 at 300 and to 3 at 200."""
    b = eng.batch(4, 512, page_tokens=T)
    b.prefill(0, [int(t) for t in rng(5).integers(0, spec.vocab, 300)])
    b.fork(0, 1)
    b.fork(0, 2)
    b.fork(0, 3, 200)
    b.set_decode_mode(mode)
    assert b.decode_mode == mode
    return b


def forced_steps(pair, spec, live, t0, n):
    """n teacher-forced steps on both batches (slot i is fed token (7 + 13 i + 31 t) % vocab, so the
    slots diverge); returns the id flips among the live slots' choices."""
    flips = 0
    for t in range(t0, t0 + n):
        pos = pair[0].positions()
        for b in pair:
            for i in live:
                b.set_position(i, int(pos[i]), (7 + 13 * i + 31 * t) % spec.vocab)
        ids = [b.decode_step() for b in pair]
        lg = [b.logits() for b in pair]
        for i in live:
            rel = norm_rel(lg[1][i], lg[0][i])
            assert rel <= 1e-3, f"step {t} slot {i}: norm_rel {rel:.3e}"   # README "Parity": the end-to-end floor
            flips += ids[0][i] != ids[1][i]
        p0, p1 = pair[0].positions(), pair[1].positions()
        assert p0.tolist() == p1.tolist()
        assert all(np.array_equal(pair[0].history(i, int(p0[i]) + 1), pair[1].history(i, int(p0[i]) + 1)) for i in live)
        assert pair[0].page_stats()[1].tolist() == pair[1].page_stats()[1].tolist()
        assert pair[0].page_refs().tolist() == pair[1].page_refs().tolist()
    return flips


@pytest.mark.parametrize("name", ["qwen2-bias-hd64", "qwen3-qknorm-hd128"])
def test_mode2_follows_forks_release_and_copy_on_write(name):
    spec = CONFIGS[name]
    eng = Q.Engine(spec, max_ctx=512).init_synthetic(SYN)
    twin, b = build(eng, spec, 0), build(eng, spec, 2)
    assert b.shared_prefix() == ([0, 0, 0, 0], [256, 256, 256, 128])
    assert twin.shared_prefix() == ([0, 1, 2, 3], [0, 0, 0, 0])
    flips = forced_steps((twin, b), spec, [0, 1, 2, 3], 0, 12)
    assert b.shared_prefix() == ([0, 0, 0, 0], [256, 256, 256, 128])   # growth is not sharing
    for x in (twin, b):
        x.release(0)
    assert b.shared_prefix() == ([0, 1, 1, 1], [0, 256, 256, 128])     # the leader moves to slot 1
    flips += forced_steps((twin, b), spec, [1, 2, 3], 12, 3)
    for x in (twin, b):
        x.set_position(2, 200, 5)                                      # into its second shared page: copy-on-write
    assert b.shared_prefix() == ([0, 1, 1, 1], [0, 128, 128, 128])     # (a leader's entry is its members' maximum)
    flips += forced_steps((twin, b), spec, [1, 2, 3], 15, 3)
    assert flips <= max_flips(12 * 4 + 6 * 3), flips


@pytest.mark.parametrize("case", ["contiguous", "fp8_kv", "mode_3"])
def test_mode2_refusals(case):
    """rc = -22, the batch unchanged: in mode 0 it continues as a twin on which the call was never made."""
    spec = CONFIGS["qwen2-bias-hd64"]
    eng = Q.Engine(spec, max_ctx=256, kv_fp8=case == "fp8_kv").init_synthetic(SYN)
    twin, b = (eng.batch(2, 256, **({} if case == "contiguous" else dict(page_tokens=T))) for _ in range(2))
    for x in (twin, b):
        x.prefill(0, [3, 4, 5])
    before = (b.decode_mode, b.positions().tolist(), b.shared_prefix())
    with pytest.raises(_lib.QieError, match=r"rc=-22.*fp8-KV" if case == "fp8_kv" else r"rc=-22"):
        b.set_decode_mode(3 if case == "mode_3" else 2)
    assert (b.decode_mode, b.positions().tolist(), b.shared_prefix()) == before
    b.set_decode_mode(0)
    assert twin.decode_step()[0] == b.decode_step()[0] and np.array_equal(twin.logits()[0], b.logits()[0])
