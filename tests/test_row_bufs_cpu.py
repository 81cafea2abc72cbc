"""CPU: the layout of the engine's row blocks (csrc/row_bufs.hpp: the decode slots, the verify
step's rows, the prefill rows, the scoring rows, each ONE allocation carved into pieces), printed
by the plain host program rowbuf_dump and checked against the byte counts the separate
allocations asked for before the blocks existed (engine.hip's batch_create, ensure_prefill_scratch,
ensure_verify_bufs and ensure_score_scratch, one hipMalloc or `take` per buffer), written here as
formulas in the model's dimensions.

Notation: R rows; H hidden; QD / KD this rank's q / kv width (heads x head_dim); I this rank's
ffn; Vl this rank's vocabulary rows, V the whole vocabulary; bf16 rows are 2 bytes per element,
fp32 partials and int32 words 4, the arg-max keys 8.  The workspace byte counts come from the
kernels' own formulas, so the test passes odd values through and expects them back."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen_inference_engine_amd", "csrc")

# (H, QD, KD, I, Vl, V, head_dim)
Q05 = (896, 14 * 64, 2 * 64, 4864, 151936, 151936, 64)         # Qwen2-0.5B
Q7 = (3584, 28 * 128, 4 * 128, 18944, 152064, 152064, 128)     # Qwen2-7B
Q7_TP2 = (3584, 14 * 128, 2 * 128, 9472, 76032, 152064, 128)   # ... one rank of two
ATTN_WS, SAMP_WS, DEC_WS, MAX_CTX = 1_234_567, 98_765, 7_654_321, 4096


def layer_need(R, H, QD, KD, I, q):
    """x, xn [R][H]; qkv [R][QD + 2 KD]; q (multi-row layers), att [R][QD]; h [R][I]; pos [R]"""
    need = {"x": R * H * 2, "xn": R * H * 2, "qkv": R * (QD + 2 * KD) * 2, "att": R * QD * 2, "h": R * I * 2,
            "pos": R * 4}
    if q:
        need["q"] = R * QD * 2
    return need


def head_need(R, Vl, V, comm):
    """logits [R][Vl], the sampler's workspace, keys [R] u64, ids / step [R]; exchange: the
    gathered logits [R][V] and the all-gather's landing buffer [tp][R][Vl] = [R][V]"""
    need = {"logits": R * Vl * 2, "samp_ws": SAMP_WS, "keys": R * 8, "ids": R * 4, "step": R * 4}
    if comm:
        need.update(logits_full=R * V * 2, gather_tmp=R * V * 2)
    return need


def decode_case(name, dims, B, comm=False):
    H, QD, KD, I, Vl, V, hd = dims
    need = layer_need(B, H, QD, KD, I, q=False)
    need.update(head_need(B, Vl, V, comm))
    # token history [B][max_ctx]; RoPE row of the current position [B][8 + head_dim] fp32; the
    # fused decode attention's partials and counters
    need.update(d_hist=B * MAX_CTX * 4, d_rope_cur=B * (8 + hd) * 4, dec_ws=DEC_WS)
    if comm:
        need["part"] = B * H * 4
    line = f"{name} decode {B} {H} {QD} {KD} {I} {Vl} {V} {ATTN_WS} {SAMP_WS} {int(comm)} {MAX_CTX} {8 + hd} {DEC_WS}"
    return name, line, need, comm


def verify_case(name, dims, comm):
    H, QD, KD, I, Vl, V, _ = dims
    R = 16
    need = layer_need(R, H, QD, KD, I, q=True)
    need.update(head_need(R, Vl, V, comm))
    need.update(attn_ws=ATTN_WS, draft=R * 4, res=(R + 1) * 4)   # res: n_out, then R ids
    if comm:
        need["part"] = R * H * 4
    return name, f"{name} verify {R} {H} {QD} {KD} {I} {Vl} {V} {ATTN_WS} {SAMP_WS} {int(comm)}", need, comm


def prefill_case(name, dims, n, fp8, comm=False):
    H, QD, KD, I, Vl, V, _ = dims
    need = layer_need(n, H, QD, KD, I, q=True)
    need["pf_ids"] = n * 4
    if fp8:   # e4m3 codes [n][widest projection input], one exponent byte per row (at least 16)
        need.update(pf_q8=n * max(H, QD, I), pf_e8=max(n, 16))
    if comm:
        need["part"] = n * H * 4
    return name, f"{name} prefill {n} {H} {QD} {KD} {I} {Vl} {V} {ATTN_WS} {SAMP_WS} {int(comm)} {int(fp8)}", need, comm


def score_case(name, n):
    return name, f"{name} score {n} 0 0 0 0 0 0 0 0 0", {"tgt": n * 4, "ids": n * 4, "lp": n * 4}, False


CASES = [decode_case(f"dec_{m}_B{B}", d, B) for m, d in (("05b", Q05), ("7b", Q7)) for B in (1, 8)]
CASES += [decode_case("dec_7b_tp2_B8_comm", Q7_TP2, 8, comm=True)]
CASES += [verify_case("ver_7b", Q7, False), verify_case("ver_7b_tp2_comm", Q7_TP2, True),
          verify_case("ver_05b", Q05, False), verify_case("ver_05b_comm", Q05, True)]
CASES += [prefill_case(f"pf_{m}_{n}{'_fp8' if fp8 else ''}", d, n, fp8)
          for m, d in (("05b", Q05), ("7b", Q7)) for n in (1, 17, 2048) for fp8 in (False, True)]
CASES += [prefill_case("pf_7b_tp2_17_comm", Q7_TP2, 17, False, comm=True)]
CASES += [score_case("score_1", 1), score_case("score_2048", 2048)]
EXCHANGE = ("part", "logits_full", "gather_tmp")


@pytest.fixture(scope="module")
def layouts():
    """One build and one run of rowbuf_dump over every case: name -> (pieces, total, align);
    pieces = [(piece, offset, bytes, pointer offset)] in carving order"""
    subprocess.run(["make", "-s", "-C", CSRC, "rowbuf_dump"], check=True)
    exe = os.path.join(CSRC, "..", "_build", "rowbuf_dump")
    out = subprocess.run([exe], input="\n".join(c[1] for c in CASES) + "\n", text=True, capture_output=True,
                         check=True).stdout
    got = {c[0]: ([], {}) for c in CASES}
    for ln in out.splitlines():
        f = ln.split()
        assert f[2] != "unlisted" and f[1] != "total_mismatch", ln
        if f[1] in ("total", "align"):
            got[f[0]][1][f[1]] = int(f[2])
        else:
            got[f[0]][0].append((f[1], int(f[2]), int(f[3]), int(f[4])))
    return {k: (p, t["total"], t["align"]) for k, (p, t) in got.items()}


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_layout(layouts, case):
    name, _, need, comm = case
    pieces, total, align = layouts[name]
    assert align >= 16 and align % 16 == 0
    names = [p[0] for p in pieces]
    assert len(set(names)) == len(names)
    # exactly the pieces the set has: none missing, and none it must not carve (the exchange
    # pieces without the exchange; q and attn_ws for decode; the head for prefill)
    assert sorted(names) == sorted(need), (sorted(names), sorted(need))
    if not comm:
        assert not set(names) & set(EXCHANGE)
    if " decode " in case[1]:
        assert "q" not in names and "attn_ws" not in names
    end = 0
    for piece, off, nbytes, ptr in pieces:
        assert ptr == off, f"{piece}: the pointer pass put it at {ptr}, the size pass at {off}"
        assert off % align == 0, f"{piece}: offset {off} is not {align}-byte aligned"
        assert off >= end, f"{piece}: starts at {off}, inside the piece before it (ends {end})"
        assert nbytes >= need[piece], f"{piece}: {nbytes} bytes < the {need[piece]} the buffer needs"
        end = off + max(nbytes, 16)
    assert total >= end and total % align == 0
