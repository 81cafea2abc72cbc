"""CPU: the attention cases of attn_cases.py judge what they claim to judge.

* Every case accepts the float64 reference (rounded to bf16) and oracle.attention in summation
  orders 0, 2 and 7 (the caller slices the cache to the context, so traps do not apply).
* kappa: the oracle's worst excess over the half-ulp term, in units of the mass, is measured
  here on the wide cases and must sit in (ORACLE_EXCESS / 2, ORACLE_EXCESS] of attn_cases.
* Mutants of the float64 reference — one key too many, one key too few, scores off by 2**-6, an
  online softmax without its rescale — are rejected by every kernel's case list, and by the
  needle and ramp cases at every (row, head) whose target or boundary key the mutant touches.
"""
import numpy as np
import pytest

import attn_cases as A

ORDERS = (0, 2, 7)
EXACT = ("needle", "ramp_up", "ramp_down")
EDGE_LENGTHS = (16, 64, 128, 256, 512)   # 256 / 512: the extend kernel's S
MUTANTS = ([("leak",), ("diag",), ("drop0",), ("past",), ("scale",), ("norescale",)]
           + [(k, E) for E in EDGE_LENGTHS for k in ("drop_e", "drop_e1")])


def mutants(kernel):
    """Every mutant whose keys the kernel's contexts hold (the prefill cases end below key 512)."""
    top = max(int(l[2].max()) for l in A.layouts(kernel))
    return [m for m in MUTANTS if len(m) == 1 or m[1] <= top]


def forms(kernel, family):
    if kernel != "decode":
        return (None,)
    if family == "needle":
        return A.DECODE_FORMS
    return ("pre",) if family.startswith("ramp") else ("ref", "pre")


def kernel_cases(oracle, kernel, shape, families=EXACT + ("wide",), traps=(None,), all_forms=True):
    for fam in families:
        for form in forms(kernel, fam)[:None if all_forms else 1]:
            for trap in (traps if fam != "wide" else (None,)):
                for s in (A.WIDE_SCALES if fam == "wide" else (None,)):
                    yield from A.cases(kernel, shape, fam, trap=trap, oracle=oracle, form=form, s=s)


def oracle_out(oracle, c):
    """oracle.attention on the cache sliced to the context, one call per run of consecutive positions."""
    out = np.empty((c.M, c.nq * c.hd), np.uint16)
    m = 0
    while m < c.M:
        b, e = m // c.rps, m + 1
        while e < c.M and e // c.rps == b and c.pos[e] == c.pos[e - 1] + 1:
            e += 1
        n = int(c.pos[e - 1]) + 1
        out[m:e] = oracle.attention(c.q[m:e], c.K[b, A.LAYER, :, :n], c.V[b, A.LAYER, :, :n], c.nq, c.nkv, c.hd, True,
                                    int(c.pos[m]))
        m = e
    return out


KS = [(k, s) for k in A.KERNELS for s in A.SHAPES[k]]


@pytest.mark.parametrize("kernel,shape", KS, ids=[f"{k}-{s[0]}-{s[1]}-{s[2]}" for k, s in KS])
def test_exact_cases_accept_reference_and_oracle(oracle, kernel, shape):
    n = 0
    try:
        for c in kernel_cases(oracle, kernel, shape, EXACT):
            ref, _ = A.ref64(c)
            assert A.accepted(c, A.to_bf16(ref.astype(np.float32))).all(), f"{c.name}: float64 reference"
            for order in ORDERS:
                oracle.set_sum_order(order)
                got = oracle_out(oracle, c)
                ok = A.accepted(c, got)
                assert ok.all(), f"oracle order {order}: " + A.describe(c, got, *np.argwhere(~ok)[0])
            n += 1
    finally:
        oracle.set_sum_order(0)
    print(f"{kernel} {shape}: {n} exact launches accepted")


@pytest.mark.parametrize("kernel", A.KERNELS)
def test_oracle_excess_sets_kappa(oracle, kernel):
    """Family 2: the float64 reference passes, the oracle's worst excess over the half-ulp term
    (orders 0, 2, 7) is the ORACLE_EXCESS the kernel's kappa is 4 x of, and the oracle passes."""
    worst, where = 0.0, None
    try:
        for shape in A.SHAPES[kernel]:
            for c in kernel_cases(oracle, kernel, shape, ("wide",)):
                ref = A.ref64(c)
                assert A.accepted(c, A.to_bf16(ref[0].astype(np.float32)), ref).all(), f"{c.name}: float64 reference"
                for order in ORDERS:
                    oracle.set_sum_order(order)
                    got = oracle_out(oracle, c)
                    x = A.excess(got, *ref).max()
                    if x > worst:
                        worst, where = x, f"{c.name} order {order}"
                    assert A.accepted(c, got, ref).all(), f"{c.name}: oracle order {order}"
    finally:
        oracle.set_sum_order(0)
    k = A.kappa(kernel)
    print(f"{kernel}: oracle excess 2**{np.log2(worst):.2f} of the mass ({where}); ORACLE_EXCESS "
          f"2**{np.log2(A.ORACLE_EXCESS[kernel]):.2f}, kappa 2**{np.log2(k):.2f}")
    assert A.ORACLE_EXCESS[kernel] / 2 < worst <= A.ORACLE_EXCESS[kernel]


@pytest.mark.parametrize("kernel,shape", KS, ids=[f"{k}-{s[0]}-{s[1]}-{s[2]}" for k, s in KS])
def test_needle_targets_cover_every_required_key(kernel, shape):
    """Key 0, pos, pos - 1, e - 1 and e at every edge a row sees, and every key of a sweep."""
    for name, maxc, pos, rps, sweep in A.layouts(kernel):
        pos, edges, sweep, tables = A.targets_of(kernel, shape, name)
        seen = set(np.concatenate([t.reshape(-1) for t in tables]).tolist())
        need = {0} | {int(p) for p in pos} | {max(int(p) - 1, 0) for p in pos}
        for E in edges:
            for e in range(E, int(pos.max()) + 1, E):
                need |= {e - 1, e}
        if sweep is not None:
            need |= set(int(t) for t in sweep)
        assert need <= seen, f"{kernel} {shape} {name}: keys {sorted(need - seen)[:8]} are no needle's target"
        for t in tables[:None if kernel == "decode" else 1]:
            t = t.reshape(len(pos), shape[2], -1)
            for m, p in enumerate(pos):
                assert p in t[m] and max(p - 1, 0) in t[m]
                assert kernel != "decode" or all(p in t[m, g] for g in range(shape[2]))   # the new token, every kv group
        assert len(tables) <= 12, f"{name}: {len(tables)} launches"


def must_reject(c, mut):
    """[M][nq] bool: the (row, head)s of an exact case that cannot survive the mutant."""
    need = np.zeros((c.M, c.nq), bool)
    kind = mut[0]
    for m in range(c.M):
        p, b = int(c.pos[m]), m // c.rps
        vis = A._visible(c, m, mut)
        if kind in ("diag", "drop0", "drop_e", "drop_e1"):
            need[m] = ~np.isin(c.target[m], vis)                       # the target key is gone
        elif kind == "leak" and c.family == "ramp_up":
            need[m] = p + 1 < c.maxc                                   # the next ramp key / the trap wins
        elif kind == "leak" and c.trap in ("nan", "inf"):
            need[m] = p == c.seq_last(b) and p + 1 < c.maxc
        elif kind == "past" and c.trap is not None and c.seq_last(b) + 1 < c.maxc:
            if c.trap != "finite" or c.family.startswith("ramp"):
                need[m] = True
            elif m % c.rps == 0:
                # the trap rows are 2 x the sequence's (row, head-in-group)s in turn, the first of them
                # at last + 1 — decode: at the stale row pos itself, so pos + 1 holds the second
                need[m, (c.kernel == "decode")::c.G] = True
    return need


@pytest.mark.parametrize("kernel", A.KERNELS)
def test_mutants_are_rejected(oracle, kernel):
    rejected = {mut: 0 for mut in mutants(kernel)}
    shapes = A.SHAPES[kernel]
    for si, shape in enumerate(shapes):
        plan = [(EXACT, (None,))]
        if si == 0:
            plan += [(EXACT, ("finite", "nan")), (("wide",), (None,))]
        for fams, traps in plan:
            for c in kernel_cases(oracle, kernel, shape, fams, traps, all_forms=False):
                if c.family == "wide":
                    if c.name.endswith("s 8") and not rejected[("scale",)]:
                        ref = A.ref64(c)
                        assert A.accepted(c, A.to_bf16(ref[0].astype(np.float32)), ref).all()
                        got = A.to_bf16(A.ref64(c, ("scale",))[0].astype(np.float32))
                        rejected[("scale",)] += int((~A.accepted(c, got, ref)).sum())
                    continue
                for mut in rejected:
                    if mut[0] == "scale":
                        continue
                    if mut[0] == "norescale":
                        need = np.zeros((c.M, c.nq), bool)
                        need[c.pos >= 64] = c.family == "ramp_up"   # a second tile whose max is larger
                    else:
                        need = must_reject(c, mut)
                    rows = np.flatnonzero(need.any(axis=1))
                    if len(rows) == 0:
                        continue
                    got = A.ref64(c, mut, rows)[0]
                    bits = np.where(np.isfinite(got), A.to_bf16(np.nan_to_num(got).astype(np.float32)), A.NAN)
                    ok = A.accepted(c, bits)
                    sel = np.zeros(c.M, bool)
                    sel[rows] = True
                    bad = ok & need & sel[:, None]
                    assert not bad.any(), f"mutant {mut} survives: " + A.describe(c, bits, *np.argwhere(bad)[0])
                    rejected[mut] += int((need & sel[:, None]).sum())
    print(f"{kernel}: (row, head)s rejected per mutant: " + ", ".join(f"{'/'.join(map(str, k))} {v}" for k, v in rejected.items()))
    missed = [k for k, v in rejected.items() if v == 0]
    assert not missed, f"{kernel}: no case rejects {missed}"
