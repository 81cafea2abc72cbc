"""Attention cases that see every key: builders, a float64 reference and the acceptance rules
shared by test_attn_cases_cpu.py (no GPU) and test_gpu_attention_keys.py (the four kernels:
the split kernel and the MFMA prefill walk behind qie_attention, qie_attention_extend and its
merge, the fused qie_attention_decode).  Pure numpy; the oracle module is passed in where a
case needs its qk-norm / RoPE.

Why: with N(0, 1) q / K / V and an absolute bar of 2**-6 the softmax is diffuse and one key
carries almost no weight — a kernel that leaks key pos + 1, drops a row's own key or the
first key of a tile stays under the bar on every row with more than a few dozen keys.

Family 1 — exact cases (np.array_equal, no tolerance).  V rows are pairwise distinct codes
over the whole cache (vcode: every element one of +-k/64, 1 <= k <= 255, so non-zero, exact
in bf16 and of magnitude in [2**-6, 4); elements 0..2 hold the row id) and the builder
asserts, in float64, 1 - w <= 2**-30 for the intended key of every (row, head): fp32 l is
then exactly 1 and the output rounds to that key's V row, bit for bit.
  * needles: the K row of the target key is the bits of the query row (after qk-norm and
    RoPE where the op applies them); q ~ N(0, 4**2) at hd 64, N(0, 3**2) at hd 128, every
    other key N(0, 0.25**2).  (row, head)s that target the same key share the query bits.
  * ramps: q = (+-8192, +-256, 0, ...), K[t] = (t // 32, t % 32, 0, ...): the dot is exactly
    +-256 t.  Ascending: every row returns V[pos] (a leaked later key or a dropped diagonal
    returns another row; the running max grows at every key).  Descending: V[0].
  * traps: the same cases with the cache past each sequence's last position (and, paged,
    the page tails, page 0 and the pages no table row uses) holding K = 2 x a query row and
    a distinct V code ("finite": a leak dominates and names itself), bf16 NaN 0x7FC0 or
    +Inf 0x7F80.  The expected output does not change.

Family 2 — arithmetic over a wide score range.  q ~ N(0, s**2), s in {1, 4, 8}, K, V ~
N(0, 1); against ref64, every element:
    |got - ref| <= half a bf16 ulp of max(|got|, |ref|) + kappa * sum_t w_t |v_t|
kappa is 4 x the oracle's own worst excess over the half-ulp term in units of the mass
(orders 0, 2 and 7 on these very inputs, measured by test_attn_cases_cpu.py — nothing is
measured from a HIP kernel), plus 2**-16 for the MFMA prefill and extend kernels, whose P is
carried in two bf16 parts (attn_mfma_tile.hpp: dropped remainder < 2**-16 of p); the decode
kernel carries three parts and the split kernel fp32 probabilities: no such term.
Measured oracle excess (ORACLE_EXCESS, worst over the committed wide cases of each kernel)
and the resulting kappa (ORACLE_EXCESS is the measurement rounded up by 0.1 in the exponent,
so that one more ulp in a libm exponential does not move the pinned constant):
    split    2**-19.47 (hd 128, m9, s 8, order 7)              ORACLE_EXCESS 2**-19.35, kappa 2**-17.35
    prefill  2**-19.17 (hd 128, two sequences, s 8, order 7)   ORACLE_EXCESS 2**-19.05, kappa 2**-17.05 + 2**-16
    extend   2**-18.44 (hd 128, pos0 1,000 n 40, s 4, order 0) ORACLE_EXCESS 2**-18.3, kappa 2**-16.3 + 2**-16
    decode   2**-19.46 (hd 64, B = 8, s 4, order 0)            ORACLE_EXCESS 2**-19.35, kappa 2**-17.35
(test_attn_cases_cpu.py fails if a measurement leaves (ORACLE_EXCESS / 2, ORACLE_EXCESS].)
The decode op's wide cases use the forms whose q / new-k bits are determined (REF RoPE
without qk-norm, bit-exact against the oracle, and QIE_ATTN_PREROPED): under qk-norm a
1-ulp flip of a q element (allowed by test_attention_decode_fused) moves a score by more
than kappa allows and says nothing about the attention.
"""
import functools
import math

import numpy as np

from conftest import rng

L, LAYER = 2, 1
NAN, INF = 0x7FC0, 0x7F80
MARGIN = 2.0 ** -30
KERNELS = ("split", "prefill", "extend", "decode")
ORACLE_EXCESS = {"split": 2.0 ** -19.35, "prefill": 2.0 ** -19.05, "extend": 2.0 ** -18.3, "decode": 2.0 ** -19.35}
TWO_PART_P = {"split": 0.0, "prefill": 2.0 ** -16, "extend": 2.0 ** -16, "decode": 0.0}
SHAPES = {"split": [(64, 8, 1), (128, 8, 2)],
          "prefill": [(64, 4, 4), (64, 14, 2), (128, 8, 1)],
          "extend": [(64, 4, 4), (64, 14, 2), (128, 16, 2)],
          "decode": [(64, 14, 2), (128, 8, 1), (128, 28, 4)]}
EDGES = {"split": (16,), "prefill": (64,), "extend": (64,), "decode": (128,)}   # extend adds S
DECODE_FORMS = ("ref", "ref_qkn", "hf_qkn", "pre")
WIDE_SCALES = (1, 4, 8)


def kappa(kernel):
    return 4 * ORACLE_EXCESS[kernel] + TWO_PART_P[kernel]


def to_bf16(a):
    """fp32 -> bf16 bits, round to nearest even (finite values)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf(a):
    return (np.asarray(a, np.uint16).astype(np.uint32) << 16).view(np.float32)


def f64(a):
    return bf(a).astype(np.float64)


# ------------------------------------------------------------------------------- V codes
_TAB = to_bf16(np.concatenate([np.arange(1, 256), -np.arange(1, 256)]).astype(np.float32) / 64)
_TAB_INDEX = {int(b): i for i, b in enumerate(_TAB)}


def vcode(ids, hd):
    """Distinct V rows [len(ids)][hd]: elements 0..2 are the id's base-500 digits."""
    ids = np.asarray(ids, np.int64)
    idx = (ids[:, None] * 131 + np.arange(hd)[None, :] * 37 + (ids[:, None] >> 5) * 7) % 510
    idx[:, 0], idx[:, 1], idx[:, 2] = ids % 500, (ids // 500) % 500, ids // 250000
    return _TAB[idx]


def vdecode(row):
    """The id of a vcode row, or None when the row is no code (a blend, NaN, ...)."""
    d = [_TAB_INDEX.get(int(x)) for x in row[:3]]
    if None in d or max(d) >= 500:
        return None
    i = d[0] + 500 * d[1] + 250000 * d[2]
    return i if np.array_equal(vcode([i], len(row))[0], row) else None


class Case:
    """One launch.  q [M][nq*hd] (as the attention sees it), pos [M], rps rows per sequence;
    K, V [B][L][nkv][maxc][hd]: what the attention must see (decode: the new row in place);
    want [M][nq*hd] bits and target [M][nq] for the exact family.  Decode only: qkv (the op's
    input), Kdev / Vdev (the cache before the call: row pos stale), knew / vnew [B][nkv*hd]
    (the oracle's appended row), form, qn / kn, eps, num, cs / sn."""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.G = self.nq // self.nkv
        self.M = len(self.pos)
        self.B = (self.M + self.rps - 1) // self.rps

    def seq_last(self, b):
        return int(self.pos[b * self.rps:(b + 1) * self.rps].max())


# --------------------------------------------------------------------- float64 reference
def _visible(c, m, mut):
    p, b = int(c.pos[m]), m // c.rps
    keys = np.arange(p + 1)
    kind = mut[0] if mut else None
    if kind == "leak" and p + 1 < c.maxc:
        keys = np.arange(p + 2)
    elif kind == "diag":
        keys = keys[:-1]
    elif kind == "drop_e":
        keys = keys[(keys % mut[1] != 0) | (keys == 0)]
    elif kind == "drop_e1":
        keys = keys[keys % mut[1] != mut[1] - 1]
    elif kind == "drop0":
        keys = keys[1:]
    elif kind == "past" and c.seq_last(b) + 1 < c.maxc:
        keys = np.append(keys, c.seq_last(b) + 1)
    return keys


def ref64(c, mut=None, rows=None):
    """Plain float64 softmax attention over the bf16 inputs: row m sees keys [0, pos[m]] of
    sequence m // rps.  Returns (out, mass = sum_t w_t |v_t|), [M][nq*hd]; rows not in `rows`
    (default: all) stay NaN.  mut: a mutant of the reference (test_attn_cases_cpu.py):
    ("leak",) key pos + 1 too, ("diag",) without the row's own key, ("drop_e", E) / ("drop_e1",
    E) without keys e / e - 1 at the multiples e >= E of E, ("drop0",), ("past",) the key after
    the sequence's last position too, ("scale",) scores x (1 + 2**-6), ("norescale",) an online
    softmax over 64-key tiles that omits the rescale when the running max grows."""
    G, hd = c.G, c.hd
    out = np.full((c.M, c.nq * hd), np.nan)
    mass = np.full((c.M, c.nq * hd), np.nan)
    Kf, Vf = f64(c.K[:, LAYER]), f64(c.V[:, LAYER])
    qf = f64(c.q).reshape(c.M, c.nkv, G, hd)
    kind = mut[0] if mut else None
    for m in (range(c.M) if rows is None else rows):
        b = m // c.rps
        keys = _visible(c, m, mut)
        if len(keys) == 0:
            continue
        for g in range(c.nkv):
            kk, vv = Kf[b, g, keys], Vf[b, g, keys]
            with np.errstate(invalid="ignore", over="ignore"):
                s = kk @ qf[m, g].T / math.sqrt(hd)            # [n][G]
                if kind == "scale":
                    s = s * (1 + 2.0 ** -6)
                if kind == "norescale":
                    m_run, l, o, a = np.full(G, -np.inf), np.zeros(G), np.zeros((G, hd)), np.zeros((G, hd))
                    for i in range(0, len(keys), 64):
                        m_run = np.maximum(m_run, s[i:i + 64].max(axis=0))
                        e = np.exp(s[i:i + 64] - m_run)
                        l += e.sum(axis=0)
                        o += e.T @ vv[i:i + 64]
                        a += e.T @ np.abs(vv[i:i + 64])
                    o, a = o / l[:, None], a / l[:, None]
                else:
                    w = np.exp(s - s.max(axis=0))
                    w /= w.sum(axis=0)
                    o, a = w.T @ vv, w.T @ np.abs(vv)
            out[m, g * G * hd:(g + 1) * G * hd] = o.reshape(-1)
            mass[m, g * G * hd:(g + 1) * G * hd] = a.reshape(-1)
    return out, mass


def one_minus_w(c):
    """[M][nq] float64: 1 - (softmax weight of the target key), exact family."""
    G, hd = c.G, c.hd
    Kf = f64(c.K[:, LAYER])
    qf = f64(c.q).reshape(c.M, c.nkv, G, hd)
    r = np.empty((c.M, c.nq))
    for m in range(c.M):
        b, p = m // c.rps, int(c.pos[m])
        for g in range(c.nkv):
            s = Kf[b, g, :p + 1] @ qf[m, g].T / math.sqrt(hd)
            t = c.target[m, g * G:(g + 1) * G]
            with np.errstate(over="ignore", invalid="ignore"):
                e = np.exp(s - s[t, np.arange(G)])
            e[t, np.arange(G)] = 0.0
            rest = e.sum(axis=0)
            r[m, g * G:(g + 1) * G] = rest / (1 + rest)
    return r


def assert_exact_inputs(c):
    """The condition on the inputs of an exact case; a case that misses it is an error."""
    assert (c.target >= 0).all() and (c.target <= c.pos[:, None]).all(), c.name
    r = one_minus_w(c)
    assert np.isfinite(r).all() and r.max() <= MARGIN, f"{c.name}: worst 1 - w = {r.max():.3e} = 2^{np.log2(r.max()):.1f}"
    v = np.abs(bf(c.V))
    fin = np.isfinite(v)
    assert (v[fin] >= 2.0 ** -7).all() and (v[fin] <= 4).all() and (fin.all() or c.trap in ("nan", "inf")), c.name
    for b in range(c.B):   # what the rows may see is finite
        assert np.isfinite(bf(c.K[b, LAYER, :, :c.seq_last(b) + 1])).all(), c.name


# ---------------------------------------------------------------------------- acceptance
def half_ulp(x):
    """Half a bf16 ulp of |x| (float64 array)."""
    e = np.floor(np.log2(np.maximum(np.abs(x), 2.0 ** -126)))
    return 2.0 ** (e - 8)


def excess(got, ref, mass):
    """Family 2: (|got - ref| - half a bf16 ulp of max(|got|, |ref|)) / mass, per element (the
    quantity kappa bounds); +inf where got is not finite."""
    g = f64(got)
    with np.errstate(invalid="ignore"):
        x = (np.abs(g - ref) - half_ulp(np.maximum(np.abs(g), np.abs(ref)))) / mass
    return np.where(np.isfinite(g), x, np.inf)


def accepted(c, got, ref=None):
    """[M][nq] bool: which (row, head)s of `got` (bf16 bits [M][nq*hd]) the case accepts.
    ref: ref64(c) of a wide case (computed here when absent)."""
    got = np.asarray(got).reshape(c.M, c.nq, c.hd)
    if c.family != "wide":
        return (got == c.want.reshape(c.M, c.nq, c.hd)).all(axis=2)
    out, mass = ref if ref is not None else ref64(c)
    x = excess(got, out.reshape(got.shape), mass.reshape(got.shape))
    return (x <= kappa(c.kernel)).all(axis=2)


def describe(c, got, m, h):
    """What a wrong (row, head) of an exact case holds, for the assertion message."""
    row = np.asarray(got).reshape(c.M, c.nq, c.hd)[m, h]
    want = c.want.reshape(c.M, c.nq, c.hd)[m, h]
    return (f"{c.name}: row {m} (pos {int(c.pos[m])}) head {h}: wanted key {int(c.target[m, h])}'s V row (code "
            f"{vdecode(want)}), got code {vdecode(row)} — {int((row != want).sum())} of {c.hd} elements differ, "
            f"first got {bf(row[:4])} want {bf(want[:4])}")


# ------------------------------------------------------------------------------ builders
@functools.lru_cache(maxsize=4)
def _base(hd, nkv, B, maxc, kind, seed):
    """Read-only base caches [B][L][nkv][maxc][hd]: K small noise / ramp / N(0, 1), V codes / N(0, 1)."""
    r = rng(seed)
    shape = (B, L, nkv, maxc, hd)
    if kind == "ramp":
        K = np.zeros(shape, np.float32)
        K[..., 0], K[..., 1] = np.arange(maxc) // 32, np.arange(maxc) % 32
        K = to_bf16(K)
    else:
        K = np.empty(shape, np.uint16)
        K[:, LAYER] = to_bf16(r.standard_normal((B, nkv, maxc, hd), dtype=np.float32) * (1.0 if kind == "wide" else 0.25))
        for l in range(L):
            if l != LAYER:
                K[:, l] = K[:, LAYER, :, :, ::-1]
    if kind == "wide":
        V = to_bf16(r.standard_normal(shape, dtype=np.float32))
    else:
        V = vcode(np.arange(B * L * nkv * maxc), hd).reshape(shape)
    K.setflags(write=False)
    V.setflags(write=False)
    return K, V


def n_cache_rows(c):
    return c.B * L * c.nkv * c.maxc


def trap_rows(c, n, g, b, id0):
    """n rows of trap content for kv head g of sequence b: (K, V) bits [n][hd]."""
    if c.trap in ("nan", "inf"):
        bits = NAN if c.trap == "nan" else INF
        return np.full((n, c.hd), bits, np.uint16), np.full((n, c.hd), bits, np.uint16)
    src = c.q[b * c.rps:(b + 1) * c.rps].reshape(-1, c.nkv, c.G, c.hd)[:, g].reshape(-1, c.hd)
    K = to_bf16(2 * bf(src))[np.arange(n) % len(src)]
    return K, vcode(id0 + np.arange(n), c.hd)


def _fill_traps(c, K, V, first):
    """Past each sequence's last position (decode: from the stale row `pos` itself)."""
    if c.trap is None:
        return
    for b in range(c.B):
        lo = c.seq_last(b) + first
        if lo >= c.maxc:
            continue
        for g in range(c.nkv):
            k, v = trap_rows(c, c.maxc - lo, g, b, 0)
            K[b, LAYER, g, lo:] = k
            if c.trap != "finite":   # finite: V keeps its (distinct) base codes
                V[b, LAYER, g, lo:] = v
        if c.trap != "finite":       # the other layer too: a wrong-layer read is not finite either
            K[b, :, :, lo:] = K[b, LAYER, 0, lo]
            V[b, :, :, lo:] = V[b, LAYER, 0, lo]


def pack(pos, nkv, G, queue, own_every, r):
    """Needle targets.  Every row takes pos and pos - 1 itself (first table; every table with
    own_every), the keys of `queue` go to rows that see them, leftover slots take random
    visible keys.  Returns target tables [M][nkv*G], as many as the queue needs."""
    M, tables = len(pos), []
    queue = sorted(set(int(t) for t in queue), reverse=True)
    while not tables or queue:
        T = np.full((M, nkv, G), -1, np.int64)
        if not tables or own_every:
            for m in range(M):
                p = int(pos[m])
                if G >= 2:
                    T[m, :, 0], T[m, :, 1] = p, max(p - 1, 0)
                else:
                    T[m, 0, 0] = p
                    T[m, 1 % nkv, 0] = max(p - 1, 0) if nkv > 1 else p
            have = set(T[T >= 0].tolist())
            queue = [t for t in queue if t not in have]
        free = [[(g, i) for i in range(G) for g in range(nkv) if T[m, g, i] < 0] for m in range(M)]
        rest, placed = [], 0
        for t in queue:
            el = [m for m in range(M) if pos[m] >= t and free[m]]
            if not el:
                rest.append(t)
                continue
            m = max(el, key=lambda j: len(free[j]))
            g, i = free[m].pop(0)
            T[m, g, i] = t
            placed += 1
        assert placed or not queue, "no slot takes the queued keys"
        for m in range(M):
            for g, i in free[m]:
                T[m, g, i] = r.integers(0, int(pos[m]) + 1)
        tables.append(T.reshape(M, nkv * G))
        queue = rest
    return tables


def _edge_keys(pos, edges):
    q = {0}
    for E in edges:
        for e in range(E, int(np.max(pos)) + 1, E):
            q.update((e - 1, e))
    return q


def _decode_io(c, oracle, q_raw, k_raw, v_raw, form):
    """qkv and the oracle's processed q / new k of a decode case; q_raw [B][nq*hd], k_raw, v_raw [B][nkv*hd]."""
    c.form, c.num = form, "hf" if form.startswith("hf") else "ref"
    c.qkn = form.endswith("qkn")
    c.eps = 1e-4 if c.num == "ref" else 1e-6
    c.cs, c.sn = oracle.rope_table(c.maxc, c.hd, 1e6, c.num)
    c.qkv = np.concatenate([q_raw, k_raw, v_raw], axis=1)
    q, k = q_raw, k_raw
    if form != "pre":
        if c.qkn:
            q = oracle.qknorm(q, c.qn, c.nq, c.hd, c.eps, c.num)
            k = oracle.qknorm(k, c.kn, c.nkv, c.hd, c.eps, c.num)
        q = oracle.rope(q, c.cs, c.sn, c.pos, c.nq, c.hd, c.num)
        k = oracle.rope(k, c.cs, c.sn, c.pos, c.nkv, c.hd, c.num)
    c.q, c.knew, c.vnew = q, k, v_raw


def _finish(c, K, V):
    """Traps, the decode op's stale / new row, expected output, and the input condition."""
    if c.kernel == "decode":
        _fill_traps(c, K, V, 0)
        c.Kdev, c.Vdev = K, V
        K, V = K.copy(), V.copy()
        for b in range(c.B):
            K[b, LAYER, :, c.pos[b]] = c.knew[b].reshape(c.nkv, c.hd)
            V[b, LAYER, :, c.pos[b]] = c.vnew[b].reshape(c.nkv, c.hd)
    else:
        _fill_traps(c, K, V, 1)
    c.K, c.V = K, V
    if c.family != "wide":
        c.want = np.empty((c.M, c.nq * c.hd), np.uint16)
        for m in range(c.M):
            for h in range(c.nq):
                c.want[m, h * c.hd:(h + 1) * c.hd] = V[m // c.rps, LAYER, h // c.G, c.target[m, h]]
        assert_exact_inputs(c)
    return c


def _new(kernel, family, shape, maxc, pos, rps, trap, name):
    hd, nq, nkv = shape
    return Case(kernel=kernel, family=family, hd=hd, nq=nq, nkv=nkv, maxc=maxc, pos=np.asarray(pos, np.int32), rps=rps,
                trap=trap, name=f"{kernel} {family} hd {hd} nq {nq} nkv {nkv} {name}" + (f" trap {trap}" if trap else ""))


def needle(kernel, shape, maxc, pos, rps, target, seed, trap, name, oracle=None, form=None, sub=0):
    c = _new(kernel, "needle", shape, maxc, pos, rps, trap, name)
    hd, G = c.hd, c.G
    c.target = np.asarray(target, np.int64)
    Kb, Vb = _base(hd, c.nkv, c.B, maxc, "needle", seed)
    K, V = Kb.copy(), Vb.copy()
    r = rng(100 * seed + 1 + sub)
    qkn = form is not None and form.endswith("qkn")
    sigma = 4.0 if hd == 64 else 3.0
    if qkn:   # the norm weight carries the magnitude
        c.qn = c.kn = to_bf16((sigma * (1 + 0.1 * r.standard_normal(hd))).astype(np.float32))
    else:
        c.qn = c.kn = None
    vec = {}
    q = np.empty((c.M, c.nq, hd), np.uint16)
    for m in range(c.M):
        for h in range(c.nq):
            key = (m // rps, h // G, int(c.target[m, h]))
            if key not in vec:
                vec[key] = to_bf16((r.standard_normal(hd) * (1.0 if qkn else sigma)).astype(np.float32))
            q[m, h] = vec[key]
    c.q = q.reshape(c.M, c.nq * hd)
    if kernel == "decode":
        k_raw = np.empty((c.M, c.nkv, hd), np.uint16)
        for b in range(c.M):
            for g in range(c.nkv):
                k_raw[b, g] = vec[(b, g, int(c.pos[b]))]   # pos is a target in every kv group
        v_raw = vcode(n_cache_rows(c) + np.arange(c.M * c.nkv), hd).reshape(c.M, c.nkv * hd)
        _decode_io(c, oracle, c.q, k_raw.reshape(c.M, -1), v_raw, form)
    qp = c.q.reshape(c.M, c.nq, hd)
    for m in range(c.M):
        for h in range(c.nq):
            if kernel != "decode" or c.target[m, h] != c.pos[m]:   # decode: the cached row at pos stays stale
                K[m // rps, LAYER, h // G, c.target[m, h]] = qp[m, h]
    return _finish(c, K, V)


def ramp(kernel, shape, maxc, pos, rps, up, trap, name, oracle=None, form=None):
    c = _new(kernel, "ramp_up" if up else "ramp_down", shape, maxc, pos, rps, trap, name)
    hd = c.hd
    Kb, Vb = _base(hd, c.nkv, c.B, maxc, "ramp", 5)
    K, V = Kb.copy(), Vb.copy()
    sign = 1.0 if up else -1.0
    q = np.zeros((c.M, c.nq, hd), np.float32)
    q[..., 0], q[..., 1] = sign * 8192, sign * 256
    c.q = to_bf16(q).reshape(c.M, c.nq * hd)
    c.target = np.repeat((c.pos if up else 0 * c.pos)[:, None], c.nq, axis=1).astype(np.int64)
    if kernel == "decode":
        assert form == "pre", "RoPE would turn the ramp's two dimensions"
        k_raw = np.stack([Kb[b, LAYER, :, c.pos[b]].reshape(-1) for b in range(c.M)])
        v_raw = vcode(n_cache_rows(c) + np.arange(c.M * c.nkv), hd).reshape(c.M, c.nkv * hd)
        c.qn = c.kn = None
        _decode_io(c, oracle, c.q, k_raw, v_raw, form)
    return _finish(c, K, V)


def wide(kernel, shape, maxc, pos, rps, s, seed, name, oracle=None, form=None):
    c = _new(kernel, "wide", shape, maxc, pos, rps, None, f"{name} s {s}")
    hd = c.hd
    Kb, Vb = _base(hd, c.nkv, c.B, maxc, "wide", seed)
    r = rng(seed + 1000 * s)
    c.q = to_bf16((r.standard_normal((c.M, c.nq * hd)) * s).astype(np.float32))
    c.target = None
    if kernel == "decode":
        k_raw = to_bf16(r.standard_normal((c.M, c.nkv * hd)).astype(np.float32))
        v_raw = to_bf16(r.standard_normal((c.M, c.nkv * hd)).astype(np.float32))
        c.qn = c.kn = None
        _decode_io(c, oracle, c.q, k_raw, v_raw, form)
    return _finish(c, Kb.copy(), Vb.copy())


# ------------------------------------------------------------------------- the case lists
def extend_split_tokens(M, maxc):
    """qie_attention_extend_split_tokens restated (the GPU test checks it against the library)."""
    S = 256 if M <= 32 else 512
    while (maxc + S - 1) // S > 64:
        S *= 2
    return S


def layouts(kernel, sweeps=True):
    """(name, maxc, pos, rows_per_seq, keys every one of which must be a needle target or None)
    of each launch shape of a kernel; the `sweep` ones are needle-only."""
    a = np.arange
    out = []
    if kernel == "split":
        out.append(("m8", 320, np.array([1, 2, 17, 33, 65, 129, 300, 320]) - 1, 1, None))
        out.append(("m9", 1100, np.array([1100, 1099, 1025, 1024, 513, 512, 511, 65, 1]) - 1, 1, None))
        if sweeps:
            out.append(("sweep65", 320, np.full(8, 64), 1, a(65)))
    elif kernel == "prefill":
        for P in (33, 130, 300):   # 300: a second workgroup of eight waves; every row targets itself: a full sweep
            out.append((f"P{P}", 320, a(P), P, a(P) if sweeps else None))
        out.append(("pos0_70", 320, 70 + a(40), 40, None))
        out.append(("repeated", 320, 40 + a(70) // 2, 70, None))
        out.append(("two_seqs", 320, np.tile(a(130), 2), 130, None))
    elif kernel == "extend":
        for n in (16, 3, 5):
            S = extend_split_tokens(n, 1152)
            pos0 = {16: S - 2, 3: S - 1, 5: S}[n]
            out.append((f"pos0_{pos0}_n{n}", 1152, pos0 + a(n), n, a(pos0 + n) if sweeps and n == 16 else None))
        out.append(("pos0_63_n2", 1152, 63 + a(2), 2, a(65) if sweeps else None))
        out.append(("pos0_1000_n40", 1152, 1000 + a(40), 40, None))
        out.append(("pos0_257_n100", 1152, 257 + a(100), 100, None))
        out.append(("two_seqs_short_last", 1152, np.concatenate([70 + a(20), 300 + a(13)]), 20, None))
    else:
        out.append(("b5", 1344, np.array([1, 2, 128, 129, 256]) - 1, 1, None))
        out.append(("b4", 1344, np.array([257, 385, 1025, 1280]) - 1, 1, None))
        # B = 8: split target 8, contexts 1,025-1,280 take two-step splits
        out.append(("b8", 1344, np.array([1025, 1100, 1152, 1153, 1279, 1280, 257, 129]) - 1, 1, None))
        if sweeps:
            out.append(("sweep257", 1344, np.full(7, 256), 1, a(257)))
    return out


def cases(kernel, shape, family, trap=None, oracle=None, form=None, sweeps=True, s=None):
    """The launches of one (kernel, head shape, family): family 'needle', 'ramp_up', 'ramp_down'
    or 'wide' (with s).  Built on demand: a case holds whole caches."""
    hd, nq, nkv = shape
    for li, (name, maxc, pos, rps, sweep) in enumerate(layouts(kernel, sweeps and family == "needle")):
        seed = 1000 * KERNELS.index(kernel) + 10 * li + hd
        if family == "needle":
            edges = EDGES[kernel] + ((extend_split_tokens(len(pos), maxc),) if kernel == "extend" else ())
            queue = _edge_keys(pos, edges) | (set(int(t) for t in sweep) if sweep is not None else set())
            for ti, T in enumerate(pack(pos, nkv, nq // nkv, queue, kernel == "decode", rng(seed))):
                yield needle(kernel, shape, maxc, pos, rps, T, seed, trap, f"{name}.{ti}", oracle, form, ti)
        elif family in ("ramp_up", "ramp_down"):
            yield ramp(kernel, shape, maxc, pos, rps, family == "ramp_up", trap, name, oracle, form)
        else:
            yield wide(kernel, shape, maxc, pos, rps, s, seed, name, oracle, form)


def targets_of(kernel, shape, layout):
    """The needle targets of every launch of one layout, without building the caches."""
    li, (name, maxc, pos, rps, sweep) = next((i, l) for i, l in enumerate(layouts(kernel)) if l[0] == layout)
    hd, nq, nkv = shape
    seed = 1000 * KERNELS.index(kernel) + 10 * li + hd
    edges = EDGES[kernel] + ((extend_split_tokens(len(pos), maxc),) if kernel == "extend" else ())
    queue = _edge_keys(pos, edges) | (set(int(t) for t in sweep) if sweep is not None else set())
    return pos, edges, sweep, pack(pos, nkv, nq // nkv, queue, kernel == "decode", rng(seed))
