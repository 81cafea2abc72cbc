"""Python host mirror of the reference driver, over libqie.so's C ABI.

Reference driver (layers/src/iengine.cu:226-456, qwen_main.cu:64-417):
``create_new_sequence`` -> ``llm()`` with ``state == prefill`` -> loop ``llm()`` with
``state == decode`` (one token per call).  Here: ``Engine`` (weights + RoPE tables),
``Batch`` (KV cache + per-sequence state for B sequences), ``Batch.prefill`` and
``Batch.decode_step`` / ``Batch.decode`` (hipGraph replays).  All compute runs in
libqie's HIP kernels; there is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib
from .spec import ModelSpec
from .weights import SynthParams

REF_PREFILL_SAMPLING = dict(top_k=50, temperature=1.0, seed=1234)   # qwen_main.cu:241
REF_DECODE_SAMPLING = dict(top_k=50, temperature=0.7, seed=1234)    # qwen_main.cu:381-388 (+ step)
REF_EOS = 151645                                                    # qwen_main.cu:257


@dataclasses.dataclass
class Sampling:
    top_k: int = 1
    temperature: float = 1.0
    top_p: float = 1.0
    seed: int = 1234

    def to_c(self) -> _lib.SamplingC:
        s = _lib.SamplingC()
        s.top_k, s.temperature, s.top_p, s.seed = self.top_k, self.temperature, self.top_p, self.seed
        return s


GREEDY = Sampling()


@dataclasses.dataclass
class SlotSampling:
    """One slot's own sampling entry (qie_slot_sampling; Batch.set_sampling): the four values of
    Sampling, min-p, the repetition / presence / frequency penalties over the window
    [max(penalty_start, q + 1 - penalty_last_n), q] of the slot's token history, and a logit
    bias per token id (-inf bans the token)."""
    top_k: int = 1
    temperature: float = 1.0
    top_p: float = 1.0
    min_p: float = 0.0
    seed: int = 1234
    repetition_penalty: float = 1.0
    presence_penalty: float = 0.0
    frequency_penalty: float = 0.0
    penalty_start: int = 0
    penalty_last_n: int = 0
    bias: Dict[int, float] = dataclasses.field(default_factory=dict)

    def to_c(self) -> _lib.SlotSamplingC:
        if len(self.bias) > _lib.QIE_SLOT_BIAS_MAX:
            raise ValueError(f"SlotSampling: {len(self.bias)} biased ids, at most {_lib.QIE_SLOT_BIAS_MAX}")
        s = _lib.SlotSamplingC()
        s.top_k, s.temperature, s.top_p, s.min_p, s.seed = self.top_k, self.temperature, self.top_p, self.min_p, self.seed
        s.repetition_penalty, s.presence_penalty = self.repetition_penalty, self.presence_penalty
        s.frequency_penalty = self.frequency_penalty
        s.penalty_start, s.penalty_last_n = self.penalty_start, self.penalty_last_n
        s.n_bias = len(self.bias)
        for i, (tok, v) in enumerate(self.bias.items()):
            s.bias_ids[i], s.bias[i] = int(tok), float(v)
        return s

    @staticmethod
    def from_c(s: _lib.SlotSamplingC) -> "SlotSampling":
        return SlotSampling(s.top_k, s.temperature, s.top_p, s.min_p, s.seed, s.repetition_penalty,
                            s.presence_penalty, s.frequency_penalty, s.penalty_start, s.penalty_last_n,
                            {int(s.bias_ids[i]): float(s.bias[i]) for i in range(s.n_bias)})

_ROLE_FIELDS = {
    "input_layernorm.weight": "attn_norm", "self_attn.q_proj.weight": "wq",
    "self_attn.k_proj.weight": "wk", "self_attn.v_proj.weight": "wv",
    "self_attn.q_proj.bias": "bq", "self_attn.k_proj.bias": "bk", "self_attn.v_proj.bias": "bv",
    "self_attn.q_norm.weight": "q_norm", "self_attn.k_norm.weight": "k_norm",
    "self_attn.o_proj.weight": "wo", "post_attention_layernorm.weight": "ffn_norm",
    "mlp.gate_proj.weight": "w_gate", "mlp.up_proj.weight": "w_up", "mlp.down_proj.weight": "w_down",
}


def weights_struct(spec: ModelSpec, ptr: Dict[str, int]):
    """Build a qie_model_weights from {full tensor name: pointer}.  Returns (struct, keepalive)."""
    layers = (_lib.LayerWeightsC * spec.n_layers)()
    for l in range(spec.n_layers):
        for short, field in _ROLE_FIELDS.items():
            setattr(layers[l], field, ptr.get(f"model.layers.{l}.{short}"))
    w = _lib.ModelWeightsC()
    w.embed = ptr["model.embed_tokens.weight"]
    w.final_norm = ptr["model.norm.weight"]
    w.lm_head = ptr["model.embed_tokens.weight"] if spec.tie_embeddings else ptr["lm_head.weight"]
    w.n_layers = spec.n_layers
    w.layers = C.cast(layers, C.POINTER(_lib.LayerWeightsC))
    return w, layers


class Comm:
    """Tensor-parallel communicator (qie_comm).  ``Comm.rccl(uid, world, rank, device)`` for
    one process per GPU (rank 0 makes ``Comm.unique_id()`` and ships the bytes to the others);
    ``Comm.local(world)`` for `world` in-process ranks on one device, one host thread each
    (the test backend; engines on it run without hipGraphs)."""

    def __init__(self, handle: int, lib, owner=None):
        self.h, self.lib, self._owner = handle, lib, owner
        w, r = C.c_int32(), C.c_int32()
        _lib.check(lib.qie_comm_rank(handle, C.byref(w), C.byref(r)), "qie_comm_rank")
        self.world, self.rank = w.value, r.value

    @staticmethod
    def unique_id() -> bytes:
        lib = _lib.load()
        buf = C.create_string_buffer(_lib.QIE_COMM_ID_BYTES)
        _lib.check(lib.qie_comm_unique_id(buf), "qie_comm_unique_id")
        return buf.raw

    @staticmethod
    def rccl(uid: bytes, world: int, rank: int, device: int) -> "Comm":
        lib = _lib.load()
        buf = C.create_string_buffer(uid, _lib.QIE_COMM_ID_BYTES)
        h = C.c_void_p()
        _lib.check(lib.qie_comm_create_rccl(buf, world, rank, device, C.byref(h)), "qie_comm_create_rccl")
        return Comm(h.value, lib)

    @staticmethod
    def peer(world: int, rank: int, device: int, exchange) -> "Comm":
        """Peer backend across processes: `exchange(handle_bytes) -> [handle of rank r for r
        in range(world)]` is the host channel (e.g. dist.FileGroup.allgather)."""
        lib = _lib.load()
        h = C.c_void_p()
        buf = C.create_string_buffer(_lib.QIE_COMM_PEER_HANDLE_BYTES)
        _lib.check(lib.qie_comm_create_peer(world, rank, device, C.byref(h), buf), "qie_comm_create_peer")
        comm = Comm(h.value, lib)
        hs = exchange(buf.raw)
        allh = C.create_string_buffer(b"".join(hs), _lib.QIE_COMM_PEER_HANDLE_BYTES * world)
        _lib.check(lib.qie_comm_peer_connect(h, allh), "qie_comm_peer_connect")
        return comm

    @staticmethod
    def peer_local(world: int) -> List["Comm"]:
        """Peer backend for `world` ranks of this process on one device (graph-capturable)."""
        lib = _lib.load()
        hs = (C.c_void_p * world)()
        _lib.check(lib.qie_comm_create_peer_local(world, hs), "qie_comm_create_peer_local")
        return [Comm(hs[r], lib) for r in range(world)]

    def peer_error(self) -> int:
        e = C.c_int32()
        _lib.check(self.lib.qie_comm_peer_error(self.h, C.byref(e)), "qie_comm_peer_error")
        return e.value

    def set_peer_mode(self, tagged: bool = True, push: bool = True) -> None:
        """Peer backend exchange form (qie_comm_peer_set_mode): tagged words polled by the
        readers, pushed by the producing GEMV (defaults), or the flagged form; the same on
        every rank, before the decode graph that should use it is captured."""
        _lib.check(self.lib.qie_comm_peer_set_mode(self.h, int(bool(tagged)), int(bool(push))),
                   "qie_comm_peer_set_mode")

    @staticmethod
    def local(world: int) -> List["Comm"]:
        lib = _lib.load()
        hs = (C.c_void_p * world)()
        _lib.check(lib.qie_comm_create_local(world, hs), "qie_comm_create_local")
        return [Comm(hs[r], lib) for r in range(world)]

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.qie_comm_destroy(self.h)
            self.h = None


class Engine:
    def __init__(self, spec: ModelSpec, device: int = 0, max_ctx: int = 4096, use_graph: bool = True,
                 comm: Optional[Comm] = None, weight_fp8: bool = False, comm_always: bool = False,
                 prefill_fp8: bool = False, weight_fp4: bool = False):
        self.lib = _lib.load()
        self.spec = spec
        self._spec_c = spec.to_c()
        opts = _lib.EngineOptsC()
        opts.device, opts.max_ctx, opts.use_graph = device, max_ctx, int(use_graph)
        opts.tp_rank, opts.tp_size = (comm.rank, comm.world) if comm else (0, 1)
        opts.tp_comm = comm.h if comm else None
        opts.weight_fp8 = int(weight_fp8)
        opts.comm_always = int(comm_always)   # exchange steps through comm even at world 1 (tests)
        # numerics flag: prefill projections on the block-scaled fp8 MFMA (activations quantised
        # per row to e4m3; needs weight_fp8) — the oracle's Model(prefill_act_fp8=True)
        opts.prefill_fp8 = int(prefill_fp8)
        # the seven layer projections in MXFP4 (e2m1 codes, 32-element blocks, e8m0 scales) for
        # every M <= 16 launch; with weight_fp8 the lm_head alone is fp8.  The model computed is
        # HostWeights.fp4_dequantized(head_fp8=weight_fp8)
        opts.weight_fp4 = int(weight_fp4)
        self.comm = comm
        self._fp8 = weight_fp8
        h = C.c_void_p()
        _lib.check(self.lib.qie_engine_create(C.byref(self._spec_c), C.byref(opts), C.byref(h)),
                   "qie_engine_create")
        self.h = h
        self.max_ctx = max_ctx
        self._keep = None

    def init_synthetic(self, p: SynthParams = SynthParams()) -> "Engine":
        _lib.check(self.lib.qie_engine_init_synthetic(self.h, p.seed, p.w_scale, p.norm_scale, p.bias_scale),
                   "qie_engine_init_synthetic")
        if p.head_boost_every > 0 and p.head_boost_log2 != 0:
            self.boost_head(p.head_boost_every, p.head_boost_log2)
        return self

    def boost_head(self, every: int, log2f: int) -> None:
        """lm_head rows r % every == 0 times 2^log2f, in place on device (SynthParams'
        peaked head; same values as HostWeights.boost_head).  bf16 engines; under tensor
        parallelism each rank scales its vocab slice (rows rank*V/tp ..), untied heads only
        (a tied head's slice is a view of the replicated embedding)."""
        if getattr(self, "_fp8", False):
            raise ValueError("boost_head: bf16 engines only")
        rows, row0 = self.spec.vocab, 0
        if self.comm is not None and self.comm.world > 1:
            if self.spec.tie_embeddings:
                raise ValueError("boost_head: tensor-parallel engines with an untied head only")
            rows = self.spec.vocab // self.comm.world
            row0 = self.comm.rank * rows
        w = _lib.ModelWeightsC()
        _lib.check(self.lib.qie_engine_weights(self.h, C.byref(w), None), "qie_engine_weights")
        _lib.check(self.lib.qie_scale_rows_pow2(w.lm_head, rows, self.spec.hidden, row0, every, log2f,
                                                self.stream), "qie_scale_rows_pow2")
        self.sync()

    def load_weights_bin(self, bin_path: str, meta_path: str, chunk_bytes: int = 1 << 28) -> "Engine":
        _lib.check(self.lib.qie_engine_load_weights_bin(self.h, bin_path.encode(), meta_path.encode(),
                                                        chunk_bytes), "qie_engine_load_weights_bin")
        return self

    def set_weights(self, dev_ptrs: Dict[str, int], keepalive=None) -> "Engine":
        w, layers = weights_struct(self.spec, dev_ptrs)
        _lib.check(self.lib.qie_engine_set_weights(self.h, C.byref(w)), "qie_engine_set_weights")
        self._keep = (w, layers, keepalive)
        return self

    @property
    def stream(self) -> int:
        return self.lib.qie_engine_stream(self.h)

    def sync(self) -> None:
        _lib.check(self.lib.qie_engine_sync(self.h), "qie_engine_sync")

    def batch(self, batch: int = 1, max_ctx: Optional[int] = None, page_tokens: Optional[int] = None,
              n_pages: int = 0) -> "Batch":
        """B sequence slots.  page_tokens selects the paged KV cache (device block table over
        a pool of n_pages pages, 0 = enough for every slot at max_ctx); None = contiguous."""
        return Batch(self, batch, max_ctx or self.max_ctx, page_tokens, n_pages)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.qie_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Prefix:
    """A saved prefix of a paged batch (Batch.save_prefix): `.ids` its token ids, `.n_tokens`
    their count; it holds a reference on the prefix's KV pages until drop()."""

    def __init__(self, batch: "Batch", handle):
        self.batch = batch
        self.h = handle
        n = int(batch.lib.qie_batch_prefix_tokens(handle, None, 0))
        if n < 0:
            _lib.check(n, "qie_batch_prefix_tokens")
        arr = (C.c_int32 * max(n, 1))()
        _lib.check(batch.lib.qie_batch_prefix_tokens(handle, arr, n), "qie_batch_prefix_tokens")
        self.ids = [int(t) for t in arr[:n]]
        self.n_tokens = n

    def drop(self) -> None:
        """Release the references; pages no slot holds return to the pool."""
        if self.h is not None and getattr(self.batch, "h", None):
            _lib.check(self.batch.lib.qie_batch_prefix_drop(self.batch.h, self.h), "qie_batch_prefix_drop")
        self.h = None


def verify_segments(items: Sequence[tuple]) -> List[tuple]:
    """Batch.verify_batch's argument shape: (seq, draft) items -> a list of (seq, [ids]).
    ValueError for an empty list or a malformed item; the table itself (slot order, row count, id
    range) is checked by the engine, all-or-nothing."""
    out: List[tuple] = []
    for item in items:
        if len(item) != 2:
            raise ValueError("verify_batch: a segment is (seq, draft)")
        out.append((int(item[0]), [int(t) for t in item[1]]))
    if not out:
        raise ValueError("verify_batch: needs one or more segments")
    return out


class Batch:
    def __init__(self, engine: Engine, batch: int, max_ctx: int, page_tokens: Optional[int] = None,
                 n_pages: int = 0):
        self.e = engine
        self.lib = engine.lib
        self.B = batch
        self.max_ctx = max_ctx
        self.paged = page_tokens is not None
        # the pool's size as qie_batch_create_paged settles it (page_tokens 0 = 128; n_pages 0 =
        # every slot at max_ctx + the scratch page); 0 for a contiguous batch
        T = (page_tokens or 128) if self.paged else 0
        self.n_pages = (n_pages or batch * ((max_ctx + T - 1) // T) + 1) if self.paged else 0
        h = C.c_void_p()
        if self.paged:
            _lib.check(self.lib.qie_batch_create_paged(engine.h, batch, max_ctx, page_tokens, n_pages, C.byref(h)),
                       "qie_batch_create_paged")
        else:
            _lib.check(self.lib.qie_batch_create(engine.h, batch, max_ctx, C.byref(h)), "qie_batch_create")
        self.h = h

    def set_sampling(self, seq: int, sampling: Optional[SlotSampling]) -> None:
        """Slot `seq` samples under its own entry from now on, in every call that samples
        (prefill, append, score, decode, verify), until it is replaced or cleared (None); a slot
        without one uses the call's Sampling.  A fork copies it; release and prefill keep it."""
        sc = sampling.to_c() if sampling is not None else None
        _lib.check(self.lib.qie_batch_set_slot_sampling(self.h, seq, C.byref(sc) if sc is not None else None),
                   "qie_batch_set_slot_sampling")

    def slot_sampling(self, seq: int) -> Optional[SlotSampling]:
        sc, is_set = _lib.SlotSamplingC(), C.c_int32(0)
        _lib.check(self.lib.qie_batch_slot_sampling(self.h, seq, C.byref(sc), C.byref(is_set)),
                   "qie_batch_slot_sampling")
        return SlotSampling.from_c(sc) if is_set.value else None

    def prefill(self, seq: int, ids: Sequence[int], sampling: Sampling = GREEDY, chunk: Optional[int] = None) -> int:
        """Start sequence `seq` with the prompt `ids`.  chunk: feed the prompt in pieces of at
        most `chunk` ids (the first through qie_prefill, the rest through append), which bounds
        the prefill scratch by the chunk; returns the last piece's token."""
        if chunk is not None:
            from .scheduler import prefill_chunks
            pieces = prefill_chunks(len(ids), chunk)
            tok = self.prefill(seq, ids[:pieces[0][1]], sampling)
            for off, n in pieces[1:]:
                tok = self.append(seq, ids[off:off + n], off, sampling)
            return tok
        arr = (C.c_int32 * len(ids))(*[int(i) for i in ids])
        out = C.c_int32(-1)
        sc = sampling.to_c()
        _lib.check(self.lib.qie_prefill(self.h, seq, arr, len(ids), C.byref(sc), C.byref(out)), "qie_prefill")
        return out.value

    def append(self, seq: int, ids: Sequence[int], pos0: Optional[int] = None, sampling: Sampling = GREEDY) -> int:
        """Extend live sequence `seq` with `ids` at positions pos0 .. pos0+len-1 over its cached
        rows [0, pos0) (qie_prefill_append); returns the token sampled after the last id.
        pos0=None: the sequence's current position — the pending current token is replaced by
        ids[0].  A smaller pos0 rewinds: rows from pos0 on are overwritten."""
        if pos0 is None:
            pos0 = int(self.positions()[seq])
        arr = (C.c_int32 * len(ids))(*[int(i) for i in ids])
        out = C.c_int32(-1)
        sc = sampling.to_c()
        _lib.check(self.lib.qie_prefill_append(self.h, seq, arr, len(ids), int(pos0), C.byref(sc), C.byref(out)),
                   "qie_prefill_append")
        return out.value

    def score_rows(self, seq: int, ids: Sequence[int], targets: Sequence[int], pos0: int = 0,
                   sampling: Sampling = GREEDY, unfused: bool = False):
        """qie_score: prefill (pos0 == 0) or append (pos0 >= 1) of `ids` that also scores every
        row.  targets[i] is the id whose log-probability row i reports (-1: none, 0.0).  Returns
        (logprobs float32 [n], greedy ids int32 [n], the sampled next id)."""
        n = len(ids)
        if len(targets) != n:
            raise ValueError("score_rows: one target per id")
        arr = (C.c_int32 * max(n, 1))(*[int(i) for i in ids])
        tgt = (C.c_int32 * max(n, 1))(*[int(t) for t in targets])
        lp = np.zeros(max(n, 1), dtype=np.float32)
        gr = np.zeros(max(n, 1), dtype=np.int32)
        out = C.c_int32(-1)
        sc = sampling.to_c()
        _lib.check(self.lib.qie_score(self.h, seq, arr, n, int(pos0), tgt, C.byref(sc),
                                      _lib.QIE_SCORE_UNFUSED if unfused else 0,
                                      lp.ctypes.data_as(C.POINTER(C.c_float)), gr.ctypes.data_as(C.POINTER(C.c_int32)),
                                      C.byref(out)), "qie_score")
        return lp[:n], gr[:n], out.value

    def score(self, seq: int, ids: Sequence[int], pos0: Optional[int] = None, sampling: Sampling = GREEDY,
              chunk: Optional[int] = None, unfused: bool = False):
        """Score the text `ids`: starts sequence `seq` with it (pos0 None or 0, as prefill) or
        extends the live sequence at pos0 >= 1 (as append), and returns (logprobs float32
        [n - 1]: the log-probability of ids[i + 1] after ids[:i + 1], greedy int32 [n]: the
        model's own arg-max after every row, next_id: the token sampled after the last id).
        chunk: score in pieces of at most `chunk` ids, the pieces after the first through
        append.  unfused: the <= 16-row head launches instead of the fused scoring head."""
        from .scheduler import score_pieces
        lps, grs, nxt = [], [], -1
        for pos, piece, targets in score_pieces(ids, chunk, 0 if pos0 is None else int(pos0)):
            lp, gr, nxt = self.score_rows(seq, piece, targets, pos, sampling, unfused)
            lps.append(lp)
            grs.append(gr)
        return np.concatenate(lps)[:-1], np.concatenate(grs), nxt

    def perplexity(self, seq: int, ids: Sequence[int], chunk: Optional[int] = None) -> float:
        """exp(-mean log-probability) of ids[1:] given what precedes each (float64)."""
        lp = self.score(seq, ids, chunk=chunk)[0].astype(np.float64)
        if lp.size == 0:
            raise ValueError("perplexity: needs at least two ids")
        return float(np.exp(-lp.mean()))

    def logprobs(self, ids: Sequence[int]) -> np.ndarray:
        """Log-probability of ids[m] (-1: skip, 0.0) under slot m's last logits (the rows
        logits() returns), float32 [B]; only B floats come back to the host."""
        if len(ids) != self.B:
            raise ValueError("logprobs: one id per slot")
        arr = (C.c_int32 * self.B)(*[int(i) for i in ids])
        out = np.zeros(self.B, dtype=np.float32)
        _lib.check(self.lib.qie_batch_logprobs(self.h, arr, out.ctypes.data_as(C.POINTER(C.c_float))),
                   "qie_batch_logprobs")
        return out

    def prefill_batch(self, seq0: int, prompts: Sequence[Sequence[int]], sampling: Sampling = GREEDY) -> List[int]:
        """Equal-length prompts into slots seq0, seq0+1, ... in one pass (qie_prefill_batch)."""
        n = len(prompts)
        length = len(prompts[0]) if n else 0
        if n == 0 or any(len(p) != length for p in prompts):
            raise ValueError("prefill_batch: needs one or more prompts of equal length")
        flat = np.ascontiguousarray(np.asarray(prompts, dtype=np.int32).reshape(-1))
        out = (C.c_int32 * n)()
        sc = sampling.to_c()
        _lib.check(self.lib.qie_prefill_batch(self.h, seq0, n, flat.ctypes.data_as(C.POINTER(C.c_int32)), length,
                                              C.byref(sc), out), "qie_prefill_batch")
        return list(out)

    def prefill_ragged(self, segments: Sequence[tuple], sampling: Sampling = GREEDY) -> List[int]:
        """Prompts and appends of any lengths in one pass (qie_prefill_ragged).  segments: a list
        of (seq, ids) or (seq, ids, pos0), slots strictly increasing; pos0 omitted or 0 starts
        the sequence as prefill does, pos0 >= 1 extends the live sequence as append does.
        Returns each segment's sampled token, in segment order."""
        from .scheduler import ragged_segments
        segs = ragged_segments(segments)
        arr = (_lib.PrefillSegC * len(segs))(*[_lib.PrefillSegC(seq, len(ids), pos0) for seq, ids, pos0 in segs])
        flat = [t for _, ids, _ in segs for t in ids]
        ids_c = (C.c_int32 * len(flat))(*flat)
        out = (C.c_int32 * len(segs))()
        sc = sampling.to_c()
        _lib.check(self.lib.qie_prefill_ragged(self.h, arr, len(segs), ids_c, C.byref(sc), out), "qie_prefill_ragged")
        return list(out)

    def decode_step(self, sampling: Sampling = GREEDY) -> List[int]:
        out = (C.c_int32 * self.B)()
        sc = sampling.to_c()
        _lib.check(self.lib.qie_decode_step(self.h, C.byref(sc), out), "qie_decode_step")
        return list(out)

    def decode(self, n_steps: int, sampling: Sampling = GREEDY, want_ids: bool = True) -> Optional[np.ndarray]:
        out = np.zeros((max(n_steps, 1), self.B), dtype=np.int32)
        sc = sampling.to_c()
        ptr = out.ctypes.data_as(C.POINTER(C.c_int32)) if want_ids else None
        _lib.check(self.lib.qie_decode(self.h, n_steps, C.byref(sc), ptr), "qie_decode")
        return out[:n_steps] if want_ids else None

    def verify(self, seq: int, draft: Sequence[int], sampling: Sampling = GREEDY) -> List[int]:
        """Speculative verify (qie_verify): `draft` holds up to 15 guesses of the tokens after
        the sequence's pending current token.  One pass over the weights scores the current
        token and every draft; returns the tokens the model itself picks, t_0 .. t_a, where a
        is the number of leading drafts it agrees with (always at least t_0).  The sequence is
        then exactly as after len(result) decode steps."""
        n = len(draft)
        arr = (C.c_int32 * max(n, 1))(*[int(i) for i in draft])
        out = (C.c_int32 * (n + 1))()
        n_out = C.c_int32(0)
        sc = sampling.to_c()
        _lib.check(self.lib.qie_verify(self.h, seq, arr, n, C.byref(sc), out, C.byref(n_out)), "qie_verify")
        self._verify_rows = n + 1
        return [int(t) for t in out[:n_out.value]]

    def verify_batch(self, items: Sequence[tuple], sampling: Sampling = GREEDY) -> List[List[int]]:
        """verify() for several slots in one pass over the weights (qie_verify_batch).  items: a
        list of (seq, draft), slots strictly increasing, every slot with its current token and
        its drafts, at most 16 rows together.  Returns each segment's tokens t_0 .. t_a in item
        order; every slot of the call is then exactly as after len(its result) decode steps,
        every other slot untouched.  verify_logits() returns the rows in item order."""
        segs = verify_segments(items)
        arr = (_lib.VerifySegC * len(segs))(*[_lib.VerifySegC(seq, len(d)) for seq, d in segs])
        flat = [t for _, d in segs for t in d]
        rows = len(flat) + len(segs)
        draft = (C.c_int32 * max(len(flat), 1))(*flat)
        out = (C.c_int32 * rows)()
        n_out = (C.c_int32 * len(segs))()
        sc = sampling.to_c()
        _lib.check(self.lib.qie_verify_batch(self.h, arr, len(segs), draft, C.byref(sc), out, n_out),
                   "qie_verify_batch")
        self._verify_rows = rows
        res, r0 = [], 0
        for z, (_, d) in enumerate(segs):
            res.append([int(t) for t in out[r0:r0 + n_out[z]]])
            r0 += len(d) + 1
        return res

    def verify_captures(self) -> int:
        """Verify steps (verify and verify_batch together) this batch has captured so far
        (diagnostics: a replayed step leaves the count unchanged; 0 without use_graph)."""
        return int(self.lib.qie_batch_debug_verify_captures(self.h))

    def verify_logprobs(self, ids: Sequence[int]) -> np.ndarray:
        """Log-probability of ids[m] (-1: skip, 0.0) under row m of the last verify() or
        verify_batch() (the rows verify_logits() returns), float32 [rows]."""
        rows = getattr(self, "_verify_rows", 0)
        if rows <= 0:
            raise _lib.QieError("verify_logprobs: no verify() has run on this batch")
        if len(ids) != rows:
            raise ValueError(f"verify_logprobs: one id per row ({rows})")
        arr = (C.c_int32 * rows)(*[int(i) for i in ids])
        out = np.zeros(rows, dtype=np.float32)
        _lib.check(self.lib.qie_verify_logprobs(self.h, arr, out.ctypes.data_as(C.POINTER(C.c_float))),
                   "qie_verify_logprobs")
        return out

    def verify_logits(self) -> np.ndarray:
        """bf16 logits [len(draft) + 1][V] of every row of the last verify() (row i scored
        the token after the current token + i drafts); after verify_batch() the rows of all
        segments in item order."""
        rows = getattr(self, "_verify_rows", 0)
        if rows <= 0:
            raise _lib.QieError("verify_logits: no verify() has run on this batch")
        out = np.zeros((rows, self.e.spec.vocab), dtype=np.uint16)
        _lib.check(self.lib.qie_verify_logits(self.h, out.ctypes.data), "qie_verify_logits")
        return out

    def logits(self) -> np.ndarray:
        out = np.zeros((self.B, self.e.spec.vocab), dtype=np.uint16)
        _lib.check(self.lib.qie_batch_logits(self.h, out.ctypes.data), "qie_batch_logits")
        return out

    def positions(self) -> np.ndarray:
        out = np.zeros(self.B, dtype=np.int32)
        _lib.check(self.lib.qie_batch_positions(self.h, out.ctypes.data_as(C.POINTER(C.c_int32))),
                   "qie_batch_positions")
        return out

    def history(self, seq: int, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=np.int32)
        _lib.check(self.lib.qie_batch_history(self.h, seq, out.ctypes.data_as(C.POINTER(C.c_int32)), n),
                   "qie_batch_history")
        return out

    def set_position(self, seq: int, pos: int, token: int) -> None:
        _lib.check(self.lib.qie_batch_set_position(self.h, seq, pos, token), "qie_batch_set_position")

    def release(self, seq: int) -> None:
        """End sequence `seq`: its KV pages return to the pool; the slot idles until the next prefill."""
        _lib.check(self.lib.qie_batch_release(self.h, seq), "qie_batch_release")

    def fork(self, src: int, dst: int, n_tokens: Optional[int] = None, step_offset: int = 0) -> None:
        """Make slot `dst` a sequence that begins as live slot `src` does (qie_batch_fork): its
        first n_tokens rows (None: all of src's, up to its position) on shared KV pages, the
        partial last page copied.  step_offset is added to the copy's sampling step counter, so
        that forks of one sampled sequence draw different tokens."""
        if n_tokens is None:
            n_tokens = int(self.positions()[src])
        _lib.check(self.lib.qie_batch_fork(self.h, src, dst, int(n_tokens), int(step_offset)), "qie_batch_fork")

    def page_refs(self) -> np.ndarray:
        """Holders per pool page (int32 [n_pages], 0 = free; page 0 is the scratch page); paged batches."""
        n = self.n_pages
        out = np.zeros(max(n, 1), dtype=np.int32)
        _lib.check(self.lib.qie_batch_page_refs(self.h, out.ctypes.data_as(C.POINTER(C.c_int32)), n),
                   "qie_batch_page_refs")
        return out[:n]

    def save_prefix(self, seq: int, n_tokens: int) -> "Prefix":
        """Keep the first n_tokens (a multiple of page_tokens) of live slot `seq` alive beyond
        the slot (qie_batch_prefix_save): a reference on their pages and a copy of their ids."""
        h = C.c_void_p()
        _lib.check(self.lib.qie_batch_prefix_save(self.h, seq, int(n_tokens), C.byref(h)), "qie_batch_prefix_save")
        return Prefix(self, h)

    def load_prefix(self, prefix: "Prefix", dst: int, token: int, n_tokens: Optional[int] = None) -> None:
        """Start slot `dst` on the saved prefix's pages (its first n_tokens, None: all) at
        position n_tokens with current token `token`; append() the rest at pos0 = n_tokens."""
        if prefix.h is None:
            raise _lib.QieError("load_prefix: the prefix was dropped")
        n = prefix.n_tokens if n_tokens is None else int(n_tokens)
        _lib.check(self.lib.qie_batch_prefix_load(self.h, prefix.h, dst, n, int(token)), "qie_batch_prefix_load")

    def page_stats(self):
        """(free pages, pages held per slot, page_tokens); zeros for a contiguous batch."""
        free, pt = C.c_int32(), C.c_int32()
        per = np.zeros(self.B, dtype=np.int32)
        _lib.check(self.lib.qie_batch_page_stats(self.h, C.byref(free), per.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 C.byref(pt)), "qie_batch_page_stats")
        return free.value, per, pt.value

    def block_table(self, seq: int, n: int) -> np.ndarray:
        out = np.zeros(n, dtype=np.int32)
        _lib.check(self.lib.qie_batch_block_table(self.h, seq, out.ctypes.data_as(C.POINTER(C.c_int32)), n),
                   "qie_batch_block_table")
        return out

    def reserve(self, seq: int, n_tokens: int) -> None:
        """Operator tier: make `seq` live and hold KV pages for positions [0, n_tokens)."""
        _lib.check(self.lib.qie_batch_reserve(self.h, seq, n_tokens), "qie_batch_reserve")

    def kv_cache(self, seq: int) -> _lib.KvCacheC:
        """KV descriptor of slot `seq` (kernels address it as sequence 0)."""
        c = _lib.KvCacheC()
        _lib.check(self.lib.qie_batch_kv_cache(self.h, seq, C.byref(c)), "qie_batch_kv_cache")
        return c

    def kv_rows(self, seq: int, layer: int, n: int):
        """Host copy of the cached K and V rows [n_kv_heads][n][head_dim] (bf16 bits) of
        positions [0, n) of `seq` at `layer` (diagnostics / tests)."""
        c = self.kv_cache(seq)
        hd, nkv, L = c.head_dim, c.n_kv_heads, c.n_layers
        out = [np.zeros((nkv, n, hd), np.uint16), np.zeros((nkv, n, hd), np.uint16)]
        if c.block_table:
            T = c.page_tokens
            pages = self.block_table(seq, (n + T - 1) // T)
            runs = [(t0, min(n, t0 + T), int(pages[t0 // T]) * c.seq_stride, T) for t0 in range(0, n, T)]
        else:
            runs = [(0, n, 0, c.max_ctx)]
        for which, base in enumerate((c.k, c.v)):
            for t0, t1, off, run in runs:
                for g in range(nkv):
                    src = base + 2 * (off + ((layer * nkv + g) * run + (t0 % run if c.block_table else t0)) * hd)
                    buf = np.zeros((t1 - t0, hd), np.uint16)
                    _lib.check(self.lib.qie_memcpy_d2h(buf.ctypes.data, src, buf.nbytes), "kv_rows")
                    out[which][g, t0:t1] = buf
        return out

    def debug_step(self, sampling: Sampling = GREEDY):
        """One eager decode step; returns (ids, residual snapshots bf16 [2L + 1][B][H]):
        slot 0 the input row, 2l + 1 after layer l's attention block, 2l + 2 after its MLP."""
        L, H = self.e.spec.n_layers, self.e.spec.hidden
        xs = np.zeros((2 * L + 1, self.B, H), np.uint16)
        out = (C.c_int32 * self.B)()
        sc = sampling.to_c()
        _lib.check(self.lib.qie_batch_debug_step(self.h, C.byref(sc), out, xs.ctypes.data), "qie_batch_debug_step")
        return list(out), xs

    def set_decode_mode(self, mode: int) -> None:
        """0: five launches per layer; 1: the persistent layer stack (qie_batch_set_decode_mode)."""
        _lib.check(self.lib.qie_batch_set_decode_mode(self.h, mode), "qie_batch_set_decode_mode")

    @property
    def decode_mode(self) -> int:
        return int(self.lib.qie_batch_decode_mode(self.h))

    def time_kernel(self, which: int = 0, iters: int = 20):
        us, by = C.c_double(), C.c_double()
        _lib.check(self.lib.qie_batch_time_kernel(self.h, which, iters, C.byref(us), C.byref(by)),
                   "qie_batch_time_kernel")
        return us.value, by.value

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.qie_batch_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
