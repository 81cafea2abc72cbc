// row_bufs.hpp — the device rows a step works on, as ONE allocation carved into pieces: the
// decode step's B slots, a verify step's 16 rows, a prefill's prompt rows, the scoring rows.
// Plain C++ (no HIP): engine.hip allocates, tools/rowbuf_dump.cpp prints the layout
// (tests/test_row_bufs_cpu.py).  A listing function names every piece once; it runs over a
// Carver without a base for the size, then over one with the allocation for the pointers, so
// the two cannot disagree and a failed allocation leaves nothing behind.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

struct qie_row_segs;

namespace qie {

// Every piece starts at a multiple of this (the kernels need 16 bytes; 256 is what the verify
// block shipped with, and profiles/row_buffers.json measured the prefill GEMMs on it)
constexpr size_t kRowPieceAlign = 256;

struct Carver {
    struct Piece {
        const char* name;
        size_t off, bytes;
    };
    char* base = nullptr;                // null: the size pass
    size_t off = 0;                      // after the listing: the block's bytes
    std::vector<Piece>* log = nullptr;   // rowbuf_dump: every piece taken

    template <class T>
    void take(const char* name, T*& p, int64_t bytes) {
        if (base) p = reinterpret_cast<T*>(base + off);
        const size_t n = (size_t)std::max<int64_t>(bytes, 16);   // never an empty piece
        if (log) log->push_back({name, off, n});
        off += (n + kRowPieceAlign - 1) / kRowPieceAlign * kRowPieceAlign;
    }
};

// What a block of rows is carved for.  Sizes are this rank's (QD, KD, I, Vl local; V global).
struct RowDims {
    int64_t rows = 0, H = 0, QD = 0, KD = 0, I = 0, Vl = 0, V = 0;
    int64_t attn_ws_bytes = 0, samp_ws_bytes = 0;   // their formulas live with the kernels
    bool layer = true;      // x, xn, qkv, att, h, pos: the rows a layer runs on
    bool q = true;          // the rotated q rows of the multi-row layer (the decode layer has none)
    bool attn_ws = true;    // that layer's attention workspace inside the block
    bool head = true;       // logits, sampler workspace, keys, ids, step
    bool exchange = false;  // use_comm: fp32 partials; with the head, the gathered logits
};

// Every pointer LayerRows and HeadBufs name, and the allocation they point into
struct RowBufs {
    void* mem = nullptr;
    size_t bytes = 0;
    int64_t rows = 0;
    uint16_t *x = nullptr, *xn = nullptr, *qkv = nullptr, *q = nullptr, *att = nullptr, *h = nullptr;
    float* part = nullptr;
    int32_t *pos = nullptr, *ids = nullptr, *step = nullptr;
    uint16_t *logits = nullptr, *logits_full = nullptr, *gather_tmp = nullptr;
    unsigned long long* keys = nullptr;
    void *samp_ws = nullptr, *attn_ws = nullptr;
};

inline void carve_rows(Carver& c, RowBufs& r, const RowDims& d) {
    const int64_t R = d.rows;
    if (d.layer) {
        c.take("x", r.x, R * d.H * 2);
        c.take("xn", r.xn, R * d.H * 2);
        c.take("qkv", r.qkv, R * (d.QD + 2 * d.KD) * 2);
        if (d.q) c.take("q", r.q, R * d.QD * 2);
        c.take("att", r.att, R * d.QD * 2);
        c.take("h", r.h, R * d.I * 2);
        c.take("pos", r.pos, R * 4);
        if (d.attn_ws) c.take("attn_ws", r.attn_ws, d.attn_ws_bytes);
        if (d.exchange) c.take("part", r.part, R * d.H * 4);
    }
    if (d.head) {
        c.take("logits", r.logits, R * d.Vl * 2);
        c.take("samp_ws", r.samp_ws, d.samp_ws_bytes);
        c.take("keys", r.keys, R * 8);
        c.take("ids", r.ids, R * 4);
        c.take("step", r.step, R * 4);
        if (d.exchange) {
            c.take("logits_full", r.logits_full, R * d.V * 2);
            c.take("gather_tmp", r.gather_tmp, R * d.V * 2);
        }
    }
}

// ---- the views the launch code takes
// The M rows a layer works on: the decode step's are the batch's B slots, a verify step's
// (qie_verify) its own M <= 16 rows of one sequence, a prefill's the prompt rows.
struct LayerRows {
    int64_t M;
    uint16_t *x, *xn, *qkv, *q, *att, *h;   // residual [M][H], normed [M][H], [M][QKVD], [M][QD] x 2, [M][I]
    float* part;                            // [M][H] fp32 partials (exchange path only)
    const int32_t* pos;                     // [M] positions on device; consecutive runs of
    int32_t rows_per_seq;                   //   rows_per_seq rows belong to one sequence
    const qie_row_segs* segs;               // set (host table): segments of any lengths instead
};
inline LayerRows layer_rows(const RowBufs& r, int64_t M, int32_t rows_per_seq, const qie_row_segs* segs = nullptr) {
    return LayerRows{M, r.x, r.xn, r.qkv, r.q, r.att, r.h, r.part, r.pos, rows_per_seq, segs};
}

// What a head launch reads and writes, from row m0 of a block on (the batch's slots m0 ..; a
// verify step's rows from 0).  logits / keys / ids / step are row m0 of the rows served.
struct HeadBufs {
    uint16_t* logits;             // [M][Vl]
    unsigned long long* keys;     // [M] (zero before the launch)
    int32_t* ids;                 // [M]
    const int32_t* step;          // [M] sampling counters
    void* samp_ws;
    uint16_t* xn;                 // [M][H] (prenorm)
    uint16_t *gather_tmp, *logits_full;   // exchange path: [tp][M][Vl], [rows][V]
    int full_row0;                // first row of logits_full the M rows land in
};
inline HeadBufs head_bufs(const RowBufs& r, int m0, int64_t Vl) {
    return HeadBufs{r.logits + m0 * Vl, r.keys + m0, r.ids + m0, r.step + m0, r.samp_ws,
                    r.xn,               r.gather_tmp, r.logits_full, m0};
}

// ---- the four sets: the shared pieces, then what only that set has, in the same block

// the decode step's B slots: token history [B][max_ctx], the current position's RoPE row
// [B][rope_cur_floats], the fused attention's split partials + counters
struct DecodeRows : RowBufs {
    int32_t* hist = nullptr;
    float* rope_cur = nullptr;
    void* dec_ws = nullptr;
};
inline RowDims decode_dims(RowDims d) {
    d.q = d.attn_ws = false;
    return d;
}
inline void carve_decode(Carver& c, DecodeRows& r, const RowDims& d, int64_t max_ctx, int64_t rope_cur_floats,
                         int64_t dec_ws_bytes) {
    carve_rows(c, r, decode_dims(d));
    c.take("d_hist", r.hist, d.rows * max_ctx * 4);
    c.take("d_rope_cur", r.rope_cur, d.rows * rope_cur_floats * 4);
    c.take("dec_ws", r.dec_ws, dec_ws_bytes);
}

// a verify step's rows: the drafted ids, the result words {n_out, ids[rows]}
struct VerifyRows : RowBufs {
    int32_t *draft = nullptr, *res = nullptr;
};
inline void carve_verify(Carver& c, VerifyRows& r, const RowDims& d) {
    carve_rows(c, r, d);
    c.take("draft", r.draft, d.rows * 4);
    c.take("res", r.res, (d.rows + 1) * 4);
}

// a prefill's rows (no head: it runs on the batch's slots; the attention workspace is sized per
// call): the prompt ids, and with fp8 activations the codes [rows][max K] and exponents [rows]
struct PrefillRows : RowBufs {
    int32_t* ids_in = nullptr;
    uint8_t *q8 = nullptr, *e8 = nullptr;
};
inline RowDims prefill_dims(RowDims d) {
    d.head = d.attn_ws = false;
    return d;
}
inline void carve_prefill(Carver& c, PrefillRows& r, const RowDims& d, bool act_fp8) {
    carve_rows(c, r, prefill_dims(d));
    c.take("pf_ids", r.ids_in, d.rows * 4);
    if (act_fp8) {
        c.take("pf_q8", r.q8, d.rows * std::max(std::max(d.H, d.QD), d.I));
        c.take("pf_e8", r.e8, d.rows);
    }
}

// the scoring rows: targets, greedy ids (RowBufs::ids), log-probabilities; nothing shared
struct ScoreRows : RowBufs {
    int32_t* tgt = nullptr;
    float* lp = nullptr;
};
inline void carve_score(Carver& c, ScoreRows& r, int64_t rows) {
    c.take("tgt", r.tgt, rows * 4);
    c.take("ids", r.ids, rows * 4);
    c.take("lp", r.lp, rows * 4);
}

}  // namespace qie
