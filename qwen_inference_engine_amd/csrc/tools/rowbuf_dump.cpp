// rowbuf_dump — prints the layout of the engine's row blocks (row_bufs.hpp) without a GPU.
// Plain host program (`make rowbuf_dump`); tests/test_row_bufs_cpu.py checks its output.
//
// stdin, one block per line:
//   name set rows H QD KD I Vl V attn_ws_bytes samp_ws_bytes exchange [extras]
// set: decode (extras: max_ctx rope_cur_floats dec_ws_bytes), verify, prefill (extras: act_fp8),
// score.  Output, per piece in carving order:
//   name piece offset bytes pointer_offset
// offset from the size pass (no base), pointer_offset = the pointer the second pass assigned
// minus its base; then `name total bytes` and `name align bytes`.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "../row_bufs.hpp"

using namespace qie;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::string name, set;
        RowDims d;
        int exchange = 0;
        if (!(in >> name >> set >> d.rows >> d.H >> d.QD >> d.KD >> d.I >> d.Vl >> d.V >> d.attn_ws_bytes >>
              d.samp_ws_bytes >> exchange)) {
            fprintf(stderr, "rowbuf_dump: bad line: %s\n", line.c_str());
            return 2;
        }
        d.exchange = exchange != 0;
        long long x0 = 0, x1 = 0, x2 = 0;
        in >> x0 >> x1 >> x2;
        DecodeRows dec;
        VerifyRows ver;
        PrefillRows pf;
        ScoreRows sc;
        auto list = [&](Carver& c) {
            if (set == "decode") carve_decode(c, dec, d, x0, x1, x2);
            else if (set == "verify") carve_verify(c, ver, d);
            else if (set == "prefill") carve_prefill(c, pf, d, x0 != 0);
            else if (set == "score") carve_score(c, sc, d.rows);
            else return false;
            return true;
        };
        std::vector<Carver::Piece> sizes;
        Carver c0;
        c0.log = &sizes;
        if (!list(c0)) {
            fprintf(stderr, "rowbuf_dump: unknown set %s\n", set.c_str());
            return 2;
        }
        // the pointer pass over a made-up base (never dereferenced): each logged offset is where
        // the piece's pointer landed, read back through the struct below
        char* const base = reinterpret_cast<char*>(uintptr_t(1) << 40);
        Carver c1{base};
        list(c1);
        const RowBufs& r = set == "decode" ? (RowBufs&)dec : set == "verify" ? (RowBufs&)ver : set == "prefill" ? (RowBufs&)pf : (RowBufs&)sc;
        struct Named { const char* name; const void* p; };
        const Named all[] = {{"x", r.x}, {"xn", r.xn}, {"qkv", r.qkv}, {"q", r.q}, {"att", r.att}, {"h", r.h},
                             {"pos", r.pos}, {"attn_ws", r.attn_ws}, {"part", r.part}, {"logits", r.logits},
                             {"samp_ws", r.samp_ws}, {"keys", r.keys}, {"ids", r.ids}, {"step", r.step},
                             {"logits_full", r.logits_full}, {"gather_tmp", r.gather_tmp},
                             {"d_hist", dec.hist}, {"d_rope_cur", dec.rope_cur}, {"dec_ws", dec.dec_ws},
                             {"draft", ver.draft}, {"res", ver.res}, {"pf_ids", pf.ids_in}, {"pf_q8", pf.q8},
                             {"pf_e8", pf.e8}, {"tgt", sc.tgt}, {"lp", sc.lp}};
        for (const auto& p : sizes) {
            long long at = -1;
            for (const Named& n : all)
                if (std::string(n.name) == p.name && n.p) at = (const char*)n.p - base;
            printf("%s %s %zu %zu %lld\n", name.c_str(), p.name, p.off, p.bytes, at);
        }
        for (const Named& n : all) {   // a pointer set without a logged piece would be a listing bug
            bool logged = false;
            for (const auto& p : sizes) logged |= std::string(n.name) == p.name;
            if (n.p && !logged) printf("%s %s unlisted\n", name.c_str(), n.name);
        }
        printf("%s total %zu\n", name.c_str(), c0.off);
        printf("%s align %zu\n", name.c_str(), kRowPieceAlign);
        if (c1.off != c0.off) printf("%s total_mismatch %zu\n", name.c_str(), c1.off);
    }
    return 0;
}
