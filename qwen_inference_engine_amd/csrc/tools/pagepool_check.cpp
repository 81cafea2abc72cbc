// pagepool_check — drives the reference-counted page pool (page_pool.hpp) without a GPU.
// Plain host program (`make pagepool_check`; `make pagepool_check_asan` builds it under
// AddressSanitizer + UBSan); tests/test_page_pool_cpu.py compares its output with a Python
// model of the same rules.
//
// stdin, one operation per line (`#` starts a comment):
//   init slots max_pages page_tokens n_pages
//   grow slot ntok          fresh pages until the slot holds ntok tokens      -> ok | fail 28
//   take                    one page off the free list                        -> page P | fail 28
//   share page              one more reference
//   drop page               one reference less (free at 0)
//   fork src dst ntok       dst released, full pages shared, a tail page taken -> ok | fail 28
//   plan slot lo hi         the writers' planning step, nothing changes
//                           -> plan first last n_private copy_index copy_rows grow fresh
//   write slot lo hi        a one-span reservation                             -> cow OLD NEW | fail 28
//   reserve slot lo hi [slot lo hi ...]   the writers' reservation over up to kMaxBatchSlots spans
//   restart slot len [slot len ...]       the same for slots that begin new sequences of len tokens
//                           -> ok NEED [cow SLOT INDEX ROWS OLD NEW]... | fail 28 need N free F
//   release slot
//   dump                    every slot's pages, the counts of pages 1.., the free list
// Every operation that changes something checks its argument ranges and answers `bad` otherwise.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../page_pool.hpp"

using namespace qie;

int main() {
    PagePool p;
    bool made = false;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        std::string op;
        long long a = 0, b = 0, c = 0, d = 0;
        in >> op;
        auto slot_ok = [&](long long s) { return made && s >= 0 && s < p.n_slots; };
        auto page_ok = [&](long long g) { return made && g >= 1 && g < p.n_pages; };
        // positions [lo, hi] of a slot (hi == lo - 1: growth to lo tokens only)
        auto span_ok = [&](long long s, long long lo, long long hi) {
            return slot_ok(s) && lo >= 0 && hi >= lo - 1 && p.pages_for(hi + 1) <= p.max_pages;
        };
        if (op == "init") {
            if (!(in >> a >> b >> c >> d) || a < 1 || b < 1 || c < 1 || d < 2 || a > 4096 || b > 4096 || d > (1 << 20)) {
                printf("bad\n");
                continue;
            }
            p.init((int)a, (int)b, (int)c, (int)d);
            made = true;
            printf("ok\n");
        } else if (op == "grow") {
            if (!(in >> a >> b) || !slot_ok(a) || b < 0 || p.pages_for(b) > p.max_pages) {
                printf("bad\n");
                continue;
            }
            if (p.missing((int)a, b) > p.free_count()) {
                printf("fail 28\n");
                continue;
            }
            p.grow((int)a, b);
            printf("ok\n");
        } else if (op == "take") {
            if (!made) printf("bad\n");
            else if (p.free_count() < 1) printf("fail 28\n");
            else printf("page %d\n", p.take());
        } else if (op == "share" || op == "drop") {
            if (!(in >> a) || !page_ok(a) || p.refs[a] < 1) {
                printf("bad\n");
                continue;
            }
            if (op == "share") p.share((int32_t)a);
            else p.drop((int32_t)a);
            printf("ok\n");
        } else if (op == "fork") {
            if (!(in >> a >> b >> c) || !slot_ok(a) || !slot_ok(b) || a == b || c < 1 ||
                p.pages_for(c) > p.held[a]) {
                printf("bad\n");
                continue;
            }
            if (!p.fork_fits((int)b, c)) {
                printf("fail 28\n");
                continue;
            }
            p.fork((int)a, (int)b, c);
            printf("ok\n");
        } else if (op == "plan") {
            if (!(in >> a >> b >> c) || !span_ok(a, b, c)) {
                printf("bad\n");
                continue;
            }
            const PagePool::WritePlan w = p.plan_write((int)a, b, c);
            printf("plan %d %d %d %d %d %lld %lld\n", w.first, w.last, w.n_private, w.copy_index, w.copy_rows,
                   (long long)w.grow, (long long)w.fresh());
        } else if (op == "write" || op == "reserve" || op == "restart") {
            // the spans: (slot lo hi)..., or for a restart (slot len)... with no slot named twice
            const bool restart = op == "restart";
            const size_t per = restart ? 2 : 3;
            std::vector<long long> v;
            while (in >> a) v.push_back(a);
            const size_t n = v.size() / per;
            bool ok = in.eof() && n >= 1 && v.size() == n * per && n <= (op == "write" ? 1 : (size_t)kMaxBatchSlots);
            PagePool::Span spans[kMaxBatchSlots];
            for (size_t i = 0; ok && i < n; i++) {
                const long long* f = &v[i * per];
                spans[i] = restart ? PagePool::Span{(int)f[0], 0, f[1] - 1, true}
                                   : PagePool::Span{(int)f[0], f[1], f[2], false};
                ok = span_ok(f[0], spans[i].lo, spans[i].hi) && (!restart || f[1] >= 1);
                for (size_t j = 0; ok && restart && j < i; j++) ok = spans[j].slot != spans[i].slot;
            }
            if (!ok) {
                printf("bad\n");
                continue;
            }
            const PagePool::Reservation r = p.plan_reserve(spans, (int)n);
            if (r.need > p.free_count()) {
                if (op == "write") printf("fail 28\n");
                else printf("fail 28 need %lld free %lld\n", (long long)r.need, (long long)p.free_count());
                continue;
            }
            PagePool::CopyJob jobs[kMaxBatchSlots];
            const int n_jobs = p.commit(r, jobs);
            if (op == "write") {
                printf("cow %d %d\n", n_jobs ? jobs[0].old_page : 0, n_jobs ? jobs[0].new_page : 0);
                continue;
            }
            printf("ok %lld", (long long)r.need);
            for (int j = 0; j < n_jobs; j++)
                printf(" cow %d %d %d %d %d", jobs[j].slot, jobs[j].index, jobs[j].rows, jobs[j].old_page,
                       jobs[j].new_page);
            printf("\n");
        } else if (op == "release") {
            if (!(in >> a) || !slot_ok(a)) {
                printf("bad\n");
                continue;
            }
            p.release((int)a);
            printf("ok\n");
        } else if (op == "dump") {
            if (!made) {
                printf("bad\n");
                continue;
            }
            for (int s = 0; s < p.n_slots; s++) {
                printf("slot %d:", s);
                for (int i = 0; i < p.held[s]; i++) printf(" %d", p.row(s)[i]);
                printf("\n");
            }
            printf("refs:");
            for (int g = 1; g < p.n_pages; g++) printf(" %d", p.refs[g]);
            printf("\nfree:");
            for (int32_t g : p.free_list) printf(" %d", g);
            printf("\n");
        } else {
            fprintf(stderr, "pagepool_check: unknown operation: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
