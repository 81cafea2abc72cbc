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
//   write slot lo hi        plan, check against the free list, apply           -> cow OLD NEW | fail 28
//   release slot
//   dump                    every slot's pages, the counts of pages 1.., the free list
// Every operation that changes something checks its argument ranges and answers `bad` otherwise.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

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
        } else if (op == "plan" || op == "write") {
            if (!(in >> a >> b >> c) || !slot_ok(a) || b < 0 || c < b - 1 || p.pages_for(c + 1) > p.max_pages) {
                printf("bad\n");
                continue;
            }
            const PagePool::WritePlan w = p.plan_write((int)a, b, c);
            if (op == "plan") {
                printf("plan %d %d %d %d %d %lld %lld\n", w.first, w.last, w.n_private, w.copy_index, w.copy_rows,
                       (long long)w.grow, (long long)w.fresh());
                continue;
            }
            if (w.fresh() > p.free_count()) {
                printf("fail 28\n");
                continue;
            }
            int32_t was = 0, now = 0;
            p.make_private((int)a, w, b, c, &was, &now);
            printf("cow %d %d\n", was, now);
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
