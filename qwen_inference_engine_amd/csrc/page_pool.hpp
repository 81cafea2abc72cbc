// Reference-counted page pool of the paged KV cache: the host block table, the
// free list, the pages held per slot and a count per page.  Plain C++, no HIP: the engine
// (engine.hip) owns the device copy of the table, tools/pagepool_check.cpp drives this header
// alone (tests/test_page_pool_cpu.py).
//
// Rules.  Page 0 is the scratch page: never handed out, never counted; a table entry of 0 means
// "no page".  Pages are handed out from the back of the free list, which starts n_pages-1 .. 1:
// page 1 first, and a page that becomes free is the next one taken (LIFO).  A slot's pages are
// its table entries [0, held).  A page may sit in several slots' tables (and in prefix handles,
// which hold plain references): refs[page] counts the holders, and the page returns to the free
// list when the count reaches 0.  Every decision is a function of the call sequence alone, so
// tensor-parallel ranks making the same calls keep identical tables.
//
// All-or-nothing: a writer describes its call as spans, plan_reserve() sums what they would take
// and changes nothing, the caller compares with free_count(), and only then commit() applies
// them (make_private and grow per span), which cannot fail.
#pragma once
#include <cstdint>
#include <vector>

namespace qie {

constexpr int kMaxBatchSlots = 8;   // the most slots a batch can have: a reservation's capacity

struct PagePool {
    int page_tokens = 0, max_pages = 0, n_pages = 0, n_slots = 0;
    std::vector<int32_t> table;       // [n_slots][max_pages]
    std::vector<int32_t> free_list;   // back() is handed out next
    std::vector<int32_t> held;        // [n_slots]
    std::vector<int32_t> refs;        // [n_pages]; refs[0] stays 0

    void init(int slots, int max_pages_, int page_tokens_, int n_pages_) {
        n_slots = slots;
        max_pages = max_pages_;
        page_tokens = page_tokens_;
        n_pages = n_pages_;
        table.assign((size_t)slots * max_pages, 0);
        held.assign(slots, 0);
        refs.assign(n_pages, 0);
        free_list.clear();
        for (int p = n_pages - 1; p >= 1; p--) free_list.push_back(p);   // page 1 handed out first
    }

    int64_t free_count() const { return (int64_t)free_list.size(); }
    int32_t* row(int slot) { return table.data() + (size_t)slot * max_pages; }
    const int32_t* row(int slot) const { return table.data() + (size_t)slot * max_pages; }
    int64_t pages_for(int64_t ntok) const { return (ntok + page_tokens - 1) / page_tokens; }
    // pages the slot still lacks to hold ntok tokens (negative: it holds more than they need)
    int64_t missing(int slot, int64_t ntok) const { return pages_for(ntok) - held[slot]; }
    // pages only this slot holds: what releasing it would return to the free list
    int64_t exclusive(int slot) const {
        int64_t n = 0;
        for (int i = 0; i < held[slot]; i++) n += refs[row(slot)[i]] == 1;
        return n;
    }

    // --- the three page operations (the caller has checked free_count())
    int32_t take() {
        const int32_t p = free_list.back();
        free_list.pop_back();
        refs[p] = 1;
        return p;
    }
    void share(int32_t page) { refs[page] += 1; }
    void drop(int32_t page) {
        if (--refs[page] == 0) free_list.push_back(page);
    }

    // --- slots
    // fresh pages until the slot holds ntok tokens
    void grow(int slot, int64_t ntok) {
        const int64_t need = pages_for(ntok);
        while (held[slot] < need) row(slot)[held[slot]++] = take();
    }
    // appends a reference to `page` as the slot's next page
    void push_shared(int slot, int32_t page) {
        share(page);
        row(slot)[held[slot]++] = page;
    }
    // the slot lets go of every page, last page first (the order a private slot's pages have
    // always returned in)
    void release(int slot) {
        int32_t* r = row(slot);
        for (int i = held[slot] - 1; i >= 0; i--) {
            drop(r[i]);
            r[i] = 0;
        }
        held[slot] = 0;
    }

    // --- forks.  dst becomes a holder of src's first ntok tokens: dst is released, the
    // ntok / page_tokens full pages are shared, and a partial last page is a fresh page of dst's
    // own (the caller copies its ntok % page_tokens rows).  fork_fits() is the check to make first:
    // the tail page against the free list plus what dst's release returns.
    bool fork_fits(int dst, int64_t ntok) const {
        return (ntok % page_tokens ? 1 : 0) <= free_count() + exclusive(dst);
    }
    void fork(int src, int dst, int64_t ntok) {
        release(dst);
        const int full = (int)(ntok / page_tokens);
        for (int i = 0; i < full; i++) push_shared(dst, row(src)[i]);
        if (ntok % page_tokens) row(dst)[held[dst]++] = take();
    }

    // --- writers.  Before positions [lo, hi] of a slot are written (hi < lo: nothing is written,
    // the slot only grows to hold lo tokens): the pages of that range the slot shares with
    // another holder must be replaced by private ones.  Rows at or past a sequence's position
    // are never read and lo is at most the position, so only the page holding lo carries rows
    // worth keeping: its rows [0, lo % page_tokens).
    struct WritePlan {
        int first = 0, last = -1;   // the slot's page indices in the range (clipped to held)
        int n_private = 0;          // shared pages among them: each takes one fresh page
        int copy_index = -1;        // the page index whose first copy_rows rows must be copied, or -1
        int copy_rows = 0;
        int64_t grow = 0;           // fresh pages beyond held to hold hi + 1 tokens
        int64_t fresh() const { return n_private + grow; }
    };
    WritePlan plan_write(int slot, int64_t lo, int64_t hi) const {
        WritePlan w;
        const int64_t ntok = hi >= lo ? hi + 1 : lo;
        const int64_t m = missing(slot, ntok);
        w.grow = m > 0 ? m : 0;
        if (hi < lo) return w;
        w.first = (int)(lo / page_tokens);
        w.last = (int)(hi / page_tokens);
        if (w.last > held[slot] - 1) w.last = held[slot] - 1;
        const int32_t* r = row(slot);
        for (int i = w.first; i <= w.last; i++)
            if (refs[r[i]] > 1) {
                w.n_private += 1;
                if (i == w.first && lo % page_tokens != 0) {
                    w.copy_index = i;
                    w.copy_rows = (int)(lo % page_tokens);
                }
            }
        return w;
    }
    // Applies a plan (ascending page index, then the growth): *old_page / *new_page receive the
    // pair of w.copy_index (0 / 0 without one).  The other holders keep the old pages untouched.
    void make_private(int slot, const WritePlan& w, int64_t lo, int64_t hi, int32_t* old_page, int32_t* new_page) {
        int32_t* r = row(slot);
        if (old_page) *old_page = 0;
        if (new_page) *new_page = 0;
        for (int i = w.first; i <= w.last; i++) {
            if (refs[r[i]] <= 1) continue;
            const int32_t was = r[i];
            r[i] = take();
            drop(was);
            if (i == w.copy_index) {
                if (old_page) *old_page = was;
                if (new_page) *new_page = r[i];
            }
        }
        grow(slot, hi >= lo ? hi + 1 : lo);
    }

    // --- the reservation: what one engine call writes, as at most kMaxBatchSlots spans, planned
    // as a whole, checked once (need <= free_count()) and then committed, which cannot fail.
    // A span is positions [lo, hi] of a slot as plan_write takes them.  restart: the slot begins a
    // new sequence of hi + 1 tokens — it lets go of all its pages first, and the pages only it
    // holds count towards the check.
    struct Span {
        int slot = 0;
        int64_t lo = 0, hi = -1;
        bool restart = false;
    };
    struct Reservation {
        int n = 0;
        int64_t need = 0;   // fresh pages the commit may take beyond what the restart slots return
        Span spans[kMaxBatchSlots];
        WritePlan plans[kMaxBatchSlots];
    };
    // rows [0, rows) of the slot's page `index` are to be copied from old_page into new_page
    struct CopyJob {
        int slot, index, rows;
        int32_t old_page, new_page;
    };
    // Changes nothing.  Every span is planned against the untouched pool, so the total errs on
    // the safe side in two corners: a page shared only among the restart slots of one call counts
    // as returned by none of them, and two spans that both plan a private copy of the same shared
    // page count two pages, although the second finds the page its own at commit.
    Reservation plan_reserve(const Span* spans, int n) const {
        Reservation r;
        r.n = n;
        for (int i = 0; i < n; i++) {
            const Span& s = r.spans[i] = spans[i];
            if (s.restart) {
                r.plans[i].grow = pages_for(s.hi + 1);   // nothing held once it has let go
                r.need += r.plans[i].grow - exclusive(s.slot);
            } else {
                r.plans[i] = plan_write(s.slot, s.lo, s.hi);
                r.need += r.plans[i].fresh();
            }
        }
        return r;
    }
    // Applies a checked reservation: the restart slots are released in span order, then every span
    // in order replaces its shared pages and grows.  jobs (kMaxBatchSlots entries) receives at most
    // one copy per span; returns their number.
    int commit(const Reservation& r, CopyJob* jobs) {
        for (int i = 0; i < r.n; i++)
            if (r.spans[i].restart) release(r.spans[i].slot);
        int n_jobs = 0;
        for (int i = 0; i < r.n; i++) {
            const Span& s = r.spans[i];
            int32_t was = 0, now = 0;
            make_private(s.slot, r.plans[i], s.lo, s.hi, &was, &now);
            // (no new page: another span of this call left the page to this slot alone)
            if (now) jobs[n_jobs++] = CopyJob{s.slot, r.plans[i].copy_index, r.plans[i].copy_rows, was, now};
        }
        return n_jobs;
    }
};

}  // namespace qie
