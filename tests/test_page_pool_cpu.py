"""CPU: the reference-counted page pool of the paged KV cache (csrc/page_pool.hpp), driven
through the plain host program pagepool_check and compared, line for line, with a small Python
model of the same rules written from DESIGN.md §18:

  * page 0 is the scratch page; pages are handed out from a LIFO free list that starts with
    page 1 on top; a page that becomes free is the next one taken;
  * a slot's release lets go of its pages last page first; a page is free when its count is 0;
  * a fork shares the full pages and takes one fresh page for a partial tail, after releasing
    the destination, and only if that page is there (free list + pages only the destination
    holds);
  * a writer of positions [lo, hi] replaces the pages of that range whose count is above 1 by
    fresh ones (ascending), copies rows [0, lo % T) of the page holding lo when that one is
    replaced, then grows to hi + 1 tokens — all or nothing against the free list;
  * a reservation is a list of such writes (spans) taken as a whole: every span is planned against
    the pool as it stands, the sum of their fresh pages is compared with the free list once, and
    only then are they applied in order (one copy per span at the most).  A restart reservation
    gives each of its slots a new sequence of len tokens: it needs the pages of all of them minus
    the pages only each slot holds, releases all its slots in order, then grows them in order.

The sanitizer build of the same program (make pagepool_check_asan) runs the same script directly."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qwen_inference_engine_amd", "csrc")


class Model:
    def __init__(self, slots, max_pages, T, n_pages):
        self.T, self.n_pages = T, n_pages
        self.rows = [[] for _ in range(slots)]
        self.refs = [0] * n_pages
        self.free = list(range(n_pages - 1, 0, -1))

    def pages_for(self, ntok):
        return -(-ntok // self.T)

    def take(self):
        p = self.free.pop()
        self.refs[p] = 1
        return p

    def drop(self, p):
        self.refs[p] -= 1
        if self.refs[p] == 0:
            self.free.append(p)

    def exclusive(self, s):
        return sum(1 for p in self.rows[s] if self.refs[p] == 1)

    def grow(self, s, ntok):
        if self.pages_for(ntok) - len(self.rows[s]) > len(self.free):
            return "fail 28"
        while len(self.rows[s]) < self.pages_for(ntok):
            self.rows[s].append(self.take())
        return "ok"

    def release(self, s):
        for p in reversed(self.rows[s]):
            self.drop(p)
        self.rows[s] = []
        return "ok"

    def fork(self, src, dst, ntok):
        tail = 1 if ntok % self.T else 0
        if tail > len(self.free) + self.exclusive(dst):
            return "fail 28"
        self.release(dst)
        for p in self.rows[src][:ntok // self.T]:
            self.refs[p] += 1
            self.rows[dst].append(p)
        if tail:
            self.rows[dst].append(self.take())
        return "ok"

    def plan(self, s, lo, hi):
        held = len(self.rows[s])
        grow = max(0, self.pages_for(hi + 1 if hi >= lo else lo) - held)
        if hi < lo:
            return (0, -1, 0, -1, 0, grow, grow)
        first, last = lo // self.T, min(hi // self.T, held - 1)
        shared = [i for i in range(first, last + 1) if self.refs[self.rows[s][i]] > 1]
        copy = first if first in shared and lo % self.T else -1
        return (first, last, len(shared), copy, lo % self.T if copy >= 0 else 0, grow, len(shared) + grow)

    def write(self, s, lo, hi):
        first, last, n_priv, copy, rows, grow, fresh = self.plan(s, lo, hi)
        if fresh > len(self.free):
            return "fail 28"
        was = now = 0
        for i in range(first, last + 1):
            old = self.rows[s][i]
            if self.refs[old] > 1:
                self.rows[s][i] = self.take()
                self.drop(old)
                if i == copy:
                    was, now = old, self.rows[s][i]
        self.grow(s, hi + 1 if hi >= lo else lo)
        return f"cow {was} {now}"

    def reserve(self, *a):
        spans = [a[i:i + 3] for i in range(0, len(a), 3)]
        need = sum(self.plan(*sp)[6] for sp in spans)          # each against the untouched pool
        if need > len(self.free):
            return f"fail 28 need {need} free {len(self.free)}"
        out = f"ok {need}"
        for s, lo, hi in spans:
            copy, rows = self.plan(s, lo, hi)[3:5]             # what is shared NOW: an earlier span may have left it
            was, now = self.write(s, lo, hi).split()[1:]
            if now != "0":
                out += f" cow {s} {copy} {rows} {was} {now}"
        return out

    def restart(self, *a):
        pairs = [a[i:i + 2] for i in range(0, len(a), 2)]
        need = sum(self.pages_for(n) for _, n in pairs) - sum(self.exclusive(s) for s, _ in pairs)
        if need > len(self.free):
            return f"fail 28 need {need} free {len(self.free)}"
        for s, _ in pairs:
            self.release(s)
        for s, n in pairs:
            self.grow(s, n)
        return f"ok {need}"

    def dump(self):
        out = [f"slot {s}:" + "".join(f" {p}" for p in r) for s, r in enumerate(self.rows)]
        out.append("refs:" + "".join(f" {c}" for c in self.refs[1:]))
        out.append("free:" + "".join(f" {p}" for p in self.free))
        return out


# T = 128.  The first block is an unshared run in the style of test_gpu_paged.py's release / reuse
# script (three prompts of 60, 200, 90 tokens in a pool of 7 usable pages, slot 1 released and
# refilled): its tables must be the ones the allocator produced before pages were counted.
SCRIPT = """
init 3 4 128 8
grow 0 60
grow 1 200
grow 2 90
dump
grow 0 129
release 1
grow 1 150
grow 1 400
grow 2 512
dump
release 0
release 1
release 2
dump
# a fork at 300: two full pages shared, the tail page fresh
grow 0 300
fork 0 2 300
dump
plan 2 300 300
plan 2 200 200
plan 0 130 170
plan 2 0 299
plan 2 256 255
# the fork rewinds to 200: page index 1 becomes private, rows [0, 72) to copy
write 2 200 200
dump
# the source rewinds to 130: its page index 1 is private again already (count 1)
write 0 130 300
dump
# a rewind to a page boundary replaces the page and copies nothing
write 2 0 0
dump
# exhaustion: 7 usable pages, all-or-nothing
grow 1 512
dump
fork 0 1 100
write 0 0 10
grow 2 512
release 1
fork 0 1 100
fork 0 1 256
dump
# plain references, as a prefix handle holds them
share 1
share 1
release 0
release 1
release 2
dump
drop 1
drop 1
take
dump
drop 1
dump
# case A: two spans of one reservation rewind into the same shared page (4 usable pages, 1 free)
init 3 4 128 5
grow 0 300
fork 0 1 256
reserve 0 130 130 1 130 130
dump
reserve 0 130 130
reserve 1 130 130
dump
# ... with 5 usable pages both fit: one copy, the second span finds the page its own, page 5 stays free
init 3 4 128 6
grow 0 300
fork 0 1 256
reserve 0 130 130 1 130 130
dump
# case B: a restart of slots that share only with each other
init 3 4 128 4
grow 0 256
fork 0 1 256
restart 0 128 1 128
dump
restart 0 128
dump
# case C: growth and a copy in one span
init 3 4 128 6
grow 0 200
fork 0 1 200
reserve 1 100 260
dump
# several spans in order; a grow-only span
init 4 4 128 12
grow 0 300
fork 0 1 300
fork 0 2 200
reserve 2 150 400 1 10 20 0 256 255 3 0 -1
dump
restart 1 500 2 1 3 129
dump
"""


def _expected(script):
    m, out = None, []
    for ln in script.splitlines():
        f = ln.split()
        if not f or f[0].startswith("#"):
            continue
        a = [int(x) for x in f[1:]]
        op = f[0]
        if op == "init":
            m = Model(*a)
            out.append("ok")
        elif op == "dump":
            out += m.dump()
        elif op == "plan":
            out.append("plan " + " ".join(str(x) for x in m.plan(*a)))
        elif op == "take":
            out.append(f"page {m.take()}" if m.free else "fail 28")
        elif op == "share":
            m.refs[a[0]] += 1
            out.append("ok")
        elif op == "drop":
            m.drop(a[0])
            out.append("ok")
        else:
            out.append(getattr(m, op)(*a))
    return out


def _run(target, script):
    subprocess.run(["make", "-s", "-C", CSRC, target], check=True, timeout=300)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(CSRC, "..", "_build", target)], input=script, text=True, capture_output=True,
                       timeout=60, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    return r.stdout.splitlines()


def test_page_pool_follows_the_model():
    got, want = _run("pagepool_check", SCRIPT), _expected(SCRIPT)
    assert got == want, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:5]
    # the script went through every outcome the rules have
    assert "fail 28" in want and any(w.startswith("cow ") and w != "cow 0 0" for w in want)


def test_unshared_page_order_is_the_allocators():
    """Page 1 first, LIFO reuse: the tables of an unshared run, written out by hand."""
    got = _run("pagepool_check", SCRIPT)
    d0 = got.index("slot 0: 1")
    assert got[d0:d0 + 5] == ["slot 0: 1", "slot 1: 2 3", "slot 2: 4", "refs: 1 1 1 1 0 0 0", "free: 7 6 5"]
    # slot 0 grows (5); slot 1's release returns 3 then 2, so its refill takes 2 then 3, then 6, 7;
    # slot 2 cannot grow to 4 pages: nothing changes
    d1 = got.index("slot 0: 1 5")
    assert got[d1:d1 + 5] == ["slot 0: 1 5", "slot 1: 2 3 6 7", "slot 2: 4", "refs: 1 1 1 1 1 1 1", "free:"]
    assert got[d1 - 1] == "fail 28"


def test_page_pool_rejects_bad_operations():
    got = _run("pagepool_check", "grow 0 1\ninit 2 2 128 4\ngrow 5 1\ngrow 0 300\nshare 3\ndrop 0\nfork 0 0 1\n"
                                 "fork 0 1 1\nplan 0 5 2\nrelease 9\n")
    assert got == ["bad", "ok", "bad", "bad", "bad", "bad", "bad", "bad", "bad", "bad"]
    # reservations: a slot out of range, more spans than a batch has slots, a length beyond
    # max_pages, an incomplete span, a restart naming a slot twice, a restart of nothing
    got = _run("pagepool_check", "init 2 2 128 4\nreserve 2 0 0\nrestart 2 10\nreserve" + " 0 0 0" * 9 + "\nrestart" +
                                 " 0 1" * 9 + "\nrestart 0 257\nreserve 0 0 256\nreserve 0 0\nrestart 0 10 0 10\n"
                                 "restart 0 0\nreserve\nreserve 0 0 0" + " 1 0 -1" * 7 + "\ndump\n")   # 8 spans: the capacity
    assert got == ["ok"] + ["bad"] * 10 + ["ok 1", "slot 0: 1", "slot 1:", "refs: 1 0 0", "free: 3 2"]


def test_reservations_by_hand():
    """The lines of cases A, B and C, written out by hand from the single-span operations."""
    got = _run("pagepool_check", SCRIPT)
    a = got.index("fail 28 need 2 free 1")
    assert got[a:a + 12] == ["fail 28 need 2 free 1", "slot 0: 1 2 3", "slot 1: 1 2", "slot 2:", "refs: 2 2 1 0",
                             "free: 4", "ok 1 cow 0 1 2 2 4", "ok 0", "slot 0: 1 4 3", "slot 1: 1 2", "slot 2:",
                             "refs: 2 1 1 1"]
    a6 = got.index("ok 2 cow 0 1 2 2 4")
    assert got[a6:a6 + 6] == ["ok 2 cow 0 1 2 2 4", "slot 0: 1 4 3", "slot 1: 1 2", "slot 2:", "refs: 2 1 1 1 0",
                              "free: 5"]
    b = got.index("fail 28 need 2 free 1", a + 1)
    assert got[b + 1:b + 6] == ["slot 0: 1 2", "slot 1: 1 2", "slot 2:", "refs: 2 2 0", "free: 3"]
    assert got[b + 6:b + 12] == ["ok 1", "slot 0: 3", "slot 1: 1 2", "slot 2:", "refs: 1 1 1", "free:"]
    c = got.index("ok 2 cow 1 0 100 1 4")
    assert got[c + 1:c + 6] == ["slot 0: 1 2", "slot 1: 4 3 5", "slot 2:", "refs: 1 1 1 1 1", "free:"]


def test_page_pool_clean_under_asan_ubsan():
    got = _run("pagepool_check_asan", SCRIPT)
    assert got == _expected(SCRIPT)
