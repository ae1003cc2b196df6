// queue_order_host.cpp -- csrc/queue_order.h, the bookkeeping of the two library queues, checked on the host (no GPU, no library).
//
// The header is driven the way runtime.hip drives it, with an `order(q, p)` that only records "queue q waits for queue p".
// Against it stands a model that knows nothing of the header's seq / synced / floor numbers:
//   * it counts the operators issued per queue itself;
//   * a recorded wait (q, p) means: q's later operators are behind everything issued on p so far;
//   * a synchronise means: everything issued so far is complete;
//   * every new operator must have each earlier operator it CONFLICTS with on its own queue, complete, or known to be behind it.
// Two operators conflict when byte ranges of theirs overlap and at least one of the two writes (an operator's scratch is a write
// of that operator); a BARRIER operator (undeclared spans, under kOverlapMinBytes, issued while `single` is on) conflicts with
// everything before and after it; an EXTERNAL WAIT on queue 0 conflicts with everything after it.
//
// Programs: random ones (dense: a few buffers, exact repeats, nested / partial / adjacent windows, in-place operators, 0..8
// reads, operators under 1 MiB and over 224 MiB, scratch that reuses earlier bytes, barriers, external waits, synchronises,
// `single` on and off; sparse: thousands of windows, so that records fall out of the table while few edges exist), directed
// eviction programs (an access, more than kUses fresh spans without one edge, the revisit from the other queue) and precision
// programs (independent work makes no edge at all, so "order everything behind everything" does not pass).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "queue_order.h"

using smhip::Span;

namespace {

struct Range { uintptr_t lo, hi; };
enum Kind { TRACKED, BARRIER, EXTERNAL };
struct Op {
    int queue;
    uint64_t index;  // the model's own count on that queue, from 1
    Kind kind;
    std::vector<Range> reads, writes;
    long serial;
};

long g_pairs = 0, g_span_pairs = 0, g_unordered = 0, g_operators = 0;

struct Machine {
    smhip::QueueOrder d;
    // the model
    uint64_t issued[2] = {0, 0};
    uint64_t behind[2][2] = {};  // behind[q][p]: q's later operators are behind p's first so-many
    uint64_t complete[2] = {0, 0};
    std::vector<Op> live;
    long waits = 0, serial = 0;
    int last_wait_q = -1, last_wait_p = -1;
    const char *program = "";

    struct Recorder {
        Machine *m;
        int operator()(int q, int p) const {
            if (q == p || q < 0 || q > 1 || p < 0 || p > 1) { printf("%s: order(%d, %d) is no edge between the two queues\n", m->program, q, p); ++g_unordered; return 0; }
            m->behind[q][p] = m->issued[p];
            ++m->waits;
            m->last_wait_q = q;
            m->last_wait_p = p;
            return 0;
        }
    };
    Recorder recorder() { return Recorder{this}; }

    static bool overlap(const std::vector<Range> &a, const std::vector<Range> &b) {
        for (const Range &x : a)
            for (const Range &y : b)
                if (x.lo < y.hi && y.lo < x.hi) return true;
        return false;
    }
    bool ordered(const Op &e, const Op &n) const {
        return e.queue == n.queue || e.index <= complete[e.queue] || e.index <= behind[n.queue][e.queue];
    }
    void check_and_keep(Op &&n) {
        n.serial = ++serial;
        ++g_operators;
        for (const Op &e : live) {
            bool conflict;
            if (e.kind != TRACKED || n.kind == BARRIER) {
                conflict = true;  // e is a barrier or an external wait: everything after it; n is a barrier: everything before it
                if (e.kind == EXTERNAL && n.kind == EXTERNAL) conflict = false;
            } else if (n.kind == EXTERNAL) {
                conflict = false;
            } else {
                conflict = overlap(e.writes, n.writes) || overlap(e.writes, n.reads) || overlap(e.reads, n.writes);
                if (conflict) ++g_span_pairs;
            }
            if (!conflict) continue;
            ++g_pairs;
            if (!ordered(e, n)) {
                if (++g_unordered <= 8)
                    printf("%s: UNORDERED operator #%ld (queue %d, its %llu., kind %d) is not behind #%ld (queue %d, its %llu., kind %d); queue %d is behind %llu of queue %d\n",
                           program, n.serial, n.queue, (unsigned long long)n.index, (int)n.kind, e.serial, e.queue, (unsigned long long)e.index, (int)e.kind, n.queue,
                           (unsigned long long)behind[n.queue][e.queue], e.queue);
            }
        }
        live.push_back(std::move(n));
    }

    // ---- what runtime.hip does, step by step
    // An operator of the C ABI: OpScope::begin, the allocations it makes for itself, its launches.  Returns its queue.
    int op(const std::vector<Span> &reads, Span write, bool barrier, const std::vector<Span> &scratch = {}) {
        size_t bytes = write.bytes;
        for (const Span &s : reads) bytes += s.bytes;
        const bool is_barrier = barrier || d.single || bytes < smhip::kOverlapMinBytes;  // what the library promises, not what the header did
        int q = -1;
        const int rc = smhip::queue_begin(d, barrier ? nullptr : reads.data(), barrier ? 0 : reads.size(), barrier ? Span{nullptr, 0} : write, barrier, true, &q,
                                          recorder(), [] { return true; });
        if (rc != 0 || q < 0 || q > 1) { printf("%s: queue_begin gave rc %d queue %d\n", program, rc, q); ++g_unordered; return 0; }
        if (is_barrier && q != 0) { printf("%s: a barrier operator on queue %d\n", program, q); ++g_unordered; }
        Op n;
        n.queue = q;
        n.index = ++issued[q];
        n.kind = is_barrier ? BARRIER : TRACKED;
        for (const Span &s : reads)
            if (s.p && s.bytes) n.reads.push_back(Range{(uintptr_t)s.p, (uintptr_t)s.p + s.bytes});
        if (write.p && write.bytes) n.writes.push_back(Range{(uintptr_t)write.p, (uintptr_t)write.p + write.bytes});
        for (const Span &s : scratch) {
            if (smhip::note_scratch(d, q, s.p, s.bytes, recorder()) != 0) { printf("%s: note_scratch failed\n", program); ++g_unordered; }
            n.writes.push_back(Range{(uintptr_t)s.p, (uintptr_t)s.p + s.bytes});
        }
        check_and_keep(std::move(n));
        return q;
    }
    void synchronise() {  // smhip_synchronize: a barrier operator, the host waits for queue 0, queues_all_complete
        op({}, Span{nullptr, 0}, true);
        complete[0] = issued[0];
        complete[1] = issued[1];
        live.clear();
        smhip::queues_all_complete(d);
    }
    void external_wait() {  // queue 0 was made to wait for an event from outside, then queues_after_external_wait
        Op n;
        n.queue = 0;
        n.index = ++issued[0];
        n.kind = EXTERNAL;
        check_and_keep(std::move(n));
        smhip::queues_after_external_wait(d);
    }
    void single(bool on) { smhip::queue_single(d, on, recorder()); }
    bool on_record(uintptr_t lo, uintptr_t hi) const {
        for (int i = 0; i < d.used; ++i)
            if (d.lo[i] == lo && d.hi[i] == hi) return true;
        return false;
    }
};

// ------------------------------------------------------------------------------------------------ random programs
struct Rng {
    uint64_t s;
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    uint64_t below(uint64_t n) { return next() % n; }
    bool one_in(uint64_t n) { return below(n) == 0; }
};

constexpr uintptr_t kBase = (uintptr_t)0x7f00 << 32;
constexpr size_t kUnit = (size_t)256 << 10;

void random_program(uint64_t seed, bool sparse, int n_ops) {
    static char name[64];
    snprintf(name, sizeof name, "%s %llu", sparse ? "sparse" : "dense", (unsigned long long)seed);
    Machine m;
    m.program = name;
    Rng r{seed * 0x9E3779B97F4A7C15ull + 1};
    std::vector<Span> history;   // spans operators used
    std::vector<Span> scratches; // the pool: blocks handed out as scratch before, and operand spans that were "freed"
    const int buffers = sparse ? 48 : 5;
    const size_t units = sparse ? 128 : 256;  // per buffer: 32 / 64 MiB
    auto fresh = [&](size_t max_units) {
        const size_t len = 1 + r.below(max_units), start = r.below(units - len + 1);
        return Span{(const void *)(kBase + ((uintptr_t)r.below(buffers) << 30) + start * kUnit), len * kUnit};
    };
    auto window = [&]() -> Span {
        const size_t max_units = sparse ? 4 : 64;
        if (history.empty()) return fresh(max_units);
        const size_t back = sparse ? history.size() : (history.size() < 64 ? history.size() : 64);
        const Span h = history[history.size() - 1 - r.below(back)];
        const uintptr_t lo = (uintptr_t)h.p;
        switch (r.below(sparse ? 24 : 8)) {
        case 0: return h;                                                                      // an exact repeat
        case 1: { const size_t cut = h.bytes / 4; return Span{(const void *)(lo + cut), h.bytes - 2 * cut}; }  // nested
        case 2: return Span{(const void *)(lo + h.bytes / 2), h.bytes};                         // partial overlap
        case 3: return Span{(const void *)(lo + h.bytes), h.bytes};                             // adjacent: touches, no overlap
        case 4: return Span{(const void *)(lo + h.bytes - 64), 4096};                           // the last 64 bytes and beyond
        case 5: return lo >= kBase + kUnit ? Span{(const void *)(lo - kUnit), kUnit} : h;      // adjacent below
        default: return fresh(max_units);
        }
    };
    for (int i = 0; i < n_ops; ++i) {
        const uint64_t what = r.below(1000);
        if (what < 3) { m.synchronise(); continue; }
        if (what < 10) { m.external_wait(); continue; }
        if (what < 14) { m.single(!m.d.single); continue; }
        if (what < 40) { m.op({}, Span{nullptr, 0}, true); continue; }  // an entry point without declared spans
        std::vector<Span> reads, scratch;
        Span write;
        if (what < 70) {  // under 1 MiB in all: a barrier operator whatever it declares
            write = Span{window().p, 4096 + r.below(64) * 1024};
            if (r.one_in(2)) reads.push_back(Span{window().p, 100000});
        } else if (what < 80 && !sparse) {  // over 224 MiB: tracked, queue 0
            write = Span{(const void *)(kBase + ((uintptr_t)62 << 30) + r.below(4) * ((size_t)64 << 20)), (size_t)128 << 20};
            reads.push_back(Span{(const void *)(kBase + ((uintptr_t)63 << 30)), ((size_t)100 << 20) + r.below(64) * kUnit});
            if (r.one_in(2)) reads.push_back(window());
        } else {
            const int n_reads = (int)r.below(9);
            for (int k = 0; k < n_reads; ++k) reads.push_back(window());
            if (n_reads && r.one_in(4)) write = reads[r.below(n_reads)];  // in place
            else if (r.one_in(12)) write = Span{nullptr, 0};              // reads only
            else write = window();
            if (r.one_in(16)) reads.push_back(Span{nullptr, 0});          // an absent operand
        }
        for (int k = (int)r.below(sparse ? 16 : 6); k < 2 && k >= 0 && r.one_in(2); ++k) {  // scratch inside the operator
            if (!scratches.empty() && r.one_in(2)) scratch.push_back(scratches[r.below(scratches.size())]);  // the pool hands an earlier block out again
            else if (!history.empty() && r.one_in(2)) scratch.push_back(history[r.below(history.size())]);   // bytes an earlier operator used, freed since
            else scratch.push_back(fresh(8));
            scratches.push_back(scratch.back());
        }
        const int q = m.op(reads, write, false, scratch);
        size_t bytes = write.bytes;
        for (const Span &s : reads) bytes += s.bytes;
        if (bytes > smhip::kOverlapMaxBytes && !m.d.single && q != 0) { printf("%s: an operator over kOverlapMaxBytes on queue %d\n", name, q); ++g_unordered; }
        for (const Span &s : reads) if (s.p && s.bytes >= kUnit) history.push_back(s);
        if (write.p && write.bytes >= kUnit) history.push_back(write);
    }
}

// ------------------------------------------------------------------------------------------------ directed eviction programs
// `first` on X from queue `first_queue`, then fresh disjoint spans until X's record has fallen out of the table -- without one
// recorded wait on the way -- then `revisit` of X from the other queue: the model's check of that operator is the test.
Span window_no(long k) { return Span{(const void *)(kBase + (uintptr_t)k * ((size_t)2 << 20)), (size_t)1 << 20}; }
bool eviction_program(bool first_writes, bool revisit_writes, int first_queue) {
    static char name[96];
    const Span X = window_no(0);
    for (int lead = 0; lead <= 1; ++lead) {
        for (int fill = smhip::kUses - 2; fill <= smhip::kUses + 3; ++fill) {
            Machine m;
            snprintf(name, sizeof name, "eviction %s on queue %d, %d fresh spans, then %s", first_writes ? "write" : "read", first_queue, fill, revisit_writes ? "write" : "read");
            m.program = name;
            long k = 1;
            if (lead) {  // one operator elsewhere, completed: the next independent operator takes queue 1
                m.op({}, window_no(k++), false);
                m.synchronise();
            }
            const long waits_before = m.waits;
            const int q_first = first_writes ? m.op({}, X, false) : m.op({X}, Span{nullptr, 0}, false);
            if (q_first != first_queue) continue;
            for (int i = 0; i < fill; ++i) m.op({}, window_no(k++), false);
            if (m.waits != waits_before || m.on_record((uintptr_t)X.p, (uintptr_t)X.p + X.bytes)) continue;  // an edge on the way, or X still on record
            const int q_revisit = revisit_writes ? m.op({}, X, false) : m.op({X}, window_no(k++), false);
            if (q_revisit == q_first) continue;
            return true;  // exercised; whether it was ordered is in g_unordered
        }
    }
    printf("eviction program (%d, %d, queue %d): NOT EXERCISED -- no run reached the revisit without an edge, off the record and from the other queue\n",
           (int)first_writes, (int)revisit_writes, first_queue);
    return false;
}

// ------------------------------------------------------------------------------------------------ precision
bool precision_programs() {
    bool ok = true;
    {   // pairwise disjoint spans: no wait at all, and the queues alternate
        Machine m;
        m.program = "precision: disjoint";
        int prev = -1;
        for (long i = 0; i < 80; ++i) {
            const int q = m.op({window_no(3 * i), window_no(3 * i + 1)}, window_no(3 * i + 2), false);
            if (q == prev) { printf("%s: operators %ld and %ld both on queue %d\n", m.program, i - 1, i, q); ok = false; }
            prev = q;
        }
        if (m.waits != 0) { printf("%s: %ld waits recorded for independent operators\n", m.program, m.waits); ok = false; }
    }
    {   // two dependent chains, interleaved: each stays on its queue, no wait; one operator that reads both results: one wait
        Machine m;
        m.program = "precision: two chains";
        const Span A = window_no(0), B = window_no(1), A2 = window_no(2), B2 = window_no(3);
        int qa = -1, qb = -1;
        for (int i = 0; i < 40; ++i) {
            const Span a_in = i % 2 ? A2 : A, a_out = i % 2 ? A : A2, b_in = i % 2 ? B2 : B, b_out = i % 2 ? B : B2;
            const int a = i % 3 == 0 ? m.op({a_out}, a_out, false) : m.op({a_in, a_out}, a_out, false);
            const int b = i % 3 == 1 ? m.op({b_out}, b_out, false) : m.op({b_in, b_out}, b_out, false);
            if (i == 0) { qa = a; qb = b; }
            if (a != qa || b != qb || qa == qb) { printf("%s: step %d on queues %d / %d, the chains began on %d / %d\n", m.program, i, a, b, qa, qb); ok = false; break; }
        }
        if (m.waits != 0) { printf("%s: %ld waits recorded for two independent chains\n", m.program, m.waits); ok = false; }
        m.op({A, B}, window_no(9), false);
        if (m.waits != 1) { printf("%s: %ld waits recorded for the operator that joins the chains, not 1\n", m.program, m.waits); ok = false; }
    }
    return ok;
}

}  // namespace

int main(int argc, char **argv) {
    const int seeds = argc > 1 ? atoi(argv[1]) : 40;
    bool ok = true;
    for (int s = 1; s <= seeds; ++s) random_program((uint64_t)s, false, 3000);
    for (int s = 1; s <= seeds; ++s) random_program((uint64_t)1000 + s, true, 4000);
    const long random_unordered = g_unordered;
    int evictions = 0;
    for (int first_queue = 0; first_queue <= 1; ++first_queue) {
        ok = eviction_program(true, false, first_queue) && ok;   // written, evicted, read
        ok = eviction_program(true, true, first_queue) && ok;    // written, evicted, written
        ok = eviction_program(false, true, first_queue) && ok;   // read, evicted, written
        evictions += 3;
    }
    const long eviction_unordered = g_unordered - random_unordered;
    const bool precise = precision_programs();
    printf("queue_order random unordered %ld, eviction programs %d unordered %ld, precision %s\n", random_unordered, evictions, eviction_unordered, precise ? "ok" : "FAILED");
    ok = ok && precise && g_unordered == 0;
    printf("queue_order %s operators %ld pairs %ld span_pairs %ld: %ld unordered\n", ok ? "ok" : "FAILED", g_operators, g_pairs, g_span_pairs, g_unordered);
    return ok ? 0 : 1;
}
