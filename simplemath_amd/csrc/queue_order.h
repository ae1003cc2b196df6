// queue_order.h -- the bookkeeping of the two library queues per device (runtime.hip: "two queues per device").
//
// Who last wrote and who last read which span on which queue, the queue an operator takes, and which cross-queue
// dependencies become event edges.  Plain host code, no HIP: the one thing that touches the device -- "order queue q behind
// everything queued on queue p so far" -- is a callable `order(q, p)` the caller passes in (0 on success; anything else is
// handed back).  runtime.hip passes the event record / wait; tests/cpp/queue_order_host.cpp passes a recorder and checks
// happens-before over random and directed programs with a model of its own.  The caller serialises all calls on one
// QueueOrder (runtime.hip: the dispatcher's mutex).
//
// What the bookkeeping promises: two operators that CONFLICT (their declared byte ranges overlap and at least one of them
// writes; an operator's scratch counts as its write) are on the same queue, or the later one's queue has been ordered
// behind the earlier one before the later one is issued.  What it cannot see falls back to order:
//   * a BARRIER operator (undeclared spans, under kOverlapMinBytes, the second queue off) runs on queue 0 behind everything
//     issued before it, and everything issued later is behind it: it raises floor[0];
//   * a FLOOR floor[p] is an operator of queue p every later operator of the other queue orders itself behind: a record
//     that drops out of the table raises it to the record's writer and readers;
//   * an EXTERNAL WAIT (queue 0 was made to wait for something outside the dispatcher) raises floor[0] as well: queue 1's
//     next operator is behind the wait.
#pragma once

#include <stddef.h>
#include <stdint.h>

namespace smhip {

struct Span { const void *p; size_t bytes; };

constexpr int kUses = 256;
constexpr size_t kOverlapMinBytes = (size_t)1 << 20;   // smaller operators are barrier operators: nothing to overlap, nothing to track
// Larger operators stay on queue 0 (tracked like the others).  Two queues do not just overlap a kernel's tail with the next
// one's head: the hardware runs the two kernels side by side, which halves the fixed cost per launch and doubles the streams
// the memory side sees at once.  Cold operands, % of peak with one / two queues (tools/cold_rates.py, profiles/r04_cold_rates_queues.txt):
// a + b at 16 / 32 / 64 MiB per array 63 / 71 / 78 -> 77 / 79 / 80, at 128 / 256 MiB 80.9 / 82.5 -> 79.7 / 78.8;
// (R, 4096) * (1, 4096) at 16 / 32 / 64 MiB 56 / 68 / 75.2 -> 65 / 74 / 75.8, at 128 MiB 79.2 -> 76.8; a * s gains up to 128 MiB.
// (A second queue of another PRIORITY, high or low, ran like one queue: no overlap at all.)
constexpr size_t kOverlapMaxBytes = (size_t)224 << 20;

struct QueueOrder {
    uint64_t seq[2] = {0, 0};      // operators issued per queue
    uint64_t synced[2][2] = {};    // synced[q][p]: queue q is ordered behind queue p's operators up to this one
    uint64_t floor[2] = {0, 0};    // every later operator is ordered behind these (evicted spans, barrier operators)
    // who last wrote / read which span: structure of arrays, so that the overlap scan of an operator (its <= 17 spans against
    // every span on record) is a handful of vector compares
    uintptr_t lo[kUses] = {}, hi[kUses] = {};
    uint64_t wseq[kUses] = {}, rseq[kUses][2] = {};
    unsigned char wq[kUses] = {};
    int used = 0, next = 0;
    int last = 1;                  // the queue the last independent operator took
    bool single = false;           // second queue off (the stream handle was handed out, sharded use, SMHIP_QUEUES=1)
    bool second = false;           // the second queue exists (the caller opens it: queue_begin's `open_second`)
    unsigned long long edges = 0, alternations = 0;  // diagnostics
};

// Orders queue q behind queue p's operators up to `need` (no-op when it already is).
template <class Order>
inline int queue_wait(QueueOrder &d, int q, int p, uint64_t need, Order &&order) {
    if (q == p || need <= d.synced[q][p] || !d.second) return 0;
    if (int rc = order(q, p)) return rc;
    d.synced[q][p] = d.seq[p];  // the event covers everything queued on p so far
    ++d.edges;
    return 0;
}
// Queue 0 waits for everything on queue 1 and becomes the point everything later is ordered behind: what an operator
// with undeclared spans, a read-back, a timing event or a hand-over to a caller's stream needs.
template <class Order>
inline int queue_barrier(QueueOrder &d, Order &&order) {
    if (d.second) {
        if (int rc = queue_wait(d, 0, 1, d.seq[1], order)) return rc;
    }
    d.floor[0] = ++d.seq[0];
    return 0;
}
// The record of span [lo, hi): the one that names exactly it, or a fresh one (what drops out of the table becomes a floor).
inline int use_slot(QueueOrder &d, uintptr_t lo, uintptr_t hi) {
    for (int i = 0; i < d.used; ++i)
        if (d.lo[i] == lo && d.hi[i] == hi) return i;
    int i;
    if (d.used < kUses) {
        i = d.used++;
    } else {
        i = d.next;
        d.next = (d.next + 1) % kUses;
        if (d.wseq[i] > d.floor[d.wq[i]]) d.floor[d.wq[i]] = d.wseq[i];
        for (int k = 0; k < 2; ++k)
            if (d.rseq[i][k] > d.floor[k]) d.floor[k] = d.rseq[i][k];
    }
    d.lo[i] = lo;
    d.hi[i] = hi;
    d.wseq[i] = d.rseq[i][0] = d.rseq[i][1] = 0;
    d.wq[i] = 0;
    return i;
}
// What an operator that reads `reads` and writes `write` must be ordered behind, per queue -- on top of the floors, which
// every operator is behind and which therefore say nothing about the queue that suits it.
inline void dependencies(const QueueOrder &d, const Span *reads, size_t n_reads, Span write, uint64_t (&need)[2]) {
    need[0] = need[1] = 0;
    const int n = d.used;
    if (write.p && write.bytes) {  // WAW and WAR
        const uintptr_t lo = reinterpret_cast<uintptr_t>(write.p), hi = lo + write.bytes;
        for (int i = 0; i < n; ++i) {
            if (d.lo[i] < hi && lo < d.hi[i]) {
                if (d.wseq[i] > need[d.wq[i]]) need[d.wq[i]] = d.wseq[i];
                if (d.rseq[i][0] > need[0]) need[0] = d.rseq[i][0];
                if (d.rseq[i][1] > need[1]) need[1] = d.rseq[i][1];
            }
        }
    }
    for (size_t r = 0; r < n_reads; ++r) {  // RAW
        if (!reads[r].p || !reads[r].bytes) continue;
        const uintptr_t lo = reinterpret_cast<uintptr_t>(reads[r].p), hi = lo + reads[r].bytes;
        for (int i = 0; i < n; ++i)
            if (d.lo[i] < hi && lo < d.hi[i] && d.wseq[i] > need[d.wq[i]]) need[d.wq[i]] = d.wseq[i];
    }
}

// An operator begins: picks its queue (*queue), orders it behind what it depends on and records its spans.  `barrier`: its
// spans are not declared; `enabled`: the process has not turned the second queue off; `open_second()` creates the second
// queue the first time a tracked operator needs it (false: it cannot be had, the device stays on one queue for good).
template <class Order, class OpenSecond>
inline int queue_begin(QueueOrder &d, const Span *reads, size_t n_reads, Span write, bool barrier, bool enabled, int *queue,
                       Order &&order, OpenSecond &&open_second) {
    *queue = 0;
    size_t bytes = write.bytes;
    for (size_t i = 0; i < n_reads; ++i) bytes += reads[i].bytes;
    if (barrier || d.single || !enabled || bytes < kOverlapMinBytes) return queue_barrier(d, order);
    if (!d.second) {
        if (!open_second()) {
            d.single = true;
            return queue_barrier(d, order);
        }
        d.second = true;
    }
    uint64_t need[2];
    dependencies(d, reads, n_reads, write, need);
    // the queue that costs no event edge; an operator that depends on nothing unfinished elsewhere takes the queue the
    // previous such operator did not
    const bool edge0 = need[1] > d.synced[0][1], edge1 = need[0] > d.synced[1][0];  // what running on queue 0 / 1 would have to wait for
    int q;
    if (bytes > kOverlapMaxBytes) q = 0;
    else if (edge0 != edge1) q = edge0 ? 1 : 0;
    else if (!edge0) { q = d.last ^ 1; d.last = q; ++d.alternations; }
    else q = 0;
    if (int rc = queue_wait(d, q, q ^ 1, need[q ^ 1] > d.floor[q ^ 1] ? need[q ^ 1] : d.floor[q ^ 1], order)) return rc;
    const uint64_t my = ++d.seq[q];
    if (write.p && write.bytes) {
        const int w = use_slot(d, reinterpret_cast<uintptr_t>(write.p), reinterpret_cast<uintptr_t>(write.p) + write.bytes);
        d.wq[w] = (unsigned char)q;
        d.wseq[w] = my;
        d.rseq[w][0] = d.rseq[w][1] = 0;
    }
    for (size_t i = 0; i < n_reads; ++i) {
        if (!reads[i].p || !reads[i].bytes) continue;
        const int r = use_slot(d, reinterpret_cast<uintptr_t>(reads[i].p), reinterpret_cast<uintptr_t>(reads[i].p) + reads[i].bytes);
        d.rseq[r][q] = my;
    }
    *queue = q;
    return 0;
}

// Bytes the operator in progress on queue q allocated for itself (partial sums, written-out periods, the temporaries of a
// cut chain): a write of that operator, ordered behind whoever used those bytes before.
template <class Order>
inline int note_scratch(QueueOrder &d, int q, const void *p, size_t bytes, Order &&order) {
    if (d.single || !d.second) return 0;  // one queue: stream order
    uint64_t need[2];
    dependencies(d, nullptr, 0, Span{p, bytes}, need);
    if (int rc = queue_wait(d, q, q ^ 1, need[q ^ 1] > d.floor[q ^ 1] ? need[q ^ 1] : d.floor[q ^ 1], order)) return rc;
    const int w = use_slot(d, reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + bytes);
    d.wq[w] = (unsigned char)q;
    d.wseq[w] = d.seq[q];
    d.rseq[w][0] = d.rseq[w][1] = 0;
    return 0;
}
// The library's stream handle is about to order something OUTSIDE the dispatcher (a caller's stream, a host wait, a peer
// copy): make queue 0's tail stand for all the library's work on the device.
template <class Order>
inline void queues_join(QueueOrder &d, Order &&order) {
    if (d.second) (void)queue_wait(d, 0, 1, d.seq[1], order);
}
// The host has just waited for queue 0 behind a barrier: everything either queue was given is finished, so nothing on
// record constrains the choice of queue any more.  (Without this an operator whose operands were last written long ago
// on queue 0 would stay on queue 0 for ever: an edge to a finished operator costs nothing on the GPU, but the policy avoids
// edges.)
inline void queues_all_complete(QueueOrder &d) {
    d.synced[0][1] = d.seq[1];
    d.synced[1][0] = d.seq[0];
}
// Queue 0 was just made to wait for something outside the dispatcher: queue 1's next operator orders itself behind that.
inline void queues_after_external_wait(QueueOrder &d) {
    d.floor[0] = ++d.seq[0];
}
// Second queue off (true) / on again (false).
template <class Order>
inline void queue_single(QueueOrder &d, bool single, Order &&order) {
    if (single && d.second) (void)queue_wait(d, 0, 1, d.seq[1], order);
    if (single) d.floor[0] = ++d.seq[0];
    d.single = single;
}

}  // namespace smhip
