// abi_args.h -- what an entry point of the C ABI works out about its arguments before it launches: element counts, the bytes a
// view spans, whether two spans share a byte, whether a pointer is aligned.  Each is written here once, for every family file.
// So are the two ways it then opens its operator's scope (SMHIP_ACQUIRE, SMHIP_ACQUIRE_OP).  Header-only, host code only.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "internal.h"     // OpScope
#include "queue_order.h"  // Span

namespace smhip {

// The product of a shape's extents.
inline int64_t element_count(const int64_t *shape, int ndim) {
    int64_t n = 1;
    for (int d = 0; d < ndim; ++d) n *= shape[d];
    return n;
}

// Bytes from a view's first element to its last, through `strides` (in elements, none negative) over `shape`; an extent of 0 adds nothing.
inline size_t span_bytes(const int64_t *shape, const int64_t *strides, int ndim, size_t esz) {
    size_t last = 0;
    for (int d = 0; d < ndim; ++d)
        if (shape[d] > 0) last += (size_t)(shape[d] - 1) * (size_t)strides[d];
    return (last + 1) * esz;
}

// Do two byte spans share a byte?  A null pointer or an empty span shares none with anything.
inline bool spans_overlap(Span x, Span y) {
    if (!x.p || !y.p || !x.bytes || !y.bytes) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(x.p), b = reinterpret_cast<uintptr_t>(y.p);
    return a < b + y.bytes && b < a + x.bytes;
}

// Is `p` off the alignment of an element of `esz` bytes (a power of two)?  A null pointer is aligned.
inline bool misaligned(const void *p, size_t esz) { return (reinterpret_cast<uintptr_t>(p) & (esz - 1)) != 0; }

}  // namespace smhip

// The two ways an entry point opens its scope (written for the part of a file where `using namespace smhip` holds).
// An entry point whose operand spans are not declared: a barrier operator (ordered behind everything, everything later
// behind it) for as long as the function runs.
#define SMHIP_ACQUIRE(stream_var)  \
    hipStream_t stream_var;        \
    OpScope op_scope_;             \
    if (int rc_ = op_scope_.begin_barrier(&stream_var)) return rc_
// An operator with declared spans: reads {ptr, bytes}..., one write.
#define SMHIP_ACQUIRE_OP(stream_var, write_span, ...)                                                         \
    hipStream_t stream_var;                                                                                  \
    OpScope op_scope_;                                                                                       \
    {                                                                                                        \
        const Span reads_[] = {__VA_ARGS__};                                                                 \
        if (int rc_ = op_scope_.begin(reads_, sizeof reads_ / sizeof reads_[0], write_span, &stream_var)) return rc_; \
    }
