// axis_plan.h -- the host-side planner toolbox of the axis families: reduce_axis.hip (sum, mean, max, min), scan_axis.hip
// (cumulative scans), argreduce_axis.hip (argmax / argmin), sort_axis.hip, topk_axis.hip, take_axis.hip, scatter_axis.hip and count.hip.  Each rule
// they share is written here once (the index-mode rules of take, scatter and bincount: index_mode.hip.h):
//   * the merging of a view's axes and the canonical walk out[o, i] = f_r a[o*so + r*sr + i*si] it may come to (Canon, ROW / COLUMN);
//   * lanes per short row (segment_lanes; segment_for where whole rows are copied) and the cutting of R into chunks when a launch
//     would have too few lanes (split_row, split_column);
//   * the capped grid (GridCap), the argument checks every entry point makes, the pooled dense copy of a view (Pooled);
//   * vec_width, ceil_div, dense strides, and the constants and the OutMap the families' kernels are written against.
// Header-only; everything but OutMap and the constants is host code.
#pragma once

#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "internal.h"
#include "smhip.h"

namespace smhip {
namespace axis_plan {

constexpr int kBlock = 256;
constexpr int kRowsInFlight = 4;                    // ROW, short rows: rows per segment in flight
constexpr int64_t kTargetLanes = (int64_t)1 << 18;  // lanes a launch should have before R is split (256 CUs x 1024)

// Where a launch's results go: out[o*oso + i*osi + c*ocs] (c = the chunk of R; 0 when R is not split).  A kernel parameter.
struct OutMap { int64_t oso, osi, ocs; };

inline int vec_width(int dtype) { return dtype == SMHIP_F64 || dtype == SMHIP_I64 ? 2 : 4; }  // elements of a 16-byte vector
inline int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// Row-major strides of `shape` over the axes that `keep` names (all of them by default), 0 for the others; returns the total.
inline int64_t dense_strides(const int64_t *shape, int ndim, int64_t *st, uint32_t keep = ~0u) {
    int64_t acc = 1;
    for (int d = ndim - 1; d >= 0; --d) {
        st[d] = 0;
        if (keep >> d & 1) st[d] = acc, acc *= shape[d];
    }
    return acc;
}

inline bool row_major(const int64_t *shape, const int64_t *strides, int ndim) {
    int64_t acc = 1;
    for (int d = ndim - 1; d >= 0; --d) {
        if (shape[d] != 1 && strides[d] != acc) return false;
        acc *= shape[d];
    }
    return true;
}

struct Ax { int64_t n, st, ost; bool red; int64_t st2 = 0; };

// Axes of extent > 1, ordered by stride (largest first, ties in index order), neighbours merged where memory -- and for kept
// axes the dense result -- runs on without a gap.  Returns the count.
// The gather (take_axis.hip) walks a result that keeps the named axis and reads a second operand: `result_strides` stands in
// for the dense strides over the kept axes, and `second` is that operand's strides, which must run on as well (Ax::st2).
inline int merge_axes(const int64_t *shape, const int64_t *strides, int ndim, uint32_t mask, bool by_index, Ax *ax,
                      const int64_t *result_strides = nullptr, const int64_t *second = nullptr) {
    int64_t ost[SMHIP_MAX_NDIM];
    dense_strides(shape, ndim, ost, ~mask);
    int n = 0;
    for (int d = 0; d < ndim; ++d)
        if (shape[d] > 1) ax[n++] = Ax{shape[d], strides[d], result_strides ? result_strides[d] : ost[d], (mask >> d & 1) != 0, second ? second[d] : 0};
    if (!by_index) std::stable_sort(ax, ax + n, [](const Ax &x, const Ax &y) { return x.st > y.st; });
    int m = 0;
    for (int k = 0; k < n; ++k) {
        if (m > 0) {
            Ax &prev = ax[m - 1];
            if (prev.red == ax[k].red && prev.st == ax[k].st * ax[k].n && (prev.red || prev.ost == ax[k].ost * ax[k].n) &&
                prev.st2 == ax[k].st2 * ax[k].n) {
                prev.n *= ax[k].n, prev.st = ax[k].st, prev.ost = ax[k].ost, prev.st2 = ax[k].st2;
                continue;
            }
        }
        ax[m++] = ax[k];
    }
    return m;
}

// The canonical walk: out[o*oso + i*osi] = f_r a[o*so + r*sr + i*si] over (O, R, I).
struct Canon {
    int64_t O = 1, R = 1, I = 1, so = 0, sr = 1, si = 1;
    int64_t oso = 1, osi = 1;
};
enum Walk { kWalkNone, kWalkRow, kWalkColumn };
// Fills `c` from a merged axis list of the form [kept] reduced [kept] with exactly one reduced group, and says which walk has
// its unit stride: ROW (I = 1, sr = 1) or COLUMN (I > 1, si = 1).  kWalkNone: another form, or no unit stride.
inline Walk canonical(const Ax *ax, int n, Canon *c) {
    int red = -1;
    for (int k = 0; k < n; ++k)
        if (ax[k].red) {
            if (red >= 0) return kWalkNone;
            red = k;
        }
    if (red < 0 || red > 1 || n - red - 1 > 1) return kWalkNone;
    *c = Canon();
    c->R = ax[red].n, c->sr = ax[red].st;
    if (red == 1) c->O = ax[0].n, c->so = ax[0].st, c->oso = ax[0].ost;
    if (red + 1 < n) c->I = ax[red + 1].n, c->si = ax[red + 1].st, c->osi = ax[red + 1].ost;
    return c->I == 1 && c->sr == 1 ? kWalkRow : c->I > 1 && c->si == 1 ? kWalkColumn : kWalkNone;
}

// ROW, short rows: a row of R elements is `loads` loads (its 16-byte vectors, then the R % W tail elements one per lane), and
// a row of at most 64 loads gets a segment of 4, 16 or 64 lanes.  0: a longer row.
inline int64_t row_loads(int64_t R, int64_t W) { return R / W + R % W; }
inline int segment_lanes(int64_t loads) { return loads <= 4 ? 4 : loads <= 16 ? 16 : loads <= 64 ? 64 : 0; }
// Rows copied whole (take, scatter): the 8, 16, 32 or 64 lanes of a wave that share a row of `per_row` lane steps.
inline int segment_for(int64_t per_row) { return per_row <= 8 ? 8 : per_row <= 16 ? 16 : per_row <= 32 ? 32 : 64; }

// Cutting R into C chunks of CL when a launch of `lanes` lanes falls short of kTargetLanes: as many chunks as make up for it,
// none shorter than `least`, CL a multiple of `unit`; and, whatever the lanes, none longer than `max_chunk` (0: no limit).
// CL = 0: R stays whole, and what the chunk length then is stays with the caller.  The length depends on the shape alone.
struct Split { int64_t C, CL; };
inline Split split_chunks(int64_t lanes, int64_t R, int64_t unit, int64_t least, int64_t max_chunk) {
    int64_t want = lanes < kTargetLanes ? std::min(ceil_div(kTargetLanes, lanes), ceil_div(R, least)) : 1;
    if (max_chunk) want = std::max(want, ceil_div(R, max_chunk));
    if (want <= 1) return Split{1, 0};
    const int64_t CL = ceil_div(ceil_div(R, want), unit) * unit;
    return Split{ceil_div(R, CL), CL};
}
// ... of a long row (or a stream): whole units -- a wave's guard-free step, 4 * 64 * W elements.
inline Split split_row(int64_t lanes, int64_t R, int64_t unit, int64_t max_chunk = 0) { return split_chunks(lanes, R, unit, unit, max_chunk); }
// ... of columns: multiples of the 4 rows in flight, at least 16 rows per chunk.
inline Split split_column(int64_t lanes, int64_t R, int64_t max_chunk = 0) { return split_chunks(lanes, R, 4, 16, max_chunk); }

// Every kernel of the three families loops over its tasks grid-stride, so its grid can be capped: HIP counts a grid in
// work-items in 32 bits, and a launch of more than 2^32 / 256 workgroups would fail.  2^20 workgroups (2^28 work-items) is
// above what any shape of the rate tables needs, so the loops run once per lane there.  Each family reads a variable of its
// own, SMHIP_<FAMILY>_GRID_CAP=<workgroups>, that lowers the cap (the tests run every loop at small sizes with it).
struct GridCap {
    unsigned cap;
    explicit GridCap(const char *text) {  // the variable's text, or null
        const long long v = text && *text ? atoll(text) : 0;
        cap = v > 0 && v < (1 << 20) ? (unsigned)v : 1u << 20;
    }
    unsigned capped(int64_t blocks) const { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(blocks, cap)); }
    unsigned blocks_for(int64_t waves) const { return capped(ceil_div(waves, kBlock / 64)); }
};

// The argument checks every entry point makes, in the order they are made: dtype and ndim, then the family's own on its
// mask or axis, then shape and strides.  `who` names the entry point in the message for smhip_last_error().
inline int check_dtype_ndim(const char *who, int dtype, int ndim) {
    if (!valid_dtype(dtype)) return fail(SMHIP_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    if (ndim < 1 || ndim > SMHIP_MAX_NDIM) return fail(SMHIP_ERR_INVALID, "%s: ndim %d outside 1..%d", who, ndim, SMHIP_MAX_NDIM);
    return SMHIP_OK;
}
inline int check_axis(const char *who, int axis, int ndim) {
    if (axis < 0 || axis >= ndim) return fail(SMHIP_ERR_INVALID, "%s: axis %d outside 0..%d", who, axis, ndim - 1);
    return SMHIP_OK;
}
inline int check_extents(const char *who, const int64_t *shape, const int64_t *strides, int ndim) {
    if (!shape || !strides) return fail(SMHIP_ERR_INVALID, "%s: null shape/strides", who);
    for (int d = 0; d < ndim; ++d)
        if (shape[d] < 0 || strides[d] < 0) return fail(SMHIP_ERR_INVALID, "%s: negative extent or stride at dim %d", who, d);
    return SMHIP_OK;
}

// A buffer from the pool, handed back when its owner ends or takes another.  The pool is stream-ordered: that is safe while
// the kernels that use the buffer are still queued.
class Pooled {
public:
    Pooled() = default;
    Pooled(const Pooled &) = delete;
    Pooled &operator=(const Pooled &) = delete;
    ~Pooled() { release(); }
    int take(size_t bytes, void **p) {
        release();
        if (int rc = smhip_alloc(&p_, bytes)) return rc;
        *p = p_;
        return SMHIP_OK;
    }
    // The dense row-major copy of a view (smhip_copy_strided's kernels), queued on `s`.
    int dense_copy(int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, hipStream_t s, const void **copy) {
        int64_t dense[SMHIP_MAX_NDIM];
        const int64_t total = dense_strides(shape, ndim, dense);
        void *p;
        if (int rc = take((size_t)total * dtype_size(dtype), &p)) return rc;
        *copy = p;
        return launch_copy_strided(dtype, a, strides, p, dense, shape, ndim, s);
    }
private:
    void release() {
        if (p_) smhip_free(p_), p_ = nullptr;
    }
    void *p_ = nullptr;
};

}  // namespace axis_plan
}  // namespace smhip
