// axis_plan.h -- the host-side merging of axes that the planners of reduce_axis.hip (axis reductions) and argreduce_axis.hip
// (argmax / argmin) share: a view's axes ordered by stride and joined where memory, and the dense result, run on without a gap.
#pragma once

#include <stdint.h>

#include <algorithm>

#include "smhip.h"

namespace smhip {
namespace axis_plan {

struct Ax { int64_t n, st, ost; bool red; };

// Axes of extent > 1, ordered by stride (largest first, ties in index order), neighbours merged where memory -- and for kept
// axes the dense result -- runs on without a gap.  Returns the count.
inline int merge_axes(const int64_t *shape, const int64_t *strides, int ndim, uint32_t mask, bool by_index, Ax *ax) {
    int64_t ost[SMHIP_MAX_NDIM];
    int64_t acc = 1;
    for (int d = ndim - 1; d >= 0; --d) {
        ost[d] = 0;
        if (!(mask >> d & 1)) ost[d] = acc, acc *= shape[d];
    }
    int n = 0;
    for (int d = 0; d < ndim; ++d)
        if (shape[d] > 1) ax[n++] = Ax{shape[d], strides[d], ost[d], (mask >> d & 1) != 0};
    if (!by_index) std::stable_sort(ax, ax + n, [](const Ax &x, const Ax &y) { return x.st > y.st; });
    int m = 0;
    for (int k = 0; k < n; ++k) {
        if (m > 0) {
            Ax &prev = ax[m - 1];
            if (prev.red == ax[k].red && prev.st == ax[k].st * ax[k].n && (prev.red || prev.ost == ax[k].ost * ax[k].n)) {
                prev.n *= ax[k].n, prev.st = ax[k].st, prev.ost = ax[k].ost;
                continue;
            }
        }
        ax[m++] = ax[k];
    }
    return m;
}

inline bool row_major(const int64_t *shape, const int64_t *strides, int ndim) {
    int64_t acc = 1;
    for (int d = ndim - 1; d >= 0; --d) {
        if (shape[d] != 1 && strides[d] != acc) return false;
        acc *= shape[d];
    }
    return true;
}

}  // namespace axis_plan
}  // namespace smhip
