// sort_axis.hip -- the order along one axis: the sorted values and / or the permutation that sorts them (smhip_sort_axis).
//
// The reference has nothing of the kind.  np.sort / np.argsort with kind="stable" is the contract (smhip.h has it in full): the
// line along the axis is sorted as (element, position) pairs,
//     ASCENDING   a number before a NaN; the smaller value first (-0 == +0); among equal values, or two NaNs, the smaller position;
//     DESCENDING  a NaN before a number; the larger value first; ties as above.
// That is a strict total order on the pairs of a line, so the result is unique: whatever network, tiling or merge partition
// produces it, the bits are the same.  The pairs travel as (the element's own bits, 32-bit position) and are compared by
// `before()` below; nothing is rebuilt from a key, so the values written are the operand's (which zero, which NaN).
//
// Planner (host only; smhip_sort_plan reports it), with axis_plan.h's merging.  The kernels sort ROWS: O lines of R contiguous
// elements, line o at a + o*so, results as dense rows [O][R].
//   input    read in place when the merged view is [kept] R with R at unit stride (a dense array sorted along its last axis,
//            but also A.T sorted along axis 0); otherwise copied into a pooled buffer whose last axis is the sort axis
//            (smhip_copy_strided's kernels with permuted destination strides).
//   output   written in place when rows [O][R] in the order the lines were taken ARE the dense row-major result; otherwise
//            written to pooled rows and scattered to the result by the same strided copy (values, and positions as int64).
//   ROW      R <= K (K = kTile elements): a line is sorted in LDS by a bitonic network of N = 2^ceil(log2 R) slots.  Each merge
//            stage opens with the mirrored step (i against i ^ (2^s - 1)) and every comparator puts the earlier pair at the
//            lower slot, so slots >= R behave as pairs that come after everything and are simply never touched: no sentinels.
//            A workgroup takes several short lines at once (as many as keep its 256 lanes busy and the grid wide).
//   MERGE    R > K: launch 1 sorts tiles of K into pooled pairs; then ceil(log2(tiles)) passes merge neighbouring runs between two
//            pooled buffers.  A workgroup produces kSlice consecutive outputs of one run pair: two lanes find the slice's ends on
//            the merge path (binary search over the pair order, in global memory), the slice's two inputs are brought into LDS,
//            and every element finds its place by counting the other side's elements that come before it.  An odd run left over
//            is a merge with an empty partner.  The last pass writes the results themselves.  The operand is read by launch 1
//            only, so sorting in place is safe.
// Every kernel loops over its tasks grid-stride under a capped grid (SMHIP_SORT_GRID_CAP).  No atomics.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "internal.h"

namespace smhip {
namespace {

using namespace axis_plan;  // kBlock, Canon, GridCap, Pooled and the planner's rules

constexpr int kTile = 4096;   // K: elements of a tile; (sizeof(T) + 4) * K = 32 / 48 KiB of LDS, so three workgroups fit the CU's 160 KiB
constexpr int kSlice = 2048;  // outputs of a merge task; divides kTile, so a slice never straddles two run pairs
constexpr int64_t kMaxAxis = (int64_t)1 << 31;  // positions travel as 32 bits

// Does pair (av, ar) come before pair (bv, br)?  ar != br within a line, so exactly one of before(a, b), before(b, a) holds.
template <typename T> __device__ __forceinline__ bool before(bool desc, T av, uint32_t ar, T bv, uint32_t br) {
    const bool first = ar < br, lt = desc ? bv < av : av < bv;
    if constexpr (std::is_floating_point<T>::value) {
        const bool an = av != av, bn = bv != bv;
        return (desc ? an && !bn : bn && !an) || lt || ((av == bv || (an && bn)) && first);
    } else {
        return lt || (av == bv && first);
    }
}

// ---- tiles: task t sorts `per` lines of R <= K (tiles == 1), or tile t % tiles of line t / tiles (per == 1), in N-slot
// segments of LDS (N = 1 << logn, a power of two >= the segment's length).  Pairs go to (pv, pr) -- the merge passes' input --
// or, when pr is null, to the results (val / idx, either may be null); all as rows of R.
template <typename T>
__global__ __launch_bounds__(kBlock) void sort_tiles_kernel(const T *__restrict__ a, int64_t lines, int64_t so, int64_t R, int64_t tiles, int per, int logn,
                                                            int desc, T *pv, uint32_t *__restrict__ pr, T *val, int64_t *__restrict__ idx) {
    __shared__ T v[kTile];
    __shared__ uint32_t r[kTile];
    const int N = 1 << logn;
    const int64_t tasks = tiles > 1 ? lines * tiles : (lines + per - 1) / per;
    for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {  // workgroup-uniform
        int64_t line0 = task * per, p0 = 0;
        int live = (int)std::min<int64_t>(per, lines - line0), len = (int)R;  // segments in use, and the length of each
        if (tiles > 1) {
            line0 = task / tiles, p0 = (task - line0 * tiles) * kTile;
            live = 1, len = (int)std::min<int64_t>(kTile, R - p0);
        }
        const int slots = live << logn;
        for (int s = threadIdx.x; s < slots; s += kBlock) {
            const int seg = s >> logn, l = s & (N - 1);
            if (l < len) v[s] = a[(line0 + seg) * so + p0 + l], r[s] = (uint32_t)(p0 + l);
        }
        __syncthreads();
        for (int k = 2; k <= N; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                for (int c = threadIdx.x; c < slots >> 1; c += kBlock) {
                    const int low = c & (j - 1), i = ((c - low) << 1) | low;  // bit j of i is clear
                    const int p = j == k >> 1 ? i ^ (k - 1) : i | j;         // the stage's first step is mirrored
                    if ((p & (N - 1)) < len) {
                        const T vi = v[i], vp = v[p];
                        const uint32_t ri = r[i], rp = r[p];
                        if (before(desc != 0, vp, rp, vi, ri)) v[i] = vp, r[i] = rp, v[p] = vi, r[p] = ri;
                    }
                }
                __syncthreads();
            }
        for (int s = threadIdx.x; s < slots; s += kBlock) {
            const int seg = s >> logn, l = s & (N - 1);
            if (l < len) {
                const int64_t at = (line0 + seg) * R + p0 + l;
                if (pr) pv[at] = v[s], pr[at] = r[s];
                else {
                    if (val) val[at] = v[s];
                    if (idx) idx[at] = (int64_t)r[s];
                }
            }
        }
        __syncthreads();  // the next task reuses the tile
    }
}

// How many of the first d pairs of merge(A, B) come from A (the merge path's crossing of diagonal d).
template <typename T>
__device__ int64_t merge_path(bool desc, const T *av, const uint32_t *ar, int64_t na, const T *bv, const uint32_t *br, int64_t nb, int64_t d) {
    int64_t lo = std::max<int64_t>(0, d - nb), hi = std::min(d, na);
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (before(desc, av[mid], ar[mid], bv[d - 1 - mid], br[d - 1 - mid])) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ---- a merge pass: line `row` of (iv, ir) holds sorted runs of L (the last one shorter); runs 2m and 2m + 1 are merged.  A task
// is kSlice consecutive outputs of a line.  Results to (ov, orr) as pairs, or, when orr is null, to val / idx (either may be null).
template <typename T>
__global__ __launch_bounds__(kBlock) void merge_pass_kernel(const T *__restrict__ iv, const uint32_t *__restrict__ ir, int64_t lines, int64_t R, int64_t L,
                                                            int desc_i, T *__restrict__ ov, uint32_t *__restrict__ orr, T *__restrict__ val,
                                                            int64_t *__restrict__ idx) {
    __shared__ T v[kSlice];
    __shared__ uint32_t r[kSlice];
    __shared__ int64_t ends[2];
    const bool desc = desc_i != 0;
    const int64_t slices = (R + kSlice - 1) / kSlice, tasks = lines * slices;
    for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {  // workgroup-uniform
        const int64_t row = task / slices, o0 = (task - row * slices) * kSlice, o1 = std::min(R, o0 + kSlice);
        const int64_t base = o0 / (2 * L) * (2 * L), na = std::min(L, R - base), nb = std::min(L, R - base - na);  // nb >= 0
        const T *av = iv + row * R + base, *bv = av + na;
        const uint32_t *ar = ir + row * R + base, *br = ar + na;
        if ((threadIdx.x & 63) == 0 && threadIdx.x < 128) {  // lane 0 of waves 0 and 1: the slice's two ends
            const int e = threadIdx.x >> 6;
            ends[e] = merge_path(desc, av, ar, na, bv, br, nb, (e ? o1 : o0) - base);
        }
        __syncthreads();
        const int64_t a0 = ends[0], a1 = ends[1], b0 = o0 - base - a0;
        const int ca = (int)(a1 - a0), cb = (int)(o1 - o0) - ca;  // ca + cb <= kSlice
        for (int e = threadIdx.x; e < ca + cb; e += kBlock) {
            const int64_t at = e < ca ? a0 + e : na + b0 + (e - ca);  // from av: B follows A in memory
            v[e] = av[at], r[e] = ar[at];
        }
        __syncthreads();
        for (int e = threadIdx.x; e < ca + cb; e += kBlock) {
            const T x = v[e];
            const uint32_t xr = r[e];
            // how many of the other side come before x: that side is sorted, so the predicate is monotone
            int lo = e < ca ? ca : 0, hi = e < ca ? ca + cb : ca;
            const int other0 = lo;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (before(desc, v[mid], r[mid], x, xr)) lo = mid + 1;
                else hi = mid;
            }
            const int64_t at = row * R + o0 + (e < ca ? e : e - ca) + (lo - other0);
            if (orr) ov[at] = x, orr[at] = xr;
            else {
                if (val) val[at] = x;
                if (idx) idx[at] = (int64_t)xr;
            }
        }
        __syncthreads();  // the next task reuses the slice and `ends`
    }
}

// ------------------------------------------------------------------------------------------------------ the planner
struct Plan {
    int route = SMHIP_SORT_ROUTE_NONE;
    bool stage_in = false, stage_out = false;
    int64_t O = 1, R = 1, I = 1;  // ori3
    int64_t lines = 0, so = 0;    // the rows the kernels sort: line o at in + o*so
    int64_t total = 0;
    int64_t tiles = 1, passes = 0;
    int per = 1, logn = 0;
    int64_t stage[SMHIP_MAX_NDIM];  // where element [idx] of the result stands in the rows [lines][R], as strides over `shape`
    int64_t chunk() const { return tiles > 1 ? kTile : R; }
    int launches() const {  // of a call that asks for both outputs, not in place
        if (route == SMHIP_SORT_ROUTE_NONE) return 0;
        if (route == SMHIP_SORT_ROUTE_COPYONLY) return 2;
        return (stage_in ? 1 : 0) + 1 + (int)passes + (stage_out ? 2 : 0);
    }
    int code() const { return route | (tiles > 1 ? SMHIP_SORT_MERGE : 0) | (stage_in || stage_out ? SMHIP_SORT_COPY : 0); }
};

void make_plan(const int64_t *shape, const int64_t *strides, int ndim, int axis, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    int64_t before_n = 1, after_n = 1;
    bool zero_stride = false;
    for (int d = 0; d < ndim; ++d) {
        if (d < axis) before_n *= shape[d];
        if (d > axis) after_n *= shape[d];
        if (shape[d] > 1 && strides[d] == 0) zero_stride = true;
    }
    p.R = shape[axis], p.O = before_n, p.I = after_n, p.total = before_n * after_n * p.R;
    if (p.total == 0) return;
    if (p.R == 1) {
        p.route = SMHIP_SORT_ROUTE_COPYONLY;
        return;
    }
    p.route = SMHIP_SORT_ROUTE_ROW;
    Ax ax[SMHIP_MAX_NDIM];
    const int n = merge_axes(shape, strides, ndim, 1u << axis, false, ax);
    Canon c;
    if (!zero_stride && canonical(ax, n, &c) == kWalkRow) {  // read in place: every kept stride is a multiple of so
        p.O = c.O, p.I = 1, p.lines = c.O, p.so = c.so;
        for (int d = 0; d < ndim; ++d) p.stage[d] = shape[d] == 1 ? 0 : d == axis ? 1 : strides[d] / c.so * p.R;
    } else {  // staged: the kept axes in index order, then the sort axis
        p.stage_in = true, p.lines = before_n * after_n, p.so = p.R;
        int64_t acc = p.R;
        for (int d = ndim - 1; d >= 0; --d) {
            if (d == axis) p.stage[d] = 1;
            else p.stage[d] = shape[d] == 1 ? 0 : acc, acc *= shape[d];
        }
    }
    p.stage_out = !row_major(shape, p.stage, ndim);
    if (p.R > kTile) {
        p.tiles = ceil_div(p.R, kTile), p.per = 1, p.logn = 12;
        for (int64_t runs = p.tiles; runs > 1; runs = ceil_div(runs, 2)) ++p.passes;
    } else {
        while (((int64_t)1 << p.logn) < p.R) ++p.logn;
        // lines per workgroup: at least 512 slots (a comparator per lane), at most a tile, and few enough for a wide grid
        const int64_t n2 = (int64_t)1 << p.logn, least = std::max<int64_t>(1, 512 / n2), most = kTile / n2;
        p.per = (int)std::min(most, std::max(least, ceil_div(p.lines, 2048)));
    }
}
static_assert(kTile == 1 << 12 && kTile % kSlice == 0, "make_plan's logn and the merge pass's slices");

// ------------------------------------------------------------------------------------------------------ launching
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_SORT_GRID_CAP")); return g; }  // the cap of every launch here, read once

template <typename T>
int run_rows(const Plan &p, int desc, const T *in, T *val, int64_t *idx, hipStream_t s) {
    if (p.tiles == 1) {
        hipLaunchKernelGGL((sort_tiles_kernel<T>), dim3(grid_cap().capped(ceil_div(p.lines, p.per))), dim3(kBlock), 0, s, in, p.lines, p.so, p.R, (int64_t)1,
                           p.per, p.logn, desc, (T *)nullptr, (uint32_t *)nullptr, val, idx);
        SMHIP_LAUNCH_CHECK("sort_axis");
        return SMHIP_OK;
    }
    // two buffers of pairs, each the values then the positions
    Pooled pool;
    void *raw;
    const size_t n = (size_t)p.lines * (size_t)p.R, half = n * (sizeof(T) + sizeof(uint32_t));
    if (int rc = pool.take(2 * half, &raw)) return rc;
    T *bv[2] = {static_cast<T *>(raw), reinterpret_cast<T *>(static_cast<char *>(raw) + half)};
    uint32_t *br[2] = {reinterpret_cast<uint32_t *>(bv[0] + n), reinterpret_cast<uint32_t *>(bv[1] + n)};
    hipLaunchKernelGGL((sort_tiles_kernel<T>), dim3(grid_cap().capped(p.lines * p.tiles)), dim3(kBlock), 0, s, in, p.lines, p.so, p.R, p.tiles, 1, p.logn, desc,
                       bv[0], br[0], (T *)nullptr, (int64_t *)nullptr);
    SMHIP_LAUNCH_CHECK("sort_axis tiles");
    const unsigned blocks = grid_cap().capped(p.lines * ceil_div(p.R, kSlice));
    int64_t L = kTile;
    for (int64_t pass = 0; pass < p.passes; ++pass, L *= 2) {
        const int from = (int)(pass & 1), to = from ^ 1;
        const bool last = pass + 1 == p.passes;
        hipLaunchKernelGGL((merge_pass_kernel<T>), dim3(blocks), dim3(kBlock), 0, s, bv[from], br[from], p.lines, p.R, L, desc, last ? (T *)nullptr : bv[to],
                           last ? (uint32_t *)nullptr : br[to], last ? val : (T *)nullptr, last ? idx : (int64_t *)nullptr);
        SMHIP_LAUNCH_CHECK("sort_axis merge");
    }
    return SMHIP_OK;
}

template <typename T>
int run_plan(const Plan &p, int desc, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, void *values_out, int64_t *index_out,
             hipStream_t s) {
    int64_t dense[SMHIP_MAX_NDIM];
    dense_strides(shape, ndim, dense);
    Pooled in_pool, val_pool, idx_pool;
    const T *in = static_cast<const T *>(a);
    if (p.stage_in) {
        void *buf;
        if (int rc = in_pool.take((size_t)p.total * sizeof(T), &buf)) return rc;
        if (int rc = launch_copy_strided(dtype, a, strides, buf, p.stage, shape, ndim, s)) return rc;
        in = static_cast<const T *>(buf);
    }
    T *val = static_cast<T *>(values_out);
    int64_t *idx = index_out;
    if (p.stage_out) {
        void *buf;
        if (values_out) {
            if (int rc = val_pool.take((size_t)p.total * sizeof(T), &buf)) return rc;
            val = static_cast<T *>(buf);
        }
        if (index_out) {
            if (int rc = idx_pool.take((size_t)p.total * sizeof(int64_t), &buf)) return rc;
            idx = static_cast<int64_t *>(buf);
        }
    }
    if (int rc = run_rows<T>(p, desc, in, val, idx, s)) return rc;
    if (p.stage_out) {
        if (values_out)
            if (int rc = launch_copy_strided(dtype, val, p.stage, values_out, dense, shape, ndim, s)) return rc;
        if (index_out)
            if (int rc = launch_copy_strided(SMHIP_I64, idx, p.stage, index_out, dense, shape, ndim, s)) return rc;
    }
    return SMHIP_OK;
}

// Validation: everything that can be said without a device or a pointer.
int sort_axis_check(const char *who, int order, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis) {
    if (order != SMHIP_SORT_ASCENDING && order != SMHIP_SORT_DESCENDING) return fail(SMHIP_ERR_INVALID, "%s: bad order %d", who, order);
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (int rc = check_axis(who, axis, ndim)) return rc;
    if (int rc = check_extents(who, shape, strides, ndim)) return rc;
    if (shape[axis] >= kMaxAxis) return fail(SMHIP_ERR_UNSUPPORTED, "%s: an axis of %lld elements (positions are 32 bits wide: below 2^31)", who, (long long)shape[axis]);
    return SMHIP_OK;
}

}  // namespace

void sort_axis_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, int *route, int *launches, int64_t *ori3, int64_t *chunk) {
    (void)dtype;  // K is the same for 4- and 8-byte elements
    Plan pl;
    make_plan(shape, strides, ndim, axis, &pl);
    if (route) *route = pl.code();
    if (launches) *launches = pl.launches();
    if (ori3) ori3[0] = pl.O, ori3[1] = pl.R, ori3[2] = pl.I;
    if (chunk) *chunk = pl.chunk();
}

int launch_sort_axis(int order, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, void *values_out,
                     int64_t *index_out, hipStream_t s) {
    Plan pl;
    make_plan(shape, strides, ndim, axis, &pl);
    if (pl.route == SMHIP_SORT_ROUTE_NONE) return SMHIP_OK;
    if (pl.route == SMHIP_SORT_ROUTE_COPYONLY) {
        int64_t dense[SMHIP_MAX_NDIM];
        axis_plan::dense_strides(shape, ndim, dense);
        if (values_out && values_out != a)
            if (int rc = launch_copy_strided(dtype, a, strides, values_out, dense, shape, ndim, s)) return rc;
        const int64_t zero = 0;
        return index_out ? launch_fill(SMHIP_I64, index_out, &zero, (size_t)pl.total, s) : SMHIP_OK;
    }
    const int desc = order == SMHIP_SORT_DESCENDING;
    switch (dtype) {
        case SMHIP_F32: return run_plan<float>(pl, desc, dtype, a, shape, strides, ndim, values_out, index_out, s);
        case SMHIP_F64: return run_plan<double>(pl, desc, dtype, a, shape, strides, ndim, values_out, index_out, s);
        case SMHIP_I32: return run_plan<int32_t>(pl, desc, dtype, a, shape, strides, ndim, values_out, index_out, s);
        case SMHIP_I64: return run_plan<int64_t>(pl, desc, dtype, a, shape, strides, ndim, values_out, index_out, s);
    }
    return fail(SMHIP_ERR_INVALID, "sort_axis: bad dtype %d", dtype);
}

}  // namespace smhip

using namespace smhip;

int smhip_sort_axis(int order, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, void *values_out,
                    int64_t *index_out) {
    if (int rc = sort_axis_check("sort_axis", order, dtype, shape, strides, ndim, axis)) return rc;
    const int64_t n = element_count(shape, ndim);
    const bool dense = axis_plan::row_major(shape, strides, ndim);
    if (n == 0) return SMHIP_OK;
    if (!a) return fail(SMHIP_ERR_INVALID, "sort_axis: null operand");
    if (!values_out && !index_out) return fail(SMHIP_ERR_INVALID, "sort_axis: neither values_out nor index_out is given");
    const size_t esz = dtype_size(dtype);
    const Span sa{a, span_bytes(shape, strides, ndim, esz)}, sv{values_out, values_out ? (size_t)n * esz : 0},
        si{index_out, index_out ? (size_t)n * sizeof(int64_t) : 0};
    // in place is the one overlap a sort can take: the operand is read whole (a line, or launch 1 of a merge) before a result is written
    if (!(values_out == a && dense) && spans_overlap(sv, sa))
        return fail(SMHIP_ERR_INVALID, "sort_axis: values_out overlaps the operand (only values_out == a with a dense operand is allowed)");
    if (spans_overlap(si, sa) || spans_overlap(si, sv)) return fail(SMHIP_ERR_INVALID, "sort_axis: index_out overlaps the operand or values_out");
    SMHIP_ACQUIRE(s);  // undeclared spans (pooled staging, the merge's pairs): ordered behind everything, recorded tiny operators flushed first
    return launch_sort_axis(order, dtype, a, shape, strides, ndim, axis, values_out, index_out, s);
}

int smhip_sort_plan(int order, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, int *route, int *launches, int64_t *ori3,
                    int64_t *chunk) {
    if (int rc = sort_axis_check("sort_plan", order, dtype, shape, strides, ndim, axis)) return rc;
    sort_axis_plan(dtype, shape, strides, ndim, axis, route, launches, ori3, chunk);
    return SMHIP_OK;
}
