// scatter_axis.hip -- writing by position along one axis: np.put_along_axis / np.put and np.add.at (smhip_scatter_axis).
//
// The reference has nothing of the kind; numpy is the contract (smhip.h has it in full).  For an axis of R elements and J
// entries per line, walked in ascending j:
//     PUT   out[..., p, ...]  = values[..., j, ...]       p = pick(idx[..., j, ...]); among equal p the largest j wins
//     ADD   out[..., p, ...] += values[..., j, ...]       one by one in ascending j, f32 accumulated in fp64 and rounded once
// A scatter with duplicate positions needs a rule for who wins, and the rule above is fixed by the data alone: the result is
// unique, the same on every run, stream and grid.  There are NO ATOMICS in this file and no two lanes ever write one address
// (the constant-1 flag store apart): the design is an inverted index whose lists stand in a fixed order.
//
// NO ADDRESS OUTSIDE `out` IS EVER FORMED.  pick() (index_mode.hip.h, shared with take_axis.hip and count.hip)
// turns the 64-bit index into a position in [0, R - 1] BEFORE anything is multiplied by a stride; under CHECKED an index outside
// [-R, R) is dropped -- it writes and adds nothing -- and any lane that meets one stores the constant 1 to *bad_out.
//
// Planner (host only; smhip_scatter_plan reports it), with axis_plan.h's merging over three stride sets: `out` is dense, so the
// walk is always out[o*oso + p*sor + i*osi] over [O] J [I]; idx and values must run on over the merged O and I groups, and one
// that does not is copied dense first through Pooled (SMHIP_SCATTER_COPY).
//   unique (the caller's promise, or J <= 1): one launch.
//     DIRECT       one entry per lane, lanes along the unit stride of the walk: idx and values are read coalesced, the store
//                  (ADD: the load and the store) is the element-granular side.
//     ROWS         idx constant along rows of I >= one vector that are contiguous in values and out: whole rows move as in
//                  take_rows_kernel (a lane segment per row, the index read once per row, 4 rows in flight per lane, 16-byte
//                  accesses when pointers and pitches allow).
//   no promise: normalise, sort, combine.
//     normalise    pick() over the index array IN ITS OWN un-broadcast shape (a 1-D ids is normalised and sorted once, not once
//                  per row) into pooled int64 keys, lines [O'][I'] of J; a dropped entry gets the key R, which sorts last.
//     sort         launch_sort_axis (ascending, stable, both outputs) along J: the sorted keys and `order`, the original j,
//                  ascending within equal keys.
//     SORTED       a lane per sorted entry and destination: PUT -- the LAST entry of a run of equal keys writes values[order];
//                  ADD -- the FIRST entry of a run loads out[p], adds the run's values in order, stores once.
//     SORTED_ROWS  the same with a lane segment per entry and its row (16-byte loads when possible).
//   The combine kernels walk the sorted ENTRIES, so their cost follows J, not R.  One destination named by very many entries is
//   summed by one lane (or segment): that is the price of the fixed order, and DESIGN.md states it.
// PUT moves 4- or 8-byte words; ADD computes in the type (integers as unsigned words: wrapping is then defined).
// Every kernel loops over its tasks grid-stride under one capped grid (SMHIP_SCATTER_GRID_CAP).
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "index_mode.hip.h"
#include "internal.h"

namespace smhip {
namespace {

using namespace axis_plan;  // kBlock, Ax, GridCap, Pooled and the planner's rules

constexpr int kRowsInFlightPerLane = 4;  // ROWS: rows a lane has loads outstanding for
constexpr int64_t kMaxSorted = (int64_t)1 << 31;  // the sort's limit on an axis

// q / d and the remainder, through 32 bits when both fit.
__device__ __forceinline__ int64_t div_small(int64_t q, int64_t d, int64_t *rem) {
    if (((uint64_t)(q | d) >> 32) == 0) {
        const uint32_t k = (uint32_t)q / (uint32_t)d;
        *rem = (int64_t)((uint32_t)q - k * (uint32_t)d);
        return (int64_t)k;
    }
    const int64_t k = q / d;
    *rem = q - k * d;
    return k;
}

// What ADD accumulates in: fp64 for f32 (the family rule of smhip_reduce_axes), the type itself otherwise.
template <typename T> struct AccOf { using type = T; };
template <> struct AccOf<float> { using type = double; };

// One lane's share of a row: a 16-byte vector of T, or one element.
template <typename T, bool Vec> struct alignas(Vec ? 16 : sizeof(T)) Pack { T v[Vec ? 16 / sizeof(T) : 1]; };

// ------------------------------------------------------------------------------------------------------ DIRECT
// Entry e of the walk [O][J][I]: idx[o*sio + j*sij + i*sii], values[o*svo + j*svj + i*svi] -> out[o*oso + p*sor + i*osi].
struct Walk3 {
    int64_t O, J, I, R, sio, sij, sii, svo, svj, svi, oso, sor, osi;
};

template <typename T, bool Add, int Mode>
__global__ __launch_bounds__(kBlock) void scatter_direct_kernel(T *__restrict__ out, const int64_t *__restrict__ idx, const T *__restrict__ val, Walk3 g,
                                                                int64_t *bad_out) {
    using A = typename AccOf<T>::type;
    bool bad = false;
    const int64_t total = g.O * g.J * g.I, step = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += step) {
        int64_t i, j;
        const int64_t oj = div_small(e, g.I, &i);
        const int64_t o = div_small(oj, g.J, &j);
        bool b = false;
        const int64_t p = pick<Mode>(idx[o * g.sio + j * g.sij + i * g.sii], g.R, b);
        bad |= b;
        if (b) continue;  // dropped
        const T v = val[o * g.svo + j * g.svj + i * g.svi];
        T *dst = out + o * g.oso + p * g.sor + i * g.osi;
        if constexpr (Add) *dst = (T)((A)*dst + (A)v);
        else *dst = v;
    }
    report_bad<Mode>(bad, bad_out);
}

// ------------------------------------------------------------------------------------------------------ ROWS
struct RowsArgs {
    int64_t O, J, I, R, sio, sij, svo, svj, oso, sor;
    int seg;  // lanes that share a row: 8, 16, 32 or 64
};

// Vec: every row of values and of out starts on a 16-byte boundary and I is a whole number of vectors.
template <typename T, bool Add, int Mode, bool Vec>
__global__ __launch_bounds__(kBlock) void scatter_rows_kernel(T *__restrict__ out, const int64_t *__restrict__ idx, const T *__restrict__ val, RowsArgs g,
                                                              int64_t *bad_out) {
    using A = typename AccOf<T>::type;
    using V = Pack<T, Vec>;
    constexpr int W = Vec ? 16 / (int)sizeof(T) : 1;
    constexpr int F = kRowsInFlightPerLane;
    const int lane = threadIdx.x & 63, segs = 64 / g.seg, sg = lane / g.seg, sl = lane - sg * g.seg;
    const int64_t rows = g.O * g.J, per_task = (int64_t)segs * F, piece = (int64_t)g.seg * W;
    const int64_t pieces = (g.I + piece - 1) / piece, tasks = (rows + per_task - 1) / per_task * pieces;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * (kBlock / 64);
    bool bad = false;
    for (int64_t task = wave; task < tasks; task += waves) {  // wave-uniform
        int64_t pc;
        const int64_t rg = div_small(task, pieces, &pc);
        const int64_t col = pc * piece + (int64_t)sl * W;
        const T *src[F];
        T *dst[F];
        V v[F];
#pragma unroll
        for (int k = 0; k < F; ++k) {
            const int64_t row = rg * per_task + (int64_t)k * segs + sg;
            src[k] = nullptr;
            if (row < rows && col < g.I) {
                int64_t o = 0, j = row;
                if (g.O > 1) o = div_small(row, g.J, &j);
                bool b = false;
                const int64_t p = pick<Mode>(idx[o * g.sio + j * g.sij], g.R, b);
                bad |= b;
                if (!b) {
                    src[k] = val + o * g.svo + j * g.svj + col;
                    dst[k] = out + o * g.oso + p * g.sor + col;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < F; ++k)
            if (src[k]) v[k] = *reinterpret_cast<const V *>(src[k]);
        if constexpr (Add) {
            V d[F];
#pragma unroll
            for (int k = 0; k < F; ++k)
                if (src[k]) d[k] = *reinterpret_cast<const V *>(dst[k]);
#pragma unroll
            for (int k = 0; k < F; ++k)
                if (src[k]) {
#pragma unroll
                    for (int w = 0; w < W; ++w) v[k].v[w] = (T)((A)d[k].v[w] + (A)v[k].v[w]);
                }
        }
#pragma unroll
        for (int k = 0; k < F; ++k)
            if (src[k]) *reinterpret_cast<V *>(dst[k]) = v[k];
    }
    report_bad<Mode>(bad, bad_out);
}

// ------------------------------------------------------------------------------------------------------ normalise
// keys[(o*Ip + i)*J + j] = pick(idx[o*sio + j*sij + i*sii]) over the index array's own extents [Op][Ip][J]; R for a dropped entry.
struct NormArgs {
    int64_t Op, Ip, J, R, sio, sij, sii;
};

template <int Mode>
__global__ __launch_bounds__(kBlock) void scatter_normalise_kernel(const int64_t *__restrict__ idx, int64_t *__restrict__ keys, NormArgs g, int64_t *bad_out) {
    bool bad = false;
    const int64_t total = g.Op * g.Ip * g.J, step = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += step) {
        int64_t j, i;
        const int64_t line = div_small(e, g.J, &j);
        const int64_t o = div_small(line, g.Ip, &i);
        bool b = false;
        const int64_t p = pick<Mode>(idx[o * g.sio + j * g.sij + i * g.sii], g.R, b);
        bad |= b;
        keys[e] = b ? g.R : p;
    }
    report_bad<Mode>(bad, bad_out);
}

// ------------------------------------------------------------------------------------------------------ SORTED
// The sorted lists: line (o*lo + i*li) of keys / order holds J entries.  lo / li are 0 where the index array broadcasts.
struct SortedArgs {
    int64_t O, J, I, R, lo, li, svo, svj, svi, oso, sor, osi;
    int seg;  // SORTED_ROWS
};

template <typename T, bool Add>
__global__ __launch_bounds__(kBlock) void scatter_sorted_kernel(T *__restrict__ out, const int64_t *__restrict__ keys, const int64_t *__restrict__ order,
                                                                const T *__restrict__ val, SortedArgs g) {
    using A = typename AccOf<T>::type;
    const int64_t total = g.O * g.I * g.J, step = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += step) {
        int64_t k, i;
        const int64_t oi = div_small(e, g.J, &k);
        const int64_t o = div_small(oi, g.I, &i);
        const int64_t *kl = keys + (o * g.lo + i * g.li) * g.J, *ol = order + (o * g.lo + i * g.li) * g.J;
        const int64_t p = kl[k];
        if ((uint64_t)p >= (uint64_t)g.R) continue;  // a dropped entry
        T *dst = out + o * g.oso + p * g.sor + i * g.osi;
        const T *vb = val + o * g.svo + i * g.svi;
        if constexpr (!Add) {
            if (k + 1 == g.J || kl[k + 1] != p) *dst = vb[ol[k] * g.svj];  // the last of its run: the largest j
        } else {
            if (k == 0 || kl[k - 1] != p) {  // the first of its run
                A acc = (A)*dst;
                for (int64_t r = k; r < g.J && kl[r] == p; ++r) acc += (A)vb[ol[r] * g.svj];
                *dst = (T)acc;
            }
        }
    }
}

// A lane segment per sorted entry (o, k) and its row of I contiguous elements.
template <typename T, bool Add, bool Vec>
__global__ __launch_bounds__(kBlock) void scatter_sorted_rows_kernel(T *__restrict__ out, const int64_t *__restrict__ keys, const int64_t *__restrict__ order,
                                                                     const T *__restrict__ val, SortedArgs g) {
    using A = typename AccOf<T>::type;
    using V = Pack<T, Vec>;
    constexpr int W = Vec ? 16 / (int)sizeof(T) : 1;
    const int lane = threadIdx.x & 63, segs = 64 / g.seg, sg = lane / g.seg, sl = lane - sg * g.seg;
    const int64_t rows = g.O * g.J, piece = (int64_t)g.seg * W;
    const int64_t pieces = (g.I + piece - 1) / piece, tasks = (rows + segs - 1) / segs * pieces;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t task = wave; task < tasks; task += waves) {  // wave-uniform
        int64_t pc;
        const int64_t rg = div_small(task, pieces, &pc);
        const int64_t col = pc * piece + (int64_t)sl * W, row = rg * segs + sg;
        if (row >= rows || col >= g.I) continue;
        int64_t o = 0, k = row;
        if (g.O > 1) o = div_small(row, g.J, &k);
        const int64_t *kl = keys + o * g.lo * g.J, *ol = order + o * g.lo * g.J;
        const int64_t p = kl[k];
        if ((uint64_t)p >= (uint64_t)g.R) continue;  // a dropped entry
        T *dst = out + o * g.oso + p * g.sor + col;
        const T *vb = val + o * g.svo + col;
        if constexpr (!Add) {
            if (k + 1 == g.J || kl[k + 1] != p) *reinterpret_cast<V *>(dst) = *reinterpret_cast<const V *>(vb + ol[k] * g.svj);
        } else {
            if (k == 0 || kl[k - 1] != p) {
                const V d = *reinterpret_cast<const V *>(dst);
                A acc[W];
#pragma unroll
                for (int w = 0; w < W; ++w) acc[w] = (A)d.v[w];
                for (int64_t r = k; r < g.J && kl[r] == p; ++r) {
                    const V v = *reinterpret_cast<const V *>(vb + ol[r] * g.svj);
#pragma unroll
                    for (int w = 0; w < W; ++w) acc[w] += (A)v.v[w];
                }
                V res;
#pragma unroll
                for (int w = 0; w < W; ++w) res.v[w] = (T)acc[w];
                *reinterpret_cast<V *>(dst) = res;
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ the planner
struct Plan {
    int route = SMHIP_SCATTER_ROUTE_NONE;
    bool unique = false, copy_idx = false, copy_val = false;
    int64_t O = 1, R = 0, J = 0, I = 1, total = 0;
    int64_t sio = 0, sij = 0, sii = 0, svo = 0, svj = 0, svi = 0, oso = 0, sor = 1, osi = 0;
    int64_t Op = 1, Ip = 1, sorted = 0;  // the index array's own extents, and the entries sorted
    int sort_launches = 0;
    int launches() const {
        if (route == SMHIP_SCATTER_ROUTE_NONE) return 0;
        return (copy_idx ? 1 : 0) + (copy_val ? 1 : 0) + (unique ? 1 : 2 + sort_launches);
    }
    int code() const { return route | (copy_idx || copy_val ? SMHIP_SCATTER_COPY : 0); }
};

// The walk of (idx_strides, val_strides) over the dense `out`, if both come to [kept] J [kept].
bool walk3(const int64_t *walk_shape, const int64_t *out_strides, const int64_t *idx_strides, const int64_t *val_strides, int ndim, int axis, Plan *pl) {
    Plan &p = *pl;
    Ax ax[SMHIP_MAX_NDIM];
    const int n = merge_axes(walk_shape, out_strides, ndim, 1u << axis, true, ax, val_strides, idx_strides);
    int red = -1;
    for (int k = 0; k < n; ++k)
        if (ax[k].red) red = k;
    const Ax *o = nullptr, *i = nullptr;
    if (red < 0) {  // J = 1: the axis is not in the list; a group stands before or after it by its stride in out
        // (two groups on the same side of the axis are axes that did not merge: not this walk)
        for (int k = 0; k < n; ++k) {
            const Ax *&side = ax[k].st >= out_strides[axis] ? o : i;
            if (side) return false;
            side = &ax[k];
        }
        p.sij = p.svj = 0;
    } else {
        if (red > 1 || n - red - 1 > 1) return false;
        if (red == 1) o = &ax[0];
        if (red + 1 < n) i = &ax[red + 1];
        p.sij = ax[red].st2, p.svj = ax[red].ost;
    }
    p.O = p.I = 1, p.sio = p.svo = p.oso = p.sii = p.svi = p.osi = 0;
    if (o) p.O = o->n, p.oso = o->st, p.sio = o->st2, p.svo = o->ost;
    if (i) p.I = i->n, p.osi = i->st, p.sii = i->st2, p.svi = i->ost;
    return true;
}

void make_plan(int flags, int dtype, const int64_t *out_shape, int ndim, int axis, const int64_t *idx_strides, const int64_t *val_strides, int64_t J, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    int64_t walk_shape[SMHIP_MAX_NDIM], out_strides[SMHIP_MAX_NDIM], dense_w[SMHIP_MAX_NDIM];
    int64_t before_n = 1, after_n = 1;
    bool empty = J == 0;
    for (int d = 0; d < ndim; ++d) {
        walk_shape[d] = d == axis ? J : out_shape[d];
        empty |= walk_shape[d] == 0;
        // an empty walk was not measured by the checks: its other extents may be anything, and the products only saturate
        if (d < axis && __builtin_mul_overflow(before_n, out_shape[d], &before_n)) before_n = INT64_MAX;
        if (d > axis && __builtin_mul_overflow(after_n, out_shape[d], &after_n)) after_n = INT64_MAX;
    }
    p.R = out_shape[axis], p.J = J, p.O = before_n, p.I = after_n;
    if (empty) return;
    p.total = before_n * after_n * J;
    p.unique = (flags & SMHIP_SCATTER_UNIQUE) != 0 || J <= 1;
    dense_strides(out_shape, ndim, out_strides);
    dense_strides(walk_shape, ndim, dense_w);
    p.sor = out_strides[axis];
    // the walk in place; else with idx dense, else with values dense, else both
    if (!walk3(walk_shape, out_strides, idx_strides, val_strides, ndim, axis, &p)) {
        if (walk3(walk_shape, out_strides, dense_w, val_strides, ndim, axis, &p)) p.copy_idx = true;
        else if (walk3(walk_shape, out_strides, idx_strides, dense_w, ndim, axis, &p)) p.copy_val = true;
        else walk3(walk_shape, out_strides, dense_w, dense_w, ndim, axis, &p), p.copy_idx = p.copy_val = true;  // always [O] J [I]
    }
    const bool rows = p.I >= vec_width(dtype) && p.sii == 0 && p.svi == 1 && p.osi == 1;  // the row kernels walk out at unit stride
    p.route = p.unique ? (rows ? SMHIP_SCATTER_ROUTE_ROWS : SMHIP_SCATTER_ROUTE_DIRECT) : (rows ? SMHIP_SCATTER_ROUTE_SORTED_ROWS : SMHIP_SCATTER_ROUTE_SORTED);
    if (!p.unique) {
        p.Op = p.O > 1 && p.sio != 0 ? p.O : 1;
        p.Ip = p.I > 1 && p.sii != 0 ? p.I : 1;
        p.sorted = p.Op * p.Ip * J;
        const int64_t shape2[2] = {p.Op * p.Ip, J}, strides2[2] = {J, 1};
        sort_axis_plan(SMHIP_I64, shape2, strides2, 2, 1, nullptr, &p.sort_launches, nullptr, nullptr);
    }
}

// ------------------------------------------------------------------------------------------------------ launching
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_SCATTER_GRID_CAP")); return g; }  // the cap of every launch here, read once

template <typename T, bool Add, int Mode>
int run_unique(const Plan &p, T *out, const int64_t *idx, const T *val, int64_t *bad, hipStream_t s) {
    constexpr int W = 16 / (int)sizeof(T);
    if (p.route == SMHIP_SCATTER_ROUTE_ROWS) {
        const bool vec = !misaligned(out, 16) && !misaligned(val, 16) && p.I % W == 0 && p.svo % W == 0 && p.svj % W == 0 && p.oso % W == 0 && p.sor % W == 0;
        const int64_t per_row = ceil_div(p.I, vec ? W : 1);  // lane steps a row takes
        const RowsArgs g{p.O, p.J, p.I, p.R, p.sio, p.sij, p.svo, p.svj, p.oso, p.sor, segment_for(per_row)};
        const int64_t piece = (int64_t)g.seg * (vec ? W : 1);
        const int64_t tasks = ceil_div(p.O * p.J, (int64_t)(64 / g.seg) * kRowsInFlightPerLane) * ceil_div(p.I, piece);
        const unsigned blocks = grid_cap().blocks_for(tasks);
        if (vec) hipLaunchKernelGGL((scatter_rows_kernel<T, Add, Mode, true>), dim3(blocks), dim3(kBlock), 0, s, out, idx, val, g, bad);
        else hipLaunchKernelGGL((scatter_rows_kernel<T, Add, Mode, false>), dim3(blocks), dim3(kBlock), 0, s, out, idx, val, g, bad);
        SMHIP_LAUNCH_CHECK("scatter_axis rows");
    } else {
        const Walk3 g{p.O, p.J, p.I, p.R, p.sio, p.sij, p.sii, p.svo, p.svj, p.svi, p.oso, p.sor, p.osi};
        hipLaunchKernelGGL((scatter_direct_kernel<T, Add, Mode>), dim3(grid_cap().capped(ceil_div(p.total, kBlock))), dim3(kBlock), 0, s, out, idx, val, g, bad);
        SMHIP_LAUNCH_CHECK("scatter_axis direct");
    }
    return SMHIP_OK;
}

template <int Mode>
int run_normalise(const Plan &p, const int64_t *idx, int64_t *keys, int64_t *bad, hipStream_t s) {
    const NormArgs g{p.Op, p.Ip, p.J, p.R, p.Op > 1 ? p.sio : 0, p.sij, p.Ip > 1 ? p.sii : 0};
    hipLaunchKernelGGL((scatter_normalise_kernel<Mode>), dim3(grid_cap().capped(ceil_div(p.sorted, kBlock))), dim3(kBlock), 0, s, idx, keys, g, bad);
    SMHIP_LAUNCH_CHECK("scatter_axis normalise");
    return SMHIP_OK;
}

template <typename T, bool Add>
int run_sorted(const Plan &p, int mode, T *out, const int64_t *idx, const T *val, int64_t *bad, hipStream_t s) {
    constexpr int W = 16 / (int)sizeof(T);
    Pooled pool;
    void *raw;
    if (int rc = pool.take((size_t)p.sorted * 2 * sizeof(int64_t), &raw)) return rc;
    int64_t *keys = static_cast<int64_t *>(raw), *order = keys + p.sorted;
    if (int rc = with_index_mode("scatter_axis", mode, [&](auto m) { return run_normalise<decltype(m)::value>(p, idx, keys, bad, s); })) return rc;
    const int64_t shape2[2] = {p.Op * p.Ip, p.J}, strides2[2] = {p.J, 1};
    if (int rc2 = launch_sort_axis(SMHIP_SORT_ASCENDING, SMHIP_I64, keys, shape2, strides2, 2, 1, keys, order, s)) return rc2;  // the keys in place
    SortedArgs g{p.O, p.J, p.I, p.R, p.Op > 1 ? p.Ip : 0, p.Ip > 1 ? 1 : 0, p.svo, p.svj, p.svi, p.oso, p.sor, p.osi, 64};
    if (p.route == SMHIP_SCATTER_ROUTE_SORTED_ROWS) {
        const bool vec = !misaligned(out, 16) && !misaligned(val, 16) && p.I % W == 0 && p.svo % W == 0 && p.svj % W == 0 && p.oso % W == 0 && p.sor % W == 0;
        g.seg = segment_for(ceil_div(p.I, vec ? W : 1));
        const int64_t piece = (int64_t)g.seg * (vec ? W : 1);
        const int64_t tasks = ceil_div(p.O * p.J, (int64_t)(64 / g.seg)) * ceil_div(p.I, piece);
        const unsigned blocks = grid_cap().blocks_for(tasks);
        if (vec) hipLaunchKernelGGL((scatter_sorted_rows_kernel<T, Add, true>), dim3(blocks), dim3(kBlock), 0, s, out, keys, order, val, g);
        else hipLaunchKernelGGL((scatter_sorted_rows_kernel<T, Add, false>), dim3(blocks), dim3(kBlock), 0, s, out, keys, order, val, g);
        SMHIP_LAUNCH_CHECK("scatter_axis sorted rows");
    } else {
        hipLaunchKernelGGL((scatter_sorted_kernel<T, Add>), dim3(grid_cap().capped(ceil_div(p.total, kBlock))), dim3(kBlock), 0, s, out, keys, order, val, g);
        SMHIP_LAUNCH_CHECK("scatter_axis sorted");
    }
    return SMHIP_OK;
}

template <typename T, bool Add>
int run_plan(const Plan &p, int mode, void *out, const int64_t *idx, const void *val, int64_t *bad, hipStream_t s) {
    T *po = static_cast<T *>(out);
    const T *pv = static_cast<const T *>(val);
    if (!p.unique) return run_sorted<T, Add>(p, mode, po, idx, pv, bad, s);
    return with_index_mode("scatter_axis", mode, [&](auto m) { return run_unique<T, Add, decltype(m)::value>(p, po, idx, pv, bad, s); });
}

// Validation: everything that can be said without a device or a pointer.
int scatter_axis_check(const char *who, int kind, int mode, int flags, int dtype, const int64_t *out_shape, int ndim, int axis, const int64_t *idx_strides,
                       const int64_t *val_strides, int64_t n_entries) {
    if (kind != SMHIP_SCATTER_PUT && kind != SMHIP_SCATTER_ADD) return fail(SMHIP_ERR_INVALID, "%s: bad kind %d", who, kind);
    if (int rc = check_index_mode(who, mode)) return rc;
    if (flags & ~SMHIP_SCATTER_UNIQUE) return fail(SMHIP_ERR_INVALID, "%s: unknown flag bits 0x%x", who, flags);
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (int rc = check_axis(who, axis, ndim)) return rc;
    if (int rc = check_extents(who, out_shape, idx_strides, ndim)) return rc;
    if (int rc = check_extents(who, out_shape, val_strides, ndim)) return rc;
    if (n_entries < 0) return fail(SMHIP_ERR_INVALID, "%s: n_entries %lld is negative", who, (long long)n_entries);
    // element counts and spans that do not fit 2^59 elements would wrap in the overlap checks: refused, not computed
    const int64_t limit = (int64_t)1 << 59;
    int64_t n = 1, n_out = 1, span_i = 0, span_v = 0;
    bool empty = n_entries == 0;
    for (int d = 0; d < ndim; ++d) empty |= d != axis && out_shape[d] == 0;
    for (int d = 0; d < ndim && !empty; ++d) {
        const int64_t w = d == axis ? n_entries : out_shape[d];
        int64_t ti, tv;
        if (__builtin_mul_overflow(n, w, &n) || n >= limit || __builtin_mul_overflow(n_out, std::max<int64_t>(out_shape[d], 1), &n_out) || n_out >= limit ||
            __builtin_mul_overflow(w - 1, idx_strides[d], &ti) || __builtin_add_overflow(span_i, ti, &span_i) || span_i >= limit ||
            __builtin_mul_overflow(w - 1, val_strides[d], &tv) || __builtin_add_overflow(span_v, tv, &span_v) || span_v >= limit)
            return fail(SMHIP_ERR_INVALID, "%s: the target or an operand's span exceeds 2^59 elements", who);
    }
    if (!empty && out_shape[axis] == 0) return fail(SMHIP_ERR_INVALID, "%s: cannot place entries on an axis of 0 elements", who);
    if (!empty && n_entries >= kMaxSorted && !(flags & SMHIP_SCATTER_UNIQUE))
        return fail(SMHIP_ERR_UNSUPPORTED, "%s: %lld entries per line without SMHIP_SCATTER_UNIQUE (the sort's positions are 32 bits wide: below 2^31)", who,
                    (long long)n_entries);
    return SMHIP_OK;
}

void scatter_axis_plan(int flags, int dtype, const int64_t *out_shape, int ndim, int axis, const int64_t *idx_strides, const int64_t *val_strides,
                       int64_t n_entries, int *route, int *launches, int64_t *orji4, int64_t *sorted_entries) {
    Plan pl;
    make_plan(flags, dtype, out_shape, ndim, axis, idx_strides, val_strides, n_entries, &pl);
    if (route) *route = pl.code();
    if (launches) *launches = pl.launches();
    if (orji4) orji4[0] = pl.O, orji4[1] = pl.R, orji4[2] = pl.J, orji4[3] = pl.I;
    if (sorted_entries) *sorted_entries = pl.sorted;
}

int launch_scatter_axis(int kind, int mode, int flags, int dtype, void *out, const int64_t *out_shape, int ndim, int axis, const int64_t *idx,
                        const int64_t *idx_strides, const void *values, const int64_t *val_strides, int64_t n_entries, int64_t *bad_out, hipStream_t s) {
    Plan pl;
    make_plan(flags, dtype, out_shape, ndim, axis, idx_strides, val_strides, n_entries, &pl);
    if (pl.route == SMHIP_SCATTER_ROUTE_NONE) return SMHIP_OK;
    if (bad_out) SMHIP_TRY(hipMemsetAsync(bad_out, 0, sizeof(int64_t), s));
    Pooled idx_pool, val_pool;
    int64_t walk_shape[SMHIP_MAX_NDIM];
    for (int d = 0; d < ndim; ++d) walk_shape[d] = d == axis ? n_entries : out_shape[d];
    if (pl.copy_idx) {
        const void *copy;
        if (int rc = idx_pool.dense_copy(SMHIP_I64, idx, walk_shape, idx_strides, ndim, s, &copy)) return rc;
        idx = static_cast<const int64_t *>(copy);
    }
    if (pl.copy_val)
        if (int rc = val_pool.dense_copy(dtype, values, walk_shape, val_strides, ndim, s, &values)) return rc;
    const bool add = kind == SMHIP_SCATTER_ADD;
    switch (dtype) {
        case SMHIP_F32: return add ? run_plan<float, true>(pl, mode, out, idx, values, bad_out, s) : run_plan<uint32_t, false>(pl, mode, out, idx, values, bad_out, s);
        case SMHIP_I32: return add ? run_plan<uint32_t, true>(pl, mode, out, idx, values, bad_out, s) : run_plan<uint32_t, false>(pl, mode, out, idx, values, bad_out, s);
        case SMHIP_F64: return add ? run_plan<double, true>(pl, mode, out, idx, values, bad_out, s) : run_plan<uint64_t, false>(pl, mode, out, idx, values, bad_out, s);
        case SMHIP_I64: return add ? run_plan<uint64_t, true>(pl, mode, out, idx, values, bad_out, s) : run_plan<uint64_t, false>(pl, mode, out, idx, values, bad_out, s);
    }
    return fail(SMHIP_ERR_INVALID, "scatter_axis: bad dtype %d", dtype);
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_scatter_axis(int kind, int mode, int flags, int dtype, void *out, const int64_t *out_shape, int ndim, int axis, const int64_t *idx,
                       const int64_t *idx_strides, const void *values, const int64_t *val_strides, int64_t n_entries, int64_t *bad_out) {
    if (int rc = scatter_axis_check("scatter_axis", kind, mode, flags, dtype, out_shape, ndim, axis, idx_strides, val_strides, n_entries)) return rc;
    int64_t n = 1, n_out = 1, walk_shape[SMHIP_MAX_NDIM];
    for (int d = 0; d < ndim; ++d) walk_shape[d] = d == axis ? n_entries : out_shape[d], n *= walk_shape[d], n_out *= out_shape[d];
    if (n == 0) return SMHIP_OK;
    if (!out || !idx || !values) return fail(SMHIP_ERR_INVALID, "scatter_axis: null target, index array or values");
    const size_t esz = dtype_size(dtype);
    const Span so{out, (size_t)n_out * esz}, si{idx, span_bytes(walk_shape, idx_strides, ndim, sizeof(int64_t))},
        sv{values, span_bytes(walk_shape, val_strides, ndim, esz)}, sb{bad_out, bad_out ? sizeof(int64_t) : 0};
    if (spans_overlap(so, si) || spans_overlap(so, sv) || spans_overlap(so, sb))
        return fail(SMHIP_ERR_INVALID, "scatter_axis: the target overlaps the index array, the values or bad_out");
    if (spans_overlap(sb, si) || spans_overlap(sb, sv)) return fail(SMHIP_ERR_INVALID, "scatter_axis: bad_out overlaps the index array or the values");
    SMHIP_ACQUIRE(s);  // undeclared spans (pooled copies, the sorted lists): ordered behind everything, recorded tiny operators flushed first
    return launch_scatter_axis(kind, mode, flags, dtype, out, out_shape, ndim, axis, idx, idx_strides, values, val_strides, n_entries, bad_out, s);
}

int smhip_scatter_plan(int kind, int mode, int flags, int dtype, const int64_t *out_shape, int ndim, int axis, const int64_t *idx_strides,
                       const int64_t *val_strides, int64_t n_entries, int *route, int *launches, int64_t *orji4, int64_t *sorted_entries) {
    if (int rc = scatter_axis_check("scatter_plan", kind, mode, flags, dtype, out_shape, ndim, axis, idx_strides, val_strides, n_entries)) return rc;
    scatter_axis_plan(flags, dtype, out_shape, ndim, axis, idx_strides, val_strides, n_entries, route, launches, orji4, sorted_entries);
    return SMHIP_OK;
}
