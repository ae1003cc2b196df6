// take_axis.hip -- picking by position along one axis: np.take_along_axis and np.take (smhip_take_axis).
//
// The reference has nothing of the kind; numpy is the contract (smhip.h has it in full):
//     out[..., j, ...] = a[..., pick(idx[..., j, ...]), ...]       pick = the index mode: CHECKED, CLIP or WRAP
// np.take(a, ids, axis) is the same call with the index array broadcast (stride 0) over every axis but `axis`.  The result is a
// copy of the operand's bits (which zero, which NaN payload): the kernels move 4- or 8-byte words and never compute on them, so
// f32 / i32 and f64 / i64 share their code, and the result is unique whatever the route, the grid or the stream.
//
// NO ADDRESS OUTSIDE `a` IS EVER FORMED.  Every kernel turns the 64-bit index it read into a position p in [0, R - 1] with pick()
// (index_mode.hip.h, shared with scatter_axis.hip and count.hip) BEFORE anything is multiplied by a stride or added to a pointer: CHECKED and CLIP clamp, WRAP takes the non-negative remainder
// (R >= 1 is checked on the host, so the range is never empty; INT64_MIN and INT64_MAX go through the same 64-bit arithmetic,
// nothing is narrowed to 32 bits first).  The offset o*sao + p*sar + i*sai is then one that the host's span check covered.
// A bad index under CHECKED is reported, not followed: any lane that meets one writes the constant 1 to *bad_out with a plain
// store (every writer stores the same value, so the race is benign).  No atomics.
//
// Planner (host only; smhip_take_plan reports it), with axis_plan.h's merging over THREE stride sets: the axes of the result are
// ordered by a's stride and merged where a, idx and the dense result all run on.  What is left must be [kept] J [kept]:
//     out[o*oso + j*osj + i*osi] = a[o*sao + pick(idx[o*sio + j*sij + i*sii])*sar + i*sai]          oji3 = {O, J, I}
// so a transposed or broadcast `a` is read in place (the walk follows a's memory; the result's strides come along).  A view that
// does not come to three axes is copied dense first through Pooled (idx alone if that is enough, else a, else both): SMHIP_TAKE_COPY.
//   LINE    I = 1, sar = 1, R <= K (32 KiB of LDS), J >= R / c: a workgroup brings `per` lines of a into LDS (16-byte loads where
//           the line allows: each line sits in LDS at the offset its address has within 16 bytes, so global and LDS vectors
//           line up), reads its indices coalesced, picks from LDS and writes the result.  Long index lines are cut into chunks
//           of picks so that few lines still make a wide grid.
//   ROWS    sai = osi = 1, sii = 0, I >= one vector: rows of I contiguous elements are copied whole.  A wave (or a segment of
//           8 / 16 / 32 lanes of it for short rows) reads the index once per row and keeps 4 rows in flight per lane; 16-byte
//           loads and stores when a, out and every row pitch are 16-byte aligned, else the same walk element by element.
//   DIRECT  everything else: one result element per lane, lanes along the unit stride of the RESULT, so idx and out are
//           coalesced and the read of a is not (it is an element-granular gather: it relies on L2 and the Infinity Cache).
// Every kernel loops over its tasks grid-stride under a capped grid (SMHIP_TAKE_GRID_CAP).
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

constexpr int kLineBytes = 32 << 10;   // LINE: the longest line staged in LDS (K = 8192 / 4096 elements); four workgroups fit a CU's 160 KiB
constexpr int kRowsInFlightPerLane = 4;  // ROWS: rows a lane has loads outstanding for
constexpr int kDefaultLineRatio = 2;   // c: LINE when J >= R / c.  profiles/take_rates.txt: on (131072, 1000) f32 DIRECT wins 1.7x at J = R / 20 and
                                       // LINE 1.08x at J = R; the straight line between the two crosses near J = 0.6 R

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

// ------------------------------------------------------------------------------------------------------ LINE
struct LineArgs {
    int64_t lines, R, J, sao, sio, sij, oso, osj, jchunk, nj;
    int per, slots;  // lines per workgroup; 16-byte slots of a line in LDS
};

template <typename U, int Mode>
__global__ __launch_bounds__(kBlock) void take_line_kernel(const U *__restrict__ a, const int64_t *__restrict__ idx, U *__restrict__ out, LineArgs g,
                                                           int64_t *bad_out) {
    extern __shared__ uint4 lds16[];
    constexpr int W = 16 / (int)sizeof(U);
    U *lds = reinterpret_cast<U *>(lds16);
    const int P = g.slots * W;  // elements between two lines in LDS
    const int64_t groups = (g.lines + g.per - 1) / g.per, tasks = groups * g.nj;
    bool bad = false;
    for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {  // workgroup-uniform
        const int64_t grp = task / g.nj, jc = task - grp * g.nj;
        const int64_t line0 = grp * g.per, j0 = jc * g.jchunk, jn = min(g.jchunk, g.J - j0);
        const int live = (int)min((int64_t)g.per, g.lines - line0);
        // the lines, slot by slot: LDS slot k of line l holds the 16 bytes at (line base rounded down to 16 bytes) + 16 k
        for (int s = threadIdx.x; s < live * g.slots; s += kBlock) {
            const int l = s / g.slots, k = s - l * g.slots;
            const U *base = a + (line0 + l) * g.sao;
            const int shift = (int)((reinterpret_cast<uintptr_t>(base) / sizeof(U)) & (W - 1));
            const int64_t e0 = (int64_t)k * W - shift;  // the line element the slot starts at
            if (e0 >= 0 && e0 + W <= g.R) {
                lds16[l * g.slots + k] = *reinterpret_cast<const uint4 *>(base + e0);
            } else {
#pragma unroll
                for (int w = 0; w < W; ++w)
                    if (e0 + w >= 0 && e0 + w < g.R) lds[l * P + k * W + w] = base[e0 + w];
            }
        }
        __syncthreads();
        const int64_t items = (int64_t)live * jn;
        for (int64_t q = threadIdx.x; q < items; q += kBlock) {
            int64_t l = 0, j = q;
            if (live > 1) l = div_small(q, jn, &j);
            const int64_t line = line0 + l;
            const int shift = (int)((reinterpret_cast<uintptr_t>(a + line * g.sao) / sizeof(U)) & (W - 1));
            const int64_t p = pick<Mode>(idx[line * g.sio + (j0 + j) * g.sij], g.R, bad);
            out[line * g.oso + (j0 + j) * g.osj] = lds[l * P + shift + p];
        }
        __syncthreads();  // the next task reuses the lines
    }
    report_bad<Mode>(bad, bad_out);
}

// ------------------------------------------------------------------------------------------------------ ROWS
struct RowsArgs {
    int64_t O, J, I, R, sao, sar, sio, sij, oso, osj;
    int seg;  // lanes that share a row: 8, 16, 32 or 64
};

// Vec: every row of a and of out starts on a 16-byte boundary and I is a whole number of vectors.
template <typename U, int Mode, bool Vec>
__global__ __launch_bounds__(kBlock) void take_rows_kernel(const U *__restrict__ a, const int64_t *__restrict__ idx, U *__restrict__ out, RowsArgs g,
                                                           int64_t *bad_out) {
    constexpr int W = Vec ? 16 / (int)sizeof(U) : 1;
    constexpr int F = kRowsInFlightPerLane;
    using V = typename std::conditional<Vec, uint4, U>::type;
    const int lane = threadIdx.x & 63, segs = 64 / g.seg, sg = lane / g.seg, sl = lane - sg * g.seg;
    const int64_t rows = g.O * g.J, per_task = (int64_t)segs * F, piece = (int64_t)g.seg * W;
    const int64_t pieces = (g.I + piece - 1) / piece, tasks = (rows + per_task - 1) / per_task * pieces;
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6), waves = (int64_t)gridDim.x * (kBlock / 64);
    bool bad = false;
    for (int64_t task = wave; task < tasks; task += waves) {  // wave-uniform
        int64_t pc;
        const int64_t rg = div_small(task, pieces, &pc);
        const int64_t col = pc * piece + (int64_t)sl * W;
        const U *src[F];
        U *dst[F];
        V v[F];
#pragma unroll
        for (int k = 0; k < F; ++k) {
            const int64_t row = rg * per_task + (int64_t)k * segs + sg;
            src[k] = nullptr;
            if (row < rows && col < g.I) {
                int64_t o = 0, j = row;
                if (g.O > 1) o = div_small(row, g.J, &j);
                const int64_t p = pick<Mode>(idx[o * g.sio + j * g.sij], g.R, bad);
                src[k] = a + o * g.sao + p * g.sar + col;
                dst[k] = out + o * g.oso + j * g.osj + col;
            }
        }
#pragma unroll
        for (int k = 0; k < F; ++k)
            if (src[k]) v[k] = *reinterpret_cast<const V *>(src[k]);
#pragma unroll
        for (int k = 0; k < F; ++k)
            if (src[k]) *reinterpret_cast<V *>(dst[k]) = v[k];
    }
    report_bad<Mode>(bad, bad_out);
}

// ------------------------------------------------------------------------------------------------------ DIRECT
// The three axes ordered by the RESULT's stride, largest first (n[2] is the unit-stride one).  sa is 0 for J, which moves
// through the picked position alone.
struct DirectArgs {
    int64_t n[3], sa[3], si[3];
    int64_t R, sar, total;
};

template <typename U, int Mode>
__global__ __launch_bounds__(kBlock) void take_direct_kernel(const U *__restrict__ a, const int64_t *__restrict__ idx, U *__restrict__ out, DirectArgs g,
                                                             int64_t *bad_out) {
    bool bad = false;
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < g.total; e += step) {
        int64_t c[3];
        const int64_t hi = div_small(e, g.n[2], &c[2]);
        c[0] = div_small(hi, g.n[1], &c[1]);
        const int64_t at = c[0] * g.si[0] + c[1] * g.si[1] + c[2] * g.si[2];
        const int64_t p = pick<Mode>(idx[at], g.R, bad);
        out[e] = a[c[0] * g.sa[0] + c[1] * g.sa[1] + c[2] * g.sa[2] + p * g.sar];
    }
    report_bad<Mode>(bad, bad_out);
}

// ------------------------------------------------------------------------------------------------------ the planner
struct Plan {
    int route = SMHIP_TAKE_ROUTE_NONE;
    bool copy_a = false, copy_idx = false;
    int64_t O = 1, J = 1, I = 1, R = 0, total = 0, K = 0;
    int64_t sao = 0, sar = 0, sai = 0, sio = 0, sij = 0, sii = 0, oso = 0, osj = 0, osi = 0;
    int per = 1, slots = 0;       // LINE
    int64_t jchunk = 0, nj = 1;   // LINE
    int launches() const { return route == SMHIP_TAKE_ROUTE_NONE ? 0 : 1 + (copy_a ? 1 : 0) + (copy_idx ? 1 : 0); }
    int code() const { return route | (copy_a || copy_idx ? SMHIP_TAKE_COPY : 0); }
};

int line_ratio() {  // c, read once
    static const int c = [] {
        const char *t = getenv("SMHIP_TAKE_LINE_RATIO");
        const long long v = t && *t ? atoll(t) : -1;
        return v >= 0 && v <= (1 << 30) ? (int)v : kDefaultLineRatio;
    }();
    return c;
}

// The walk of (a_strides, idx_strides) over the dense result, if it comes to [kept] J [kept].
bool walk3(const int64_t *out_shape, const int64_t *a_strides, const int64_t *idx_strides, int ndim, int axis, Plan *pl) {
    Plan &p = *pl;
    int64_t ost[SMHIP_MAX_NDIM];
    dense_strides(out_shape, ndim, ost);
    Ax ax[SMHIP_MAX_NDIM];
    const int n = merge_axes(out_shape, a_strides, ndim, 1u << axis, false, ax, ost, idx_strides);
    int red = -1;
    for (int k = 0; k < n; ++k)
        if (ax[k].red) red = k;
    const Ax *o = nullptr, *i = nullptr;
    if (red < 0) {  // J = 1: the axis is not in the list, and stands wherever its stride puts it
        if (n > 2) return false;
        if (n == 2) o = &ax[0], i = &ax[1];
        else if (n == 1) (ax[0].st >= a_strides[axis] ? o : i) = &ax[0];
        p.J = 1, p.sar = a_strides[axis], p.sij = 0, p.osj = 0;
    } else {
        if (red > 1 || n - red - 1 > 1) return false;
        if (red == 1) o = &ax[0];
        if (red + 1 < n) i = &ax[red + 1];
        p.J = ax[red].n, p.sar = ax[red].st, p.sij = ax[red].st2, p.osj = ax[red].ost;
    }
    p.O = p.I = 1, p.sao = p.sio = p.oso = p.sai = p.sii = p.osi = 0;
    if (o) p.O = o->n, p.sao = o->st, p.sio = o->st2, p.oso = o->ost;
    if (i) p.I = i->n, p.sai = i->st, p.sii = i->st2, p.osi = i->ost;
    // o and i play the same part in the walk.  A stride-0 axis of a sorts last and lands on I; with no O it is better seen as
    // O lines that share one line of a (a row broadcast against the index array is LINE's case, not DIRECT's)
    if (p.O == 1 && p.I > 1 && p.sai == 0) {
        p.O = p.I, p.sao = 0, p.sio = p.sii, p.oso = p.osi;
        p.I = 1, p.sai = p.sii = p.osi = 0;
    }
    return true;
}

void make_plan(int dtype, const int64_t *a_strides, int64_t a_extent, const int64_t *idx_strides, const int64_t *out_shape, int ndim, int axis, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    int64_t before_n = 1, after_n = 1;
    for (int d = 0; d < ndim; ++d) (d < axis ? before_n : d > axis ? after_n : p.J) *= out_shape[d];
    p.O = before_n, p.I = after_n, p.R = a_extent, p.total = before_n * after_n * p.J;
    const int esz = (int)dtype_size(dtype), W = vec_width(dtype);
    p.K = kLineBytes / esz;
    if (p.total == 0) return;
    // the walk in place; else with idx dense, else with a dense, else both
    int64_t dense_a[SMHIP_MAX_NDIM], dense_i[SMHIP_MAX_NDIM], shape_a[SMHIP_MAX_NDIM];
    for (int d = 0; d < ndim; ++d) shape_a[d] = d == axis ? a_extent : out_shape[d];
    dense_strides(shape_a, ndim, dense_a);
    dense_strides(out_shape, ndim, dense_i);
    if (!walk3(out_shape, a_strides, idx_strides, ndim, axis, &p)) {
        if (walk3(out_shape, a_strides, dense_i, ndim, axis, &p)) p.copy_idx = true;
        else if (walk3(out_shape, dense_a, idx_strides, ndim, axis, &p)) p.copy_a = true;
        else walk3(out_shape, dense_a, dense_i, ndim, axis, &p), p.copy_a = p.copy_idx = true;  // always [O] J [I]
    }
    const int64_t c = line_ratio();
    if (p.I == 1 && p.sar == 1 && p.R <= p.K && c > 0 && p.J >= ceil_div(p.R, c)) {
        p.route = SMHIP_TAKE_ROUTE_LINE;
        p.slots = (int)ceil_div(p.R + W - 1, W);  // a line and the up to W - 1 elements its address stands past a 16-byte boundary
        // lines per workgroup: enough for about 1024 elements of work, no more than the LDS budget holds, few enough for a wide grid
        const int64_t least = std::max<int64_t>(1, 1024 / std::max(p.R, p.J)), most = std::max<int64_t>(1, kLineBytes / (p.slots * 16));
        p.per = (int)std::min(p.O, std::min(most, std::max(least, ceil_div(p.O, 4096))));
        // picks per task: the whole index line, unless the lines alone make a narrow grid; never fewer than a line costs to stage
        const int64_t groups = ceil_div(p.O, p.per), want = std::max<int64_t>(1, 1024 / groups);
        p.jchunk = std::min(p.J, std::max(std::max<int64_t>(256, p.R), ceil_div(p.J, want)));
        p.nj = ceil_div(p.J, p.jchunk);
    } else if (p.I >= W && p.sai == 1 && p.osi == 1 && p.sii == 0) {
        p.route = SMHIP_TAKE_ROUTE_ROWS;
    } else {
        p.route = SMHIP_TAKE_ROUTE_DIRECT;
    }
}

// ------------------------------------------------------------------------------------------------------ launching
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_TAKE_GRID_CAP")); return g; }  // the cap of every launch here, read once

template <typename U, int Mode>
int run_mode(const Plan &p, const U *a, const int64_t *idx, U *out, int64_t *bad, hipStream_t s) {
    constexpr int W = 16 / (int)sizeof(U);
    if (p.route == SMHIP_TAKE_ROUTE_LINE) {
        const LineArgs g{p.O, p.R, p.J, p.sao, p.sio, p.sij, p.oso, p.osj, p.jchunk, p.nj, p.per, p.slots};
        hipLaunchKernelGGL((take_line_kernel<U, Mode>), dim3(grid_cap().capped(ceil_div(p.O, p.per) * p.nj)), dim3(kBlock), (size_t)p.per * p.slots * 16, s, a,
                           idx, out, g, bad);
        SMHIP_LAUNCH_CHECK("take_axis line");
    } else if (p.route == SMHIP_TAKE_ROUTE_ROWS) {
        const bool vec = !misaligned(a, 16) && !misaligned(out, 16) && p.I % W == 0 && p.sar % W == 0 && p.sao % W == 0 && p.oso % W == 0 && p.osj % W == 0;
        const int64_t per_row = ceil_div(p.I, vec ? W : 1);  // lane steps a row takes
        RowsArgs g{p.O, p.J, p.I, p.R, p.sao, p.sar, p.sio, p.sij, p.oso, p.osj, segment_for(per_row)};
        const int64_t piece = (int64_t)g.seg * (vec ? W : 1);
        const int64_t tasks = ceil_div(p.O * p.J, (int64_t)(64 / g.seg) * kRowsInFlightPerLane) * ceil_div(p.I, piece);
        const unsigned blocks = grid_cap().blocks_for(tasks);
        if (vec) hipLaunchKernelGGL((take_rows_kernel<U, Mode, true>), dim3(blocks), dim3(kBlock), 0, s, a, idx, out, g, bad);
        else hipLaunchKernelGGL((take_rows_kernel<U, Mode, false>), dim3(blocks), dim3(kBlock), 0, s, a, idx, out, g, bad);
        SMHIP_LAUNCH_CHECK("take_axis rows");
    } else {
        // the three axes by the result's stride; an axis of extent 1 goes first, whatever stride it carries
        struct A3 { int64_t n, sa, si, os; } x[3] = {{p.O, p.sao, p.sio, p.oso}, {p.J, 0, p.sij, p.osj}, {p.I, p.sai, p.sii, p.osi}};
        std::stable_sort(x, x + 3, [](const A3 &l, const A3 &r) { return (l.n == 1 ? INT64_MAX : l.os) > (r.n == 1 ? INT64_MAX : r.os); });
        DirectArgs g;
        for (int k = 0; k < 3; ++k) g.n[k] = x[k].n, g.sa[k] = x[k].sa, g.si[k] = x[k].si;
        g.R = p.R, g.sar = p.sar, g.total = p.total;
        hipLaunchKernelGGL((take_direct_kernel<U, Mode>), dim3(grid_cap().capped(ceil_div(p.total, kBlock))), dim3(kBlock), 0, s, a, idx, out, g, bad);
        SMHIP_LAUNCH_CHECK("take_axis direct");
    }
    return SMHIP_OK;
}

template <typename U>
int run_plan(const Plan &p, int mode, const void *a, const int64_t *idx, void *out, int64_t *bad, hipStream_t s) {
    const U *pa = static_cast<const U *>(a);
    U *po = static_cast<U *>(out);
    return with_index_mode("take_axis", mode, [&](auto m) { return run_mode<U, decltype(m)::value>(p, pa, idx, po, bad, s); });
}

// Validation: everything that can be said without a device or a pointer.
int take_axis_check(const char *who, int mode, int dtype, const int64_t *a_strides, int64_t a_extent, const int64_t *idx_strides, const int64_t *out_shape,
                    int ndim, int axis) {
    if (int rc = check_index_mode(who, mode)) return rc;
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (int rc = check_axis(who, axis, ndim)) return rc;
    if (int rc = check_extents(who, out_shape, a_strides, ndim)) return rc;
    if (int rc = check_extents(who, out_shape, idx_strides, ndim)) return rc;
    if (a_extent < 0) return fail(SMHIP_ERR_INVALID, "%s: a_extent %lld is negative", who, (long long)a_extent);
    // element counts and spans that do not fit 2^59 elements would wrap in the overlap checks: refused, not computed
    const int64_t limit = (int64_t)1 << 59;
    int64_t n = 1, span_a = 0, span_i = 0;
    bool empty = false;
    for (int d = 0; d < ndim; ++d) empty |= out_shape[d] == 0;
    for (int d = 0; d < ndim && !empty; ++d) {
        int64_t ta, ti;
        if (__builtin_mul_overflow(n, out_shape[d], &n) || n >= limit ||
            __builtin_mul_overflow((d == axis ? std::max<int64_t>(a_extent, 1) : out_shape[d]) - 1, a_strides[d], &ta) ||
            __builtin_add_overflow(span_a, ta, &span_a) || span_a >= limit || __builtin_mul_overflow(out_shape[d] - 1, idx_strides[d], &ti) ||
            __builtin_add_overflow(span_i, ti, &span_i) || span_i >= limit)
            return fail(SMHIP_ERR_INVALID, "%s: the result or an operand's span exceeds 2^59 elements", who);
    }
    if (a_extent == 0) {
        if (!empty) return fail(SMHIP_ERR_INVALID, "%s: cannot take from an axis of 0 elements into a result that is not empty", who);
    }
    return SMHIP_OK;
}

void take_axis_plan(int dtype, const int64_t *a_strides, int64_t a_extent, const int64_t *idx_strides, const int64_t *out_shape, int ndim, int axis,
                    int *route, int *launches, int64_t *oji3, int64_t *chunk) {
    Plan pl;
    make_plan(dtype, a_strides, a_extent, idx_strides, out_shape, ndim, axis, &pl);
    if (route) *route = pl.code();
    if (launches) *launches = pl.launches();
    if (oji3) oji3[0] = pl.O, oji3[1] = pl.J, oji3[2] = pl.I;
    if (chunk) *chunk = pl.K;
}

int launch_take_axis(int mode, int dtype, const void *a, const int64_t *a_strides, int64_t a_extent, const int64_t *idx, const int64_t *idx_strides,
                     const int64_t *out_shape, int ndim, int axis, void *out, int64_t *bad_out, hipStream_t s) {
    Plan pl;
    make_plan(dtype, a_strides, a_extent, idx_strides, out_shape, ndim, axis, &pl);
    if (pl.route == SMHIP_TAKE_ROUTE_NONE) return SMHIP_OK;
    if (bad_out) SMHIP_TRY(hipMemsetAsync(bad_out, 0, sizeof(int64_t), s));
    Pooled a_pool, idx_pool;
    if (pl.copy_a) {
        int64_t shape_a[SMHIP_MAX_NDIM];
        for (int d = 0; d < ndim; ++d) shape_a[d] = d == axis ? a_extent : out_shape[d];
        if (int rc = a_pool.dense_copy(dtype, a, shape_a, a_strides, ndim, s, &a)) return rc;
    }
    if (pl.copy_idx) {
        const void *copy;
        if (int rc = idx_pool.dense_copy(SMHIP_I64, idx, out_shape, idx_strides, ndim, s, &copy)) return rc;
        idx = static_cast<const int64_t *>(copy);
    }
    return dtype_size(dtype) == 4 ? run_plan<uint32_t>(pl, mode, a, idx, out, bad_out, s) : run_plan<uint64_t>(pl, mode, a, idx, out, bad_out, s);
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_take_axis(int mode, int dtype, const void *a, const int64_t *a_strides, int64_t a_extent, const int64_t *idx, const int64_t *idx_strides,
                    const int64_t *out_shape, int ndim, int axis, void *out, int64_t *bad_out) {
    if (int rc = take_axis_check("take_axis", mode, dtype, a_strides, a_extent, idx_strides, out_shape, ndim, axis)) return rc;
    int64_t n = 1, shape_a[SMHIP_MAX_NDIM];
    for (int d = 0; d < ndim; ++d) n *= out_shape[d], shape_a[d] = d == axis ? a_extent : out_shape[d];
    if (n == 0) return SMHIP_OK;
    if (!a || !idx || !out) return fail(SMHIP_ERR_INVALID, "take_axis: null operand, index array or result");
    const size_t esz = dtype_size(dtype);
    const Span sa{a, span_bytes(shape_a, a_strides, ndim, esz)}, si{idx, span_bytes(out_shape, idx_strides, ndim, sizeof(int64_t))},
        so{out, (size_t)n * esz}, sb{bad_out, bad_out ? sizeof(int64_t) : 0};
    if (spans_overlap(so, sa) || spans_overlap(so, si) || spans_overlap(so, sb))
        return fail(SMHIP_ERR_INVALID, "take_axis: the result overlaps the operand, the index array or bad_out");
    if (spans_overlap(sb, sa) || spans_overlap(sb, si)) return fail(SMHIP_ERR_INVALID, "take_axis: bad_out overlaps the operand or the index array");
    SMHIP_ACQUIRE(s);  // undeclared spans (pooled dense copies): ordered behind everything, recorded tiny operators flushed first
    return launch_take_axis(mode, dtype, a, a_strides, a_extent, idx, idx_strides, out_shape, ndim, axis, out, bad_out, s);
}

int smhip_take_plan(int mode, int dtype, const int64_t *a_strides, int64_t a_extent, const int64_t *idx_strides, const int64_t *out_shape, int ndim, int axis,
                    int *route, int *launches, int64_t *oji3, int64_t *chunk) {
    if (int rc = take_axis_check("take_plan", mode, dtype, a_strides, a_extent, idx_strides, out_shape, ndim, axis)) return rc;
    take_axis_plan(dtype, a_strides, a_extent, idx_strides, out_shape, ndim, axis, route, launches, oji3, chunk);
    return SMHIP_OK;
}
