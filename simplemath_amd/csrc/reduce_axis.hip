// reduce_axis.hip -- sum, mean, max and min along chosen axes (smhip_reduce_axes).
//
// The reference has no axis reduction at all: every reduction it offers folds the whole array (dot_product,
// include/math/product.h).  NumPy's np.sum / np.mean / np.max / np.min over `axis` is the contract here:
//   sum    f32: fp64 accumulation, rounded once;  f64: fp64;  i32 / i64: wrapping in the type's width (bit-exact in any order)
//   mean   fp64 sum / count, rounded once (integer types: SMHIP_ERR_UNSUPPORTED)
//   max / min   exact; NaN propagates (which of +-0 a tie returns is not specified)
//
// Planner (host only; smhip_reduce_plan reports it).  The rules every axis family plans by are written once, in axis_plan.h:
// the merging of axes, the canonical walk, lanes per short row, the split of R, the capped grid, the argument checks and the
// pooled dense copy.  What is here is their use, and what only the reductions have: several reduced groups and CHANNEL.
// Size-1 axes are dropped, the rest ordered by stride (largest first) and neighbours that are adjacent in memory -- and, for
// kept axes, in the result -- merged.  One reduced axis between at most one kept axis outside it and one inside it is the
// canonical problem
//     out[o, i] = reduce_r a[o*so + r*sr + i*si]          (O, R, I)
// so sum(A.T, 0) is the same walk as sum(A, 1) and a transposed view is never copied.  Anything else:
//   * several reduced groups (axes 0 and 2 of a 3-D array): one pass per group, innermost first, through a dense
//     intermediate in the accumulator type (fp64 for float sums, so an f32 sum is still rounded once);
//   * a walk with no unit stride (stepped views), a broadcast (stride 0) axis, or kept axes that do not merge: the operand
//     is copied dense first (smhip_copy_strided's kernels) and planned again.
// Routes (every load a 16-byte vector where the layout has one; gfx950 takes them at any element-aligned address):
//   ROW      I = 1, sr = 1.  Rows of at most 64 vectors: a SEGMENT of g = 4, 16 or 64 lanes per row, one load per lane, four
//            rows per segment in flight, folded by the DPP scan of wave.hip cut to g lanes.  Longer rows: a wave per row,
//            four vectors per lane in flight.
//   COLUMN   si = 1.  A lane owns 4 consecutive kept columns and walks R, four rows in flight; lanes are packed over
//            (o, chunk, column quad), so few columns per outer index do not leave workgroups idle.
// Every kernel loops over its tasks grid-stride under a capped grid (SMHIP_REDUCE_GRID_CAP): any O fits HIP's 32-bit work-item count.
//   CHANNEL  si = 1, sr = I <= 8, R >= 1024 (NHWC per-channel: (N,H,W,3) over axes 0-2 is O = 1, R = N*H*W, I = 3): the (R, I) block is
//            one dense stream; a workgroup step covers 256 * I vectors, a multiple of I elements, so each lane's vector
//            slots belong to fixed channels -- per-slot accumulators, no divide in the loop, folded into channels at the end.
//   SPLIT    when O x I leaves too few lanes for 256 CUs, R is cut into chunks whose length depends on the shape alone;
//            each chunk's partial goes to [O][I][chunk] and ONE finishing launch (the ROW kernels over those rows) folds
//            them in index order.  No float atomics anywhere: the bits depend on dtype, kind, shape and merged layout only.
#include <stdlib.h>

#include <algorithm>
#include <limits>
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "fold.hip.h"
#include "internal.h"
#include "ops.hip.h"
#include "wave.hip.h"

namespace smhip {
namespace {

using namespace dev;
using namespace axis_plan;  // kBlock, kRowsInFlight, OutMap and the planner's rules

constexpr int kChannelMax = 8;                 // CHANNEL route: at most this many kept columns
constexpr int64_t kChannelMinR = 4 * kBlock;    // ... and at least one workgroup step of stream (256 * I vectors) per outer
                                                // index: shorter blocks go to COLUMN, whose lanes pack several (o, c) tasks

// ---- ROW, short rows: a segment of g lanes per row, every row at most g loads (vectors, then the R % W tail elements one
// per lane).  A wave covers kRowsInFlight * 64 / g consecutive rows (rows of the outer index, stride so); row = o, or for a
// finishing launch o * I2 + i (the partials of output (o, i)), written to out[(row / I2)*oso + (row % I2)*osi].
template <typename TI, typename TO, int K>
__global__ __launch_bounds__(kBlock) void row_short_kernel(const TI *__restrict__ a, int64_t rows, int64_t so, int64_t R, int g, int64_t I2,
                                                           TO *__restrict__ out, OutMap om, double divisor, int nt) {
    typedef typename Acc<TI, K>::type A;
    typedef typename VecTraits<TI>::vec_t V;
    constexpr int W = VecTraits<TI>::width;
    const int lane = threadIdx.x & 63, seg_lane = lane & (g - 1);
    const int64_t segs = 64 / g;
    const int64_t nvec = R / W, tail = R - nvec * W;
    const int64_t waves = (rows + kRowsInFlight * segs - 1) / (kRowsInFlight * segs), grid_waves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); wave < waves; wave += grid_waves) {  // wave-uniform
    const int64_t row0 = wave * kRowsInFlight * segs + lane / g;
    TI x[kRowsInFlight];
    A acc[kRowsInFlight];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) acc[u] = identity<A, K>();
    // vectors: all loads of the lane issued before the first use
    if (seg_lane < nvec) {
        V v[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
            const int64_t row = row0 + u * segs;
            if (row < rows) v[u] = load_stream_if(TI, reinterpret_cast<const V *>(a + row * so + (int64_t)seg_lane * W), nt);
        }
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
            if (row0 + u * segs < rows) {
#pragma unroll
                for (int k = 0; k < W; ++k) acc[u] = fold<A, K>(acc[u], widen<TI, A>(v[u][k]));
            }
        }
    } else if (seg_lane < nvec + tail) {
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
            const int64_t row = row0 + u * segs;
            x[u] = row < rows ? a[row * so + nvec * W + (seg_lane - nvec)] : TI(0);
        }
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u)
            if (row0 + u * segs < rows) acc[u] = fold<A, K>(acc[u], widen<TI, A>(x[u]));
    }
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
        const A t = segment_fold(acc[u], g, identity<A, K>(), fold<A, K>);
        const int64_t row = row0 + u * segs;
        if (seg_lane == g - 1 && row < rows) {
            const int64_t o = row / I2, i = row - o * I2;
            out[o * om.oso + i * om.osi] = finish<TO, A>(t, divisor);
        }
    }
    }
}

// ---- ROW, long rows: a wave per (row, chunk of R); chunk length CL is a multiple of 4 * 64 vectors, so every chunk but a
// row's last is walked without guards, four vectors per lane in flight.
template <typename TI, typename TO, int K>
__global__ __launch_bounds__(kBlock) void row_long_kernel(const TI *__restrict__ a, int64_t rows, int64_t so, int64_t R, int64_t CL, int64_t C,
                                                          int64_t I2, TO *__restrict__ out, OutMap om, double divisor, int nt) {
    typedef typename Acc<TI, K>::type A;
    typedef typename VecTraits<TI>::vec_t V;
    constexpr int W = VecTraits<TI>::width;
    constexpr int U = 4;
    const int lane = threadIdx.x & 63;
    const int64_t tasks = rows * C, grid_waves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t task = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); task < tasks; task += grid_waves) {  // wave-uniform
    const int64_t row = task / C, c = task - row * C;
    const int64_t start = c * CL, len = std::min(CL, R - start);
    const TI *p = a + row * so + start;
    const V *pv = reinterpret_cast<const V *>(p);
    const int64_t nvec = len / W, tail = len - nvec * W;
    A acc = identity<A, K>();
    int64_t j = 0;
    for (; j + U * 64 <= nvec; j += U * 64) {
        V v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = load_stream_if(TI, pv + j + u * 64 + lane, nt);
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int k = 0; k < W; ++k) acc = fold<A, K>(acc, widen<TI, A>(v[u][k]));
    }
    for (int64_t q = j + lane; q < nvec; q += 64) {
        const V v = load_stream_if(TI, pv + q, nt);
#pragma unroll
        for (int k = 0; k < W; ++k) acc = fold<A, K>(acc, widen<TI, A>(v[k]));
    }
    if (lane < tail) acc = fold<A, K>(acc, widen<TI, A>(p[nvec * W + lane]));
    acc = segment_fold(acc, 64, identity<A, K>(), fold<A, K>);
    if (lane == kWaveTotalLane) {
        const int64_t o = row / I2, i = row - o * I2;
        out[o * om.oso + i * om.osi + c * om.ocs] = finish<TO, A>(acc, divisor);
    }
    }
}

// ---- COLUMN: a lane owns kept columns i0 .. i0 + 3 of outer index o and walks rows [c*CL, c*CL + CL) of R.  Lanes are
// numbered (o, c, quad) with the quad fastest and packed without gaps: with few columns (I = 9 .. 1023, or I <= 8 over short
// R) one wave still covers several (o, c) tasks instead of leaving most of a workgroup idle.  Grid-stride over the lanes.
template <typename TI, typename TO, int K>
__global__ __launch_bounds__(kBlock) void column_kernel(const TI *__restrict__ a, int64_t O, int64_t so, int64_t R, int64_t sr, int64_t I,
                                                        int64_t CL, int64_t C, TO *__restrict__ out, OutMap om, double divisor, int nt) {
    typedef typename Acc<TI, K>::type A;
    typedef typename Quad<TI>::type Q;
    constexpr int U = 4;
    const int64_t nq = (I + 3) / 4, lanes = O * C * nq, grid_lanes = (int64_t)gridDim.x * kBlock;
    for (int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x; l < lanes; l += grid_lanes) {
    const int64_t oc = l / nq, i0 = (l - oc * nq) * 4, o = oc / C, c = oc - o * C;
    const int64_t r0 = c * CL, r1 = std::min(R, r0 + CL);
    const TI *p = a + o * so + i0;
    A acc[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] = identity<A, K>();
    if (i0 + 4 <= I) {
        int64_t r = r0;
        for (; r + U <= r1; r += U) {
            Q v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const Q *q = reinterpret_cast<const Q *>(p + (r + u) * sr);
                v[u] = (nt & kLoadNt) ? __builtin_nontemporal_load(q) : *q;
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) acc[k] = fold<A, K>(acc[k], widen<TI, A>(v[u][k]));
        }
        for (; r < r1; ++r) {
            const Q v = *reinterpret_cast<const Q *>(p + r * sr);
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = fold<A, K>(acc[k], widen<TI, A>(v[k]));
        }
    } else {
        const int64_t live = I - i0;  // 1 .. 3 columns
        for (int64_t r = r0; r < r1; ++r)
            for (int64_t k = 0; k < live; ++k) acc[k] = fold<A, K>(acc[k], widen<TI, A>(p[r * sr + k]));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (i0 + k < I) out[o * om.oso + (i0 + k) * om.osi + c * om.ocs] = finish<TO, A>(acc[k], divisor);
    }
}

// ---- CHANNEL: the (R, I) block of outer index o is a dense stream of L = R*I elements; workgroup (o, c) walks elements
// [c*CL, c*CL + CL), CL a multiple of the step S = 256 * I vectors.  Lane t's vector u of a step starts at element
// (t + 256 u) * W of it, so slot (u, k) always holds channel ((t + 256 u) * W + k) mod I.
// LOOP = false: one task per workgroup (the grid covers them all).  As a loop the body takes 159 VGPRs for the fp64 sums
// (three waves per SIMD) instead of 112 (four) -- the f32 per-channel sum ran at 63 % of peak instead of 77 % -- so the loop
// is compiled only for grids that the cap cuts short.
template <typename TI, typename TO, int K, bool LOOP>
__global__ __launch_bounds__(kBlock) void channel_kernel(const TI *__restrict__ a, int64_t O, int64_t so, int64_t L, int I, int64_t CL, int64_t C,
                                                         TO *__restrict__ out, OutMap om, double divisor, int nt) {
    typedef typename Acc<TI, K>::type A;
    typedef typename VecTraits<TI>::vec_t V;
    constexpr int W = VecTraits<TI>::width;
    const int t = threadIdx.x;
    __shared__ A lds[kBlock / 64];
    for (int64_t task = blockIdx.x; task < O * C; task += gridDim.x) {  // workgroup-uniform
    const int64_t o = task / C, c = task - o * C;
    const TI *p = a + o * so;
    const int64_t step = (int64_t)kBlock * I * W;
    const int64_t e_begin = c * CL, e_end = std::min(L, e_begin + CL);
    A acc[kChannelMax][W];
#pragma unroll
    for (int u = 0; u < kChannelMax; ++u)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[u][k] = identity<A, K>();
    int64_t e0 = e_begin;
    for (; e0 + step <= e_end; e0 += step) {
        V v[kChannelMax];
#pragma unroll
        for (int u = 0; u < kChannelMax; ++u)
            if (u < I) v[u] = load_stream_if(TI, reinterpret_cast<const V *>(p + e0 + (int64_t)(t + kBlock * u) * W), nt);
#pragma unroll
        for (int u = 0; u < kChannelMax; ++u)
            if (u < I)
#pragma unroll
                for (int k = 0; k < W; ++k) acc[u][k] = fold<A, K>(acc[u][k], widen<TI, A>(v[u][k]));
    }
    if (e0 < e_end) {  // the stream's last, partial step
#pragma unroll
        for (int u = 0; u < kChannelMax; ++u)
            if (u < I)
#pragma unroll
                for (int k = 0; k < W; ++k) {
                    const int64_t e = e0 + (int64_t)(t + kBlock * u) * W + k;
                    if (e < e_end) acc[u][k] = fold<A, K>(acc[u][k], widen<TI, A>(p[e]));
                }
    }
    const int lane = t & 63, wave = t >> 6;
    for (int ch = 0; ch < I; ++ch) {
        A v = identity<A, K>();
#pragma unroll
        for (int u = 0; u < kChannelMax; ++u)
            if (u < I)
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if ((int)((((int64_t)(t + kBlock * u)) * W + k) % I) == ch) v = fold<A, K>(v, acc[u][k]);
        v = segment_fold(v, 64, identity<A, K>(), fold<A, K>);
        if (lane == kWaveTotalLane) lds[wave] = v;
        __syncthreads();
        if (t == 0) {
            A s = lds[0];
#pragma unroll
            for (int w = 1; w < kBlock / 64; ++w) s = fold<A, K>(s, lds[w]);
            out[o * om.oso + ch * om.osi + c * om.ocs] = finish<TO, A>(s, divisor);
        }
        __syncthreads();
    }
    if constexpr (!LOOP) break;
    }
}

// ------------------------------------------------------------------------------------------------------ the planner
enum Route { kRouteNone = SMHIP_REDUCE_ROUTE_NONE, kRouteRow = SMHIP_REDUCE_ROUTE_ROW, kRouteColumn = SMHIP_REDUCE_ROUTE_COLUMN,
             kRouteChannel = SMHIP_REDUCE_ROUTE_CHANNEL, kRouteFill = SMHIP_REDUCE_ROUTE_FILL, kRouteGather = SMHIP_REDUCE_ROUTE_GATHER };

struct Pass : Canon {
    int route = kRouteNone;
    int64_t C = 1, CL = 0;  // chunks of R (C > 1: a finishing launch) and their length (elements of the row / stream, rows of a column)
    int g = 0;              // ROW: lanes per row (4, 16, 64), 0 = a wave per row
};
struct Plan {
    bool copy = false;      // dense copy of the operand first
    int npasses = 0;
    Pass pass[SMHIP_MAX_NDIM];
    int launches = 0;
    int route_code = kRouteNone;
    int64_t ori[3] = {0, 0, 0};
    // kRouteGather (no reduced extent > 1): the kept axes, for a strided copy
    int64_t total_out = 0, total_r = 0;
};

// Splits and row segments of one canonical pass; counts its launches.  An unsplit pass walks one chunk of R rounded up to
// whole steps (ROW, CHANNEL) or of R itself (COLUMN).
void shape_pass(Pass &p, int dtype, int *launches) {
    const int64_t W = vec_width(dtype);
    Split sp{1, 0};
    if (p.route == kRouteRow) {
        p.g = segment_lanes(row_loads(p.R, W));
        if (p.g == 0) {
            const int64_t unit = 4 * 64 * W;  // one guard-free step of a wave
            p.CL = ceil_div(p.R, unit) * unit;
            sp = split_row(p.O * 64, p.R, unit);
        }
    } else if (p.route == kRouteColumn) {
        p.CL = p.R;
        sp = split_column(p.O * ceil_div(p.I, 4), p.R);
    } else if (p.route == kRouteChannel) {  // the (R, I) block as one stream of L elements
        const int64_t L = p.R * p.I, step = (int64_t)kBlock * p.I * W;
        p.CL = ceil_div(L, step) * step;
        sp = split_row(p.O * kBlock, L, step);
    }
    p.C = 1;
    if (sp.CL) p.C = sp.C, p.CL = sp.CL;
    *launches += p.C > 1 ? 2 : 1;
}

// COLUMN's refinement: few kept columns that lie side by side, and at least a workgroup step of stream per outer index.
bool channel_walk(const Canon &c) { return c.I <= kChannelMax && c.sr == c.I && c.R >= kChannelMinR; }

// Canonical single pass of a merged axis list, if it has one.
bool single_pass(const Ax *ax, int n, Pass *p) {
    Pass q;
    const Walk walk = canonical(ax, n, &q);
    if (walk == kWalkNone) return false;
    q.route = walk == kWalkRow ? kRouteRow : channel_walk(q) ? kRouteChannel : kRouteColumn;
    *p = q;
    return true;
}

// Validation: everything that can be said without a device.
int check_args(const char *who, int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, uint32_t mask) {
    if (kind < SMHIP_REDUCE_SUM || kind > SMHIP_REDUCE_MIN) return fail(SMHIP_ERR_INVALID, "%s: bad kind %d", who, kind);
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (mask == 0 || (mask >> ndim) != 0) return fail(SMHIP_ERR_INVALID, "%s: axes mask 0x%x empty or beyond ndim %d", who, mask, ndim);
    if (int rc = check_extents(who, shape, strides, ndim)) return rc;
    if (kind == SMHIP_REDUCE_MEAN && (dtype == SMHIP_I32 || dtype == SMHIP_I64))
        return fail(SMHIP_ERR_UNSUPPORTED, "%s: mean of an integer type", who);
    int64_t nout = 1, nr = 1;
    for (int d = 0; d < ndim; ++d) ((mask >> d & 1) ? nr : nout) *= shape[d];
    if (nout > 0 && nr == 0 && kind != SMHIP_REDUCE_SUM) return fail(SMHIP_ERR_INVALID, "%s: mean / max / min over an empty extent", who);
    return SMHIP_OK;
}

// Host-only: the whole route of a call.
void make_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, uint32_t mask, Plan *pl) {
    *pl = Plan();
    int64_t nout = 1, nr = 1;
    bool any_red = false, zero_stride = false;
    for (int d = 0; d < ndim; ++d) {
        ((mask >> d & 1) ? nr : nout) *= shape[d];
        if ((mask >> d & 1) && shape[d] > 1) any_red = true;
        if (shape[d] > 1 && strides[d] == 0) zero_stride = true;
    }
    pl->total_out = nout, pl->total_r = nr;
    if (nout == 0) return;  // nothing to write
    if (nr == 0) {          // sum over an empty extent: zeros
        pl->route_code = kRouteFill, pl->launches = 1, pl->ori[0] = nout, pl->ori[1] = 0, pl->ori[2] = 1;
        return;
    }
    if (!any_red) {  // every reduced extent is 1: the result is the kept elements themselves
        pl->route_code = kRouteGather, pl->launches = 1, pl->ori[0] = nout, pl->ori[1] = 1, pl->ori[2] = 1;
        return;
    }
    Ax ax[SMHIP_MAX_NDIM];
    int n = merge_axes(shape, strides, ndim, mask, false, ax);
    Pass p;
    if (!zero_stride && single_pass(ax, n, &p)) {
        pl->npasses = 1, pl->pass[0] = p;
    } else {
        // dense in index order (copied there first unless it already is), one pass per reduced group, innermost first
        pl->copy = zero_stride || !row_major(shape, strides, ndim);
        int64_t dense[SMHIP_MAX_NDIM];
        dense_strides(shape, ndim, dense);
        n = merge_axes(shape, dense, ndim, mask, true, ax);
        while (true) {
            int last = -1;
            for (int k = 0; k < n; ++k)
                if (ax[k].red) last = k;
            if (last < 0) break;
            Pass q;
            q.R = ax[last].n;
            q.I = last + 1 < n ? ax[last + 1].n : 1;
            q.O = 1;
            for (int k = 0; k < last; ++k) q.O *= ax[k].n;
            q.sr = q.I, q.si = 1, q.so = q.R * q.I;
            q.oso = q.I, q.osi = 1;  // the pass's result: dense (O, I)
            q.route = q.I == 1 ? kRouteRow : channel_walk(q) ? kRouteChannel : kRouteColumn;
            pl->pass[pl->npasses++] = q;
            // what remains: the axes before it, and the kept one after it merged onto the kept one before it (dense)
            if (last + 1 < n) {
                if (last >= 1) {
                    ax[last - 1].n *= ax[last + 1].n;
                    n = last;
                } else {
                    ax[0] = ax[1];
                    n = 1;
                }
            } else {
                n = last;
            }
        }
    }
    pl->launches = pl->copy ? 1 : 0;
    for (int k = 0; k < pl->npasses; ++k) shape_pass(pl->pass[k], dtype, &pl->launches);
    const Pass &f = pl->pass[0];
    pl->route_code = f.route | (pl->copy ? SMHIP_REDUCE_COPY : 0) | (pl->npasses > 1 ? SMHIP_REDUCE_PASSES : 0);
    for (int k = 0; k < pl->npasses; ++k)
        if (pl->pass[k].C > 1) pl->route_code |= SMHIP_REDUCE_SPLIT;
    pl->ori[0] = f.O, pl->ori[1] = f.R, pl->ori[2] = f.I;
}

// ------------------------------------------------------------------------------------------------------ launching
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_REDUCE_GRID_CAP")); return g; }  // the cap of every launch here, read once

// One canonical pass: in (TI) -> out (TO) at `om`, with split and finishing launch as planned.
template <typename TI, typename TO, typename S, int K>
int run_pass(const Pass &p, const TI *in, TO *out, OutMap om, double divisor, hipStream_t s) {
    const size_t in_bytes = (size_t)(p.O * p.R * p.I) * sizeof(TI);
    const int nt = stream_policy({{in, in_bytes}}, {nullptr, 0});
    S *part = nullptr;
    ScratchLease lease;
    OutMap pm = om;
    if (p.C > 1) {
        double *buf;
        if (int rc = lease.take((size_t)(p.O * p.I * p.C), &buf)) return rc;  // sizeof(S) <= 8
        part = reinterpret_cast<S *>(buf);
        pm = OutMap{p.I * p.C, p.C, 1};
    }
    // the first launch writes TO when R is whole, S (partials) when it is split
    auto first = [&](auto *dst, OutMap m, double div) -> int {
        typedef typename std::remove_pointer<decltype(dst)>::type D;
        if (p.route == kRouteRow && p.g > 0) {
            const int64_t waves = ceil_div(p.O, kRowsInFlight * (64 / p.g));
            hipLaunchKernelGGL((row_short_kernel<TI, D, K>), dim3(grid_cap().blocks_for(waves)), dim3(kBlock), 0, s, in, p.O, p.so, p.R, p.g, (int64_t)1, dst, m, div, nt);
        } else if (p.route == kRouteRow) {
            hipLaunchKernelGGL((row_long_kernel<TI, D, K>), dim3(grid_cap().blocks_for(p.O * p.C)), dim3(kBlock), 0, s, in, p.O, p.so, p.R, p.CL, p.C, (int64_t)1, dst, m, div, nt);
        } else if (p.route == kRouteColumn) {
            const int64_t lanes = p.O * p.C * ceil_div(p.I, 4);
            hipLaunchKernelGGL((column_kernel<TI, D, K>), dim3(grid_cap().capped(ceil_div(lanes, kBlock))), dim3(kBlock), 0, s, in, p.O, p.so, p.R, p.sr, p.I, p.CL, p.C, dst, m, div, nt);
        } else {
            if (p.O * p.C <= (int64_t)grid_cap().cap)
                hipLaunchKernelGGL((channel_kernel<TI, D, K, false>), dim3(grid_cap().capped(p.O * p.C)), dim3(kBlock), 0, s, in, p.O, p.so, p.R * p.I, (int)p.I, p.CL, p.C, dst, m, div, nt);
            else
                hipLaunchKernelGGL((channel_kernel<TI, D, K, true>), dim3(grid_cap().capped(p.O * p.C)), dim3(kBlock), 0, s, in, p.O, p.so, p.R * p.I, (int)p.I, p.CL, p.C, dst, m, div, nt);
        }
        SMHIP_LAUNCH_CHECK("reduce_axes");
        return SMHIP_OK;
    };
    if (p.C == 1) return first(out, om, divisor);
    if (int rc = first(part, pm, 0.0)) return rc;
    // finishing: rows (o, i) of C partials each, in index order
    const int64_t rows = p.O * p.I;
    if (const int g = segment_lanes(row_loads(p.C, VecTraits<S>::width))) {
        const int64_t waves = ceil_div(rows, kRowsInFlight * (64 / g));
        hipLaunchKernelGGL((row_short_kernel<S, TO, K>), dim3(grid_cap().blocks_for(waves)), dim3(kBlock), 0, s, part, rows, p.C, p.C, g, p.I, out, om, divisor, 0);
    } else {
        hipLaunchKernelGGL((row_long_kernel<S, TO, K>), dim3(grid_cap().blocks_for(rows)), dim3(kBlock), 0, s, part, rows, p.C, p.C, p.C, (int64_t)1, p.I, out, om, divisor, 0);
    }
    SMHIP_LAUNCH_CHECK("reduce_axes finish");
    return SMHIP_OK;
}

// T: element type; S: what partial and intermediate results are kept in (fp64 for float sums, T otherwise).
// TO: what the call writes -- T, or double for the unrounded fp64 sum (launch_reduce_sum64).
template <typename T, typename TO, int K>
int run_plan(const Plan &pl, int dtype, const T *a, const int64_t *shape, const int64_t *strides, int ndim, TO *out, double divisor, hipStream_t s) {
    typedef typename std::conditional<K == kSum && std::is_floating_point<T>::value, double, T>::type S;
    Pooled copy, tmp[2];
    const void *dense = a;
    if (pl.copy)
        if (int rc = copy.dense_copy(dtype, a, shape, strides, ndim, s, &dense)) return rc;
    const T *in = static_cast<const T *>(dense);
    const int np = pl.npasses;
    if (np == 1) {
        const Pass &p = pl.pass[0];
        return run_pass<T, TO, S, K>(p, in, out, OutMap{p.oso, p.osi, 0}, divisor, s);
    }
    // several reduced groups: T -> S, S -> S ..., S -> T (the mean's division at the very end)
    const S *prev = nullptr;
    for (int k = 0; k < np; ++k) {
        const Pass &p = pl.pass[k];
        const OutMap om{p.oso, p.osi, 0};
        if (k == np - 1) return run_pass<S, TO, S, K>(p, prev, out, om, divisor, s);
        void *buf;  // the pass two back, whose result this owner hands back first, has been queued before
        if (int rc = tmp[k & 1].take((size_t)(p.O * p.I) * sizeof(S), &buf)) return rc;
        S *dst = static_cast<S *>(buf);
        int rc = k == 0 ? run_pass<T, S, S, K>(p, in, dst, om, 0.0, s) : run_pass<S, S, S, K>(p, prev, dst, om, 0.0, s);
        if (rc) return rc;
        prev = dst;
    }
    return SMHIP_OK;
}

template <typename T>
int run_kind(int kind, const Plan &pl, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, void *out, hipStream_t s) {
    const T *pa = static_cast<const T *>(a);
    T *po = static_cast<T *>(out);
    switch (kind) {
        case SMHIP_REDUCE_SUM: return run_plan<T, T, kSum>(pl, dtype, pa, shape, strides, ndim, po, 0.0, s);
        case SMHIP_REDUCE_MEAN: return run_plan<T, T, kSum>(pl, dtype, pa, shape, strides, ndim, po, (double)pl.total_r, s);
        case SMHIP_REDUCE_MAX: return run_plan<T, T, kMax>(pl, dtype, pa, shape, strides, ndim, po, 0.0, s);
        case SMHIP_REDUCE_MIN: return run_plan<T, T, kMin>(pl, dtype, pa, shape, strides, ndim, po, 0.0, s);
    }
    return fail(SMHIP_ERR_INVALID, "reduce_axes: bad kind %d", kind);
}

int reduce_axes_check(const char *who, int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, uint32_t axes_mask) {
    return check_args(who, kind, dtype, shape, strides, ndim, axes_mask);
}

void reduce_axes_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, uint32_t axes_mask, int *route, int *launches, int64_t *ori3) {
    Plan pl;
    make_plan(dtype, shape, strides, ndim, axes_mask, &pl);
    if (route) *route = pl.route_code;
    if (launches) *launches = pl.launches;
    if (ori3) ori3[0] = pl.ori[0], ori3[1] = pl.ori[1], ori3[2] = pl.ori[2];
}

int launch_reduce_axes(int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, uint32_t axes_mask, void *out,
                       hipStream_t s) {
    Plan pl;
    make_plan(dtype, shape, strides, ndim, axes_mask, &pl);
    if (pl.route_code == kRouteNone) return SMHIP_OK;
    if (pl.route_code == kRouteFill) {
        const uint64_t zero = 0;  // 0 in every element type
        return launch_fill(dtype, out, &zero, (size_t)pl.total_out, s);
    }
    if (pl.route_code == kRouteGather) {
        int64_t ost[SMHIP_MAX_NDIM];
        axis_plan::dense_strides(shape, ndim, ost, ~axes_mask);
        return launch_copy_strided(dtype, a, strides, out, ost, shape, ndim, s);
    }
    switch (dtype) {
        case SMHIP_F32: return run_kind<float>(kind, pl, dtype, a, shape, strides, ndim, out, s);
        case SMHIP_F64: return run_kind<double>(kind, pl, dtype, a, shape, strides, ndim, out, s);
        case SMHIP_I32: return run_kind<int32_t>(kind, pl, dtype, a, shape, strides, ndim, out, s);
        case SMHIP_I64: return run_kind<int64_t>(kind, pl, dtype, a, shape, strides, ndim, out, s);
    }
    return fail(SMHIP_ERR_INVALID, "reduce_axes: bad dtype %d", dtype);
}

}  // namespace

// What moments_axis.hip takes from here: the route of a call, and the call's sums kept in fp64 -- what MEAN divides before it rounds.
void reduce_sum_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, uint32_t axes_mask, int *route, int *launches, int64_t *ori3) {
    reduce_axes_plan(dtype, shape, strides, ndim, axes_mask, route, launches, ori3);
}
int launch_reduce_sum64(int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, uint32_t axes_mask, double *out, hipStream_t s) {
    Plan pl;
    make_plan(dtype, shape, strides, ndim, axes_mask, &pl);
    if (pl.npasses == 0 || (dtype != SMHIP_F32 && dtype != SMHIP_F64)) return fail(SMHIP_ERR_INVALID, "reduce_sum64: no walk for this call");
    if (dtype == SMHIP_F64) return run_plan<double, double, kSum>(pl, dtype, static_cast<const double *>(a), shape, strides, ndim, out, 0.0, s);
    return run_plan<float, double, kSum>(pl, dtype, static_cast<const float *>(a), shape, strides, ndim, out, 0.0, s);
}

}  // namespace smhip

using namespace smhip;

int smhip_reduce_axes(int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, uint32_t axes_mask, void *out) {
    if (int rc = reduce_axes_check("reduce_axes", kind, dtype, shape, strides, ndim, axes_mask)) return rc;
    int64_t n = 1, nout = 1;
    for (int d = 0; d < ndim; ++d) n *= shape[d], nout *= (axes_mask >> d & 1) ? 1 : shape[d];
    if (nout == 0) return SMHIP_OK;
    if (!out || (n && !a)) return fail(SMHIP_ERR_INVALID, "reduce_axes: null buffer");
    SMHIP_ACQUIRE(s);  // a reduction: undeclared spans, ordered behind everything (recorded tiny operators flushed first)
    return launch_reduce_axes(kind, dtype, a, shape, strides, ndim, axes_mask, out, s);
}

int smhip_reduce_plan(int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, uint32_t axes_mask, int *route, int *launches,
                      int64_t *ori3) {
    if (int rc = reduce_axes_check("reduce_plan", kind, dtype, shape, strides, ndim, axes_mask)) return rc;
    reduce_axes_plan(dtype, shape, strides, ndim, axes_mask, route, launches, ori3);
    return SMHIP_OK;
}
