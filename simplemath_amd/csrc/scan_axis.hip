// scan_axis.hip -- cumulative sum, product, max and min along one axis (smhip_scan_axis).
//
// The reference has no scan.  NumPy's np.cumsum / np.cumprod / np.maximum.accumulate / np.minimum.accumulate over `axis` is
// the contract: out[..., r, ...] = fold over k <= r of a[..., k, ...], inclusive and forward, in the accumulators of
// fold.hip.h (fp64 for float sums and products, each output rounded once; wrapping 64-bit for integer ones; T for max / min).
//
// Planner (host only; smhip_scan_plan reports it).  Size-1 axes are dropped; an operand that is dense in row-major order
// is the canonical problem
//     out[o, r, i] = scan_r a[o, r, i]          (O, R, I) = (extents before the axis, the axis, extents after it)
// with both sides dense in that order.  Any other operand (a transposed or stepped view, a stride-0 axis, a sub-block) is
// copied dense first (smhip_copy_strided's kernels, a pooled temporary): there are no transposing scan kernels.  Lanes per
// short row, the capped grid, the argument checks and that copy are axis_plan.h's; when R is split is the scans' own rule.
// Routes:
//   COPYONLY  R = 1: the result is the operand.
//   ROW       I = 1.  Rows of at most 64 loads (16-byte vectors, then the R % W tail elements one per lane): a SEGMENT of
//             g = 4, 16 or 64 lanes per row, four rows per segment in flight.  Longer rows: a workgroup walks its row in
//             tiles of 256 x 4 vectors with the running value in a register.  In both a lane scans its own vector serially,
//             the lanes' totals are scanned by the DPP moves of wave.hip.h, and (long rows) the waves' totals cross through
//             LDS -- one barrier per tile, the buffer alternating.
//   COLUMN    I > 1.  A lane owns 4 consecutive i (one 16-byte vector; the last 1 .. 3 columns by scalar accesses) and a few
//             consecutive rows of a block, which it scans with 4 accumulators; the 16 row groups of a workgroup meet in LDS.
//             All loads of a block are in flight together and none depends on the carry.
//   SPLIT     when the launch would have too few lanes, R is cut into chunks whose length the shape and the element size decide.
//             Launch 1 (the same walks, storing nothing) leaves each chunk's total in its own slot, [O][chunk][I] in the
//             accumulator type; launch 2 starts each chunk from the fold, in index order, of the totals before it.
// No workgroup ever waits for another: carries between chunks cross a launch boundary, never a flag in memory.  Every value
// that meets another in a fold covers the run of elements just before it, so a result is the fold of a[0..r] under one fixed
// parenthesisation: deterministic, and a float product can overflow only where a run of consecutive factors does.
// Every kernel loops over its tasks grid-stride under a capped grid (SMHIP_SCAN_GRID_CAP); indices are 64-bit throughout.
// `a` and `out` may be the same dense array: a lane (ROW: a workgroup) stores only what it has loaded itself.
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
using namespace axis_plan;  // kBlock, kRowsInFlight, kTargetLanes and the planner's shared rules

constexpr int kWaves = kBlock / 64;
constexpr int kTileVecs = 4;      // ROW, long rows: vectors per lane and tile
// When R is split.  The split reads the operand twice (3 x sizeof(T) per element instead of 2), so it is taken only where
// the one-launch walk would leave most of the machine idle: ROW with fewer than 1024 rows (a workgroup each), COLUMN with
// fewer than 64 workgroups (a quarter of the CUs).  A split COLUMN launch aims at 1024 workgroups.
constexpr int64_t kRowSplitBelowRows = kTargetLanes / kBlock, kColumnSplitBelowGroups = 64, kColumnTargetGroups = 1024;
constexpr int64_t kRowMaxChunks = kBlock;  // ROW: a workgroup folds the totals before its chunk in one step, one per lane
constexpr int64_t kColumnMaxChunks = 1024;  // COLUMN: a lane folds at most 1024 / 16 totals before its chunk

// A vector store through a pointer whose TYPE carries the element alignment (a function template would drop it).
#define SMHIP_SCAN_STORE(q, v, pol)                    \
    do {                                               \
        if ((pol) & kStoreKeep) *(q) = (v);            \
        else __builtin_nontemporal_store((v), (q));    \
    } while (0)

// ---- ROW, short rows: a segment of g lanes per row, every row at most g loads.  A wave covers kRowsInFlight * 64 / g
// consecutive rows.
template <typename T, int K>
__global__ __launch_bounds__(kBlock) void row_short_kernel(const T *a, T *out, int64_t rows, int64_t R, int g, int pol) {
    typedef typename Acc<T, K>::type A;
    typedef typename VecTraits<T>::vec_t V;
    constexpr int W = VecTraits<T>::width;
    const A id = identity<A, K>();
    const int lane = threadIdx.x & 63, seg_lane = lane & (g - 1);
    const int64_t segs = 64 / g;
    const int64_t nvec = R / W, tail = R - nvec * W;
    const bool is_vec = seg_lane < nvec, is_tail = !is_vec && seg_lane < nvec + tail;
    const int64_t waves = (rows + kRowsInFlight * segs - 1) / (kRowsInFlight * segs), grid_waves = (int64_t)gridDim.x * kWaves;
    for (int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); wave < waves; wave += grid_waves) {  // wave-uniform
        const int64_t row0 = wave * kRowsInFlight * segs + lane / g;
        A x[kRowsInFlight][W];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u)
#pragma unroll
            for (int k = 0; k < W; ++k) x[u][k] = id;
        if (is_vec) {  // all loads of the lane issued before the first use
            V v[kRowsInFlight];
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) {
                const int64_t row = row0 + u * segs;
                if (row < rows) v[u] = load_stream_if(T, reinterpret_cast<const V *>(a + row * R + (int64_t)seg_lane * W), pol);
            }
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u)
                if (row0 + u * segs < rows) {
#pragma unroll
                    for (int k = 0; k < W; ++k) x[u][k] = widen<T, A>(v[u][k]);
                }
        } else if (is_tail) {
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) {
                const int64_t row = row0 + u * segs;
                if (row < rows) x[u][0] = widen<T, A>(a[row * R + nvec * W + (seg_lane - nvec)]);
            }
        }
        // the lane's own elements, then the lanes before it in the segment (all 64 lanes are here: the DPP moves need them)
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
#pragma unroll
            for (int k = 1; k < W; ++k) x[u][k] = fold<A, K>(x[u][k - 1], x[u][k]);
            const A before = segment_scan(segment_prev(x[u][W - 1], g, lane, id), g, lane, id, fold<A, K>);
#pragma unroll
            for (int k = 0; k < W; ++k) x[u][k] = fold<A, K>(before, x[u][k]);
        }
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {
            const int64_t row = row0 + u * segs;
            if (row >= rows) continue;
            if (is_vec) {
                V o;
#pragma unroll
                for (int k = 0; k < W; ++k) o[k] = finish<T, A>(x[u][k], 0.0);
                SMHIP_SCAN_STORE(reinterpret_cast<V *>(out + row * R + (int64_t)seg_lane * W), o, pol);
            } else if (is_tail) {
                out[row * R + nvec * W + (seg_lane - nvec)] = finish<T, A>(x[u][0], 0.0);
            }
        }
    }
}

// ---- ROW, long rows: workgroup task (row, chunk c) walks elements [c*CL, c*CL + CL) of its row tile by tile.  Vector j of a
// tile belongs to lane j % 256, slot u = j / 256 (loads coalesced), so the tile's order is (u, wave, lane, element).
// TOTAL: launch 1 of a split -- nothing is stored but the chunk's total, part[row*C + c].  Otherwise `part` (when not null)
// holds those totals and the chunk starts from the fold of part[row*C .. row*C + c - 1]; C <= 256, one per lane.
template <typename T, int K, bool TOTAL>
__global__ __launch_bounds__(kBlock) void row_long_kernel(const T *a, T *out, int64_t rows, int64_t R, int64_t CL, int64_t C,
                                                          typename Acc<T, K>::type *part, int pol) {
    typedef typename Acc<T, K>::type A;
    typedef typename VecTraits<T>::vec_t V;
    constexpr int W = VecTraits<T>::width, U = kTileVecs;
    constexpr int64_t kTile = (int64_t)kBlock * U * W;
    const A id = identity<A, K>();
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    __shared__ A totals[2][U][kWaves];
    __shared__ A before_chunk[kWaves];
    int buf = 0;
    for (int64_t task = blockIdx.x; task < rows * C; task += gridDim.x) {  // workgroup-uniform
        const int64_t row = task / C, c = task - row * C;
        const int64_t start = c * CL, len = std::min(CL, R - start);
        const T *p = a + row * R + start;
        T *q = out + row * R + start;
        A carry = id;
        if (!TOTAL && part && c > 0) {  // workgroup-uniform
            A v = t < c ? part[row * C + t] : id;
            v = wave_scan(v, lane, id, fold<A, K>);
            if (lane == kWaveTotalLane) before_chunk[w] = v;
            __syncthreads();
#pragma unroll
            for (int k = 0; k < kWaves; ++k) carry = fold<A, K>(carry, before_chunk[k]);
            __syncthreads();
        }
        for (int64_t base = 0; base < len; base += kTile) {
            A x[U][W];
            if (base + kTile <= len) {
                V v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) v[u] = load_stream_if(T, reinterpret_cast<const V *>(p + base) + u * kBlock + t, pol);
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int k = 0; k < W; ++k) x[u][k] = widen<T, A>(v[u][k]);
            } else {  // the chunk's last, partial tile
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t e0 = base + ((int64_t)u * kBlock + t) * W;
                    if (e0 + W <= len) {
                        const V v = *reinterpret_cast<const V *>(p + e0);
#pragma unroll
                        for (int k = 0; k < W; ++k) x[u][k] = widen<T, A>(v[k]);
                    } else {
#pragma unroll
                        for (int k = 0; k < W; ++k) x[u][k] = e0 + k < len ? widen<T, A>(p[e0 + k]) : id;
                    }
                }
            }
            A before[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
#pragma unroll
                for (int k = 1; k < W; ++k) x[u][k] = fold<A, K>(x[u][k - 1], x[u][k]);
                before[u] = wave_scan(segment_prev(x[u][W - 1], 64, lane, id), lane, id, fold<A, K>);
            }
            if (lane == kWaveTotalLane) {
#pragma unroll
                for (int u = 0; u < U; ++u) totals[buf][u][w] = fold<A, K>(before[u], x[u][W - 1]);
            }
            __syncthreads();
            // the (slot, wave) totals in the tile's order: what lies before this wave's part of slot u, and the new carry
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < kWaves; ++k) {
                    if (k == w) before[u] = fold<A, K>(carry, before[u]);
                    carry = fold<A, K>(carry, totals[buf][u][k]);
                }
            buf ^= 1;  // the next tile writes the other buffer: one barrier per tile is enough
            if constexpr (!TOTAL) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int64_t e0 = base + ((int64_t)u * kBlock + t) * W;
                    if (e0 + W <= len) {
                        V o;
#pragma unroll
                        for (int k = 0; k < W; ++k) o[k] = finish<T, A>(fold<A, K>(before[u], x[u][k]), 0.0);
                        SMHIP_SCAN_STORE(reinterpret_cast<V *>(q + e0), o, pol);
                    } else {
#pragma unroll
                        for (int k = 0; k < W; ++k)
                            if (e0 + k < len) q[e0 + k] = finish<T, A>(fold<A, K>(before[u], x[u][k]), 0.0);
                    }
                }
            }
        }
        if (TOTAL && t == 0) part[row * C + c] = carry;
    }
}

// ---- COLUMN: workgroup task (o, chunk c, strip) covers columns [strip * 64, strip * 64 + 64) of outer index o and walks rows
// [c*CL, c*CL + CL) in blocks of 16 x U rows.  Lane (ty, tx) of the 16 x 16 workgroup owns columns i0 .. i0 + 3 (quad tx of the
// strip; 16 lanes read 256 contiguous bytes of a row) and rows ty*U .. ty*U + U - 1 of the block: it loads them all, scans
// down them with 4 accumulators, and leaves its 4 totals in LDS.  After ONE barrier (the buffer alternates) every lane folds,
// in row order, the totals of the lanes above it onto the running value of its columns and stores its rows.  The loads of a
// block do not depend on the carry, and a launch has 16 times the lanes of a walk with one lane per quad.
// TOTAL and `part` ([O][C][I]) as in row_long_kernel: lane ty folds a run of consecutive chunks' totals, the 16 runs meet in LDS.
constexpr int kColTX = 16, kColTY = kBlock / kColTX;
constexpr int kColStrip = 4 * kColTX;  // columns per workgroup
template <typename T> struct ColRows { static constexpr int value = sizeof(T) == 4 ? 16 : 8; };  // 256 bytes per lane in flight
template <typename T, int K, bool TOTAL>
__global__ __launch_bounds__(kBlock) void column_kernel(const T *a, T *out, int64_t O, int64_t R, int64_t I, int64_t CL, int64_t C,
                                                        typename Acc<T, K>::type *part, int pol) {
    typedef typename Acc<T, K>::type A;
    typedef typename Quad<T>::type Q;
    constexpr int U = ColRows<T>::value;
    const A id = identity<A, K>();
    const int t = threadIdx.x, tx = t % kColTX, ty = t / kColTX;
    const int64_t strips = (I + kColStrip - 1) / kColStrip, tasks = O * C * strips;
    __shared__ A totals[2][kColTY][kColTX][4];
    int buf = 0;
    for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {  // workgroup-uniform
        const int64_t oc = task / strips, strip = task - oc * strips, o = oc / C, c = oc - o * C;
        const int64_t i0 = strip * kColStrip + tx * 4;
        const int live = (int)std::max<int64_t>(0, std::min<int64_t>(4, I - i0));  // 0: a lane beyond the last column
        const int64_t r0 = c * CL, r1 = std::min(R, r0 + CL);
        const T *p = a + o * R * I + i0;
        T *q = out + o * R * I + i0;
        A carry[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) carry[k] = id;
        if (!TOTAL && part && c > 0) {  // workgroup-uniform
            const int64_t per = (c + kColTY - 1) / kColTY, c0 = std::min<int64_t>(c, ty * per), c1 = std::min<int64_t>(c, c0 + per);
            const A *pp = part + o * C * I + i0;
            A v[4] = {id, id, id, id};
            for (int64_t cc = c0; cc < c1; ++cc)
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < live) v[k] = fold<A, K>(v[k], pp[cc * I + k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) totals[buf][ty][tx][k] = v[k];
            __syncthreads();
#pragma unroll
            for (int y = 0; y < kColTY; ++y)
#pragma unroll
                for (int k = 0; k < 4; ++k) carry[k] = fold<A, K>(carry[k], totals[buf][y][tx][k]);
            buf ^= 1;
        }
        for (int64_t rb = r0; rb < r1; rb += kColTY * U) {
            const int64_t my0 = rb + ty * U;
            A x[U][4];
            if (live == 4) {
                Q v[U];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (my0 + u < r1) {
                        const Q *s = reinterpret_cast<const Q *>(p + (my0 + u) * I);
                        v[u] = (pol & kLoadNt) ? __builtin_nontemporal_load(s) : *s;
                    }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int k = 0; k < 4; ++k) x[u][k] = my0 + u < r1 ? widen<T, A>(v[u][k]) : id;
            } else {  // the last 1 .. 3 columns, or none
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int k = 0; k < 4; ++k) x[u][k] = (k < live && my0 + u < r1) ? widen<T, A>(p[(my0 + u) * I + k]) : id;
            }
#pragma unroll
            for (int u = 1; u < U; ++u)
#pragma unroll
                for (int k = 0; k < 4; ++k) x[u][k] = fold<A, K>(x[u - 1][k], x[u][k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) totals[buf][ty][tx][k] = x[U - 1][k];
            __syncthreads();
            A before[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) before[k] = carry[k];
#pragma unroll 2  // (fully unrolled, the 64 LDS values are all kept in registers: 260 VGPRs, one wave per SIMD)
            for (int y = 0; y < kColTY; ++y)
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    carry[k] = fold<A, K>(carry[k], totals[buf][y][tx][k]);
                    before[k] = y < ty ? carry[k] : before[k];  // what lies above this lane's rows
                }
            buf ^= 1;  // the next block writes the other buffer: one barrier per block is enough
            if constexpr (!TOTAL) {
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    if (my0 + u >= r1) continue;
                    if (live == 4) {
                        Q res;
#pragma unroll
                        for (int k = 0; k < 4; ++k) res[k] = finish<T, A>(fold<A, K>(before[k], x[u][k]), 0.0);
                        SMHIP_SCAN_STORE(reinterpret_cast<Q *>(q + (my0 + u) * I), res, pol);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < live) q[(my0 + u) * I + k] = finish<T, A>(fold<A, K>(before[k], x[u][k]), 0.0);
                    }
                }
            }
        }
        if (TOTAL && ty == 0) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < live) part[(o * C + c) * I + i0 + k] = carry[k];
        }
    }
}

// ------------------------------------------------------------------------------------------------------ the planner
struct Plan {
    int route = SMHIP_SCAN_ROUTE_NONE;
    bool copy = false;
    int launches = 0;
    int64_t O = 0, R = 0, I = 0;
    int64_t C = 1, CL = 0;  // chunks of R (C > 1: two launches) and their length
    int g = 0;              // ROW: lanes per row (4, 16, 64), 0 = a workgroup per row
    int code() const { return route | (C > 1 ? SMHIP_SCAN_SPLIT : 0) | (copy ? SMHIP_SCAN_COPY : 0); }
};

void make_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, Plan *pl) {
    *pl = Plan();
    int64_t O = 1, I = 1;
    for (int d = 0; d < ndim; ++d) {
        if (d < axis) O *= shape[d];
        if (d > axis) I *= shape[d];
    }
    const int64_t R = shape[axis];
    pl->O = O, pl->R = R, pl->I = I, pl->CL = R;
    if (O * R * I == 0) return;
    if (R == 1) {
        pl->route = SMHIP_SCAN_ROUTE_COPYONLY, pl->launches = 1;
        return;
    }
    pl->copy = !row_major(shape, strides, ndim);
    const int64_t W = vec_width(dtype);
    if (I == 1) {
        pl->route = SMHIP_SCAN_ROUTE_ROW;
        pl->g = segment_lanes(row_loads(R, W));
        if (pl->g == 0 && O < kRowSplitBelowRows) {
            const int64_t tile = (int64_t)kBlock * kTileVecs * W;
            const int64_t want = std::min({ceil_div(kRowSplitBelowRows, O), R / tile, kRowMaxChunks});  // a chunk: at least a tile
            if (want > 1) {
                pl->CL = ceil_div(ceil_div(R, want), tile) * tile;
                pl->C = ceil_div(R, pl->CL);
            }
        }
    } else {
        pl->route = SMHIP_SCAN_ROUTE_COLUMN;
        const int64_t groups = O * ceil_div(I, kColStrip);
        if (groups < kColumnSplitBelowGroups) {
            const int64_t block = kColTY * (W == 4 ? ColRows<float>::value : ColRows<double>::value);  // rows of a workgroup's block
            const int64_t want = std::min({ceil_div(kColumnTargetGroups, groups), R / block, kColumnMaxChunks});  // a chunk: at least a block
            if (want > 1) {
                pl->CL = ceil_div(ceil_div(R, want), block) * block;
                pl->C = ceil_div(R, pl->CL);
            }
        }
    }
    pl->launches = (pl->copy ? 1 : 0) + (pl->C > 1 ? 2 : 1);
}

// ------------------------------------------------------------------------------------------------------ launching
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_SCAN_GRID_CAP")); return g; }  // the cap of every launch here, read once

template <typename T, int K>
int run_scan(const Plan &pl, const T *in, T *out, hipStream_t s) {
    typedef typename Acc<T, K>::type A;
    const size_t bytes = (size_t)(pl.O * pl.R * pl.I) * sizeof(T);
    const int pol = stream_policy({{in, bytes}}, {out, bytes});
    A *part = nullptr;
    ScratchLease lease;
    if (pl.C > 1) {
        double *buf;
        if (int rc = lease.take((size_t)(pl.O * pl.C * pl.I), &buf)) return rc;  // sizeof(A) <= 8
        part = reinterpret_cast<A *>(buf);
    }
    if (pl.route == SMHIP_SCAN_ROUTE_ROW && pl.g > 0) {
        const int64_t per_wave = kRowsInFlight * (64 / pl.g), waves = ceil_div(pl.O, per_wave);
        hipLaunchKernelGGL((row_short_kernel<T, K>), dim3(grid_cap().blocks_for(waves)), dim3(kBlock), 0, s, in, out, pl.O, pl.R, pl.g, pol);
    } else if (pl.route == SMHIP_SCAN_ROUTE_ROW) {
        const dim3 grid(grid_cap().capped(pl.O * pl.C));
        if (pl.C > 1) {
            hipLaunchKernelGGL((row_long_kernel<T, K, true>), grid, dim3(kBlock), 0, s, in, out, pl.O, pl.R, pl.CL, pl.C, part, pol);
            SMHIP_LAUNCH_CHECK("scan_axis totals");
        }
        hipLaunchKernelGGL((row_long_kernel<T, K, false>), grid, dim3(kBlock), 0, s, in, out, pl.O, pl.R, pl.CL, pl.C, part, pol);
    } else {
        const dim3 grid(grid_cap().capped(pl.O * pl.C * ceil_div(pl.I, kColStrip)));
        if (pl.C > 1) {
            hipLaunchKernelGGL((column_kernel<T, K, true>), grid, dim3(kBlock), 0, s, in, out, pl.O, pl.R, pl.I, pl.CL, pl.C, part, pol);
            SMHIP_LAUNCH_CHECK("scan_axis totals");
        }
        hipLaunchKernelGGL((column_kernel<T, K, false>), grid, dim3(kBlock), 0, s, in, out, pl.O, pl.R, pl.I, pl.CL, pl.C, part, pol);
    }
    SMHIP_LAUNCH_CHECK("scan_axis");
    return SMHIP_OK;
}

template <typename T>
int run_kind(int kind, const Plan &pl, const void *in, void *out, hipStream_t s) {
    const T *pi = static_cast<const T *>(in);
    T *po = static_cast<T *>(out);
    switch (kind) {
        case SMHIP_SCAN_SUM: return run_scan<T, kSum>(pl, pi, po, s);
        case SMHIP_SCAN_PROD: return run_scan<T, kProd>(pl, pi, po, s);
        case SMHIP_SCAN_MAX: return run_scan<T, kMax>(pl, pi, po, s);
        case SMHIP_SCAN_MIN: return run_scan<T, kMin>(pl, pi, po, s);
    }
    return fail(SMHIP_ERR_INVALID, "scan_axis: bad kind %d", kind);
}

// Validation: everything that can be said without a device.
int scan_axis_check(const char *who, int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis) {
    if (kind < SMHIP_SCAN_SUM || kind > SMHIP_SCAN_MIN) return fail(SMHIP_ERR_INVALID, "%s: bad kind %d", who, kind);
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (int rc = check_axis(who, axis, ndim)) return rc;
    return check_extents(who, shape, strides, ndim);
}

void scan_axis_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, int *route, int *launches, int64_t *ori3,
                    int64_t *chunk) {
    Plan pl;
    make_plan(dtype, shape, strides, ndim, axis, &pl);
    if (route) *route = pl.code();
    if (launches) *launches = pl.launches;
    if (ori3) ori3[0] = pl.O, ori3[1] = pl.R, ori3[2] = pl.I;
    if (chunk) *chunk = pl.CL;
}

int launch_scan_axis(int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, void *out,
                     hipStream_t s) {
    Plan pl;
    make_plan(dtype, shape, strides, ndim, axis, &pl);
    if (pl.route == SMHIP_SCAN_ROUTE_NONE) return SMHIP_OK;
    if (pl.route == SMHIP_SCAN_ROUTE_COPYONLY) {
        int64_t dense[SMHIP_MAX_NDIM];
        axis_plan::dense_strides(shape, ndim, dense);
        return a == out ? SMHIP_OK : launch_copy_strided(dtype, a, strides, out, dense, shape, ndim, s);
    }
    axis_plan::Pooled copy;
    const void *in = a;
    if (pl.copy)
        if (int rc = copy.dense_copy(dtype, a, shape, strides, ndim, s, &in)) return rc;
    switch (dtype) {
        case SMHIP_F32: return run_kind<float>(kind, pl, in, out, s);
        case SMHIP_F64: return run_kind<double>(kind, pl, in, out, s);
        case SMHIP_I32: return run_kind<int32_t>(kind, pl, in, out, s);
        case SMHIP_I64: return run_kind<int64_t>(kind, pl, in, out, s);
    }
    return fail(SMHIP_ERR_INVALID, "scan_axis: bad dtype %d", dtype);
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_scan_axis(int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, void *out) {
    if (int rc = scan_axis_check("scan_axis", kind, dtype, shape, strides, ndim, axis)) return rc;
    const int64_t n = element_count(shape, ndim);
    const bool dense = axis_plan::row_major(shape, strides, ndim);
    if (n == 0) return SMHIP_OK;
    if (!a || !out) return fail(SMHIP_ERR_INVALID, "scan_axis: null buffer");
    if (!(out == a && dense)) {  // in place is the one overlap a scan can take: a lane stores only what it has loaded itself
        const size_t esz = dtype_size(dtype);
        if (spans_overlap(Span{a, span_bytes(shape, strides, ndim, esz)}, Span{out, (size_t)n * esz}))
            return fail(SMHIP_ERR_INVALID, "scan_axis: the result overlaps the operand (only out == a with a dense operand is allowed)");
    }
    SMHIP_ACQUIRE(s);  // undeclared spans (a pooled copy, the chunks' totals): ordered behind everything, recorded tiny operators flushed first
    return launch_scan_axis(kind, dtype, a, shape, strides, ndim, axis, out, s);
}

int smhip_scan_plan(int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, int *route, int *launches,
                    int64_t *ori3, int64_t *chunk) {
    if (int rc = scan_axis_check("scan_plan", kind, dtype, shape, strides, ndim, axis)) return rc;
    scan_axis_plan(dtype, shape, strides, ndim, axis, route, launches, ori3, chunk);
    return SMHIP_OK;
}
