// argreduce_axis.hip -- where the maximum / minimum along one axis stands, and optionally its value (smhip_argreduce_axis).
//
// The reference has nothing of the kind.  NumPy's np.argmax / np.argmin over `axis` is the contract: the FIRST position of the
// extreme along the axis, and the first NaN if there is one.  The fold runs on pairs (v, r) = (value, position along the axis):
//     a NaN beats a non-NaN; among two NaNs, or two equal values (-0 == +0), the smaller r wins; otherwise the larger
//     (ARG_MAX) or smaller (ARG_MIN) v wins.
// That combine is associative, commutative and idempotent, so the result -- index and value bits -- is the same whatever the
// partition of the work: no ordering has to be kept between lanes, waves, chunks or launches.
//
// Planner (host only; smhip_argreduce_plan reports it), by the shared rules of axis_plan.h.  Its merging: size-1 axes dropped,
// the rest ordered by stride, kept neighbours that are adjacent in memory and in the result merged.  The named axis is the
// only reduced one, so R is exactly that axis and r needs no unravelling.  [kept] R [kept] with a unit stride is the canonical
//     out[o, i] = arg_r a[o*so + r*sr + i*si]          (O, R, I)
// so argmax(A.T, 0) is the walk of argmax(A, 1).  A walk with no unit stride, a stride-0 axis, or kept axes that do not merge
// to one outer and one inner: the operand is copied dense first (smhip_copy_strided's kernels) and planned again.
// Routes (16-byte vector loads at any element-aligned address; segments and splits by axis_plan.h's rules, no chunk longer than 2^31):
//   ROW      I = 1, sr = 1.  Rows of at most 64 loads: a SEGMENT of g = 4, 16 or 64 lanes per row, four rows per segment in
//            flight.  Longer rows: a wave per (row, chunk), four vectors per lane in flight.
//   COLUMN   si = 1.  A lane owns 4 consecutive kept columns and walks R, four rows in flight; lanes packed over (o, chunk, quad).
//   SPLIT    when O x I leaves too few lanes, R is cut into chunks whose length depends on the shape alone; each chunk leaves
//            its (value, index) partial in pooled scratch, [O][I][chunk], and a finishing launch folds the partials (two
//            finishing launches when a row has more than kFinishWhole partials: the first folds runs of kFinishRun).
// Inside a lane the position is a 32-bit offset from the chunk's start (the planner keeps chunks within 2^31) and a lane
// meets its elements in rising order, so there a later element wins only when it is strictly better or the first NaN: two
// compares per element.  The offset is widened once, when the lane's pair leaves the kernel; everything that addresses
// memory is 64-bit.  Lanes meet through the pair form of the DPP fold (wave.hip.h: segment_fold_pair).  Every kernel loops
// over its tasks grid-stride under a capped grid (SMHIP_ARGREDUCE_GRID_CAP).  No atomics, no LDS.
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

constexpr int64_t kMaxChunk = (int64_t)1 << 31;     // a chunk's positions fit 32 bits
constexpr int64_t kFinishWhole = 4096, kFinishRun = 1024;  // partials a finishing wave folds: a whole row up to 4096, else runs of 1024
constexpr uint32_t kEmpty32 = 0xffffffffu;          // the position of a lane that holds no element: never preferred
constexpr int64_t kEmpty64 = std::numeric_limits<int64_t>::max();

// The value no element is worse than; beside kEmpty it is the pair fold's identity.
template <typename T, bool MAX> __device__ __forceinline__ T worst() { return identity<T, MAX ? kMax : kMin>(); }

// (av, ar) <- (bv, br) where b stands LATER along the axis than everything a has met: only a strictly better value or the
// first NaN replaces a.  A lane seeds a with (worst, its first position): an element equal to `worst` has worst's very bits.
template <typename T, bool MAX> __device__ __forceinline__ void take_later(T &av, uint32_t &ar, T bv, uint32_t br) {
    bool t;
    if constexpr (std::is_floating_point<T>::value) t = (MAX ? !(bv <= av) : !(bv >= av)) && av == av;
    else t = MAX ? bv > av : bv < av;
    av = t ? bv : av;
    ar = t ? br : ar;
}
// The pair combine in full, for pairs in any order.
template <typename T, bool MAX> struct Take {
    template <typename R> __device__ __forceinline__ void operator()(T &av, R &ar, T bv, R br) const {
        const bool better = MAX ? bv > av : bv < av, first = br < ar;
        bool t;
        if constexpr (std::is_floating_point<T>::value) {
            const bool an = av != av, bn = bv != bv;
            t = an ? (bn && first) : (bn || better || (bv == av && first));
        } else {
            t = better || (bv == av && first);
        }
        av = t ? bv : av;
        ar = t ? br : ar;
    }
};

// ---- ROW, short rows: a segment of g lanes per row, every row at most g loads (vectors, then the R % W tail elements one
// per lane).  A wave covers kRowsInFlight * 64 / g consecutive rows (stride so); row o's pair goes to out[o * oso].
template <typename T, bool MAX>
__global__ __launch_bounds__(kBlock) void row_short_kernel(const T *__restrict__ a, int64_t rows, int64_t so, int64_t R, int g,
                                                           int64_t *__restrict__ idx_out, T *__restrict__ val_out, int64_t oso, int nt) {
    typedef typename VecTraits<T>::vec_t V;
    constexpr int W = VecTraits<T>::width;
    const int lane = threadIdx.x & 63, seg_lane = lane & (g - 1);
    const int64_t segs = 64 / g;
    const int64_t nvec = R / W, tail = R - nvec * W;
    const bool is_vec = seg_lane < nvec, is_tail = !is_vec && seg_lane < nvec + tail;
    const uint32_t first = is_vec ? (uint32_t)seg_lane * W : is_tail ? (uint32_t)(nvec * W + (seg_lane - nvec)) : kEmpty32;
    const int64_t waves = (rows + kRowsInFlight * segs - 1) / (kRowsInFlight * segs), grid_waves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); wave < waves; wave += grid_waves) {  // wave-uniform
        const int64_t row0 = wave * kRowsInFlight * segs + lane / g;
        T bv[kRowsInFlight];
        uint32_t br[kRowsInFlight];
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) bv[u] = worst<T, MAX>(), br[u] = first;
        if (is_vec) {  // all loads of the lane issued before the first use
            V v[kRowsInFlight];
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) {
                const int64_t row = row0 + u * segs;
                if (row < rows) v[u] = load_stream_if(T, reinterpret_cast<const V *>(a + row * so + (int64_t)seg_lane * W), nt);
            }
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u)
                if (row0 + u * segs < rows) {
#pragma unroll
                    for (int k = 0; k < W; ++k) take_later<T, MAX>(bv[u], br[u], v[u][k], first + k);
                }
        } else if (is_tail) {
            T x[kRowsInFlight];
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) {
                const int64_t row = row0 + u * segs;
                x[u] = row < rows ? a[row * so + first] : worst<T, MAX>();
            }
#pragma unroll
            for (int u = 0; u < kRowsInFlight; ++u) take_later<T, MAX>(bv[u], br[u], x[u], first);
        }
#pragma unroll
        for (int u = 0; u < kRowsInFlight; ++u) {  // all 64 lanes are here: the DPP moves need them
            segment_fold_pair(bv[u], br[u], g, worst<T, MAX>(), kEmpty32, Take<T, MAX>());
            const int64_t row = row0 + u * segs;
            if (seg_lane == g - 1 && row < rows) {
                idx_out[row * oso] = (int64_t)br[u];
                if (val_out) val_out[row * oso] = bv[u];
            }
        }
    }
}

// ---- ROW, long rows: a wave per (row, chunk of R); chunk length CL is a multiple of 4 * 64 vectors, so every chunk but a
// row's last is walked without guards, four vectors per lane in flight.  The pair of (row, chunk c) goes to out[row*oso + c*ocs].
template <typename T, bool MAX>
__global__ __launch_bounds__(kBlock) void row_long_kernel(const T *__restrict__ a, int64_t rows, int64_t so, int64_t R, int64_t CL, int64_t C,
                                                          int64_t *__restrict__ idx_out, T *__restrict__ val_out, OutMap om, int nt) {
    typedef typename VecTraits<T>::vec_t V;
    constexpr int W = VecTraits<T>::width;
    constexpr int U = 4;
    const int lane = threadIdx.x & 63;
    const int64_t tasks = rows * C, grid_waves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t task = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); task < tasks; task += grid_waves) {  // wave-uniform
        const int64_t row = task / C, c = task - row * C;
        const int64_t start = c * CL, len = std::min(CL, R - start);  // len <= 2^31
        const T *p = a + row * so + start;
        const V *pv = reinterpret_cast<const V *>(p);
        const int64_t nvec = len / W, tail = len - nvec * W;
        T bv = worst<T, MAX>();
        uint32_t br = lane < nvec ? (uint32_t)lane * W : lane < tail ? (uint32_t)(nvec * W) + lane : kEmpty32;  // the lane's first position
        uint32_t off = (uint32_t)lane * W;
        int64_t j = 0;
        for (; j + U * 64 <= nvec; j += U * 64) {
            V v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = load_stream_if(T, pv + j + u * 64 + lane, nt);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < W; ++k) take_later<T, MAX>(bv, br, v[u][k], off + (uint32_t)(u * 64 * W + k));
            off += U * 64 * W;
        }
        for (int64_t q = j + lane; q < nvec; q += 64) {
            const V v = load_stream_if(T, pv + q, nt);
#pragma unroll
            for (int k = 0; k < W; ++k) take_later<T, MAX>(bv, br, v[k], (uint32_t)(q * W) + k);
        }
        if (lane < tail) take_later<T, MAX>(bv, br, p[nvec * W + lane], (uint32_t)(nvec * W) + lane);
        segment_fold_pair(bv, br, 64, worst<T, MAX>(), kEmpty32, Take<T, MAX>());
        if (lane == kWaveTotalLane) {
            const int64_t at = row * om.oso + c * om.ocs;
            idx_out[at] = start + (int64_t)br;
            if (val_out) val_out[at] = bv;
        }
    }
}

// ---- COLUMN: a lane owns kept columns i0 .. i0 + 3 of outer index o and walks rows [c*CL, c*CL + CL) of R, four rows in
// flight.  Lanes are numbered (o, c, quad) with the quad fastest and packed without gaps.  Grid-stride over the lanes.
template <typename T, bool MAX>
__global__ __launch_bounds__(kBlock) void column_kernel(const T *__restrict__ a, int64_t O, int64_t so, int64_t R, int64_t sr, int64_t I,
                                                        int64_t CL, int64_t C, int64_t *__restrict__ idx_out, T *__restrict__ val_out, OutMap om, int nt) {
    typedef typename Quad<T>::type Q;
    constexpr int U = 4;
    const int64_t nq = (I + 3) / 4, lanes = O * C * nq, grid_lanes = (int64_t)gridDim.x * kBlock;
    for (int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x; l < lanes; l += grid_lanes) {
        const int64_t oc = l / nq, i0 = (l - oc * nq) * 4, o = oc / C, c = oc - o * C;
        const int64_t r0 = c * CL, r1 = std::min(R, r0 + CL);  // r0 < r1, r1 - r0 <= 2^31
        const T *p = a + o * so + i0 + r0 * sr;
        const int64_t n = r1 - r0;
        T bv[4];
        uint32_t br[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) bv[k] = worst<T, MAX>(), br[k] = 0;
        if (i0 + 4 <= I) {
            int64_t r = 0;
            for (; r + U <= n; r += U) {
                Q v[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const Q *q = reinterpret_cast<const Q *>(p + (r + u) * sr);
                    v[u] = (nt & kLoadNt) ? __builtin_nontemporal_load(q) : *q;
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int k = 0; k < 4; ++k) take_later<T, MAX>(bv[k], br[k], v[u][k], (uint32_t)r + u);
            }
            for (; r < n; ++r) {
                const Q v = *reinterpret_cast<const Q *>(p + r * sr);
#pragma unroll
                for (int k = 0; k < 4; ++k) take_later<T, MAX>(bv[k], br[k], v[k], (uint32_t)r);
            }
        } else {
            const int live = (int)(I - i0);  // 1 .. 3 columns
            for (int64_t r = 0; r < n; ++r)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < live) take_later<T, MAX>(bv[k], br[k], p[r * sr + k], (uint32_t)r);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (i0 + k < I) {
                const int64_t at = o * om.oso + (i0 + k) * om.osi + c * om.ocs;
                idx_out[at] = r0 + (int64_t)br[k];
                if (val_out) val_out[at] = bv[k];
            }
    }
}

// ---- finishing: row j of the partials holds C pairs (pv, pi)[j*C .. j*C + C); a wave per (row, run of FL of them), four
// loads per lane in flight, the pairs in any order (the full combine).  Pair (row, run c) goes to
// out[(row / I2)*oso + (row % I2)*osi + c*ocs].
template <typename T, bool MAX>
__global__ __launch_bounds__(kBlock) void finish_kernel(const T *__restrict__ pv, const int64_t *__restrict__ pi, int64_t rows, int64_t C, int64_t FL,
                                                        int64_t C2, int64_t I2, int64_t *__restrict__ idx_out, T *__restrict__ val_out, OutMap om) {
    constexpr int U = 4;
    const int lane = threadIdx.x & 63;
    const Take<T, MAX> take{};
    const int64_t tasks = rows * C2, grid_waves = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t task = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); task < tasks; task += grid_waves) {  // wave-uniform
        const int64_t row = task / C2, c = task - row * C2;
        const int64_t begin = row * C + c * FL, end = row * C + std::min(C, c * FL + FL);
        T bv = worst<T, MAX>();
        int64_t br = kEmpty64;
        for (int64_t q = begin + lane; q < end; q += U * 64) {
            T v[U];
            int64_t r[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool in = q + u * 64 < end;
                v[u] = in ? pv[q + u * 64] : worst<T, MAX>();
                r[u] = in ? pi[q + u * 64] : kEmpty64;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) take(bv, br, v[u], r[u]);
        }
        segment_fold_pair(bv, br, 64, worst<T, MAX>(), kEmpty64, take);
        if (lane == kWaveTotalLane) {
            const int64_t o = row / I2, i = row - o * I2, at = o * om.oso + i * om.osi + c * om.ocs;
            idx_out[at] = br;
            if (val_out) val_out[at] = bv;
        }
    }
}

// ------------------------------------------------------------------------------------------------------ the planner
struct Plan : Canon {
    int route = SMHIP_ARG_ROUTE_NONE;
    bool copy = false;
    int launches = 0;
    int64_t C = 1, CL = 0;     // chunks of R (C > 1: finishing launches) and their length
    int g = 0;                 // ROW: lanes per row (4, 16, 64), 0 = a wave per (row, chunk)
    int64_t total = 0, nout = 0;
    int code() const { return route | (C > 1 ? SMHIP_ARG_SPLIT : 0) | (copy ? SMHIP_ARG_COPY : 0); }
};

// Splits and row segments; a chunk is never longer than kMaxChunk, and an unsplit walk's chunk is R.
void shape_plan(Plan &p, int dtype) {
    const int64_t W = vec_width(dtype);
    Split sp{1, 0};
    if (p.route == SMHIP_ARG_ROUTE_ROW) {
        p.g = segment_lanes(row_loads(p.R, W));
        if (p.g == 0) sp = split_row(p.O * 64, p.R, 4 * 64 * W, kMaxChunk);  // unit: one guard-free step of a wave
    } else {
        sp = split_column(p.O * ceil_div(p.I, 4), p.R, kMaxChunk);
    }
    p.C = 1, p.CL = p.R;
    if (sp.CL) p.C = sp.C, p.CL = sp.CL;
    p.launches = (p.copy ? 1 : 0) + 1 + (p.C > 1 ? (p.C > kFinishWhole ? 2 : 1) : 0);
}

void make_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    int64_t before = 1, after = 1;
    bool zero_stride = false;
    for (int d = 0; d < ndim; ++d) {
        if (d < axis) before *= shape[d];
        if (d > axis) after *= shape[d];
        if (shape[d] > 1 && strides[d] == 0) zero_stride = true;
    }
    p.R = shape[axis], p.nout = before * after, p.total = p.nout * p.R;
    p.O = before, p.I = after;
    if (p.total == 0) return;  // nothing to write (R = 0 with a result to write is refused by the checks)
    Ax ax[SMHIP_MAX_NDIM];
    const int n = merge_axes(shape, strides, ndim, 1u << axis, false, ax);
    Canon c;
    const Walk walk = zero_stride ? kWalkNone : canonical(ax, n, &c);
    if (walk != kWalkNone) {
        static_cast<Canon &>(p) = c;
        p.route = walk == kWalkRow ? SMHIP_ARG_ROUTE_ROW : SMHIP_ARG_ROUTE_COLUMN;
    } else {  // dense in index order (copied there first unless it already is; R = 1 comes here too)
        p.copy = zero_stride || !row_major(shape, strides, ndim);
        p.route = after == 1 ? SMHIP_ARG_ROUTE_ROW : SMHIP_ARG_ROUTE_COLUMN;
        p.so = p.R * after, p.sr = after, p.si = 1, p.oso = after, p.osi = 1;
    }
    shape_plan(p, dtype);
}

// ------------------------------------------------------------------------------------------------------ launching
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_ARGREDUCE_GRID_CAP")); return g; }  // the cap of every launch here, read once

template <typename T, bool MAX>
int run_plan(const Plan &p, const T *in, int64_t *idx_out, T *val_out, hipStream_t s) {
    const int nt = stream_policy({{in, (size_t)p.total * sizeof(T)}}, {nullptr, 0});
    if (p.route == SMHIP_ARG_ROUTE_ROW && p.g > 0) {
        const int64_t waves = ceil_div(p.O, kRowsInFlight * (64 / p.g));
        hipLaunchKernelGGL((row_short_kernel<T, MAX>), dim3(grid_cap().blocks_for(waves)), dim3(kBlock), 0, s, in, p.O, p.so, p.R, p.g, idx_out, val_out, p.oso, nt);
        SMHIP_LAUNCH_CHECK("argreduce_axis");
        return SMHIP_OK;
    }
    // the first launch writes the result when R is whole, the chunks' pairs ([O][I][chunk]) when it is split
    T *fv = val_out;
    int64_t *fi = idx_out;
    OutMap fm{p.oso, p.osi, 0};
    ScratchLease lease;
    const int64_t rows = p.O * p.I, C2 = p.C > kFinishWhole ? ceil_div(p.C, kFinishRun) : 0;  // C2: the pairs of the first finishing launch
    T *v2 = nullptr;
    int64_t *i2 = nullptr;
    if (p.C > 1) {
        const size_t pairs = (size_t)(rows * (p.C + C2));
        double *buf;
        if (int rc = lease.take(2 * pairs, &buf)) return rc;  // positions, then values (sizeof(T) <= 8)
        fi = reinterpret_cast<int64_t *>(buf), fv = reinterpret_cast<T *>(buf + pairs);
        i2 = fi + rows * p.C, v2 = fv + rows * p.C;
        fm = OutMap{p.I * p.C, p.C, 1};
    }
    if (p.route == SMHIP_ARG_ROUTE_ROW) {
        hipLaunchKernelGGL((row_long_kernel<T, MAX>), dim3(grid_cap().blocks_for(p.O * p.C)), dim3(kBlock), 0, s, in, p.O, p.so, p.R, p.CL, p.C, fi, fv, fm, nt);
    } else {
        const int64_t lanes = p.O * p.C * ceil_div(p.I, 4);
        hipLaunchKernelGGL((column_kernel<T, MAX>), dim3(grid_cap().capped(ceil_div(lanes, kBlock))), dim3(kBlock), 0, s, in, p.O, p.so, p.R, p.sr, p.I, p.CL, p.C, fi, fv, fm, nt);
    }
    SMHIP_LAUNCH_CHECK("argreduce_axis");
    if (p.C == 1) return SMHIP_OK;
    int64_t C = p.C;
    if (C2 > 0) {  // runs of kFinishRun pairs first: [rows][C] -> [rows][C2]
        hipLaunchKernelGGL((finish_kernel<T, MAX>), dim3(grid_cap().blocks_for(rows * C2)), dim3(kBlock), 0, s, fv, fi, rows, C, kFinishRun, C2, (int64_t)1, i2, v2, OutMap{C2, 0, 1});
        SMHIP_LAUNCH_CHECK("argreduce_axis finish");
        fv = v2, fi = i2, C = C2;
    }
    hipLaunchKernelGGL((finish_kernel<T, MAX>), dim3(grid_cap().blocks_for(rows)), dim3(kBlock), 0, s, fv, fi, rows, C, C, (int64_t)1, p.I, idx_out, val_out, OutMap{p.oso, p.osi, 0});
    SMHIP_LAUNCH_CHECK("argreduce_axis finish");
    return SMHIP_OK;
}

template <typename T>
int run_kind(int kind, const Plan &pl, const void *in, int64_t *idx_out, void *val_out, hipStream_t s) {
    if (kind == SMHIP_ARG_MAX) return run_plan<T, true>(pl, static_cast<const T *>(in), idx_out, static_cast<T *>(val_out), s);
    return run_plan<T, false>(pl, static_cast<const T *>(in), idx_out, static_cast<T *>(val_out), s);
}

// Validation: everything that can be said without a device or a pointer.
int argreduce_axis_check(const char *who, int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis) {
    if (kind != SMHIP_ARG_MAX && kind != SMHIP_ARG_MIN) return fail(SMHIP_ERR_INVALID, "%s: bad kind %d", who, kind);
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (int rc = check_axis(who, axis, ndim)) return rc;
    if (int rc = check_extents(who, shape, strides, ndim)) return rc;
    int64_t nout = 1;
    for (int d = 0; d < ndim; ++d)
        if (d != axis) nout *= shape[d];
    if (nout > 0 && shape[axis] == 0) return fail(SMHIP_ERR_INVALID, "%s: argmax / argmin over an empty extent", who);
    return SMHIP_OK;
}

void argreduce_axis_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, int *route, int *launches, int64_t *ori3,
                         int64_t *chunk) {
    Plan pl;
    make_plan(dtype, shape, strides, ndim, axis, &pl);
    if (route) *route = pl.code();
    if (launches) *launches = pl.launches;
    if (ori3) ori3[0] = pl.O, ori3[1] = pl.R, ori3[2] = pl.I;
    if (chunk) *chunk = pl.CL;
}

int launch_argreduce_axis(int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis,
                          int64_t *index_out, void *value_out, hipStream_t s) {
    Plan pl;
    make_plan(dtype, shape, strides, ndim, axis, &pl);
    if (pl.route == SMHIP_ARG_ROUTE_NONE) return SMHIP_OK;
    axis_plan::Pooled copy;
    const void *in = a;
    if (pl.copy)
        if (int rc = copy.dense_copy(dtype, a, shape, strides, ndim, s, &in)) return rc;
    switch (dtype) {
        case SMHIP_F32: return run_kind<float>(kind, pl, in, index_out, value_out, s);
        case SMHIP_F64: return run_kind<double>(kind, pl, in, index_out, value_out, s);
        case SMHIP_I32: return run_kind<int32_t>(kind, pl, in, index_out, value_out, s);
        case SMHIP_I64: return run_kind<int64_t>(kind, pl, in, index_out, value_out, s);
    }
    return fail(SMHIP_ERR_INVALID, "argreduce_axis: bad dtype %d", dtype);
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_argreduce_axis(int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, int64_t *index_out,
                         void *value_out) {
    if (int rc = argreduce_axis_check("argreduce_axis", kind, dtype, shape, strides, ndim, axis)) return rc;
    int64_t nout = 1;
    for (int d = 0; d < ndim; ++d)
        if (d != axis) nout *= shape[d];
    if (nout == 0) return SMHIP_OK;
    if (!a || !index_out) return fail(SMHIP_ERR_INVALID, "argreduce_axis: null buffer");
    const size_t esz = dtype_size(dtype);
    const Span sa{a, span_bytes(shape, strides, ndim, esz)}, si{index_out, (size_t)nout * sizeof(int64_t)}, sv{value_out, value_out ? (size_t)nout * esz : 0};
    if (spans_overlap(si, sa) || spans_overlap(sv, sa) || spans_overlap(si, sv))
        return fail(SMHIP_ERR_INVALID, "argreduce_axis: index_out / value_out overlap the operand or each other");
    // the operand's span and the index result are declared; the call still orders itself behind everything and everything
    // later behind it (a pooled copy, the chunks' pairs and value_out are not declared), recorded tiny operators flushed first
    hipStream_t s;
    OpScope op_scope_;
    if (int rc = op_scope_.begin(&sa, 1, si, &s, true)) return rc;
    return launch_argreduce_axis(kind, dtype, a, shape, strides, ndim, axis, index_out, value_out, s);
}

int smhip_argreduce_plan(int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, int *route, int *launches,
                         int64_t *ori3, int64_t *chunk) {
    if (int rc = argreduce_axis_check("argreduce_plan", kind, dtype, shape, strides, ndim, axis)) return rc;
    argreduce_axis_plan(dtype, shape, strides, ndim, axis, route, launches, ori3, chunk);
    return SMHIP_OK;
}
