// softmax_axis.hip -- softmax, log_softmax and logsumexp along one axis, fused per line (smhip_softmax_axis): an axis reduction whose
// result has the operand's shape (LOGSUMEXP: the reduction's).  f32 and f64.
//
// The contract and the error bounds are smhip.h's ("softmax"); the per-line arithmetic is sm_softmax.h's, shared with the host
// check: the maximum m of a line (a NaN propagates), e_r = exp(x_r - m) with the difference in fp64, S = the fp64 sum of the e_r,
// and e_r / S, (x_r - m) - ln S or m + ln S formed in fp64 and rounded once.  Every sum runs in a fixed order: a lane's elements in
// index order, the lanes of a wave through wave.hip.h's DPP folds, the waves of a workgroup and the chunks of a line in rising
// order.  No float atomics, so the bits depend on kind, dtype and the merged layout alone, not on the run, the stream or the grid.
//
// Planner (host only; smhip_softmax_plan reports it), with axis_plan.h's merging over out[o, r, i] <- a[o*so + r*sr + i*si]:
//   ROW      I = 1, sr = 1, and the result's lines contiguous too.
//     held   R <= L: ONE launch, one read, one write.  A row of at most 64 loads (its 16-byte vectors, then R % W elements one
//            per lane) takes a segment of 4 / 16 / 64 lanes with one vector a lane (row_small_kernel); a row of at most 256 vectors a
//            wave with 4 vectors a lane, a longer one a workgroup with 8 (row_held_kernel): the line stays in registers between the
//            maximum, the sum and the store.  L = 256 lanes * 8 vectors: 8192 floats, 4096 doubles.
//     SPLIT  R > L: the line is cut into C chunks of CL <= L elements (split_row: more of them when the lines are few).  Launch 1 is
//            row_held_kernel on the chunks, writing a pair (m_c, S_c) each into a pooled fp64 buffer; launch 2 (combine_kernel)
//            folds a line's pairs in chunk order, S = sum S_c exp(m_c - m) with the factor by the f64 exp, and leaves (m, S or ln S)
//            per line -- or the LOGSUMEXP result, which ends there; launch 3 (row_apply_kernel) reads x again and writes.
//   COLUMN   I > 1, si = 1 (the first or a middle axis; softmax(A.T, -1) read in place): a lane owns the 16 bytes of W consecutive
//            columns and walks R three times -- maximum, sum, store (column_kernel) -- so the traffic is three reads; the second and
//            third walk of a short column come from the cache.  SPLIT (split_column, when the lanes are few): the same kernel folds
//            chunks of R into pairs, combine_kernel as above, and the kernel's third walk writes.
//   COPY     no unit stride in the walk, a stepped or stride-0 axis, result lines that are not contiguous for ROW: the operand is
//            copied dense through the pool first and takes one of the routes above.
//   FILL     LOGSUMEXP over an empty axis: every result -inf.   NONE  nothing to write.
// Every kernel loops over its tasks under a capped grid (SMHIP_SOFTMAX_GRID_CAP); all index arithmetic is int64.
#include <stdlib.h>

#include <algorithm>
#include <limits>
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "internal.h"
#include "sm_softmax.h"
#include "wave.hip.h"

namespace smhip {
namespace {

using namespace axis_plan;  // kBlock, Canon, GridCap, Pooled and the planner's rules
using namespace smsoftmax;  // the per-line arithmetic

constexpr int kWaves = kBlock / 64;
constexpr int kWaveVecs = 4, kBlockVecs = 8;  // 16-byte vectors a lane holds: a wave per line, a workgroup per line

// W consecutive elements (16 bytes) at any element-aligned address (gfx950 takes 16-byte accesses there).
template <typename T> struct VecOf;
template <> struct VecOf<float> { typedef float type __attribute__((ext_vector_type(4), aligned(4))); static constexpr int W = 4; };
template <> struct VecOf<double> { typedef double type __attribute__((ext_vector_type(2), aligned(8))); static constexpr int W = 2; };
template <typename T> constexpr int64_t line_limit() { return (int64_t)kBlock * kBlockVecs * VecOf<T>::W; }  // L

template <typename T> __device__ __forceinline__ T neg_inf() { return -std::numeric_limits<T>::infinity(); }
__device__ __forceinline__ double plus(double x, double y) { return x + y; }
__device__ __forceinline__ int64_t dev_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// The f64 exp's {T, tail} table (2 KiB) in LDS, staged once per workgroup; the f32 exp has none.
template <typename T> struct ExpTab {
    static constexpr int kDoubles = std::is_same<T, double>::value ? smpow64::kExpTabDoubles : 1;
    smpow64::TabAoS tab;
    __device__ __forceinline__ void init(double *lds) {
        tab.logtab = nullptr, tab.exptab = lds;
        if constexpr (std::is_same<T, double>::value) {
            for (int i = threadIdx.x; i < kDoubles; i += kBlock) lds[i] = smpow64::kExpTab[i];
            __syncthreads();
        }
    }
};

// e[k] = exp(x[k] - m[k]) for W elements; returns their sum in index order.
template <typename T, int W> __device__ __forceinline__ double exps(const T (&x)[W], const double (&m)[W], T (&e)[W], const ExpTab<T> &et) {
    double d[W];
#pragma unroll
    for (int k = 0; k < W; ++k) d[k] = (double)x[k] - m[k];
    if constexpr (std::is_same<T, float>::value) exp_diff_n<W>(d, e);
    else exp_diff_n<W>(d, e, et.tab);
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < W; ++k) s += (double)e[k];
    return s;
}
template <typename T, int W> __device__ __forceinline__ double exps(const T (&x)[W], double m, T (&e)[W], const ExpTab<T> &et) {
    double mm[W];
#pragma unroll
    for (int k = 0; k < W; ++k) mm[k] = m;
    return exps<T, W>(x, mm, e, et);
}
// One element of SOFTMAX (from e) or LOG_SOFTMAX (from x): `fin` = S or ln S.  (The kernels' operand and result pointers carry no
// __restrict__: out == a is the in-place form.)
template <typename T> __device__ __forceinline__ T finish_elem(int kind, bool sp, T x, T e, double m, double fin) {
    if (sp) return special_value<T>(kind, (T)m);
    return kind == kSoftmax ? finish_softmax<T>(e, fin) : finish_log_softmax<T>((double)x - m, fin);
}
template <typename T> __device__ __forceinline__ T finish_line(bool sp, double m, double S) { return sp ? (T)m : finish_logsumexp<T>(m, log_sum(S)); }

// ---- ROW, rows of at most 64 loads: a segment of g = 4, 16 or 64 lanes per row, one load per lane.
template <typename T>
__global__ __launch_bounds__(kBlock) void row_small_kernel(const T *a, int64_t rows, int64_t so, int R, int g, int kind, T *out, int64_t oo) {
    typedef typename VecOf<T>::type V;
    constexpr int W = VecOf<T>::W;
    __shared__ __attribute__((aligned(16))) double exp_lds[ExpTab<T>::kDoubles];
    ExpTab<T> et;
    et.init(exp_lds);
    const int lane = threadIdx.x & 63, sl = lane & (g - 1), last = lane | (g - 1);
    const int64_t segs = 64 / g, waves = dev_ceil_div(rows, segs), grid_waves = (int64_t)gridDim.x * kWaves;
    const int nvec = R / W, tail = R - nvec * W;
    for (int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); wave < waves; wave += grid_waves) {  // wave-uniform
        const int64_t row = wave * segs + lane / g;
        const bool live = row < rows;
        T x[W], e[W];
#pragma unroll
        for (int k = 0; k < W; ++k) x[k] = neg_inf<T>();
        if (live) {
            if (sl < nvec) {
                const V v = *reinterpret_cast<const V *>(a + row * so + (int64_t)sl * W);
#pragma unroll
                for (int k = 0; k < W; ++k) x[k] = v[k];
            } else if (sl < nvec + tail) {
                x[0] = a[row * so + (int64_t)nvec * W + (sl - nvec)];
            }
        }
        T mx = x[0];
#pragma unroll
        for (int k = 1; k < W; ++k) mx = line_max(mx, x[k]);
        mx = dev::segment_fold(mx, g, neg_inf<T>(), line_max<T>);
        const double m = (double)__shfl(mx, last);
        const bool sp = special(m);
        double s = exps<T, W>(x, sp ? 0.0 : m, e, et);
        s = dev::segment_fold(s, g, 0.0, plus);
        const double S = __shfl(s, last);
        if (!live) continue;
        if (kind == kLogSumExp) {
            if (sl == 0) out[row * oo] = finish_line<T>(sp, m, S);
            continue;
        }
        const double fin = kind == kSoftmax ? S : log_sum(sp ? 1.0 : S);
        if (sl < nvec) {
            V v;
#pragma unroll
            for (int k = 0; k < W; ++k) v[k] = finish_elem<T>(kind, sp, x[k], e[k], m, fin);
            *reinterpret_cast<V *>(out + row * oo + (int64_t)sl * W) = v;
        } else if (sl < nvec + tail) {
            out[row * oo + (int64_t)nvec * W + (sl - nvec)] = finish_elem<T>(kind, sp, x[0], e[0], m, fin);
        }
    }
}

// ---- ROW, a line (or a chunk of a line) of at most G * NV vectors held in registers: G = 64, a wave per task, or G = kBlock, a
// workgroup per task.  Task (line, c) is elements [c*CL, min(R, c*CL + CL)) of the line.  pairs == null (C = 1): the results are
// written; else the chunk's pair (m_c, S_c) goes to pairs[2 * task].
template <typename T, int G, int NV>
__global__ __launch_bounds__(kBlock) void row_held_kernel(const T *a, int64_t lines, int64_t so, int64_t R, int64_t CL, int64_t C, int kind,
                                                          T *out, int64_t oo, double *__restrict__ pairs) {
    typedef typename VecOf<T>::type V;
    constexpr int W = VecOf<T>::W;
    constexpr bool kWave = G == 64;
    static_assert(G == 64 || G == kBlock, "a wave or the workgroup");
    __shared__ __attribute__((aligned(16))) double exp_lds[ExpTab<T>::kDoubles];
    __shared__ T lds_m[kWaves];
    __shared__ double lds_s[kWaves];
    ExpTab<T> et;
    et.init(exp_lds);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, gl = kWave ? lane : (int)threadIdx.x;  // the lane's number in its group
    const int64_t tasks = lines * C;
    const int64_t first = kWave ? (int64_t)blockIdx.x * kWaves + wave : (int64_t)blockIdx.x, step = kWave ? (int64_t)gridDim.x * kWaves : (int64_t)gridDim.x;
    for (int64_t task = first; task < tasks; task += step) {  // group-uniform
        const int64_t line = task / C, c = task - line * C, start = c * CL;
        const int len = (int)std::min<int64_t>(CL, R - start), nvec = len / W, tail = len - nvec * W;
        const T *p = a + line * so + start;
        V v[NV];
        T xt[1] = {neg_inf<T>()}, et1[1];
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int q = u * G + gl;
            if (q < nvec) {
                v[u] = *reinterpret_cast<const V *>(p + (int64_t)q * W);
            } else {
#pragma unroll
                for (int k = 0; k < W; ++k) v[u][k] = neg_inf<T>();
            }
        }
        if (gl < tail) xt[0] = p[(int64_t)nvec * W + gl];
        T mx = xt[0];
#pragma unroll
        for (int u = 0; u < NV; ++u)
            if (u * G < nvec) {
#pragma unroll
                for (int k = 0; k < W; ++k) mx = line_max(mx, v[u][k]);
            }
        mx = dev::segment_fold(mx, 64, neg_inf<T>(), line_max<T>);
        double m;
        if constexpr (kWave) {
            m = (double)__shfl(mx, dev::kWaveTotalLane);
        } else {
            if (lane == dev::kWaveTotalLane) lds_m[wave] = mx;
            __syncthreads();
            T t = lds_m[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) t = line_max(t, lds_m[w]);
            m = (double)t;
        }
        const bool sp = special(m);
        const double ms = sp ? 0.0 : m;
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < NV; ++u)
            if (u * G < nvec) {
                T x[W], e[W];
#pragma unroll
                for (int k = 0; k < W; ++k) x[k] = v[u][k];
                s += exps<T, W>(x, ms, e, et);
                if (kind == kSoftmax) {
#pragma unroll
                    for (int k = 0; k < W; ++k) v[u][k] = e[k];
                }
            }
        s += exps<T, 1>(xt, ms, et1, et);
        s = dev::segment_fold(s, 64, 0.0, plus);
        double S;
        if constexpr (kWave) {
            S = __shfl(s, dev::kWaveTotalLane);
        } else {
            if (lane == dev::kWaveTotalLane) lds_s[wave] = s;
            __syncthreads();
            S = lds_s[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) S += lds_s[w];
        }
        if (pairs) {
            if (gl == 0) pairs[2 * task] = m, pairs[2 * task + 1] = sp ? 0.0 : S;
            continue;
        }
        if (kind == kLogSumExp) {
            if (gl == 0) out[line * oo] = finish_line<T>(sp, m, S);
            continue;
        }
        const double fin = kind == kSoftmax ? S : log_sum(sp ? 1.0 : S);
        T *po = out + line * oo + start;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int q = u * G + gl;
            if (q < nvec) {
                V r;
#pragma unroll
                for (int k = 0; k < W; ++k) r[k] = finish_elem<T>(kind, sp, v[u][k], v[u][k], m, fin);
                *reinterpret_cast<V *>(po + (int64_t)q * W) = r;
            }
        }
        if (gl < tail) po[(int64_t)nvec * W + gl] = finish_elem<T>(kind, sp, xt[0], et1[0], m, fin);
    }
}

// ---- SPLIT: the pairs of a line into one.  Line (o, i) of `lines` = O * I has its chunk c's pair at pairs[2 * ((o*C + c)*I + i)]
// (ROW: I = 1).  A segment of g = 1, 4, 16 or 64 lanes per line: lane sl takes chunks sl, sl + g, ... in rising order, the lanes are
// folded by DPP -- a fixed order.  LOGSUMEXP writes its result to out[o*oso + i*osi]; the others leave stat[2 * line] = {m, S or ln S}.
template <typename T>
__global__ __launch_bounds__(kBlock) void combine_kernel(const double *__restrict__ pairs, int64_t lines, int64_t C, int64_t I, int g, int kind,
                                                         double *__restrict__ stat, T *out, int64_t oso, int64_t osi) {
    const int lane = threadIdx.x & 63, sl = lane & (g - 1), last = lane | (g - 1);
    const int64_t segs = 64 / g, waves = dev_ceil_div(lines, segs), grid_waves = (int64_t)gridDim.x * kWaves;
    for (int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); wave < waves; wave += grid_waves) {  // wave-uniform
        const int64_t line = wave * segs + lane / g;
        const bool live = line < lines;
        const int64_t o = line / I, i = line - o * I, base = o * C * I + i;
        double mx = -std::numeric_limits<double>::infinity();
        if (live)
            for (int64_t c = sl; c < C; c += g) mx = line_max(mx, pairs[2 * (base + c * I)]);
        mx = dev::segment_fold(mx, g, -std::numeric_limits<double>::infinity(), line_max<double>);
        const double m = __shfl(mx, last);
        const bool sp = special(m);
        double s = 0.0;
        if (live && !sp)
            for (int64_t c = sl; c < C; c += g) s += rescale(pairs[2 * (base + c * I)], pairs[2 * (base + c * I) + 1], m);
        s = dev::segment_fold(s, g, 0.0, plus);
        if (live && sl == g - 1) {
            if (kind == kLogSumExp) out[o * oso + i * osi] = finish_line<T>(sp, m, s);
            else stat[2 * line] = m, stat[2 * line + 1] = sp ? 0.0 : kind == kSoftmax ? s : log_sum(s);
        }
    }
}

// ---- ROW SPLIT, the last launch: chunk (line, c) again, a workgroup per task, with the line's {m, S or ln S} from stat.
template <typename T>
__global__ __launch_bounds__(kBlock) void row_apply_kernel(const T *a, int64_t lines, int64_t so, int64_t R, int64_t CL, int64_t C, int kind,
                                                           const double *__restrict__ stat, T *out, int64_t oo) {
    typedef typename VecOf<T>::type V;
    constexpr int W = VecOf<T>::W;
    __shared__ __attribute__((aligned(16))) double exp_lds[ExpTab<T>::kDoubles];
    ExpTab<T> et;
    et.init(exp_lds);
    const int64_t tasks = lines * C;
    for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {
        const int64_t line = task / C, c = task - line * C, start = c * CL;
        const int len = (int)std::min<int64_t>(CL, R - start), nvec = len / W, tail = len - nvec * W;
        const T *p = a + line * so + start;
        T *po = out + line * oo + start;
        const double m = stat[2 * line], fin = stat[2 * line + 1];
        const bool sp = special(m);
        const double ms = sp ? 0.0 : m;
        for (int q = threadIdx.x; q < nvec; q += kBlock) {
            const V v = *reinterpret_cast<const V *>(p + (int64_t)q * W);
            T x[W], e[W] = {};
#pragma unroll
            for (int k = 0; k < W; ++k) x[k] = v[k];
            if (kind == kSoftmax) exps<T, W>(x, ms, e, et);
            V r;
#pragma unroll
            for (int k = 0; k < W; ++k) r[k] = finish_elem<T>(kind, sp, x[k], e[k], m, fin);
            *reinterpret_cast<V *>(po + (int64_t)q * W) = r;
        }
        if ((int)threadIdx.x < tail) {
            T x[1] = {p[(int64_t)nvec * W + threadIdx.x]}, e[1];
            exps<T, 1>(x, ms, e, et);
            po[(int64_t)nvec * W + threadIdx.x] = finish_elem<T>(kind, sp, x[0], e[0], m, fin);
        }
    }
}

// ---- COLUMN: lane (o, c, q) owns columns i0 = q*W .. i0 + W - 1 of outer index o and rows [c*CL, c*CL + CL) of R, numbered with q
// fastest and packed without gaps.  phase 0: the whole column (C = 1) -- maximum, sum, store.  phase 1: the chunk's pairs.
// phase 2: the store, with the column's {m, S or ln S} from stat.  Results at out[o*oo + r*orr + i*oi] (LOGSUMEXP: o*oo + i*oi).
enum ColumnPhase { kColumnWhole = 0, kColumnFold = 1, kColumnApply = 2 };
template <typename T>
__global__ __launch_bounds__(kBlock) void column_kernel(const T *a, int64_t O, int64_t so, int64_t R, int64_t sr, int64_t I, int64_t CL, int64_t C,
                                                        int kind, int phase, T *out, int64_t oo, int64_t orr, int64_t oi,
                                                        double *__restrict__ pairs, const double *__restrict__ stat) {
    typedef typename VecOf<T>::type V;
    constexpr int W = VecOf<T>::W;
    __shared__ __attribute__((aligned(16))) double exp_lds[ExpTab<T>::kDoubles];
    ExpTab<T> et;
    et.init(exp_lds);
    const int64_t nq = dev_ceil_div(I, W), lanes = O * C * nq, grid_lanes = (int64_t)gridDim.x * kBlock;
    for (int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x; l < lanes; l += grid_lanes) {
        const int64_t oc = l / nq, i0 = (l - oc * nq) * W, o = oc / C, c = oc - o * C;
        const int64_t r0 = c * CL, r1 = std::min(R, r0 + CL);
        const int live = (int)std::min<int64_t>(W, I - i0);
        const T *p = a + o * so + i0;
        auto load = [&](int64_t r, T (&x)[W]) {
            if (live == W) {
                const V v = *reinterpret_cast<const V *>(p + r * sr);
#pragma unroll
                for (int k = 0; k < W; ++k) x[k] = v[k];
            } else {
#pragma unroll
                for (int k = 0; k < W; ++k) x[k] = k < live ? p[r * sr + k] : neg_inf<T>();
            }
        };
        T x[W], e[W] = {};
        double m[W], ms[W], fin[W];
        bool sp[W];
        if (phase == kColumnApply) {
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const int64_t line = o * I + std::min<int64_t>(i0 + k, I - 1);
                m[k] = stat[2 * line], fin[k] = stat[2 * line + 1];
            }
        } else {
            T mx[W];
#pragma unroll
            for (int k = 0; k < W; ++k) mx[k] = neg_inf<T>();
            for (int64_t r = r0; r < r1; ++r) {
                load(r, x);
#pragma unroll
                for (int k = 0; k < W; ++k) mx[k] = line_max(mx[k], x[k]);
            }
#pragma unroll
            for (int k = 0; k < W; ++k) m[k] = (double)mx[k], fin[k] = 0.0;
        }
#pragma unroll
        for (int k = 0; k < W; ++k) sp[k] = special(m[k]), ms[k] = sp[k] ? 0.0 : m[k];
        if (phase != kColumnApply) {
            for (int64_t r = r0; r < r1; ++r) {  // the sums, each column's in row order
                load(r, x);
                exps<T, W>(x, ms, e, et);
#pragma unroll
                for (int k = 0; k < W; ++k) fin[k] += (double)e[k];
            }
            if (phase == kColumnFold) {
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if (k < live) {
                        const int64_t at = 2 * ((o * C + c) * I + i0 + k);
                        pairs[at] = m[k], pairs[at + 1] = sp[k] ? 0.0 : fin[k];
                    }
                continue;
            }
            if (kind == kLogSumExp) {
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if (k < live) out[o * oo + (i0 + k) * oi] = finish_line<T>(sp[k], m[k], fin[k]);
                continue;
            }
            if (kind == kLogSoftmax) {
#pragma unroll
                for (int k = 0; k < W; ++k) fin[k] = log_sum(sp[k] ? 1.0 : fin[k]);
            }
        }
        T *po = out + o * oo + i0 * oi;
        for (int64_t r = r0; r < r1; ++r) {
            load(r, x);
            if (kind == kSoftmax) exps<T, W>(x, ms, e, et);
            V res;
#pragma unroll
            for (int k = 0; k < W; ++k) res[k] = finish_elem<T>(kind, sp[k], x[k], e[k], m[k], fin[k]);
            if (live == W && oi == 1) {
                *reinterpret_cast<V *>(po + r * orr) = res;
            } else {
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if (k < live) po[r * orr + k * oi] = res[k];
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------------ the planner
struct Plan {
    int route = SMHIP_SOFTMAX_ROUTE_NONE;
    bool copy = false, split = false;
    Canon c;                       // the walk, over the operand or its dense copy
    int64_t O = 1, R = 1, I = 1;   // ori3
    int64_t orr = 1;               // SOFTMAX / LOG_SOFTMAX: the result's stride along the axis
    int64_t total = 0, results = 0;
    int g = 0;                     // ROW: lanes per row (4, 16, 64), 0 = a wave or a workgroup per line
    bool wave = false;             // ROW held: a wave per line
    int64_t C = 1, CL = 0;         // chunks of R and their length
    int64_t L = 0;
    int reads = 0, levels = 0, launches = 0;
    int code() const { return route | (split ? SMHIP_SOFTMAX_SPLIT : 0) | (copy ? SMHIP_SOFTMAX_COPY : 0); }
};

// The walk of a view, read in place: ROW / COLUMN, or kWalkNone when it must be copied dense first.
Walk walk_of(int kind, const int64_t *shape, const int64_t *strides, int ndim, int axis, Canon *c, int64_t *orr) {
    int64_t dense[SMHIP_MAX_NDIM];
    const int64_t total = dense_strides(shape, ndim, dense);
    for (int d = 0; d < ndim; ++d)
        if (shape[d] > 1 && strides[d] == 0) return kWalkNone;
    *orr = dense[axis];
    if (shape[axis] == 1) {  // every element a line of its own: the dense operand as `total` rows of 1
        if (!row_major(shape, strides, ndim)) return kWalkNone;
        *c = Canon();
        c->O = total, c->so = 1, c->oso = 1, *orr = 1;
        return kWalkRow;
    }
    Ax ax[SMHIP_MAX_NDIM];
    // SOFTMAX / LOG_SOFTMAX write the operand's shape: kept axes merge where the FULL dense result runs on; LOGSUMEXP the reduction's
    const int n = merge_axes(shape, strides, ndim, 1u << axis, false, ax, kind == kLogSumExp ? nullptr : dense);
    const Walk w = canonical(ax, n, c);
    if (w == kWalkRow && kind != kLogSumExp && *orr != 1) return kWalkNone;  // the result's lines would be strided
    return w;
}

void make_plan(int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    int64_t before_n = 1, after_n = 1;
    for (int d = 0; d < ndim; ++d) {
        if (d < axis) before_n *= shape[d];
        if (d > axis) after_n *= shape[d];
    }
    p.R = shape[axis], p.O = before_n, p.I = after_n, p.total = before_n * after_n * p.R;
    p.results = kind == kLogSumExp ? before_n * after_n : p.total;
    p.L = dtype == SMHIP_F64 ? line_limit<double>() : line_limit<float>();
    if (p.results == 0) return;
    if (p.R == 0) {  // LOGSUMEXP over nothing
        p.route = SMHIP_SOFTMAX_ROUTE_FILL, p.launches = 1;
        return;
    }
    Walk w = walk_of(kind, shape, strides, ndim, axis, &p.c, &p.orr);
    if (w == kWalkNone) {
        int64_t dense[SMHIP_MAX_NDIM];
        dense_strides(shape, ndim, dense);
        p.copy = true;
        w = walk_of(kind, shape, dense, ndim, axis, &p.c, &p.orr);  // a dense array always has one
    }
    if (p.R > 1) p.O = p.c.O, p.I = p.c.I;
    const int64_t W = vec_width(dtype);
    const int finish = kind == kLogSumExp ? 0 : 1;  // SPLIT: the launch that writes
    if (w == kWalkRow) {
        p.route = SMHIP_SOFTMAX_ROUTE_ROW;
        p.g = segment_lanes(row_loads(p.R, W));
        if (p.g == 0 && p.R > p.L) {
            const Split sp = split_row(p.c.O * kBlock, p.R, kBlock * W, p.L);
            p.split = true, p.C = sp.C, p.CL = sp.CL;
        } else {
            p.CL = p.R, p.wave = p.R <= 64 * kWaveVecs * W;
        }
    } else {
        p.route = SMHIP_SOFTMAX_ROUTE_COLUMN;
        const Split sp = split_column(p.c.O * ceil_div(p.c.I, W), p.R);
        p.CL = p.R;
        if (sp.CL) p.split = true, p.C = sp.C, p.CL = sp.CL;
    }
    p.reads = w == kWalkColumn ? 3 : p.split ? 2 : 1;
    p.levels = p.split ? 2 : 1;
    p.launches = (p.copy ? 1 : 0) + p.levels + (p.split ? finish : 0);
}

// ------------------------------------------------------------------------------------------------------ launching
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_SOFTMAX_GRID_CAP")); return g; }  // the cap of every launch here, read once

template <typename T>
int run_plan(const Plan &p, int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, void *out_v, hipStream_t s) {
    Pooled copy_pool, pair_pool;
    const T *in = static_cast<const T *>(a);
    T *out = static_cast<T *>(out_v);
    if (p.copy) {
        const void *dense;
        if (int rc = copy_pool.dense_copy(dtype, a, shape, strides, ndim, s, &dense)) return rc;
        in = static_cast<const T *>(dense);
    }
    const Canon &c = p.c;
    const bool row = p.route == SMHIP_SOFTMAX_ROUTE_ROW;
    const int64_t lines = c.O * c.I;
    double *pairs = nullptr, *stat = nullptr;
    if (p.split) {
        void *raw;
        if (int rc = pair_pool.take((size_t)(2 * lines * p.C + 2 * lines) * sizeof(double), &raw)) return rc;
        pairs = static_cast<double *>(raw), stat = pairs + 2 * lines * p.C;
    }
    const int64_t tasks = lines * p.C;
    if (row) {
        if (p.g) {
            hipLaunchKernelGGL((row_small_kernel<T>), dim3(grid_cap().blocks_for(ceil_div(c.O, 64 / p.g))), dim3(kBlock), 0, s, in, c.O, c.so, (int)p.R, p.g, kind, out, c.oso);
        } else if (p.wave) {
            hipLaunchKernelGGL((row_held_kernel<T, 64, kWaveVecs>), dim3(grid_cap().blocks_for(tasks)), dim3(kBlock), 0, s, in, c.O, c.so, p.R, p.CL, p.C, kind, out, c.oso,
                               (double *)nullptr);
        } else {
            hipLaunchKernelGGL((row_held_kernel<T, kBlock, kBlockVecs>), dim3(grid_cap().capped(tasks)), dim3(kBlock), 0, s, in, c.O, c.so, p.R, p.CL, p.C, kind, out,
                               c.oso, pairs);
        }
        SMHIP_LAUNCH_CHECK("softmax_axis row");
    } else {
        const int64_t lanes = c.O * p.C * ceil_div(c.I, VecOf<T>::W);
        hipLaunchKernelGGL((column_kernel<T>), dim3(grid_cap().capped(ceil_div(lanes, kBlock))), dim3(kBlock), 0, s, in, c.O, c.so, p.R, c.sr, c.I, p.CL, p.C, kind,
                           p.split ? (int)kColumnFold : (int)kColumnWhole, out, c.oso, p.orr, c.osi, pairs, (const double *)nullptr);
        SMHIP_LAUNCH_CHECK("softmax_axis column");
    }
    if (!p.split) return SMHIP_OK;
    const int g = p.C <= 1 ? 1 : p.C <= 4 ? 4 : p.C <= 16 ? 16 : 64;
    hipLaunchKernelGGL((combine_kernel<T>), dim3(grid_cap().blocks_for(ceil_div(lines, 64 / g))), dim3(kBlock), 0, s, (const double *)pairs, lines, p.C, c.I, g, kind, stat,
                       out, c.oso, c.osi);
    SMHIP_LAUNCH_CHECK("softmax_axis combine");
    if (kind == kLogSumExp) return SMHIP_OK;
    if (row) {
        hipLaunchKernelGGL((row_apply_kernel<T>), dim3(grid_cap().capped(tasks)), dim3(kBlock), 0, s, in, c.O, c.so, p.R, p.CL, p.C, kind, (const double *)stat, out, c.oso);
    } else {
        const int64_t lanes = c.O * p.C * ceil_div(c.I, VecOf<T>::W);
        hipLaunchKernelGGL((column_kernel<T>), dim3(grid_cap().capped(ceil_div(lanes, kBlock))), dim3(kBlock), 0, s, in, c.O, c.so, p.R, c.sr, c.I, p.CL, p.C, kind,
                           (int)kColumnApply, out, c.oso, p.orr, c.osi, (double *)nullptr, (const double *)stat);
    }
    SMHIP_LAUNCH_CHECK("softmax_axis apply");
    return SMHIP_OK;
}

int launch_softmax_axis(int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, void *out, hipStream_t s) {
    Plan pl;
    make_plan(kind, dtype, shape, strides, ndim, axis, &pl);
    if (pl.route == SMHIP_SOFTMAX_ROUTE_NONE) return SMHIP_OK;
    if (pl.route == SMHIP_SOFTMAX_ROUTE_FILL) {
        const float f = -std::numeric_limits<float>::infinity();
        const double d = -std::numeric_limits<double>::infinity();
        return launch_fill(dtype, out, dtype == SMHIP_F64 ? (const void *)&d : (const void *)&f, (size_t)pl.results, s);
    }
    if (dtype == SMHIP_F64) return run_plan<double>(pl, kind, dtype, a, shape, strides, ndim, out, s);
    return run_plan<float>(pl, kind, dtype, a, shape, strides, ndim, out, s);
}

// Validation: everything that can be said without a device or a pointer.
int softmax_check(const char *who, int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis) {
    if (kind < SMHIP_SOFTMAX || kind > SMHIP_LOGSUMEXP) return fail(SMHIP_ERR_INVALID, "%s: bad kind %d", who, kind);
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (dtype != SMHIP_F32 && dtype != SMHIP_F64) return fail(SMHIP_ERR_UNSUPPORTED, "%s: an integer element type (f32 and f64 only)", who);
    if (int rc = check_axis(who, axis, ndim)) return rc;
    return check_extents(who, shape, strides, ndim);
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_softmax_axis(int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, void *out) {
    if (int rc = softmax_check("softmax_axis", kind, dtype, shape, strides, ndim, axis)) return rc;
    const int64_t total = element_count(shape, ndim);
    int64_t results = total;
    if (kind == SMHIP_LOGSUMEXP) {
        results = 1;
        for (int d = 0; d < ndim; ++d)
            if (d != axis) results *= shape[d];
    }
    if (results == 0) return SMHIP_OK;
    if (!out || (total && !a)) return fail(SMHIP_ERR_INVALID, "softmax_axis: null buffer");
    const size_t esz = dtype_size(dtype);
    const Span sa{a, total ? span_bytes(shape, strides, ndim, esz) : 0}, so{out, (size_t)results * esz};
    if (spans_overlap(sa, so) && !(kind != SMHIP_LOGSUMEXP && a == out && row_major(shape, strides, ndim)))
        return fail(SMHIP_ERR_INVALID, "softmax_axis: `out` overlaps the operand (only out == a with a dense operand, SOFTMAX or LOG_SOFTMAX, is in place)");
    SMHIP_ACQUIRE(s);  // undeclared spans (the pooled copy, the pairs): ordered behind everything, recorded tiny operators flushed first
    return launch_softmax_axis(kind, dtype, a, shape, strides, ndim, axis, out, s);
}

int smhip_softmax_plan(int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, int *route, int *launches, int64_t *ori3,
                       int64_t *info3) {
    if (int rc = softmax_check("softmax_plan", kind, dtype, shape, strides, ndim, axis)) return rc;
    Plan pl;
    make_plan(kind, dtype, shape, strides, ndim, axis, &pl);
    if (route) *route = pl.code();
    if (launches) *launches = pl.launches;
    if (ori3) ori3[0] = pl.O, ori3[1] = pl.R, ori3[2] = pl.I;
    if (info3) info3[0] = pl.L, info3[1] = pl.reads, info3[2] = pl.levels;
    return SMHIP_OK;
}
