// moments_axis.hip -- var, std, var_mean along chosen axes (smhip_moments_axes) and standardize along one (smhip_standardize_axis):
// centred second moments in fp64, f32 and f64.
//
// The contract and the error bounds are smhip.h's ("var / std / standardize"); the per-line arithmetic is sm_moments.h's, shared with
// the host check: mean = S / N from the fp64 sum S, d_k = x_k - mean in fp64, the pair (sum d, sum d^2), M2 = sum d^2 - (sum d)^2 / N,
// and the quotient, its square root or d_k / sqrt(var + eps) rounded once.  Every sum runs in a fixed order: a lane's elements in index
// order, the lanes of a wave through wave.hip.h's DPP folds, the chunks of a line in rising order.  No float atomics, so the bits
// depend on kind, dtype, ddof and the merged layout alone.
//
// S is ALWAYS the sum smhip_reduce_axes forms for the same call, in its order: that is what makes the mean output equal MEAN's bit
// for bit.  A held line sums its registers in the order of reduce's ROW kernels (a segment's lanes one load each; a wave's lane its
// vectors lane, lane + 64, ... and then a tail element; the DPP fold); every other route runs reduce's own walk first
// (launch_reduce_sum64: the sums left in fp64 in a pooled buffer).
//
// Planner (host only; smhip_moments_plan / smhip_standardize_plan report it), over out[o, i] <- a[o*so + r*sr + i*si]:
//   ROW held  I = 1, sr = 1, R <= L: ONE launch, one read.  A row of at most 64 loads takes a segment of 4 / 16 / 64 lanes
//             (row_small_kernel), a longer one a wave with 4 vectors a lane (row_wave_kernel): the line stays in registers between its
//             sum, the centred sums and the store.  L = 64 lanes * 4 vectors: 1024 floats, 512 doubles -- the longest line whose
//             register order IS reduce's (beyond it reduce cuts rows into wave-sized chunks by the number of rows).  standardize
//             writes y from the same registers.
//   not held  (ROW beyond L, COLUMN, CHANNEL): reduce's walk for S, then a second walk of the operand folding (sum d, sum d^2)
//             against S / N (row_pass_kernel: a wave per (row, chunk); column_pass_kernel: a lane per 16 bytes of columns and chunk of
//             rows -- CHANNEL is walked as COLUMN here), each chunk's pair into its own pooled slot, and finish_kernel folding a
//             line's pairs in chunk order and writing.  SPLIT: more than one chunk.  Two reads.
//   COPY      no unit stride, a stepped or stride-0 axis: the operand is copied dense first.  Several reduced groups that do not
//             merge: S by reduce's passes over the dense operand, then a second copy with the reduced axes innermost, walked as ROW.
//   UNIT      N = 1: the kept elements copied, then x - x in place (0, or NaN for a NaN or an infinity).
//   standardize, not held: the same three launches leave {mean, sqrt(var + eps)} per line in fp64; apply_row_kernel /
//             apply_column_kernel read x once more and write: three reads.
// Every kernel loops over its tasks under a capped grid (SMHIP_MOMENTS_GRID_CAP); all index arithmetic is int64.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <limits>
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "internal.h"
#include "sm_moments.h"
#include "wave.hip.h"

namespace smhip {
namespace {

using namespace axis_plan;  // kBlock, Canon, GridCap, Pooled and the planner's rules
using namespace smmoments;  // the per-line arithmetic

constexpr int kWaves = kBlock / 64;
constexpr int kWaveVecs = 4;  // 16-byte vectors a lane holds when a wave holds a line

// W consecutive elements (16 bytes) at any element-aligned address (gfx950 takes 16-byte accesses there).
template <typename T> struct VecOf;
template <> struct VecOf<float> { typedef float type __attribute__((ext_vector_type(4), aligned(4))); static constexpr int W = 4; };
template <> struct VecOf<double> { typedef double type __attribute__((ext_vector_type(2), aligned(8))); static constexpr int W = 2; };
template <typename T> constexpr int64_t line_limit() { return (int64_t)64 * kWaveVecs * VecOf<T>::W; }  // L

__device__ __forceinline__ double plus(double x, double y) { return x + y; }
__device__ __forceinline__ int64_t dev_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// What a launch finishes with: the kind, N and N - ddof as doubles, eps.
struct Fin { int kind; double N, divisor, eps; };

// ---- ROW held, rows of at most 64 loads: a segment of g = 4, 16 or 64 lanes per row, one load per lane (a vector, or one of the
// R % W tail elements).  VAR / STD: out[row * oo] (and mean[row * oo]); STANDARDIZE: the row at out + row * oo.
template <typename T>
__global__ __launch_bounds__(kBlock) void row_small_kernel(const T *a, int64_t rows, int64_t so, int R, int g, Fin f, T *out, int64_t oo, T *mean_out) {
    typedef typename VecOf<T>::type V;
    constexpr int W = VecOf<T>::W;
    const int lane = threadIdx.x & 63, sl = lane & (g - 1), last = lane | (g - 1);
    const int64_t segs = 64 / g, waves = dev_ceil_div(rows, segs), grid_waves = (int64_t)gridDim.x * kWaves;
    const int nvec = R / W, tail = R - nvec * W;
    for (int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); wave < waves; wave += grid_waves) {  // wave-uniform
        const int64_t row = wave * segs + lane / g;
        const bool live = row < rows;
        T x[W];
        int cnt = 0;  // the elements this lane holds
#pragma unroll
        for (int k = 0; k < W; ++k) x[k] = T(0);
        if (live) {
            if (sl < nvec) {
                const V v = *reinterpret_cast<const V *>(a + row * so + (int64_t)sl * W);
#pragma unroll
                for (int k = 0; k < W; ++k) x[k] = v[k];
                cnt = W;
            } else if (sl < nvec + tail) {
                x[0] = a[row * so + (int64_t)nvec * W + (sl - nvec)];
                cnt = 1;
            }
        }
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < W; ++k)
            if (k < cnt) acc = acc + (double)x[k];
        acc = dev::segment_fold(acc, g, 0.0, plus);
        const double S = __shfl(acc, last), mean = mean_of(S, f.N);
        Sums s = zero();
#pragma unroll
        for (int k = 0; k < W; ++k)
            if (k < cnt) add(s, centre(x[k], mean));
        s.sd = dev::segment_fold(s.sd, g, 0.0, plus);
        s.sq = dev::segment_fold(s.sq, g, 0.0, plus);
        const Sums t{__shfl(s.sd, last), __shfl(s.sq, last)};
        if (!live) continue;
        const double var = variance(t, f.N, f.divisor);
        if (f.kind != kStandardize) {
            if (sl == 0) {
                out[row * oo] = finish<T>(f.kind, var);
                if (mean_out) mean_out[row * oo] = finish_mean<T>(S, f.N);
            }
            continue;
        }
        const double den = denominator(var, f.eps);
        if (sl < nvec) {
            V v;
#pragma unroll
            for (int k = 0; k < W; ++k) v[k] = standardized<T>(centre(x[k], mean), den);
            *reinterpret_cast<V *>(out + row * oo + (int64_t)sl * W) = v;
        } else if (sl < nvec + tail) {
            out[row * oo + (int64_t)nvec * W + (sl - nvec)] = standardized<T>(centre(x[0], mean), den);
        }
    }
}

// ---- ROW held, a row of at most 64 * kWaveVecs vectors: a wave per row; lane l holds vectors l, l + 64, ... and tail element l.
template <typename T>
__global__ __launch_bounds__(kBlock) void row_wave_kernel(const T *a, int64_t rows, int64_t so, int R, Fin f, T *out, int64_t oo, T *mean_out) {
    typedef typename VecOf<T>::type V;
    constexpr int W = VecOf<T>::W;
    constexpr int NV = kWaveVecs;
    const int lane = threadIdx.x & 63;
    const int nvec = R / W, tail = R - nvec * W;
    const int64_t grid_waves = (int64_t)gridDim.x * kWaves;
    for (int64_t row = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); row < rows; row += grid_waves) {  // wave-uniform
        const T *p = a + row * so;
        V v[NV];
        T xt = T(0);
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int q = u * 64 + lane;
            if (q < nvec) {
                v[u] = *reinterpret_cast<const V *>(p + (int64_t)q * W);
            } else {
#pragma unroll
                for (int k = 0; k < W; ++k) v[u][k] = T(0);
            }
        }
        if (lane < tail) xt = p[(int64_t)nvec * W + lane];
        double acc = 0.0;
#pragma unroll
        for (int u = 0; u < NV; ++u)
            if (u * 64 + lane < nvec) {
#pragma unroll
                for (int k = 0; k < W; ++k) acc = acc + (double)v[u][k];
            }
        if (lane < tail) acc = acc + (double)xt;
        acc = dev::segment_fold(acc, 64, 0.0, plus);
        const double S = __shfl(acc, dev::kWaveTotalLane), mean = mean_of(S, f.N);
        Sums s = zero();
#pragma unroll
        for (int u = 0; u < NV; ++u)
            if (u * 64 + lane < nvec) {
#pragma unroll
                for (int k = 0; k < W; ++k) add(s, centre(v[u][k], mean));
            }
        if (lane < tail) add(s, centre(xt, mean));
        s.sd = dev::segment_fold(s.sd, 64, 0.0, plus);
        s.sq = dev::segment_fold(s.sq, 64, 0.0, plus);
        const Sums t{__shfl(s.sd, dev::kWaveTotalLane), __shfl(s.sq, dev::kWaveTotalLane)};
        const double var = variance(t, f.N, f.divisor);
        if (f.kind != kStandardize) {
            if (lane == 0) {
                out[row * oo] = finish<T>(f.kind, var);
                if (mean_out) mean_out[row * oo] = finish_mean<T>(S, f.N);
            }
            continue;
        }
        const double den = denominator(var, f.eps);
        T *po = out + row * oo;
#pragma unroll
        for (int u = 0; u < NV; ++u) {
            const int q = u * 64 + lane;
            if (q < nvec) {
                V r;
#pragma unroll
                for (int k = 0; k < W; ++k) r[k] = standardized<T>(centre(v[u][k], mean), den);
                *reinterpret_cast<V *>(po + (int64_t)q * W) = r;
            }
        }
        if (lane < tail) po[(int64_t)nvec * W + lane] = standardized<T>(centre(xt, mean), den);
    }
}

// ---- the second pass, ROW: a wave per (row, chunk c of CL elements); the row's fp64 sum at sum[row * ss].  The chunk's pair goes
// to pairs[2 * (row * C + c)].  Four vectors per lane in flight.
template <typename T>
__global__ __launch_bounds__(kBlock) void row_pass_kernel(const T *__restrict__ a, int64_t rows, int64_t so, int64_t R, int64_t CL, int64_t C,
                                                          const double *__restrict__ sum, int64_t ss, double N, double *__restrict__ pairs) {
    typedef typename VecOf<T>::type V;
    constexpr int W = VecOf<T>::W;
    constexpr int U = 4;
    const int lane = threadIdx.x & 63;
    const int64_t tasks = rows * C, grid_waves = (int64_t)gridDim.x * kWaves;
    for (int64_t task = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); task < tasks; task += grid_waves) {  // wave-uniform
        const int64_t row = task / C, c = task - row * C, start = c * CL, len = std::min(CL, R - start);
        const T *p = a + row * so + start;
        const int64_t nvec = len / W, tail = len - nvec * W;
        const double mean = mean_of(sum[row * ss], N);
        Sums s = zero();
        int64_t j = 0;
        for (; j + U * 64 <= nvec; j += U * 64) {
            V v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) v[u] = *reinterpret_cast<const V *>(p + (j + u * 64 + lane) * W);
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int k = 0; k < W; ++k) add(s, centre(v[u][k], mean));
        }
        for (int64_t q = j + lane; q < nvec; q += 64) {
            const V v = *reinterpret_cast<const V *>(p + q * W);
#pragma unroll
            for (int k = 0; k < W; ++k) add(s, centre(v[k], mean));
        }
        if (lane < tail) add(s, centre(p[nvec * W + lane], mean));
        s.sd = dev::segment_fold(s.sd, 64, 0.0, plus);
        s.sq = dev::segment_fold(s.sq, 64, 0.0, plus);
        if (lane == dev::kWaveTotalLane) pairs[2 * task] = s.sd, pairs[2 * task + 1] = s.sq;
    }
}

// ---- the second pass, COLUMN: lane (o, c, q) owns columns i0 = q*W .. i0 + W - 1 of outer index o and rows [c*CL, c*CL + CL) of R,
// numbered with q fastest.  Column (o, i)'s fp64 sum at sum[o*sso + i*ssi]; its chunk's pair at pairs[2 * ((o*I + i)*C + c)].
template <typename T>
__global__ __launch_bounds__(kBlock) void column_pass_kernel(const T *__restrict__ a, int64_t O, int64_t so, int64_t R, int64_t sr, int64_t I, int64_t CL,
                                                             int64_t C, const double *__restrict__ sum, int64_t sso, int64_t ssi, double N,
                                                             double *__restrict__ pairs) {
    typedef typename VecOf<T>::type V;
    constexpr int W = VecOf<T>::W;
    const int64_t nq = dev_ceil_div(I, W), lanes = O * C * nq, grid_lanes = (int64_t)gridDim.x * kBlock;
    for (int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x; l < lanes; l += grid_lanes) {
        const int64_t oc = l / nq, i0 = (l - oc * nq) * W, o = oc / C, c = oc - o * C;
        const int64_t r0 = c * CL, r1 = std::min(R, r0 + CL);
        const int live = (int)std::min<int64_t>(W, I - i0);
        const T *p = a + o * so + i0;
        double mean[W];
        Sums s[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            mean[k] = mean_of(sum[o * sso + std::min<int64_t>(i0 + k, I - 1) * ssi], N);
            s[k] = zero();
        }
        if (live == W) {
            for (int64_t r = r0; r < r1; ++r) {
                const V v = *reinterpret_cast<const V *>(p + r * sr);
#pragma unroll
                for (int k = 0; k < W; ++k) add(s[k], centre(v[k], mean[k]));
            }
        } else {
            for (int64_t r = r0; r < r1; ++r)
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if (k < live) add(s[k], centre(p[r * sr + k], mean[k]));
        }
#pragma unroll
        for (int k = 0; k < W; ++k)
            if (k < live) {
                const int64_t at = 2 * ((o * I + i0 + k) * C + c);
                pairs[at] = s[k].sd, pairs[at + 1] = s[k].sq;
            }
    }
}

// ---- the pairs of a line into its result.  Line (o, i) of `lines` = O * I has its C pairs at pairs[2 * (line * C)], its sum at
// sum[o*sso + i*ssi].  A segment of g = 1, 4, 16 or 64 lanes per line: lane sl takes chunks sl, sl + g, ... in rising order, the lanes
// are folded by DPP -- a fixed order.  VAR / STD write out (and mean_out) at [o*oso + i*osi]; STANDARDIZE leaves stat[2 * line] =
// {mean, sqrt(var + eps)}.
template <typename T>
__global__ __launch_bounds__(kBlock) void finish_kernel(const double *__restrict__ pairs, const double *__restrict__ sum, int64_t lines, int64_t C, int64_t I,
                                                        int g, Fin f, int64_t sso, int64_t ssi, T *__restrict__ out, T *__restrict__ mean_out, int64_t oso,
                                                        int64_t osi, double *__restrict__ stat) {
    const int lane = threadIdx.x & 63, sl = lane & (g - 1);
    const int64_t segs = 64 / g, waves = dev_ceil_div(lines, segs), grid_waves = (int64_t)gridDim.x * kWaves;
    for (int64_t wave = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); wave < waves; wave += grid_waves) {  // wave-uniform
        const int64_t line = wave * segs + lane / g;
        const bool live = line < lines;
        Sums s = zero();
        if (live)
            for (int64_t c = sl; c < C; c += g) s = merge(s, Sums{pairs[2 * (line * C + c)], pairs[2 * (line * C + c) + 1]});
        s.sd = dev::segment_fold(s.sd, g, 0.0, plus);
        s.sq = dev::segment_fold(s.sq, g, 0.0, plus);
        if (live && sl == g - 1) {
            const int64_t o = line / I, i = line - o * I;
            const double S = sum[o * sso + i * ssi], var = variance(s, f.N, f.divisor);
            if (f.kind == kStandardize) {
                stat[2 * line] = mean_of(S, f.N), stat[2 * line + 1] = denominator(var, f.eps);
            } else {
                out[o * oso + i * osi] = finish<T>(f.kind, var);
                if (mean_out) mean_out[o * oso + i * osi] = finish_mean<T>(S, f.N);
            }
        }
    }
}

// ---- standardize, not held, ROW: chunk (line, c) of CL elements, a workgroup per task, with the line's {mean, denominator} from stat.
// (Operand and result carry no __restrict__: out == a is the in-place form.)
template <typename T>
__global__ __launch_bounds__(kBlock) void apply_row_kernel(const T *a, int64_t lines, int64_t so, int64_t R, int64_t CL, int64_t C,
                                                           const double *__restrict__ stat, T *out, int64_t oo) {
    typedef typename VecOf<T>::type V;
    constexpr int W = VecOf<T>::W;
    const int64_t tasks = lines * C;
    for (int64_t task = blockIdx.x; task < tasks; task += gridDim.x) {
        const int64_t line = task / C, c = task - line * C, start = c * CL, len = std::min(CL, R - start);
        const int64_t nvec = len / W, tail = len - nvec * W;
        const T *p = a + line * so + start;
        T *po = out + line * oo + start;
        const double mean = stat[2 * line], den = stat[2 * line + 1];
        for (int64_t q = threadIdx.x; q < nvec; q += kBlock) {
            const V v = *reinterpret_cast<const V *>(p + q * W);
            V r;
#pragma unroll
            for (int k = 0; k < W; ++k) r[k] = standardized<T>(centre(v[k], mean), den);
            *reinterpret_cast<V *>(po + q * W) = r;
        }
        if ((int64_t)threadIdx.x < tail) po[nvec * W + threadIdx.x] = standardized<T>(centre(p[nvec * W + threadIdx.x], mean), den);
    }
}

// ---- standardize, not held, COLUMN: the lanes of column_pass_kernel; results at out[o*oo + r*orr + i*oi].
template <typename T>
__global__ __launch_bounds__(kBlock) void apply_column_kernel(const T *a, int64_t O, int64_t so, int64_t R, int64_t sr, int64_t I, int64_t CL, int64_t C,
                                                              const double *__restrict__ stat, T *out, int64_t oo, int64_t orr, int64_t oi) {
    typedef typename VecOf<T>::type V;
    constexpr int W = VecOf<T>::W;
    const int64_t nq = dev_ceil_div(I, W), lanes = O * C * nq, grid_lanes = (int64_t)gridDim.x * kBlock;
    for (int64_t l = (int64_t)blockIdx.x * kBlock + threadIdx.x; l < lanes; l += grid_lanes) {
        const int64_t oc = l / nq, i0 = (l - oc * nq) * W, o = oc / C, c = oc - o * C;
        const int64_t r0 = c * CL, r1 = std::min(R, r0 + CL);
        const int live = (int)std::min<int64_t>(W, I - i0);
        const T *p = a + o * so + i0;
        T *po = out + o * oo + i0 * oi;
        double mean[W], den[W];
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const int64_t line = o * I + std::min<int64_t>(i0 + k, I - 1);
            mean[k] = stat[2 * line], den[k] = stat[2 * line + 1];
        }
        for (int64_t r = r0; r < r1; ++r) {
            if (live == W && oi == 1) {
                const V v = *reinterpret_cast<const V *>(p + r * sr);
                V res;
#pragma unroll
                for (int k = 0; k < W; ++k) res[k] = standardized<T>(centre(v[k], mean[k]), den[k]);
                *reinterpret_cast<V *>(po + r * orr) = res;
            } else {
#pragma unroll
                for (int k = 0; k < W; ++k)
                    if (k < live) po[r * orr + k * oi] = standardized<T>(centre(p[r * sr + k], mean[k]), den[k]);
            }
        }
    }
}

// ---- UNIT (N = 1): p[i] <- the result of a line that is p[i] alone, in place.
template <typename T> __global__ __launch_bounds__(kBlock) void unit_kernel(T *p, int64_t n, Fin f) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const T x = p[i];
        Sums s = zero();
        const double d = centre(x, mean_of(0.0 + (double)x, 1.0));
        add(s, d);
        const double var = variance(s, 1.0, f.divisor);
        p[i] = f.kind == kStandardize ? standardized<T>(d, denominator(var, f.eps)) : finish<T>(f.kind, var);
    }
}

// ------------------------------------------------------------------------------------------------------ the planner
struct Plan {
    int route = SMHIP_MOMENTS_ROUTE_NONE;
    bool copy = false, split = false, held = false;  // copy: the dense copy of the view
    bool groups = false;          // several reduced groups: the copy with the reduced axes innermost
    Canon c;                      // the walk, over the operand or its dense copy
    int64_t orr = 1;              // standardize: the result's stride along the axis
    int64_t nout = 0, N = 0;
    int g = 0;                    // ROW held: lanes per row (4, 16, 64), 0 = a wave per row
    int64_t C = 1, CL = 0;        // chunks of R in the second pass and their length
    int64_t L = 0;
    int reads = 0, levels = 0, launches = 0;
    int code() const { return route | (split ? SMHIP_MOMENTS_SPLIT : 0) | (copy || groups ? SMHIP_MOMENTS_COPY : 0); }
};

int route_of(int reduce_code) {
    const int base = reduce_code & 0xff;
    return base == SMHIP_REDUCE_ROUTE_ROW ? SMHIP_MOMENTS_ROUTE_ROW : base == SMHIP_REDUCE_ROUTE_COLUMN ? SMHIP_MOMENTS_ROUTE_COLUMN : SMHIP_MOMENTS_ROUTE_CHANNEL;
}

// Held or not, and the chunks of the second pass.  `sum_launches`: what reduce's walk takes for S.
void shape_plan(Plan &p, int dtype, int sum_launches, bool standardize) {
    const int64_t W = vec_width(dtype);
    const bool row = p.route == SMHIP_MOMENTS_ROUTE_ROW;
    if (row && p.c.R <= p.L && !p.groups) {
        p.held = true, p.g = segment_lanes(row_loads(p.c.R, W));
        p.reads = 1, p.levels = 1, p.launches = (p.copy ? 1 : 0) + 1;
        return;
    }
    Split sp{1, 0};
    if (row) sp = split_row(p.c.O * 64, p.c.R, 4 * 64 * W);
    else sp = split_column(p.c.O * ceil_div(p.c.I, W), p.c.R);
    p.C = 1, p.CL = p.c.R;
    if (sp.CL) p.C = sp.C, p.CL = sp.CL;
    p.split = p.C > 1;
    p.reads = standardize ? 3 : 2, p.levels = 2;
    p.launches = (p.copy ? 1 : 0) + (p.groups ? 1 : 0) + sum_launches + 2 + (standardize ? 1 : 0);
}

void make_moments_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, uint32_t mask, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    int64_t nout = 1, N = 1;
    bool any_red = false;
    for (int d = 0; d < ndim; ++d) {
        ((mask >> d & 1) ? N : nout) *= shape[d];
        if ((mask >> d & 1) && shape[d] > 1) any_red = true;
    }
    p.nout = nout, p.N = N;
    p.L = dtype == SMHIP_F64 ? line_limit<double>() : line_limit<float>();
    if (nout == 0 || N == 0) return;
    if (!any_red) {
        p.route = SMHIP_MOMENTS_ROUTE_UNIT, p.c.O = nout, p.reads = 1, p.levels = 1, p.launches = 2;
        return;
    }
    int rc = 0, sum_launches = 0;
    int64_t ori[3], dense[SMHIP_MAX_NDIM];
    reduce_sum_plan(dtype, shape, strides, ndim, mask, &rc, &sum_launches, ori);
    const int64_t *st = strides;
    if (rc & SMHIP_REDUCE_COPY) {  // what reduce copies dense, this does too, and plans on the copy
        p.copy = true;
        dense_strides(shape, ndim, dense);
        st = dense;
        reduce_sum_plan(dtype, shape, dense, ndim, mask, &rc, &sum_launches, ori);
    }
    if (rc & SMHIP_REDUCE_PASSES) {  // the reduced axes innermost in a second copy: nout rows of N
        p.groups = true;
        p.route = SMHIP_MOMENTS_ROUTE_ROW;
        p.c = Canon();
        p.c.O = nout, p.c.R = N, p.c.so = N, p.c.oso = 1;
    } else {
        Ax ax[SMHIP_MAX_NDIM];
        const int n = merge_axes(shape, st, ndim, mask, false, ax);
        canonical(ax, n, &p.c);
        p.route = route_of(rc);
    }
    shape_plan(p, dtype, sum_launches, false);
}

// standardize's walk of a view, read in place: ROW / COLUMN, or kWalkNone when it must be copied dense first.  The kept axes merge
// where the FULL dense result runs on.
Walk standardize_walk(const int64_t *shape, const int64_t *strides, int ndim, int axis, Canon *c, int64_t *orr) {
    int64_t dense[SMHIP_MAX_NDIM];
    dense_strides(shape, ndim, dense);
    for (int d = 0; d < ndim; ++d)
        if (shape[d] > 1 && strides[d] == 0) return kWalkNone;
    *orr = dense[axis];
    Ax ax[SMHIP_MAX_NDIM];
    const int n = merge_axes(shape, strides, ndim, 1u << axis, false, ax, dense);
    const Walk w = canonical(ax, n, c);
    if (w == kWalkRow && *orr != 1) return kWalkNone;  // the result's lines would be strided
    return w;
}

// The walk (O, R, I) as the 3-D view reduce plans S on.
void canon_view(const Canon &c, int64_t *shape3, int64_t *strides3) {
    shape3[0] = c.O, shape3[1] = c.R, shape3[2] = c.I;
    strides3[0] = c.O > 1 ? c.so : 0, strides3[1] = c.sr, strides3[2] = c.I > 1 ? c.si : 0;
}

void make_standardize_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    const int64_t total = element_count(shape, ndim);
    p.N = shape[axis], p.nout = total;
    p.L = dtype == SMHIP_F64 ? line_limit<double>() : line_limit<float>();
    if (total == 0) return;
    if (p.N == 1) {
        p.route = SMHIP_MOMENTS_ROUTE_UNIT, p.c.O = total, p.reads = 1, p.levels = 1, p.launches = 2;
        return;
    }
    Walk w = standardize_walk(shape, strides, ndim, axis, &p.c, &p.orr);
    if (w == kWalkNone) {
        int64_t dense[SMHIP_MAX_NDIM];
        dense_strides(shape, ndim, dense);
        p.copy = true;
        w = standardize_walk(shape, dense, ndim, axis, &p.c, &p.orr);  // a dense array always has one
    }
    p.route = w == kWalkRow ? SMHIP_MOMENTS_ROUTE_ROW : SMHIP_MOMENTS_ROUTE_COLUMN;
    int sum_launches = 0;
    if (!(w == kWalkRow && p.c.R <= p.L)) {
        int64_t s3[3], t3[3], ori[3];
        int rc;
        canon_view(p.c, s3, t3);
        reduce_sum_plan(dtype, s3, t3, 3, 2u, &rc, &sum_launches, ori);
    }
    shape_plan(p, dtype, sum_launches, true);
}

// ------------------------------------------------------------------------------------------------------ launching
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_MOMENTS_GRID_CAP")); return g; }  // the cap of every launch here, read once

template <typename T> int run_held(const Plan &p, const T *in, Fin f, T *out, int64_t oo, T *mean_out, hipStream_t s) {
    const Canon &c = p.c;
    if (p.g) {
        hipLaunchKernelGGL((row_small_kernel<T>), dim3(grid_cap().blocks_for(ceil_div(c.O, 64 / p.g))), dim3(kBlock), 0, s, in, c.O, c.so, (int)c.R, p.g, f, out, oo, mean_out);
    } else {
        hipLaunchKernelGGL((row_wave_kernel<T>), dim3(grid_cap().blocks_for(c.O)), dim3(kBlock), 0, s, in, c.O, c.so, (int)c.R, f, out, oo, mean_out);
    }
    SMHIP_LAUNCH_CHECK("moments held");
    return SMHIP_OK;
}

// The second pass over the walk p.c of `in` and the finishing launch: S at sum[o*sso + i*ssi].
template <typename T>
int run_second(const Plan &p, const T *in, const double *sum, int64_t sso, int64_t ssi, Fin f, T *out, T *mean_out, int64_t oso, int64_t osi, double *stat,
               Pooled *pair_pool, hipStream_t s) {
    const Canon &c = p.c;
    const int64_t lines = c.O * c.I;
    void *raw;
    if (int rc = pair_pool->take((size_t)(2 * lines * p.C) * sizeof(double), &raw)) return rc;
    double *pairs = static_cast<double *>(raw);
    if (p.route == SMHIP_MOMENTS_ROUTE_ROW) {
        hipLaunchKernelGGL((row_pass_kernel<T>), dim3(grid_cap().blocks_for(lines * p.C)), dim3(kBlock), 0, s, in, c.O, c.so, c.R, p.CL, p.C, sum, sso, f.N, pairs);
    } else {
        const int64_t lanes = c.O * p.C * ceil_div(c.I, VecOf<T>::W);
        hipLaunchKernelGGL((column_pass_kernel<T>), dim3(grid_cap().capped(ceil_div(lanes, kBlock))), dim3(kBlock), 0, s, in, c.O, c.so, c.R, c.sr, c.I, p.CL, p.C, sum, sso,
                           ssi, f.N, pairs);
    }
    SMHIP_LAUNCH_CHECK("moments second pass");
    const int g = p.C <= 1 ? 1 : p.C <= 4 ? 4 : p.C <= 16 ? 16 : 64;
    hipLaunchKernelGGL((finish_kernel<T>), dim3(grid_cap().blocks_for(ceil_div(lines, 64 / g))), dim3(kBlock), 0, s, (const double *)pairs, sum, lines, p.C, c.I, g, f, sso,
                       ssi, out, mean_out, oso, osi, stat);
    SMHIP_LAUNCH_CHECK("moments finish");
    return SMHIP_OK;
}

template <typename T> int run_unit(T *p, int64_t n, Fin f, hipStream_t s) {
    hipLaunchKernelGGL((unit_kernel<T>), dim3(grid_cap().capped(ceil_div(n, kBlock))), dim3(kBlock), 0, s, p, n, f);
    SMHIP_LAUNCH_CHECK("moments unit");
    return SMHIP_OK;
}

template <typename T>
int run_moments(const Plan &p, int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, uint32_t mask, int64_t ddof, void *out_v,
                void *mean_v, hipStream_t s) {
    const Fin f{kind, (double)p.N, (double)(p.N - ddof), 0.0};
    T *out = static_cast<T *>(out_v), *mean_out = static_cast<T *>(mean_v);
    if (p.route == SMHIP_MOMENTS_ROUTE_UNIT) {  // the kept elements, as reduce's own copy of them
        int64_t ost[SMHIP_MAX_NDIM];
        dense_strides(shape, ndim, ost, ~mask);
        if (int rc = launch_copy_strided(dtype, a, strides, out, ost, shape, ndim, s)) return rc;
        if (mean_out)
            if (int rc = launch_copy_strided(dtype, a, strides, mean_out, ost, shape, ndim, s)) return rc;
        return run_unit<T>(out, p.nout, f, s);
    }
    Pooled copy_pool, group_pool, sum_pool, pair_pool;
    const T *in = static_cast<const T *>(a);
    int64_t dense[SMHIP_MAX_NDIM];
    const int64_t *st = strides;
    if (p.copy) {
        const void *d;
        if (int rc = copy_pool.dense_copy(dtype, a, shape, strides, ndim, s, &d)) return rc;
        in = static_cast<const T *>(d);
        dense_strides(shape, ndim, dense);
        st = dense;
    }
    if (p.held) return run_held<T>(p, in, f, out, p.c.oso, mean_out, s);
    void *raw;
    if (int rc = sum_pool.take((size_t)p.nout * sizeof(double), &raw)) return rc;
    double *sum = static_cast<double *>(raw);
    if (int rc = launch_reduce_sum64(dtype, in, shape, st, ndim, mask, sum, s)) return rc;
    if (p.groups) {  // kept axes first, reduced axes last, each in index order
        int64_t pshape[SMHIP_MAX_NDIM], pst[SMHIP_MAX_NDIM], pdense[SMHIP_MAX_NDIM];
        int n = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int d = 0; d < ndim; ++d)
                if ((int)(mask >> d & 1) == pass) pshape[n] = shape[d], pst[n] = st[d], ++n;
        const int64_t total = dense_strides(pshape, ndim, pdense);
        void *g;
        if (int rc = group_pool.take((size_t)total * sizeof(T), &g)) return rc;
        if (int rc = launch_copy_strided(dtype, in, pst, g, pdense, pshape, ndim, s)) return rc;
        in = static_cast<const T *>(g);
    }
    return run_second<T>(p, in, sum, p.c.oso, p.c.osi, f, out, mean_out, p.c.oso, p.c.osi, nullptr, &pair_pool, s);
}

template <typename T>
int run_standardize(const Plan &p, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, double eps, int64_t ddof, void *out_v,
                    hipStream_t s) {
    const Fin f{kStandardize, (double)p.N, (double)(p.N - ddof), eps};
    T *out = static_cast<T *>(out_v);
    if (p.route == SMHIP_MOMENTS_ROUTE_UNIT) {
        if (a != out_v) {  // (in place: a is dense)
            int64_t dense[SMHIP_MAX_NDIM];
            dense_strides(shape, ndim, dense);
            if (int rc = launch_copy_strided(dtype, a, strides, out, dense, shape, ndim, s)) return rc;
        }
        return run_unit<T>(out, p.nout, f, s);
    }
    Pooled copy_pool, sum_pool, pair_pool;
    const T *in = static_cast<const T *>(a);
    if (p.copy) {
        const void *d;
        if (int rc = copy_pool.dense_copy(dtype, a, shape, strides, ndim, s, &d)) return rc;
        in = static_cast<const T *>(d);
    }
    const Canon &c = p.c;
    if (p.held) return run_held<T>(p, in, f, out, c.oso, nullptr, s);
    const int64_t lines = c.O * c.I;
    void *raw;
    if (int rc = sum_pool.take((size_t)(3 * lines) * sizeof(double), &raw)) return rc;
    double *sum = static_cast<double *>(raw), *stat = sum + lines;
    int64_t s3[3], t3[3];
    canon_view(c, s3, t3);
    if (int rc = launch_reduce_sum64(dtype, in, s3, t3, 3, 2u, sum, s)) return rc;
    if (int rc = run_second<T>(p, in, sum, c.I, 1, f, (T *)nullptr, (T *)nullptr, 0, 0, stat, &pair_pool, s)) return rc;
    if (p.route == SMHIP_MOMENTS_ROUTE_ROW) {
        hipLaunchKernelGGL((apply_row_kernel<T>), dim3(grid_cap().capped(lines * p.C)), dim3(kBlock), 0, s, in, lines, c.so, c.R, p.CL, p.C, (const double *)stat, out, c.oso);
    } else {
        const int64_t lanes = c.O * p.C * ceil_div(c.I, VecOf<T>::W);
        hipLaunchKernelGGL((apply_column_kernel<T>), dim3(grid_cap().capped(ceil_div(lanes, kBlock))), dim3(kBlock), 0, s, in, c.O, c.so, c.R, c.sr, c.I, p.CL, p.C,
                           (const double *)stat, out, c.oso, p.orr, c.osi);
    }
    SMHIP_LAUNCH_CHECK("standardize apply");
    return SMHIP_OK;
}

// Validation: everything that can be said without a device or a pointer.
int float_only(const char *who, int dtype, int ndim) {
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (dtype != SMHIP_F32 && dtype != SMHIP_F64) return fail(SMHIP_ERR_UNSUPPORTED, "%s: an integer element type (f32 and f64 only)", who);
    return SMHIP_OK;
}
int moments_check(const char *who, int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, uint32_t mask, int64_t ddof) {
    if (kind < SMHIP_MOMENT_VAR || kind > SMHIP_MOMENT_STD) return fail(SMHIP_ERR_INVALID, "%s: bad kind %d", who, kind);
    if (int rc = float_only(who, dtype, ndim)) return rc;
    if (mask == 0 || (mask >> ndim) != 0) return fail(SMHIP_ERR_INVALID, "%s: axes mask 0x%x empty or beyond ndim %d", who, mask, ndim);
    if (int rc = check_extents(who, shape, strides, ndim)) return rc;
    if (ddof < 0) return fail(SMHIP_ERR_INVALID, "%s: ddof %lld is negative", who, (long long)ddof);
    int64_t nout = 1, N = 1;
    for (int d = 0; d < ndim; ++d) ((mask >> d & 1) ? N : nout) *= shape[d];
    if (nout > 0 && N == 0) return fail(SMHIP_ERR_INVALID, "%s: a variance over an empty extent", who);
    if (nout > 0 && N - ddof <= 0) return fail(SMHIP_ERR_INVALID, "%s: N - ddof = %lld - %lld is not positive", who, (long long)N, (long long)ddof);
    return SMHIP_OK;
}
int standardize_check(const char *who, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, double eps, int64_t ddof) {
    if (int rc = float_only(who, dtype, ndim)) return rc;
    if (int rc = check_axis(who, axis, ndim)) return rc;
    if (int rc = check_extents(who, shape, strides, ndim)) return rc;
    if (!(eps >= 0.0) || eps > std::numeric_limits<double>::max()) return fail(SMHIP_ERR_INVALID, "%s: eps %g is negative, NaN or infinite", who, eps);
    if (ddof < 0) return fail(SMHIP_ERR_INVALID, "%s: ddof %lld is negative", who, (long long)ddof);
    if (element_count(shape, ndim) > 0 && shape[axis] - ddof <= 0)
        return fail(SMHIP_ERR_INVALID, "%s: N - ddof = %lld - %lld is not positive", who, (long long)shape[axis], (long long)ddof);
    return SMHIP_OK;
}

void report(const Plan &pl, int *route, int *launches, int64_t *ori3, int64_t *info3) {
    if (route) *route = pl.code();
    if (launches) *launches = pl.launches;
    if (ori3) ori3[0] = pl.c.O, ori3[1] = pl.route == SMHIP_MOMENTS_ROUTE_NONE ? pl.N : pl.c.R, ori3[2] = pl.c.I;
    if (info3) info3[0] = pl.L, info3[1] = pl.reads, info3[2] = pl.levels;
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_moments_axes(int kind, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, uint32_t axes_mask, int64_t ddof, void *out,
                       void *out_mean_or_null) {
    if (int rc = moments_check("moments_axes", kind, dtype, shape, strides, ndim, axes_mask, ddof)) return rc;
    Plan pl;
    make_moments_plan(dtype, shape, strides, ndim, axes_mask, &pl);
    if (pl.nout == 0) return SMHIP_OK;
    if (!out || !a) return fail(SMHIP_ERR_INVALID, "moments_axes: null buffer");
    const size_t esz = dtype_size(dtype);
    const Span sa{a, span_bytes(shape, strides, ndim, esz)}, so{out, (size_t)pl.nout * esz}, sm{out_mean_or_null, (size_t)pl.nout * esz};
    if (spans_overlap(sa, so) || spans_overlap(sa, sm) || spans_overlap(so, sm))
        return fail(SMHIP_ERR_INVALID, "moments_axes: the operand and the outputs overlap");
    SMHIP_ACQUIRE(s);  // undeclared spans (the pooled copy, sums and pairs): ordered behind everything, recorded tiny operators flushed first
    if (dtype == SMHIP_F64) return run_moments<double>(pl, kind, dtype, a, shape, strides, ndim, axes_mask, ddof, out, out_mean_or_null, s);
    return run_moments<float>(pl, kind, dtype, a, shape, strides, ndim, axes_mask, ddof, out, out_mean_or_null, s);
}

int smhip_moments_plan(int kind, int dtype, const int64_t *shape, const int64_t *strides, int ndim, uint32_t axes_mask, int64_t ddof, int *route, int *launches,
                       int64_t *ori3, int64_t *info3) {
    if (int rc = moments_check("moments_plan", kind, dtype, shape, strides, ndim, axes_mask, ddof)) return rc;
    Plan pl;
    make_moments_plan(dtype, shape, strides, ndim, axes_mask, &pl);
    report(pl, route, launches, ori3, info3);
    return SMHIP_OK;
}

int smhip_standardize_axis(int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, double eps, int64_t ddof, void *out) {
    if (int rc = standardize_check("standardize_axis", dtype, shape, strides, ndim, axis, eps, ddof)) return rc;
    const int64_t total = element_count(shape, ndim);
    if (total == 0) return SMHIP_OK;
    if (!out || !a) return fail(SMHIP_ERR_INVALID, "standardize_axis: null buffer");
    const size_t esz = dtype_size(dtype);
    const Span sa{a, span_bytes(shape, strides, ndim, esz)}, so{out, (size_t)total * esz};
    if (spans_overlap(sa, so) && !(a == out && row_major(shape, strides, ndim)))
        return fail(SMHIP_ERR_INVALID, "standardize_axis: `out` overlaps the operand (only out == a with a dense operand is in place)");
    Plan pl;
    make_standardize_plan(dtype, shape, strides, ndim, axis, &pl);
    SMHIP_ACQUIRE(s);
    if (dtype == SMHIP_F64) return run_standardize<double>(pl, dtype, a, shape, strides, ndim, eps, ddof, out, s);
    return run_standardize<float>(pl, dtype, a, shape, strides, ndim, eps, ddof, out, s);
}

int smhip_standardize_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, double eps, int64_t ddof, int *route, int *launches,
                           int64_t *ori3, int64_t *info3) {
    if (int rc = standardize_check("standardize_plan", dtype, shape, strides, ndim, axis, eps, ddof)) return rc;
    Plan pl;
    make_standardize_plan(dtype, shape, strides, ndim, axis, &pl);
    report(pl, route, launches, ori3, info3);
    return SMHIP_OK;
}
