// sm_moments.h -- the per-line arithmetic of var, std, var_mean and standardize (moments_axis.hip), f32 and f64, compiled for the
// gfx950 kernels and (tests/cpp/moments_host_check.cpp) for the host, like sm_softmax.h.
//
// A line x_0 .. x_{N-1} whose fp64 sum S was formed in a fixed order:
//   mean  = S / N                                    (fp64, unrounded; the mean OUTPUT is this rounded once)
//   d_k   = (double)x_k - mean                       (fp64)
//   sd    = sum d_k,  sq = sum d_k^2                 (fp64, each term of sq by one fused multiply-add: add())
//   M2    = sq - sd * sd / N                         (the two-pass sum plus the Chan-Golub-LeVeque correction; clamped at +0)
//   VAR   = M2 / (N - ddof),  STD = sqrt(VAR)        (fp64, rounded once to T)
//   y_k   = d_k / sqrt(VAR + eps)                    (standardize; fp64, rounded once)
// sq - sd^2 / N equals the exact sum of (x_k - mean_exact)^2 for ANY value of `mean` in exact arithmetic, so the mean's own rounding
// error reaches M2 only at second order in 2^-53.  A piece of a line carries the pair (sd, sq) about the LINE's mean; pieces are
// merged by adding the halves in piece order (merge).  A NaN or an infinity in the line makes d_k NaN (inf - inf) and with it
// every result; a constant line whose fp64 sum is exact has d_k = +0 throughout and gives exactly +0.
#pragma once

#include <stdint.h>

#include "sm_pow.h"  // SM_POW_FN, SM_POW_FMA

#if defined(__HIP_DEVICE_COMPILE__)
#define SM_MOMENTS_SQRT(x) __builtin_sqrt(x)
#else
#define SM_MOMENTS_SQRT(x) sqrt(x)
#endif

namespace smmoments {

enum Kind { kVar = 0, kStd = 1, kStandardize = 2 };  // 0, 1 = smhip_moment_kind; 2: the kernels' own word for standardize

struct Sums { double sd, sq; };  // sum d, sum d^2 about the line's mean

SM_POW_FN Sums zero() { return Sums{0.0, 0.0}; }
SM_POW_FN double mean_of(double S, double N) { return S / N; }
template <typename T> SM_POW_FN double centre(T x, double mean) { return (double)x - mean; }
SM_POW_FN void add(Sums &s, double d) { s.sd += d, s.sq = SM_POW_FMA(d, d, s.sq); }
SM_POW_FN Sums merge(Sums a, Sums b) { return Sums{a.sd + b.sd, a.sq + b.sq}; }

// M2 of a whole line.  Rounding can leave it a hair below zero where the exact value is 0; a NaN stays a NaN.
SM_POW_FN double m2(Sums s, double N) {
    const double v = s.sq - s.sd * s.sd / N;
    return v < 0.0 ? 0.0 : v;
}
SM_POW_FN double variance(Sums s, double N, double divisor) { return m2(s, N) / divisor; }  // divisor = N - ddof > 0
SM_POW_FN double denominator(double var, double eps) { return SM_MOMENTS_SQRT(var + eps); }

// fp64 in, one rounding to T.
template <typename T> SM_POW_FN T finish(int kind, double var) { return kind == kStd ? (T)SM_MOMENTS_SQRT(var) : (T)var; }
template <typename T> SM_POW_FN T finish_mean(double S, double N) { return (T)(S / N); }
template <typename T> SM_POW_FN T standardized(double d, double denom) { return (T)(d / denom); }

}  // namespace smmoments
