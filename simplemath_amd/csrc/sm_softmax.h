// sm_softmax.h -- the per-line arithmetic of softmax, log_softmax and logsumexp (softmax_axis.hip), f32 and f64, compiled for the
// gfx950 kernels and (tests/cpp/softmax_host_check.cpp) for the host, like sm_convert.h and sm_random.h.
//
// A line x_0 .. x_{R-1} with maximum m (a NaN anywhere makes m a NaN: line_max below) and d_r = x_r - m:
//   m NaN, +inf or -inf    SOFTMAX / LOG_SOFTMAX: NaN everywhere;  LOGSUMEXP: m itself (special)
//   otherwise              e_r = exp(d_r), S = sum e_r in fp64;  e_r / S,  d_r - ln S,  m + ln S, each formed in fp64, rounded once
// f32: d_r is formed in fp64 -- exact while the two floats' exponents are within 29 of each other, and rounded at 2^-53 relative
// beyond that (at most 104 * 2^-53 in the exponent where e_r is not already +0) -- and enters sm_unary.h's exp core on its fp64
// side, never rounded to f32.  f64: d_r in fp64, sm_unary.h's f64 exp.  ln S is smunary::log, once per line.
// A partial result of a piece of a line is the pair (m_c, S_c) with S_c = 0 when m_c is not finite; pieces are combined
// by rescaling S_c with exp(m_c - m) in fp64 (rescale, combine).
#pragma once

#include "sm_unary.h"

namespace smsoftmax {

enum Kind { kSoftmax = 0, kLogSoftmax = 1, kLogSumExp = 2 };  // = smhip_softmax_kind

// The running maximum of a line: a NaN on either side propagates (fold.hip.h's kMax).
template <typename T> SM_POW_FN T line_max(T x, T y) { return (x > y || x != x) ? x : y; }

// Is the line's maximum one of the special rows of the table (NaN, +inf, -inf)?
SM_POW_FN bool special(double m) { return !(m - m == 0.0); }
// What a special line holds: NaN for SOFTMAX / LOG_SOFTMAX, m itself for LOGSUMEXP.
template <typename T> SM_POW_FN T special_value(int kind, T m) {
    if (kind == kLogSumExp) return m;
    if constexpr (sizeof(T) == 4) return smunary::bits_f32(0x7fc00000u);
    else return smunary::bits_f64(0x7ff8000000000000ULL);
}

// e = exp(d) for W differences d <= 0 (-inf included) of an ordinary line.  f32: below -104 the result is +0 (exp(-104) = 2^-150.04
// already rounds to it), so the clamp and the core agree there; the argument stays fp64 all the way.
template <int W> SM_POW_FN void exp_diff_n(const double (&d)[W], float (&e)[W]) {
    double dc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) dc[k] = d[k] < -104.0 ? -104.0 : d[k];
    smunary::expf_core_n<W>(dc, e);
#pragma unroll
    for (int k = 0; k < W; ++k) e[k] = d[k] < -104.0 ? 0.0f : e[k];
}
// f64: below -746 the result is +0 (exp(-745.14) is half the smallest subnormal).  `tab` as smunary::exp_core takes it.
template <int W, typename TAB> SM_POW_FN void exp_diff_n(const double (&d)[W], double (&e)[W], const TAB &tab) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const bool far = d[k] <= -746.0;
        const double c = smunary::exp_core(far ? 0.0 : d[k], tab);
        e[k] = far ? 0.0 : c;
    }
}

// The three finishing formulas: fp64 in, one rounding to T.
template <typename T, typename E> SM_POW_FN T finish_softmax(E e, double S) { return (T)((double)e / S); }
template <typename T> SM_POW_FN T finish_log_softmax(double d, double lnS) { return (T)(d - lnS); }
template <typename T> SM_POW_FN T finish_logsumexp(double m, double lnS) { return (T)(m + lnS); }

// ln S for the sum of an ordinary line (S >= 1: the maximum's own term is exactly 1), from the tables in constant memory / on the host.
SM_POW_FN double log_sum(double S) { return smunary::log(S); }

// A piece's sum S_c (relative to its own maximum m_c) relative to the line's maximum m >= m_c, m finite: S_c exp(m_c - m), the
// factor by the f64 exp.  A piece without a finite maximum (all -inf) carries S_c = 0 and adds nothing.
SM_POW_FN double rescale(double m_c, double S_c, double m) {
    if (S_c == 0.0 || m_c == m) return S_c;
    return S_c * smunary::exp(m_c - m);
}
// Two partial pairs into one: (m1, S1) then (m2, S2), in that order.
struct Pair { double m, S; };
SM_POW_FN Pair combine(Pair a, Pair b) {
    Pair r;
    r.m = line_max(a.m, b.m);
    r.S = special(r.m) ? 0.0 : rescale(a.m, a.S, r.m) + rescale(b.m, b.S, r.m);
    return r;
}

}  // namespace smsoftmax
