// sm_quantile.h -- the arithmetic of quantile, percentile and median along an axis (quantile_axis.hip), f32 and f64, compiled for the
// gfx950 kernels and (tests/cpp/quantile_host_check.cpp) for the host, like sm_moments.h.
//
// A line of R elements in sort's ascending order s_0 .. s_{R-1}, every zero read as +0, and a probability q in [0, 1]:
//   h = (R - 1) * q (fp64, one rounding),  j = floor(h),  g = h - j (exact)
//   LINEAR    lo = s[j], hi = s[min(j + 1, R - 1)], interpolated with g
//   LOWER     s[floor(h)]        HIGHER   s[ceil(h)]        NEAREST   s[rint(h)], ties to even
//   MIDPOINT  LINEAR with g = 0.5 where h is not an integer, else s[h]
// Interpolation (numpy's _lerp), in fp64 from the exactly converted elements, rounded to T once:
//   g == 0 -> lo (hi is not consulted);  lo == hi -> lo;  else with d = hi - lo:  g < 0.5 ? lo + d * g : hi - d * (1 - g)
// Each product, sum and difference is ONE IEEE operation: contraction is switched off inside interpolate().  A NaN result is the
// canonical quiet NaN, whatever produced it.
//
// key_of is the monotone key of topk_axis.hip, ascending only: a < b in the order exactly when key_of(a) < key_of(b); -0 and +0 share
// a key, every NaN has the one key above +inf's.  The radix select reads a key from its top byte down (digit()); an element is never
// rebuilt from its key.
#pragma once

#include <stdint.h>
#include <string.h>

#include "sm_pow.h"  // SM_POW_FN

#if defined(__HIP_DEVICE_COMPILE__)
#define SM_QUANTILE_FLOOR(x) __builtin_floor(x)
#define SM_QUANTILE_CEIL(x) __builtin_ceil(x)
#define SM_QUANTILE_RINT(x) __builtin_rint(x)
#else
#include <math.h>
#define SM_QUANTILE_FLOOR(x) floor(x)
#define SM_QUANTILE_CEIL(x) ceil(x)
#define SM_QUANTILE_RINT(x) rint(x)
#endif

namespace smquantile {

enum Method { kLinear = 0, kLower = 1, kHigher = 2, kNearest = 3, kMidpoint = 4 };  // = smhip_quantile_method

template <typename T> struct KeyType;
template <> struct KeyType<float> { using type = uint32_t; };
template <> struct KeyType<double> { using type = uint64_t; };
template <typename T> using KeyOf = typename KeyType<T>::type;

template <typename T> SM_POW_FN KeyOf<T> key_of(T x) {
    using K = KeyOf<T>;
    const K top = (K)1 << (sizeof(K) * 8 - 1);
    K u;
    memcpy(&u, &x, sizeof u);
    if (x != x) return ~(K)0;  // one key for every NaN, above +inf's (no number has it)
    if (u == top) u = 0;       // -0 == +0
    return (u & top) ? (K)~u : (K)(u | top);
}
// The 8-bit digit that pass `pass` (0 = the top byte) of a radix select reads, and whether a key agrees with `prefix` on the digits of
// the passes before it.
template <typename K> SM_POW_FN int shift_of(int pass) { return ((int)sizeof(K) - 1 - pass) * 8; }
template <typename K> SM_POW_FN uint32_t digit(K key, int pass) { return (uint32_t)(key >> shift_of<K>(pass)) & 255u; }
template <typename K> SM_POW_FN bool agrees(K key, K prefix, int passes_done) {
    return passes_done == 0 || ((key ^ prefix) >> shift_of<K>(passes_done - 1)) == 0;
}

// What an element is read as: a zero of either sign is +0.
template <typename T> SM_POW_FN T canonical(T x) { return x == (T)0 ? (T)0 : x; }
template <typename T> SM_POW_FN T quiet_nan() {
    KeyOf<T> bits = sizeof(T) == 4 ? (KeyOf<T>)0x7fc00000u : (KeyOf<T>)0x7ff8000000000000ull;
    T x;
    memcpy(&x, &bits, sizeof x);
    return x;
}

// The ranks of one probability: lo = s[j], hi = s[j1] consulted only when g != 0 (then j1 = j + 1 <= R - 1).
struct Rank { int64_t j, j1; double g; };

SM_POW_FN Rank rank_of(int64_t R, double q, int method) {
    const double h = (double)(R - 1) * q;  // q in [0, 1], R >= 1: 0 <= h <= R - 1
    double j = SM_QUANTILE_FLOOR(h), g = h - j;
    switch (method) {
        case kLower: g = 0.0; break;
        case kHigher: j = SM_QUANTILE_CEIL(h), g = 0.0; break;
        case kNearest: j = SM_QUANTILE_RINT(h), g = 0.0; break;  // the default rounding mode: ties to even
        case kMidpoint: g = g != 0.0 ? 0.5 : 0.0; break;
        default: break;
    }
    Rank r;
    r.j = (int64_t)j, r.g = g;
    r.j1 = g != 0.0 ? r.j + 1 : r.j;  // g != 0 means h < R - 1, so j + 1 <= R - 1
    return r;
}

// lo, hi: elements read as canonical(); the result in fp64, to be rounded to T once (finish()).  A host compiler other than clang
// must be given -ffp-contract=off.
SM_POW_FN double interpolate(double lo, double hi, double g) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    if (g == 0.0 || lo == hi) return lo;
    const double d = hi - lo;
    if (g < 0.5) {
        const double p = d * g;
        return lo + p;
    }
    const double r = 1.0 - g, p = d * r;
    return hi - p;
}
template <typename T> SM_POW_FN T finish(T lo, T hi, double g) {
    const double v = interpolate((double)lo, (double)hi, g);
    const T r = (T)v;
    return r != r ? quiet_nan<T>() : r;
}

}  // namespace smquantile
