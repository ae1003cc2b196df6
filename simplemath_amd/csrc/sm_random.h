// sm_random.h -- the counter-based generator behind smhip_random, shared by the gfx950 kernels (random.hip) and, compiled for
// the host by tests/cpp/random_host_check.cpp, by the CPU check of the definition itself.
//
// Element i of a call is a pure function of (seed, stream, offset, i): never of the address, the grid or the run.
//   Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants):
//     key     = (low, high) 32 bits of `seed`
//     counter = (low 32 of b, high 32 of b, low 32 of `stream`, high 32 of `stream`),  b = offset + block index in the call
//   One block is four 32-bit words w0..w3.
//   32-bit draws: element i uses word i % 4 of block i / 4.
//   64-bit draws: element i uses x = w[2 (i % 2)] | w[2 (i % 2) + 1] << 32 of block i / 2.
//   kind        types        draw   rule
//   BITS        i32 / i64    32/64  the word / x, reinterpreted as signed
//   UNIFORM     f32          32     u = (w >> 8) * 2^-24 in [0, 1);  lo + u * span, two roundings in f32 (span = hi - lo, rounded on the host)
//   UNIFORM     f64          64     u = (x >> 11) * 2^-53;  the same in f64
//   INTEGERS    i32 / i64    64     lo + mulhi64(x, R), R = hi - lo, 1 <= R <= 2^32.  mulhi64 maps the 2^64 values of x onto R bins of
//                                   floor(2^64 / R) or that plus one values each: a bin's probability is off by at most 2^-64, a relative
//                                   bias of at most R / 2^64 <= 2^-32.  (Unbiased rejection sampling is out of scope.)
//   BERNOULLI   all four     32     T(1) if (uint64) w < thr else T(0),  thr = floor(p * 2^32) computed in fp64 on the host (p = 1: all ones)
//   NORMAL      f32          32     Box-Muller on the word pairs (w0, w1) and (w2, w3) of block i / 4:
//                                   u1 = ((wa >> 8) + 1) * 2^-24 in (0, 1],  t = (wb >> 8) * 2^-24,  r = sqrt(-2 logf(u1)),
//                                   z0 = r * cospi(2t), z1 = r * sinpi(2t); elements 4b .. 4b + 3 are z0, z1 of the first pair, then of
//                                   the second.  mean + std * z, two roundings.
//   NORMAL      f64          64     one pair per block: u1 = ((x01 >> 11) + 1) * 2^-53, t = (x23 >> 11) * 2^-53; elements 2b, 2b + 1 are z0, z1
//   A call of n elements consumes ceil(n / 4) blocks (32-bit draws) or ceil(n / 2) (64-bit draws; INTEGERS of i32 included).
//
// cospi(2t) and sinpi(2t): t = m / 2^B is a dyadic rational (B = 24 / 53), so the reduction to an octant is exact integer work on
// m: the top three bits name the octant, the rest -- reflected in the odd octants -- is an angle of at most 1/8 turn, on which
// fdlibm's two kernels (k_sin.c / k_cos.c: sin and cos on [-pi/4, pi/4] of an argument given as head + tail) are evaluated in
// fp64.  f32 rounds that value once (measured: 0.5 ULP); f64 carries the tail of 2 pi x.  t = 1/4 gives a cosine of exactly 0
// and t = 0 a sine of exactly 0 (the sine kernel of 0 is 0), with a sign bit that is not specified.
// logf / log are sm_unary.h's (u1 is positive and normal: their ordinary paths); sqrt is the correctly rounded one.
// Everything is written so that host and device give the same bits (-ffp-contract=off, no fast-math intrinsics).
#pragma once

#include <stdint.h>

#include "sm_unary.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define SM_RND_SQRTF(x) __builtin_sqrtf(x)
#define SM_RND_SQRT(x) __builtin_sqrt(x)
#else
#define SM_RND_SQRTF(x) sqrtf(x)
#define SM_RND_SQRT(x) sqrt(x)
#endif

namespace smrandom {

enum Kind { BITS = 0, UNIFORM = 1, INTEGERS = 2, BERNOULLI = 3, NORMAL = 4 };  // = smhip_random_kind

// ------------------------------------------------------------------------------------------------------- Philox4x32-10
// hi and lo of each product come from ONE 32 x 32 -> 64 multiply (v_mad_u64_u32 on gfx950): 20 wide multiplies per block, the
// first of which the compiler moves to the scalar unit when `stream` is uniform, as the key schedule.
// (Taken as two multiplies, v_mul_lo_u32 + v_mul_hi_u32, every kind is slower: DESIGN.md, "Random draws".)
SM_POW_FN void philox4x32_10(const uint32_t (&ctr)[4], const uint32_t (&key)[2], uint32_t (&out)[4]) {
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3], k0 = key[0], k1 = key[1];
#pragma unroll
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// Block b of (seed, stream).
SM_POW_FN void block_words(uint64_t seed, uint64_t stream, uint64_t b, uint32_t (&w)[4]) {
    const uint32_t ctr[4] = {(uint32_t)b, (uint32_t)(b >> 32), (uint32_t)stream, (uint32_t)(stream >> 32)};
    const uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    philox4x32_10(ctr, key, w);
}

SM_POW_FN uint64_t mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// ------------------------------------------------------------------------------------------- cospi(2t), sinpi(2t)
// fdlibm's __kernel_sin / __kernel_cos (Sun Microsystems, 1993; freely distributable): |x| <= pi/4, y the tail of x.
SM_POW_FN double kernel_sin(double x, double y) {
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x, v = z * x;
    const double r = S2 + z * (S3 + z * (S4 + z * (S5 + z * S6)));
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
SM_POW_FN double kernel_cos(double x, double y) {
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = x * x, w = z * z;
    const double r = z * (C1 + z * (C2 + z * C3)) + (w * w) * (C4 + z * (C5 + z * C6));
    const double hz = 0.5 * z, h = 1.0 - hz;
    return h + (((1.0 - h) - hz) + (z * r - x * y));
}

// {cos, sin} of 2 pi m / 2^B for 0 <= m < 2^B, in fp64.  TAIL: carry the low part of 2 pi x (the f64 draws).
template <int B, bool TAIL>
SM_POW_FN void cossin_turn(uint64_t m, double *c, double *s) {
    const uint32_t q = (uint32_t)(m >> (B - 3));                     // the octant
    const uint64_t f = m & (((uint64_t)1 << (B - 3)) - 1);
    const uint64_t g = (q & 1) ? ((uint64_t)1 << (B - 3)) - f : f;  // reflected in the odd octants: 0 .. 2^(B-3)
    const double x = (double)(int64_t)g * (B == 24 ? 0x1p-24 : 0x1p-53);  // exact; at most 1/8 turn
    const double a = x * 0x1.921fb54442d18p+2;                       // 2 pi, head
    double tail = 0.0;
    if (TAIL) tail = SM_POW_FMA(x, 0x1.921fb54442d18p+2, -a) + x * 0x1.1a62633145c07p-52;
    const double C = kernel_cos(a, tail), S = kernel_sin(a, tail);
    const bool swap = ((q + 1) & 2) != 0, cneg = ((q + 2) & 4) != 0, sneg = q >= 4;
    const double cv = swap ? S : C, sv = swap ? C : S;
    *c = cneg ? -cv : cv;
    *s = sneg ? -sv : sv;
}

// The pieces of the f32 normal, of the 24-bit integers the words give: k = wa >> 8, m = wb >> 8.
SM_POW_FN float radius_f32(uint32_t k) {
    const float u1 = (float)(k + 1u) * 0x1p-24f;  // (0, 1]
    const float x[1] = {u1};
    float l[1];
    const int none[1] = {0};
    smunary::logf_core_n<1, false>(x, l, smpow::kLogTab, none);  // = smunary::logf(u1): u1 is positive and normal
    return SM_RND_SQRTF(-2.0f * l[0]);
}
SM_POW_FN void cossin_f32(uint32_t m, float *c, float *s) {
    double cd, sd;
    cossin_turn<24, false>(m, &cd, &sd);
    *c = (float)cd;
    *s = (float)sd;
}
// ... and of the f64 normal: k = x01 >> 11, m = x23 >> 11 (53 bits each).
SM_POW_FN double radius_f64(uint64_t k) {
    const double u1 = (double)(int64_t)(k + 1u) * 0x1p-53;  // (0, 1]
    const double l = smunary::log_core<false>(u1, smpow64::TabAoS{smpow64::kLogTab, smpow64::kExpTab});  // = smunary::log(u1)
    return SM_RND_SQRT(-2.0 * l);
}
SM_POW_FN void cossin_f64(uint64_t m, double *c, double *s) { cossin_turn<53, true>(m, c, s); }

// --------------------------------------------------------------------------------------------------------- the kinds
// A call's parameters in the element type (smhip_random converts them on the host).
template <typename T>
struct Params {
    T a, b;       // UNIFORM: lo, span.  NORMAL: mean, std
    int64_t lo;   // INTEGERS
    uint64_t u;   // INTEGERS: R.  BERNOULLI: thr
};

// Elements one block gives.
template <int KIND, typename T>
struct PerBlock {
    static constexpr int value = KIND == INTEGERS ? 2 : KIND == BERNOULLI ? 4 : sizeof(T) == 8 ? 2 : 4;
};
constexpr int per_block(int kind, int elem_size) { return kind == INTEGERS ? 2 : kind == BERNOULLI ? 4 : elem_size == 8 ? 2 : 4; }

SM_POW_FN uint64_t join64(uint32_t lo, uint32_t hi) { return (uint64_t)lo | ((uint64_t)hi << 32); }

// The PerBlock<KIND, T>::value elements of one block.
template <int KIND, typename T>
SM_POW_FN void block_values(const uint32_t (&w)[4], const Params<T> &p, T *v) {
    if constexpr (KIND == BITS) {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (T)w[k];
        } else {
            v[0] = (T)join64(w[0], w[1]);
            v[1] = (T)join64(w[2], w[3]);
        }
    } else if constexpr (KIND == UNIFORM) {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const T t = (T)(w[k] >> 8) * (T)0x1p-24f * p.b;
                v[k] = p.a + t;
            }
        } else {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const T t = (T)(int64_t)(join64(w[2 * k], w[2 * k + 1]) >> 11) * (T)0x1p-53 * p.b;
                v[k] = p.a + t;
            }
        }
    } else if constexpr (KIND == INTEGERS) {
#pragma unroll
        for (int k = 0; k < 2; ++k) v[k] = (T)(int64_t)((uint64_t)p.lo + mulhi64(join64(w[2 * k], w[2 * k + 1]), p.u));
    } else if constexpr (KIND == BERNOULLI) {
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = (uint64_t)w[k] < p.u ? (T)1 : (T)0;
    } else {
        if constexpr (sizeof(T) == 4) {
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const float r = radius_f32(w[2 * k] >> 8);
                float c, s;
                cossin_f32(w[2 * k + 1] >> 8, &c, &s);
                const float z0 = r * c, z1 = r * s;
                const float t0 = p.b * z0, t1 = p.b * z1;
                v[2 * k] = p.a + t0;
                v[2 * k + 1] = p.a + t1;
            }
        } else {
            const double r = radius_f64(join64(w[0], w[1]) >> 11);
            double c, s;
            cossin_f64(join64(w[2], w[3]) >> 11, &c, &s);
            const double z0 = r * c, z1 = r * s;
            const double t0 = p.b * z0, t1 = p.b * z1;
            v[0] = p.a + t0;
            v[1] = p.a + t1;
        }
    }
}

}  // namespace smrandom
