// sm_unary.h -- exp and log evaluated in registers, f32 and f64, shared by the gfx950 kernels and (compiled for the
// host by tests/cpp/unary_host_check.cpp) by the CPU check of the algorithms themselves.
//
// The reference has no counterpart (its README's "Important Note": vector exp / log were tried and given up at the range
// reduction).  They are the two halves of the pow evaluations beside this file, each cheaper than pow, and reuse their
// tables.  Bar: <= 1 ULP of the true value everywhere, C99 Annex F special values.  Measured: f32 over EVERY float on the
// device 0.986 (exp) and 0.5001 ULP (log) against the fp64 value (tests/cpp/unary_exhaustive.hip); f64 on the host sweep 0.75
// and 0.50 ULP against long double (profiles/unary_accuracy.txt).
//
// f32 (sm_pow.h's tables and polynomials):
//   exp x   E = x * log2(e) in fp64 (the product's error, 2^-53 relative, is far below the result's ULP even at
//           |E| = 150);  n = rint(E), f = float(E - n), |f| <= 1/2;  2^f = 1 + f P(f), degree-5 P in (packed) f32;
//           v_ldexp_f32 by n: correct subnormals, +0 and +inf from one path.  No table.
//           Per element on gfx950: cvt, mul, rndne, add, cvt, cvt_i32 on the fp64 side, 3 packed-f32 fma (6 v_pk_fma_f32 per pair),
//           ldexp, and 5.5 compares / selects of the clamp and the special-value test: 16.5 (read off chain_kernel's disassembly).
//   log x   log2 x = e + logc[i] + r Q(r) exactly as pow's first half (128-entry {invc, logc} table in LDS, degree-3 Q in
//           fp64, relative accuracy 2^-37 -- kept near x = 1, whose interval has {invc, logc} = {1, 0});
//           ln x = log2 x * ln 2 still in fp64, rounded to f32 ONCE: 0.5 ULP + 2^-13.
//           Per element: 6 fma, mul, add and 3 conversions on the fp64 side, 8 integer ops, 1 ds_read_b128: 22.
// f64 (sm_pow64.h's tables):
//   exp x   x = (k + j/128) ln2 + r, |r| < ln2/256 (two-constant Cody-Waite, the high part exact);
//           e^x = 2^k T[j] (1 + tail[j] + r + r^2/2 + ... + r^5/120); v_ldexp_f64.  27 per element: 9 fma, 4 mul, 3 add, rndne, cvt_i32,
//           ldexp, 6 integer ops, 1 ds_read_b128.
//   log x   x = 2^k z, interval i of 128: r = z invc[i] - 1 exactly as r + rlo;
//           ln x = k ln2 + logc[i] + r - r^2/2 + r^3 (...) accumulated as hi + lo (error-free sums, fma residuals) and
//           rounded once at the end.  57 per element: 22 add, 15 fma, 7.5 mul, a conversion, 8 integer ops, 2 LDS reads.
// W elements are evaluated side by side; polynomial constants come from constant memory (SGPRs); the special values are
// handled on a path of their own that a wavefront only enters when one of its lanes holds one.
#pragma once

#include "sm_pow.h"
#include "sm_pow64.h"

namespace smunary {

using smpow::bits_f32;
using smpow::bits_f64;
using smpow::f32_bits;
using smpow::f64_bits;

#if defined(__HIPCC__)
#define SM_UNARY_CONST inline __constant__ double
#else
#define SM_UNARY_CONST static const double
#endif
// {log2(e), ln(2)}: in constant memory for the same reason as sm_pow.h's (a 64-bit literal costs two v_mov_b32 per use)
SM_UNARY_CONST kScale[2] = {0x1.71547652b82fep+0, 0x1.62e42fefa39efp-1};
#undef SM_UNARY_CONST

// ------------------------------------------------------------------------------------------------------------ f32 exp
// 2^(x log2 e) for W finite x with |x| <= 104 (n within [-151, 151]: ldexp covers overflow and the subnormal range).
// The entry with the argument in fp64 (sm_softmax.h: a difference x - m that f32 cannot hold goes in without being rounded to it);
// the f32 entry below widens and comes here, so both are the same arithmetic.
template <int W>
SM_POW_FN void expf_core_n(const double (&x)[W], float (&out)[W]) {
    float ff[W];
    int ni[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const double E = x[k] * kScale[0];
        const double n = SM_POW_RINT(E);
        ff[k] = (float)(E - n);  // |f| <= 1/2
        ni[k] = smpow::sat_i32(n);
    }
    float qf[W];
#if defined(__HIP_DEVICE_COMPILE__)
    if constexpr (W % 2 == 0) {  // packed f32: two elements per v_pk_fma_f32 (sm_pow.h: pow_core_n)
        typedef float f2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int k = 0; k < W; k += 2) {
            const f2 f = {ff[k], ff[k + 1]};
            f2 q = {smpow::kP[5], smpow::kP[5]};
            q = __builtin_elementwise_fma(q, f, (f2){smpow::kP[4], smpow::kP[4]});
            q = __builtin_elementwise_fma(q, f, (f2){smpow::kP[3], smpow::kP[3]});
            q = __builtin_elementwise_fma(q, f, (f2){smpow::kP[2], smpow::kP[2]});
            q = __builtin_elementwise_fma(q, f, (f2){smpow::kP[1], smpow::kP[1]});
            q = __builtin_elementwise_fma(q, f, (f2){smpow::kP[0], smpow::kP[0]});
            q = __builtin_elementwise_fma(q, f, (f2){1.0f, 1.0f});
            qf[k] = q[0];
            qf[k + 1] = q[1];
        }
    } else
#endif
    {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            float q = smpow::kP[5];
            q = SM_POW_FMAF(q, ff[k], smpow::kP[4]);
            q = SM_POW_FMAF(q, ff[k], smpow::kP[3]);
            q = SM_POW_FMAF(q, ff[k], smpow::kP[2]);
            q = SM_POW_FMAF(q, ff[k], smpow::kP[1]);
            q = SM_POW_FMAF(q, ff[k], smpow::kP[0]);
            qf[k] = SM_POW_FMAF(q, ff[k], 1.0f);  // in [0.70, 1.42]
        }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] = SM_POW_LDEXPF(qf[k], ni[k]);
}
template <int W>
SM_POW_FN void expf_core_n(const float (&x)[W], float (&out)[W]) {
    double xd[W];
#pragma unroll
    for (int k = 0; k < W; ++k) xd[k] = (double)x[k];
    expf_core_n<W>(xd, out);
}

// e^x for W independent x.  Ordinary <=> |x| <= 104 (finite): exp(-104) = 2^-150.04 already rounds to +0 and exp(89) is
// beyond FLT_MAX, so everything outside is a constant.
template <int W>
SM_POW_FN void expf_n(const float (&x)[W], float (&out)[W]) {
    const uint32_t LIM = 0x42d00000u;  // 104.0f
    uint32_t worst = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const uint32_t ax = f32_bits(x[k]) & 0x7fffffffu;
        worst = ax > worst ? ax : worst;
    }
    if (!smpow::any_lane(worst > LIM)) {
        expf_core_n<W>(x, out);
        return;
    }
    float xs[W], core[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        float v = x[k];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(v));  // opaque: nothing of this path is hoisted above the branch (sm_pow.h: pow_n)
#endif
        xs[k] = (f32_bits(v) & 0x7fffffffu) > LIM ? 0.0f : v;
    }
    expf_core_n<W>(xs, core);
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const uint32_t ix = f32_bits(x[k]), ax = ix & 0x7fffffffu;
        uint32_t r = f32_bits(core[k]);
        r = ax > LIM ? ((ix >> 31) ? 0u : 0x7f800000u) : r;  // underflow to +0 (exp(-inf) too), overflow to +inf
        r = ax > 0x7f800000u ? 0x7fc00000u : r;              // NaN
        out[k] = bits_f32(r);
    }
}

// ------------------------------------------------------------------------------------------------------------ f32 log
// ln(ax) for W finite positive NORMAL ax (eadj[k] joins the exponent: the special path passes -24 with a pre-scaled
// subnormal).  `tab` = smpow::kLogTab's layout (an LDS copy on the device).
template <int W, bool ADJ>
SM_POW_FN void logf_core_n(const float (&ax)[W], float (&out)[W], const double *tab, const int (&eadj)[W]) {
    double r[W], p[W], le[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const uint32_t ix = f32_bits(ax[k]);
        const uint32_t tmp = ix - smpow::kOff;
        const uint32_t idx = (tmp >> (23 - smpow::kTabBits)) & (uint32_t)(smpow::kTabN - 1);
        const int e = ((int32_t)tmp >> 23) + (ADJ ? eadj[k] : 0);
        const double z = (double)bits_f32(ix - (tmp & 0xff800000u));
        const double invc = tab[2 * idx], logc = tab[2 * idx + 1];
        r[k] = SM_POW_FMA(z, invc, -1.0);  // exact when invc == 1
        le[k] = logc + (double)e;
    }
#pragma unroll
    for (int k = 0; k < W; ++k) p[k] = smpow::kC[3];
#pragma unroll
    for (int k = 0; k < W; ++k) p[k] = SM_POW_FMA(p[k], r[k], smpow::kC[2]);
#pragma unroll
    for (int k = 0; k < W; ++k) p[k] = SM_POW_FMA(p[k], r[k], smpow::kC[1]);
#pragma unroll
    for (int k = 0; k < W; ++k) p[k] = SM_POW_FMA(p[k], r[k], smpow::kC[0]);
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] = (float)(SM_POW_FMA(r[k], p[k], le[k]) * kScale[1]);  // log2(ax) * ln 2, rounded once
}

template <int W>
SM_POW_FN void logf_n(const float (&x)[W], float (&out)[W], const double *tab) {
    const uint32_t INF = 0x7f800000u, MINNORM = 0x00800000u;
    // ordinary <=> positive, finite and normal <=> ix - MINNORM < INF - MINNORM (unsigned; sm_pow.h: pow_n)
    uint32_t worst = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const uint32_t tx = f32_bits(x[k]) - MINNORM;
        worst = tx > worst ? tx : worst;
    }
    int eadj[W];
    if (!smpow::any_lane(worst >= INF - MINNORM)) {
        logf_core_n<W, false>(x, out, tab, eadj);
        return;
    }
    float axc[W], core[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
        float v = x[k];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(v));
#endif
        const uint32_t ix = f32_bits(v);
        const bool sub = ix - 1u < MINNORM - 1u;           // positive subnormal: scale by 2^24 (exact), carry -24 into e
        const bool plain = ix - MINNORM < INF - MINNORM;
        axc[k] = sub ? v * 16777216.0f : (plain ? v : 1.0f);  // special lanes are overwritten below
        eadj[k] = sub ? -24 : 0;
    }
    logf_core_n<W, true>(axc, core, tab, eadj);
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const uint32_t ix = f32_bits(x[k]), ax = ix & 0x7fffffffu;
        uint32_t r = f32_bits(core[k]);
        r = (ix >> 31) ? 0x7fc00000u : r;   // log(x < 0) = NaN (-inf too)
        r = ax == 0 ? 0xff800000u : r;      // log(+-0) = -inf
        r = ix == INF ? INF : r;            // log(+inf) = +inf
        r = ax > INF ? 0x7fc00000u : r;     // NaN
        out[k] = bits_f32(r);
    }
}

// One element, the table read from where it lives (constant memory on the device): vector tails and the host check.
SM_POW_FN float expf(float x) {
    const float xs[1] = {x};
    float r[1];
    expf_n<1>(xs, r);
    return r[0];
}
SM_POW_FN float logf(float x) {
    const float xs[1] = {x};
    float r[1];
    logf_n<1>(xs, r, smpow::kLogTab);
    return r[0];
}

// ------------------------------------------------------------------------------------------------------------ f64 exp
// The exp half of smpow64::pow_core_t with E = x exactly (no low part, nothing to clamp): finite x, |x| < 746.
template <typename TAB>
SM_POW_FN double exp_core(double x, const TAB &tab) {
    const double InvLn2N = 0x1.71547652b82fep+7, Ln2hiN = 0x1.62e42f8000000p-8, Ln2loN = 0x1.be8e7bcd5e4f2p-34;
    const double kd = SM_POW_RINT(x * InvLn2N);  // |kd| < 2^18: kd * Ln2hiN is exact
    const int ki = smpow::sat_i32(kd);
    double rr = SM_POW_FMA(-kd, Ln2hiN, x);
    rr = SM_POW_FMA(-kd, Ln2loN, rr);
    const int j = ki & (smpow64::kN - 1), e = ki >> 7;  // arithmetic shift: floor
    const double th = tab.th(j), trel = tab.trel(j);
    const double r2 = rr * rr;
    // trel + rr + rr^2 (1/2 + rr (1/6 + rr (1/24 + rr/120))); the innermost step as (rr + 5)/120
    double u = (rr + 5.0) * 0x1.1111111111111p-7;
    u = smpow64::fma_c(u, rr, 0x1.5555555555555p-3);
    u = SM_POW_FMA(u, rr, 0.5);
    const double q = SM_POW_FMA(u, r2, trel + rr);
    return SM_POW_LDEXP(SM_POW_FMA(th, q, th), e);  // ldexp: correct subnormals, +0, +inf
}
// Every x: beyond +-746 the result is +0 / +inf (exp(-745.14) is half the smallest subnormal, exp(709.79) overflows).
template <typename TAB>
SM_POW_FN double exp_general(double x, const TAB &tab) {
    const uint64_t ix = f64_bits(x), ax = ix & 0x7fffffffffffffffULL;
    const bool far = ax >= 0x4087500000000000ULL;  // 746.0
    const double core = exp_core(far ? 0.0 : x, tab);
    uint64_t r = f64_bits(core);
    r = far ? ((ix >> 63) ? 0ULL : 0x7ff0000000000000ULL) : r;
    r = ax > 0x7ff0000000000000ULL ? 0x7ff8000000000000ULL : r;
    return bits_f64(r);
}
template <int W, typename TAB>
SM_POW_FN void exp_n(const double (&x)[W], double (&out)[W], const TAB &tab) {
    uint32_t worst = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {
        const uint32_t h = (uint32_t)(f64_bits(x[k]) >> 32) & 0x7fffffffu;
        worst = h > worst ? h : worst;
    }
    if (!smpow::any_lane(worst >= 0x40875000u)) {
#pragma unroll
        for (int k = 0; k < W; ++k) out[k] = exp_core(x[k], tab);
        return;
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
        double xs = x[k];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(xs));
#endif
        out[k] = exp_general(xs, tab);
    }
}

// ------------------------------------------------------------------------------------------------------------ f64 log
// The log half of smpow64::pow_core_t: ln(ax) for finite ax > 0, rounded once from its hi + lo form.  SUB = false: ax is
// known to be normal.
template <bool SUB, typename TAB>
SM_POW_FN double log_core(double ax, const TAB &tab) {
    uint32_t hi = (uint32_t)(f64_bits(ax) >> 32), lw = (uint32_t)f64_bits(ax);
    int sub = 0;
    if constexpr (SUB) {
        if (hi < 0x00100000u) {  // subnormal: normalise
            const uint64_t nx = f64_bits(ax * 0x1p52);
            hi = (uint32_t)(nx >> 32);
            lw = (uint32_t)nx;
            sub = 52;
        }
    }
    const uint32_t tmp = hi - (uint32_t)(smpow64::kOff >> 32);
    const int i = (int)((tmp >> (20 - 7)) & (smpow64::kN - 1));
    const int k = ((int32_t)tmp >> 20) - sub;
    const double z = smpow::make_f64(hi - (tmp & 0xfff00000u), lw);
    const double invc = tab.invc(i), logc = tab.logc(i), logctail = tab.logctail(i);
    const double kd = (double)k;
    const double Ln2hi = 0x1.62e42f8000000p-1, Ln2lo = 0x1.be8e7bcd5e4f2p-27;
    const double ph = z * invc, pl = SM_POW_FMA(z, invc, -ph);  // z*invc = ph + pl exactly
    const double rm = ph - 1.0;                                 // exact (Sterbenz)
    const double r = rm + pl, rlo = (rm - r) + pl;
    const double t1 = SM_POW_FMA(kd, Ln2hi, logc);  // exact
    const double t2 = t1 + r;
    const double lo1 = SM_POW_FMA(kd, Ln2lo, logctail);
    const double lo2 = (t1 - t2) + r;
    const double ar = -0.5 * r, ar2 = r * ar;
    const double hi2 = t2 + ar2;
    const double lo3 = SM_POW_FMA(ar, r, -ar2);
    const double lo4 = (t2 - hi2) + ar2;
    // r^3 (1/3 - r/4 + r^2/5 - ...), as a polynomial in s = -r/2 (sm_pow64.h: pow_core_t)
    double p = smpow64::fma4_c(ar, 0x1.2492492492492p+1);       // 16/7
    p = smpow64::fma_c(p, ar, 0x1.5555555555555p+0);            //  4/3
    p = smpow64::fma_c(p, ar, 0x1.999999999999ap-1);            //  4/5
    p = SM_POW_FMA(p, ar, 0.5);
    p = smpow64::fma_c(p, ar, 0x1.5555555555555p-2);            //  1/3
    const double r3 = (r * r) * r;
    const double lo = SM_POW_FMA(p, r3, (((lo1 + lo2) + lo3) + lo4) + rlo);
    return hi2 + lo;
}
template <typename TAB>
SM_POW_FN double log_general(double x, const TAB &tab) {
    const uint64_t INF = 0x7ff0000000000000ULL;
    const uint64_t ix = f64_bits(x), ax = ix & 0x7fffffffffffffffULL;
    const bool plain = ix - 1ULL < INF - 1ULL;  // positive, finite, non-zero (subnormals included)
    const double core = log_core<true>(plain ? x : 1.0, tab);
    uint64_t r = f64_bits(core);
    r = (ix >> 63) ? 0x7ff8000000000000ULL : r;  // log(x < 0) = NaN
    r = ax == 0 ? 0xfff0000000000000ULL : r;     // log(+-0) = -inf
    r = ix == INF ? INF : r;                     // log(+inf) = +inf
    r = ax > INF ? 0x7ff8000000000000ULL : r;    // NaN
    return bits_f64(r);
}
template <int W, typename TAB>
SM_POW_FN void log_n(const double (&x)[W], double (&out)[W], const TAB &tab) {
    uint32_t worst = 0;
#pragma unroll
    for (int k = 0; k < W; ++k) {  // ordinary <=> positive and normal: visible in the high word (sm_pow64.h: oddness)
        const uint32_t d = (uint32_t)(f64_bits(x[k]) >> 32) - smpow64::kMinNormalHi;
        worst = d > worst ? d : worst;
    }
    if (!smpow::any_lane(worst >= smpow64::kOrdinarySpan)) {
#pragma unroll
        for (int k = 0; k < W; ++k) out[k] = log_core<false>(x[k], tab);
        return;
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
        double xs = x[k];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(xs));
#endif
        out[k] = log_general(xs, tab);
    }
}

SM_POW_FN double exp(double x) {
    const double xs[1] = {x};
    double r[1];
    exp_n<1>(xs, r, smpow64::TabAoS{smpow64::kLogTab, smpow64::kExpTab});
    return r[0];
}
SM_POW_FN double log(double x) {
    const double xs[1] = {x};
    double r[1];
    log_n<1>(xs, r, smpow64::TabAoS{smpow64::kLogTab, smpow64::kExpTab});
    return r[0];
}

}  // namespace smunary
