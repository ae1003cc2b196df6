// Host check of simplemath_amd/csrc/sm_unary.h (the same source the gfx950 kernels inline): the largest distance, in ULPs of
// the result type, between each function and the true value over a dense sweep, plus the C99 Annex F special values.
//   f32: reference = glibc's fp64 exp / log of the argument (NOT expf / logf: a second f32 routine would add its own error)
//   f64: reference = expl / logl in long double (64-bit significand)
// Prints, per function, "<name> max_ulp <x> over <count> (x=<worst argument>)" and, once, "lattice_mismatches <n>".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

#include "sm_unary.h"

static uint64_t mix(uint64_t x) { x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ULL; x ^= x >> 27; x *= 0x94D049BB133111EBULL; x ^= x >> 31; return x; }
static float f32_of(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static uint32_t bits_of(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static double f64_of(uint64_t u) { double f; memcpy(&f, &u, 8); return f; }
static uint64_t bits_of(double f) { uint64_t u; memcpy(&u, &f, 8); return u; }

// |got - want| in units of the spacing of T's grid at `want` (the subnormal spacing below the smallest normal; an
// infinite result counts as the grid point after the largest finite one)
template <typename T, typename R>
static double ulp_error(T got, R want) {
    constexpr int kMant = std::numeric_limits<T>::digits - 1, kMinExp = std::numeric_limits<T>::min_exponent - 1;  // 23 / -126, 52 / -1022
    const R top = std::ldexp((R)1, std::numeric_limits<T>::max_exponent);
    if (got != got) return 1e30;
    R g = std::isinf(got) ? (got > 0 ? top : -top) : (R)got;
    R w = want > top ? top : (want < -top ? -top : want);
    int e;
    std::frexp(w, &e);  // |w| = m 2^e, m in [0.5, 1)
    e -= 1;
    if (e < kMinExp) e = kMinExp;
    if (w == 0) e = kMinExp;
    const R d = g > w ? g - w : w - g;
    return (double)std::ldexp(d, kMant - e);
}

struct Worst { double ulp = 0; double x = 0; uint64_t count = 0; };
template <typename T> static void note(Worst &w, double err, T x) { if (err > w.ulp) { w.ulp = err; w.x = (double)x; } ++w.count; }

int main(int argc, char **argv) {
    const uint64_t scale = argc > 1 ? strtoull(argv[1], nullptr, 10) : 1;  // 1: the full sweep
    const uint64_t n32 = 2200000 * scale, n64 = 1000000 * scale;
    Worst wexpf, wlogf, wexp, wlog;

    // ---- f32 exp: any bit pattern (every binade, both signs, subnormals), the range that matters, tiny arguments, ...
    for (uint64_t i = 0; i < n32 * 4; ++i) {
        const uint64_t h = mix(i * 0x9E3779B97F4A7C15ULL + 1);
        float x;
        switch (i & 3) {
            case 0: x = f32_of((uint32_t)h); break;
            case 1: x = -105.0f + (float)((h >> 40) * 0x1.0p-24) * 195.0f; break;
            case 2: x = f32_of(((uint32_t)h & 0x807fffffu) | ((uint32_t)((h >> 32) % 140) << 23)); break;  // |x| < 2^13, every binade below alike (subnormals: exponent 0)
            default: x = ((float)((h >> 40) * 0x1.0p-24) - 0.5f) * 2.0f; break;
        }
        if (x != x) continue;
        note(wexpf, ulp_error<float, double>(smunary::expf(x), std::exp((double)x)), x);
    }
    // ... and every value within 64 ULP of the overflow threshold, the underflow-to-zero threshold and the first subnormal result
    for (float centre : {88.72284f, -103.972084f, -87.33655f, 0.0f}) {
        const uint32_t c = bits_of(centre);
        for (int d = -64; d <= 64; ++d) {
            const float x = centre == 0.0f ? f32_of((uint32_t)(d < 0 ? 0x80000000u - d : d)) : f32_of(c + d);
            note(wexpf, ulp_error<float, double>(smunary::expf(x), std::exp((double)x)), x);
        }
    }
    // ---- f32 log: any positive bit pattern (every binade, subnormals), a range around 1, a dense cluster at 1, subnormals
    for (uint64_t i = 0; i < n32 * 4; ++i) {
        const uint64_t h = mix(i * 0x9E3779B97F4A7C15ULL + 2);
        float x;
        switch (i & 3) {
            case 0: x = f32_of((uint32_t)h & 0x7fffffffu); break;
            case 1: x = 0.01f + (float)((h >> 40) * 0x1.0p-24) * 99.99f; break;
            case 2: x = 1.0f + ((float)((h >> 40) * 0x1.0p-24) - 0.5f) * ((h & 1) ? 1e-3f : 0.6f); break;
            default: x = f32_of((uint32_t)h & 0x007fffffu); break;
        }
        if (x != x || std::isinf(x) || x == 0.0f) continue;
        note(wlogf, ulp_error<float, double>(smunary::logf(x), std::log((double)x)), x);
    }
    for (int d = -64; d <= 64; ++d) {
        const float x = f32_of(0x3f800000u + d);
        note(wlogf, ulp_error<float, double>(smunary::logf(x), std::log((double)x)), x);
    }
    // ---- f64 exp
    for (uint64_t i = 0; i < n64 * 4; ++i) {
        const uint64_t h = mix(i * 0x9E3779B97F4A7C15ULL + 3);
        double x;
        switch (i & 3) {
            case 0: x = f64_of(h); break;
            case 1: x = -750.0 + (double)(h >> 11) * 0x1.0p-53 * 1460.0; break;
            case 2: x = f64_of((h & 0x800fffffffffffffULL) | ((uint64_t)((h >> 52) % 1034) << 52)); break;  // |x| < 2^11, every binade below alike
            default: x = ((double)(h >> 11) * 0x1.0p-53 - 0.5) * 2.0; break;
        }
        if (x != x) continue;
        note(wexp, ulp_error<double, long double>(smunary::exp(x), expl((long double)x)), x);
    }
    for (double centre : {709.782712893384, -745.1332191019411, -708.3964185322641}) {
        const uint64_t c = bits_of(centre);
        for (int d = -64; d <= 64; ++d) {
            const double x = f64_of(c + d);
            note(wexp, ulp_error<double, long double>(smunary::exp(x), expl((long double)x)), x);
        }
    }
    // ---- f64 log
    for (uint64_t i = 0; i < n64 * 4; ++i) {
        const uint64_t h = mix(i * 0x9E3779B97F4A7C15ULL + 4);
        double x;
        switch (i & 3) {
            case 0: x = f64_of(h & 0x7fffffffffffffffULL); break;
            case 1: x = 0.01 + (double)(h >> 11) * 0x1.0p-53 * 99.99; break;
            case 2: x = 1.0 + ((double)(h >> 11) * 0x1.0p-53 - 0.5) * ((h & 1) ? 1e-3 : 0.6); break;
            default: x = f64_of(h & 0x000fffffffffffffULL); break;
        }
        if (x != x || std::isinf(x) || x == 0.0) continue;
        note(wlog, ulp_error<double, long double>(smunary::log(x), logl((long double)x)), x);
    }
    for (int d = -64; d <= 64; ++d) {
        const double x = f64_of(0x3ff0000000000000ULL + d);
        note(wlog, ulp_error<double, long double>(smunary::log(x), logl((long double)x)), x);
    }
    printf("expf max_ulp %.4f over %llu (x=%a)\n", wexpf.ulp, (unsigned long long)wexpf.count, wexpf.x);
    printf("logf max_ulp %.4f over %llu (x=%a)\n", wlogf.ulp, (unsigned long long)wlogf.count, wlogf.x);
    printf("exp max_ulp %.4f over %llu (x=%a)\n", wexp.ulp, (unsigned long long)wexp.count, wexp.x);
    printf("log max_ulp %.4f over %llu (x=%a)\n", wlog.ulp, (unsigned long long)wlog.count, wlog.x);

    // ---- the special values: identical to libm's answer, sign of zero included; NaN for NaN
    int bad = 0;
    auto same32 = [&](const char *what, float x, float got, float want) {
        const bool ok = (got != got && want != want) || bits_of(got) == bits_of(want);
        if (!ok) { ++bad; printf("lattice %s x=%a got=%a want=%a\n", what, x, got, want); }
    };
    auto same64 = [&](const char *what, double x, double got, double want) {
        const bool ok = (got != got && want != want) || bits_of(got) == bits_of(want);
        if (!ok) { ++bad; printf("lattice %s x=%a got=%a want=%a\n", what, x, got, want); }
    };
    const float inff = std::numeric_limits<float>::infinity(), nanf_ = std::numeric_limits<float>::quiet_NaN();
    for (float x : {0.0f, -0.0f, inff, -inff, nanf_, -nanf_, 1000.0f, -1000.0f, 89.0f, -104.5f, -150.0f, 3.4028235e38f, -3.4028235e38f, 1e-45f, -1e-45f,
                    f32_of(0x7fa00000u) /* signalling NaN */})
        same32("expf", x, smunary::expf(x), (float)std::exp((double)x));
    for (float x : {0.0f, -0.0f, inff, -inff, nanf_, -nanf_, 1.0f, -1.0f, -1e-45f, -3.4028235e38f, f32_of(0x7fa00000u)})
        same32("logf", x, smunary::logf(x), (float)std::log((double)x));
    for (float x : {1e-45f, 1.17549435e-38f, 1.1754942e-38f, 3.4028235e38f, 2.0f, 0.5f})  // finite results at the edges: correctly rounded here
        same32("logf", x, smunary::logf(x), (float)std::log((double)x));
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    for (double x : {0.0, -0.0, inf, -inf, nan, -nan, 1000.0, -1000.0, 746.0, -746.0, 1e300, -1e300, 1.7976931348623157e308, -1.7976931348623157e308,
                     f64_of(0x7ff4000000000000ULL)})
        same64("exp", x, smunary::exp(x), std::exp(x));
    for (double x : {5e-324, -5e-324, 1e-320, -1e-310})  // exp of a subnormal is 1 to the last bit
        same64("exp", x, smunary::exp(x), 1.0);
    for (double x : {0.0, -0.0, inf, -inf, nan, -nan, 1.0, -1.0, -5e-324, -1.7976931348623157e308, f64_of(0x7ff4000000000000ULL)})
        same64("log", x, smunary::log(x), std::log(x));
    printf("lattice_mismatches %d\n", bad);
    return 0;
}
