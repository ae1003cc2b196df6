// convert_host_check.cpp -- the 12 conversions of simplemath_amd/csrc/sm_convert.h (the source the gfx950 kernels inline) compiled for
// the CPU and checked over edge sets against expectations computed another way:
//   integer -> float   round to nearest even done in integer arithmetic on the magnitude, and long double (64-bit significand:
//                      every int64_t exactly) rounded once
//   float -> float     the bits taken apart and rounded in integer arithmetic
//   float -> integer   the rule written out on the double value: NaN -> 0, trunc, compared against 2^31 / 2^63
// No GPU library involved.  Exits non-zero at the first mismatch.  Built with -fsanitize=undefined,float-cast-overflow it also shows that
// no out-of-range cast is reachable.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sm_convert.h"

namespace {

uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
uint64_t bits(double x) { uint64_t u; memcpy(&u, &x, 8); return u; }
float f32_of(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
double f64_of(uint64_t u) { double x; memcpy(&x, &u, 8); return x; }

long long checked = 0;

[[noreturn]] void die(const char *pair, const char *in, const char *got, const char *want) {
    printf("MISMATCH %s: in %s got %s want %s\n", pair, in, got, want);
    exit(1);
}

// |x| rounded to P significant bits, nearest even, as magnitude * 2^0: returns (q, shift) with value q * 2^shift, q <= 2^P
void round_mag(uint64_t mag, int P, uint64_t *q, int *shift) {
    *q = mag;
    *shift = 0;
    if (mag == 0) return;
    const int e = 63 - __builtin_clzll(mag);
    if (e < P) return;
    const int sh = e - (P - 1);
    uint64_t v = mag >> sh;
    const uint64_t rem = mag & (((uint64_t)1 << sh) - 1), half = (uint64_t)1 << (sh - 1);
    if (rem > half || (rem == half && (v & 1))) ++v;
    *q = v;
    *shift = sh;
}

template <typename F>
F int_to_float_expected(int64_t x) {
    const bool neg = x < 0;
    const uint64_t mag = neg ? 0ull - (uint64_t)x : (uint64_t)x;
    uint64_t q;
    int sh;
    round_mag(mag, sizeof(F) == 4 ? 24 : 53, &q, &sh);
    const F r = std::ldexp((F)q, sh);  // q <= 2^P: exact
    return neg ? -r : r;
}

template <typename I, typename F>
void check_int_to_float(const char *pair, I x, F got) {
    const F want = int_to_float_expected<F>((int64_t)x);
    const F want_ld = (F)(long double)x;
    ++checked;
    if (bits(got) != bits(want) || bits(got) != bits(want_ld)) {
        char a[64], b[64], c[64];
        snprintf(a, sizeof a, "%" PRId64, (int64_t)x);
        snprintf(b, sizeof b, "%a", (double)got);
        snprintf(c, sizeof c, "%a / %a", (double)want, (double)want_ld);
        die(pair, a, b, c);
    }
}

// the rule on the double value
template <typename I>
I float_to_int_expected(double d) {
    if (std::isnan(d)) return 0;
    const double t = std::trunc(d);
    if (sizeof(I) == 4) {
        if (t >= 2147483648.0) return (I)INT32_MAX;
        if (t < -2147483648.0) return (I)INT32_MIN;
        return (I)(int64_t)t;  // |t| <= 2^31: fits int64_t, and the narrowing keeps the value
    }
    if (t >= 9223372036854775808.0) return (I)INT64_MAX;
    if (t <= -9223372036854775808.0) return (I)INT64_MIN;
    return (I)(int64_t)t;
}

template <typename F, typename I>
void check_float_to_int(const char *pair, F x, I got) {
    const I want = float_to_int_expected<I>((double)x);
    ++checked;
    if (got != want) {
        char a[64], b[64], c[64];
        snprintf(a, sizeof a, "%a", (double)x);
        snprintf(b, sizeof b, "%" PRId64, (int64_t)got);
        snprintf(c, sizeof c, "%" PRId64, (int64_t)want);
        die(pair, a, b, c);
    }
}

double widen_expected(float x, bool *nan) {
    const uint32_t u = bits(x);
    const int e = (int)((u >> 23) & 0xff);
    const uint32_t m = u & 0x7fffffu;
    const bool neg = u >> 31;
    *nan = e == 255 && m != 0;
    double r;
    if (e == 255) r = INFINITY;
    else if (e == 0) r = std::ldexp((double)m, -149);
    else r = std::ldexp((double)(m | 0x800000u), e - 150);
    return neg ? -r : r;
}

float narrow_expected(double x, bool *nan) {
    const uint64_t u = bits(x);
    const int e = (int)((u >> 52) & 0x7ff);
    const uint64_t m = u & 0xfffffffffffffull;
    const bool neg = u >> 63;
    *nan = e == 2047 && m != 0;
    float r;
    if (e == 2047) r = INFINITY;
    else if (e == 0) r = 0.0f;  // below 2^-1022: far under half the smallest float subnormal
    else {
        const int E = e - 1023;                       // value = M * 2^(E - 52), M in [2^52, 2^53)
        const uint64_t M = m | ((uint64_t)1 << 52);
        const int quantum = E - 23 > -149 ? E - 23 : -149;  // the weight of the result's last bit
        const int sh = quantum - (E - 52);            // >= 29
        if (sh >= 64) r = 0.0f;
        else {
            uint64_t v = M >> sh;
            const uint64_t rem = M & (((uint64_t)1 << sh) - 1), half = (uint64_t)1 << (sh - 1);
            if (rem > half || (rem == half && (v & 1))) ++v;
            r = std::ldexp((float)v, quantum);  // v <= 2^24: exact; beyond the largest float: +inf, as the rule says
        }
    }
    return neg ? -r : r;
}

std::vector<float> f32_sources() {
    std::vector<float> v;
    const uint32_t mant[] = {0u, 1u, 1u << 22, (1u << 22) - 1, (1u << 22) + 1, 0x7fffffu};
    for (uint32_t s = 0; s < 2; ++s)
        for (uint32_t e = 0; e < 256; ++e)
            for (uint32_t m : mant) v.push_back(f32_of((s << 31) | (e << 23) | m));  // +-0, +-inf and NaNs are among them
    const float extra[] = {2147483648.0f, 2147483520.0f, -2147483648.0f, -2147483904.0f, 9223372036854775808.0f, 9223371487098961920.0f,
                           -9223372036854775808.0f, -9223373136366403584.0f, 0.9f, -0.9f, 1.5f, -1.5f, 0.5f, -0.5f, 1.0f, -1.0f,
                           4294967296.0f, -4294967296.0f, 16777216.0f, 16777217.0f, 8388607.5f, -8388607.5f};
    for (float x : extra) v.push_back(x);
    uint64_t lcg = 12345;
    for (int i = 0; i < 200000; ++i) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        v.push_back(f32_of((uint32_t)(lcg >> 32)));
    }
    return v;
}

std::vector<double> f64_sources() {
    std::vector<double> v;
    const uint64_t h = (uint64_t)1 << 51;
    const uint64_t mant[] = {0ull, 1ull, h, h - 1, h + 1, 0xfffffffffffffull, (uint64_t)1 << 28, ((uint64_t)1 << 28) + 1, ((uint64_t)1 << 28) - 1,
                             ((uint64_t)3 << 28), ((uint64_t)3 << 28) + 1, ((uint64_t)3 << 28) - 1};  // the last six: ties of the f32 rounding
    for (uint64_t s = 0; s < 2; ++s)
        for (uint64_t e = 0; e < 2048; ++e)
            for (uint64_t m : mant) v.push_back(f64_of((s << 63) | (e << 52) | m));
    const double extra[] = {2147483648.0, 2147483520.0, 2147483647.99, 2147483647.0, -2147483648.0, -2147483648.99, -2147483649.0, -2147483649.5,
                            9223372036854775808.0, 9223372036854774784.0, -9223372036854775808.0, -9223372036854777856.0, 0.9, -0.9, 1.5, -1.5,
                            1e39, -1e39, 1e-40, -1e-40, 1e-46, -1e-46, 0x1.ffffffp+127, 0x1.fffffefffffffp+127, 0x1.ffffff0000001p+127,
                            0x1.fffffep+127, 0x1p-149, 0x1p-150, 0x1.0000000000001p-150, 0x1.8p-149, 0x1p-126, 0x1.fffffffffffffp-127};
    for (double x : extra) v.push_back(x);
    uint64_t lcg = 999;
    for (int i = 0; i < 200000; ++i) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        v.push_back(f64_of(lcg));
        // a double inside float's range, so that the narrowing's rounding (and not only its overflow) is exercised
        v.push_back(f64_of((lcg & 0x800fffffffffffffull) | ((uint64_t)(1023 - 160 + (lcg >> 52) % 300) << 52)));
    }
    return v;
}

std::vector<int64_t> i64_sources() {
    std::vector<int64_t> v;
    auto both = [&](uint64_t u) {
        v.push_back((int64_t)u);
        v.push_back((int64_t)(0ull - u));
    };
    for (int p = 0; p < 64; ++p) {
        const uint64_t b = (uint64_t)1 << p;
        both(b);
        both(b + 1);
        both(b - 1);
        for (int drop : {24, 53}) {  // the ties of the f32 / f64 rounding and their neighbours
            if (p < drop) continue;
            const uint64_t t = (uint64_t)1 << (p - drop);
            for (uint64_t k : {t, 3 * t}) {
                both(b + k);
                both(b + k + 1);
                both(b + k - 1);
            }
        }
    }
    for (int64_t x : {INT64_MIN, INT64_MAX, (int64_t)INT32_MIN, (int64_t)INT32_MAX, (int64_t)0, ((int64_t)1 << 60) + ((int64_t)1 << 36) + 1,
                      -(((int64_t)1 << 60) + ((int64_t)1 << 36) + 1)})
        v.push_back(x);
    uint64_t lcg = 777;
    for (int i = 0; i < 200000; ++i) {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        v.push_back((int64_t)lcg >> (int)((lcg >> 3) % 64));  // every magnitude
    }
    return v;
}

}  // namespace

int main() {
    using namespace smconvert;
    const std::vector<float> fs = f32_sources();
    const std::vector<double> ds = f64_sources();
    const std::vector<int64_t> ls = i64_sources();
    std::vector<int32_t> is;
    for (int64_t x : ls) is.push_back(i64_to_i32(x));  // the low words: +-2^p, +-(2^p +- 1), the f32 ties, INT_MIN / INT_MAX among them

    if (i64_to_f32(((int64_t)1 << 60) + ((int64_t)1 << 36) + 1) != 0x1.000002p+60f) {
        printf("MISMATCH i64->f32: 2^60 + 2^36 + 1 was rounded twice\n");
        return 1;
    }
    for (int64_t x : ls) {
        const int32_t lo = i64_to_i32(x);
        ++checked;
        if ((uint32_t)lo != (uint32_t)((uint64_t)x & 0xffffffffu)) die("i64->i32", "?", "?", "the low 32 bits");
        check_int_to_float<int64_t, float>("i64->f32", x, i64_to_f32(x));
        check_int_to_float<int64_t, double>("i64->f64", x, i64_to_f64(x));
        check_int_to_float<int64_t, float>("i64->f32 (convert<>)", x, convert<float>(x));
    }
    for (int32_t x : is) {
        const int64_t w = i32_to_i64(x);
        ++checked;
        if (w != (x < 0 ? -(int64_t)(0u - (uint32_t)x) : (int64_t)(uint32_t)x)) die("i32->i64", "?", "?", "sign extension");
        check_int_to_float<int32_t, float>("i32->f32", x, i32_to_f32(x));
        check_int_to_float<int32_t, double>("i32->f64", x, i32_to_f64(x));
        if ((int64_t)i32_to_f64(x) != (int64_t)x) die("i32->f64", "?", "?", "exact");
    }
    for (float x : fs) {
        check_float_to_int<float, int32_t>("f32->i32", x, f32_to_i32(x));
        check_float_to_int<float, int64_t>("f32->i64", x, f32_to_i64(x));
        bool nan;
        const double want = widen_expected(x, &nan), got = f32_to_f64(x);
        ++checked;
        if (nan ? !std::isnan(got) : bits(got) != bits(want)) {
            char a[64], b[64], c[64];
            snprintf(a, sizeof a, "%a", (double)x);
            snprintf(b, sizeof b, "%a", got);
            snprintf(c, sizeof c, "%a", want);
            die("f32->f64", a, b, c);
        }
    }
    for (double x : ds) {
        check_float_to_int<double, int32_t>("f64->i32", x, f64_to_i32(x));
        check_float_to_int<double, int64_t>("f64->i64", x, f64_to_i64(x));
        bool nan;
        const float want = narrow_expected(x, &nan), got = f64_to_f32(x);
        ++checked;
        if (nan ? !std::isnan(got) : bits(got) != bits(want)) {
            char a[64], b[64], c[64];
            snprintf(a, sizeof a, "%a", x);
            snprintf(b, sizeof b, "%a", (double)got);
            snprintf(c, sizeof c, "%a", (double)want);
            die("f64->f32", a, b, c);
        }
    }
    // the named cases of the contract, spelt out
    struct { double in; int32_t i32; int64_t i64; } named[] = {
        {NAN, 0, 0}, {-0.0, 0, 0}, {-0.9, 0, 0}, {0.9, 0, 0}, {1.5, 1, 1}, {-1.5, -1, -1}, {INFINITY, INT32_MAX, INT64_MAX},
        {-INFINITY, INT32_MIN, INT64_MIN}, {2147483647.99, INT32_MAX, 2147483647}, {-2147483648.99, INT32_MIN, -2147483648LL},
        {2147483648.0, INT32_MAX, 2147483648LL}, {9223372036854775808.0, INT32_MAX, INT64_MAX}, {9223372036854774784.0, INT32_MAX, 9223372036854774784LL},
        {1e300, INT32_MAX, INT64_MAX}, {-1e300, INT32_MIN, INT64_MIN}};
    for (const auto &c : named) {
        ++checked;
        if (f64_to_i32(c.in) != c.i32 || f64_to_i64(c.in) != c.i64) {
            printf("MISMATCH named case %a: got %d / %" PRId64 "\n", c.in, f64_to_i32(c.in), f64_to_i64(c.in));
            return 1;
        }
    }
    printf("convert_host_check: %lld checks over %zu f32, %zu f64, %zu i64 and %zu i32 sources, 0 mismatches\n", checked, fs.size(), ds.size(), ls.size(),
           is.size());
    return 0;
}
