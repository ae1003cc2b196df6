// random_host_check.cpp -- simplemath_amd/csrc/sm_random.h (the source the gfx950 kernels inline) compiled for the CPU: no GPU library.
//   random_host_check kat                                the three Random123 known answers of Philox4x32-10
//   random_host_check values SEED STREAM OFFSET N        the first N elements of every kind / dtype as hexadecimal bit patterns, one line
//                                                        each: "<kind> <dtype> <bits> ..."; parameters as kValueParams below
//   random_host_check accuracy                           the pieces of the normal against long double: f32 over all 2^24 inputs, f64 over
//                                                        2^22 pseudo-random 53-bit inputs and the edge sets; one line per piece:
//                                                        "<piece> max_ulp <error> at <argument>"
//   random_host_check                                    kat + accuracy
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>

#include "sm_random.h"

using namespace smrandom;

// ---------------------------------------------------------------------------------------------------------- known answers
static int run_kat() {
    struct Case { uint32_t ctr[4], key[2], want[4]; };
    const Case cases[3] = {
        {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
        {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
        {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
    };
    int bad = 0;
    for (const Case &c : cases) {
        uint32_t out[4];
        philox4x32_10(c.ctr, c.key, out);
        std::printf("kat %08x %08x %08x %08x\n", out[0], out[1], out[2], out[3]);
        bad += std::memcmp(out, c.want, sizeof out) != 0;
    }
    // the same through block_words: (seed, stream, b) -> (key, counter)
    uint32_t w[4];
    block_words(0x299f31d0a4093822ull, 0x0370734413198a2eull, 0x85a308d3243f6a88ull, w);
    bad += std::memcmp(w, cases[2].want, sizeof w) != 0;
    std::printf("kat: %d mismatches\n", bad);
    return bad;
}

// ------------------------------------------------------------------------------------------------------------------ values
// The parameters of the `values` mode (tests/test_random_host.py mirrors them).
static const double kUniform[2] = {0.0, 1.0}, kNormal[2] = {0.0, 1.0}, kIntegers[2] = {-7.0, 993.0}, kBernoulli = 0.3;

template <typename T>
static void print_bits(T v) {
    if constexpr (sizeof(T) == 4) {
        uint32_t b;
        std::memcpy(&b, &v, 4);
        std::printf(" %08x", b);
    } else {
        uint64_t b;
        std::memcpy(&b, &v, 8);
        std::printf(" %016llx", (unsigned long long)b);
    }
}

template <int KIND, typename T>
static void print_values(const char *kind, const char *dtype, uint64_t seed, uint64_t stream, uint64_t offset, uint64_t n, const Params<T> &p) {
    constexpr int PB = PerBlock<KIND, T>::value;
    std::printf("%s %s", kind, dtype);
    for (uint64_t b = 0; b * PB < n; ++b) {
        uint32_t w[4];
        block_words(seed, stream, offset + b, w);
        T v[PB];
        block_values<KIND, T>(w, p, v);
        for (int k = 0; k < PB && b * PB + k < n; ++k) print_bits(v[k]);
    }
    std::printf("\n");
}

template <typename T>
static Params<T> params(double a, double b, int64_t lo, uint64_t u) {
    Params<T> p;
    p.a = (T)a, p.b = (T)b, p.lo = lo, p.u = u;
    return p;
}

static int run_values(uint64_t seed, uint64_t stream, uint64_t offset, uint64_t n) {
    const uint64_t thr = (uint64_t)std::floor(kBernoulli * 0x1p32);
    const int64_t ilo = (int64_t)kIntegers[0];
    const uint64_t R = (uint64_t)(kIntegers[1] - kIntegers[0]);
    print_values<BITS, int32_t>("bits", "i32", seed, stream, offset, n, params<int32_t>(0, 0, 0, 0));
    print_values<BITS, int64_t>("bits", "i64", seed, stream, offset, n, params<int64_t>(0, 0, 0, 0));
    print_values<UNIFORM, float>("uniform", "f32", seed, stream, offset, n, params<float>(kUniform[0], kUniform[1] - kUniform[0], 0, 0));
    print_values<UNIFORM, double>("uniform", "f64", seed, stream, offset, n, params<double>(kUniform[0], kUniform[1] - kUniform[0], 0, 0));
    print_values<INTEGERS, int32_t>("integers", "i32", seed, stream, offset, n, params<int32_t>(0, 0, ilo, R));
    print_values<INTEGERS, int64_t>("integers", "i64", seed, stream, offset, n, params<int64_t>(0, 0, ilo, R));
    print_values<BERNOULLI, float>("bernoulli", "f32", seed, stream, offset, n, params<float>(0, 0, 0, thr));
    print_values<BERNOULLI, double>("bernoulli", "f64", seed, stream, offset, n, params<double>(0, 0, 0, thr));
    print_values<BERNOULLI, int32_t>("bernoulli", "i32", seed, stream, offset, n, params<int32_t>(0, 0, 0, thr));
    print_values<BERNOULLI, int64_t>("bernoulli", "i64", seed, stream, offset, n, params<int64_t>(0, 0, 0, thr));
    print_values<NORMAL, float>("normal", "f32", seed, stream, offset, n, params<float>(kNormal[0], kNormal[1], 0, 0));
    print_values<NORMAL, double>("normal", "f64", seed, stream, offset, n, params<double>(kNormal[0], kNormal[1], 0, 0));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- accuracy
// |got - want| in spacings of T at want (test_unary.cpp's measure).
template <typename T>
static double ulps(T got, long double want) {
    if (want == 0) return got == 0 ? 0.0 : std::numeric_limits<double>::infinity();
    int e;
    std::frexp((double)want, &e);
    const long double ulp = std::ldexp(1.0L, e - std::numeric_limits<T>::digits);
    return (double)(std::fabs((long double)got - want) / ulp);
}

// {cos, sin} of 2 pi m / 2^B in long double: the octant reduction in integers, the functions on at most 1/8 turn.
static void cossin_ref(uint64_t m, int B, long double *c, long double *s) {
    const unsigned q = (unsigned)(m >> (B - 3));
    const uint64_t one = (uint64_t)1 << (B - 3), f = m & (one - 1), g = (q & 1) ? one - f : f;
    const long double two_pi = 6.283185307179586476925286766559005768L;
    const long double a = two_pi * std::ldexp((long double)g, -B);
    const long double C = g == one ? sqrtl(0.5L) : cosl(a), S = g == one ? sqrtl(0.5L) : sinl(a);
    switch (q) {
        case 0: *c = C, *s = S; break;
        case 1: *c = S, *s = C; break;
        case 2: *c = -S, *s = C; break;
        case 3: *c = -C, *s = S; break;
        case 4: *c = -C, *s = -S; break;
        case 5: *c = -S, *s = -C; break;
        case 6: *c = S, *s = -C; break;
        default: *c = C, *s = -S; break;
    }
}

struct Worst {
    double err = 0;
    uint64_t arg = 0;
    void see(double e, uint64_t a) {
        if (e > err) err = e, arg = a;
    }
    void print(const char *what) const { std::printf("%s max_ulp %.4f at %llu\n", what, err, (unsigned long long)arg); }
};

static uint64_t g_state = 0x243f6a8885a308d3ull;
static uint64_t next53() {
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (z ^ (z >> 31)) >> 11;
}

static int run_accuracy() {
    int bad = 0;
    {   // f32: every input
        Worst wr, wc, ws;
        for (uint32_t k = 0; k < (1u << 24); ++k) {
            const long double u1 = std::ldexp((long double)(k + 1), -24);
            wr.see(ulps<float>(radius_f32(k), sqrtl(-2.0L * logl(u1))), k);
            float c, s;
            cossin_f32(k, &c, &s);
            long double rc, rs;
            cossin_ref(k, 24, &rc, &rs);
            wc.see(ulps<float>(c, rc), k);
            ws.see(ulps<float>(s, rs), k);
        }
        wr.print("r_f32"), wc.print("cospi_f32"), ws.print("sinpi_f32");
        float c, s;
        cossin_f32(1u << 22, &c, &s);  // t = 1/4
        bad += c != 0.0f || s != 1.0f;
        cossin_f32(0, &c, &s);
        bad += s != 0.0f || c != 1.0f;
        bad += radius_f32((1u << 24) - 1) != 0.0f;  // u1 = 1
    }
    {   // f64: 2^22 pseudo-random 53-bit inputs and the edges
        Worst wr, wc, ws;
        auto radius = [&](uint64_t k) {
            const long double u1 = std::ldexp((long double)(k + 1), -53);
            wr.see(ulps<double>(radius_f64(k), sqrtl(-2.0L * logl(u1))), k);
        };
        auto turn = [&](uint64_t m) {
            double c, s;
            cossin_f64(m, &c, &s);
            long double rc, rs;
            cossin_ref(m, 53, &rc, &rs);
            wc.see(ulps<double>(c, rc), m);
            ws.see(ulps<double>(s, rs), m);
        };
        for (int i = 0; i < (1 << 22); ++i) {
            radius(next53());
            turn(next53());
        }
        const uint64_t top = (uint64_t)1 << 53;
        radius(0), radius(top - 2), radius(top - 1);  // u1 = 2^-53, 1 - 2^-53, 1
        for (int o = 0; o <= 8; ++o)
            for (int64_t d = -64; d <= 64; ++d) {
                const int64_t m = (int64_t)(o * (top >> 3)) + d;
                if (m >= 0 && m < (int64_t)top) turn((uint64_t)m);
            }
        wr.print("r_f64"), wc.print("cospi_f64"), ws.print("sinpi_f64");
        double c, s;
        cossin_f64(top >> 2, &c, &s);
        bad += c != 0.0 || s != 1.0;
        cossin_f64(0, &c, &s);
        bad += s != 0.0 || c != 1.0;
        bad += radius_f64(top - 1) != 0.0;
    }
    std::printf("accuracy: %d exact-value mismatches\n", bad);
    return bad;
}

int main(int argc, char **argv) {
    const char *mode = argc > 1 ? argv[1] : "all";
    if (!std::strcmp(mode, "kat")) return run_kat() ? 1 : 0;
    if (!std::strcmp(mode, "values") && argc == 6)
        return run_values(std::strtoull(argv[2], nullptr, 0), std::strtoull(argv[3], nullptr, 0), std::strtoull(argv[4], nullptr, 0), std::strtoull(argv[5], nullptr, 0));
    if (!std::strcmp(mode, "accuracy")) return run_accuracy() ? 1 : 0;
    if (!std::strcmp(mode, "all")) {
        const int bad = run_kat() + run_accuracy();
        return bad ? 1 : 0;
    }
    std::fprintf(stderr, "usage: random_host_check [kat | values SEED STREAM OFFSET N | accuracy]\n");
    return 2;
}
