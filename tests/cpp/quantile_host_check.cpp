// quantile_host_check.cpp -- the host-and-device arithmetic of quantile / percentile / median (csrc/sm_quantile.h) on the host.
//
//   select   a key-only radix select written here over the header's digit rule (key_of, digit, agrees: 8 bits a pass from the top,
//            stopping when the bin that holds the rank holds one element) against std::nth_element and a full sort under the order of
//            the keys: random lines, heavy ties, zeros of both signs, infinities, NaNs, constant lines; every rank of short lines, a
//            spread of ranks of long ones.  The element found is read as canonical(): a zero is +0.
//   ranks    (j, j1, g) of rank_of for every method at R = 1 .. 5 and q in {0, 1/3, 0.5, 1 - 2^-53, 1}, against the rules of
//            include/smhip.h worked out here in long double and by hand.
//   lerp     the interpolation's special cases: g == 0 (hi not consulted, even a NaN one), lo == hi (equal infinities stay), opposite
//            infinities and an infinity on the side the formula starts from give the canonical NaN, one infinite neighbour on the other
//            side gives the infinity, both branches of numpy's _lerp, an fp64 difference that overflows, one rounding to float.
// No GPU library involved.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "sm_quantile.h"

using namespace smquantile;

static int failures = 0;
static long checks = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        ++checks;                              \
        if (!(cond)) {                         \
            if (++failures <= 20) {            \
                printf("FAIL %s: ", #cond);    \
                printf(__VA_ARGS__);           \
                printf("\n");                  \
            }                                  \
        }                                      \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static uint64_t next() {
    rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return rng_state >> 11;
}
static double uniform() { return ((double)next() + 0.5) / 9007199254740992.0; }  // (0, 1)
static double normal() { return sqrt(-2.0 * log(uniform())) * cos(6.283185307179586 * uniform()); }

template <typename T> static KeyOf<T> bits_of(T x) {
    KeyOf<T> u;
    memcpy(&u, &x, sizeof u);
    return u;
}

// The radix select of the kernels, one lane: the element of rank `rank` (from 0) of v, read as canonical(); *passes = the passes it ran.
template <typename T> static T radix_select(const std::vector<T> &v, size_t rank, int *passes) {
    using K = KeyOf<T>;
    K prefix = 0;
    uint32_t need = (uint32_t)rank + 1;
    int done = 0;
    for (int pass = 0; pass < (int)sizeof(K); ++pass) {
        uint32_t hist[256] = {0};
        for (T x : v) {
            const K key = key_of(x);
            if (agrees(key, prefix, pass)) ++hist[digit(key, pass)];
        }
        uint32_t running = 0;
        for (uint32_t b = 0; b < 256; ++b) {
            if (running < need && need <= running + hist[b]) {
                prefix |= (K)b << shift_of<K>(pass), need -= running, done = pass + 1;
                if (hist[b] == 1) pass = (int)sizeof(K);  // the element is known
                break;
            }
            running += hist[b];
        }
    }
    *passes = done;
    T found = quiet_nan<T>();
    int writers = 0;
    for (T x : v)
        if (agrees(key_of(x), prefix, done)) {
            const T c = canonical(x);
            if (writers++ && !(c != c)) CHECK(bits_of(c) == bits_of(found), "two writers with different bits");
            found = c;
        }
    CHECK(writers >= 1, "nobody agrees with the prefix");
    return found;
}

template <typename T> static void check_select(const std::vector<T> &v, const char *what) {
    std::vector<T> sorted(v);
    const auto by_key = [](T a, T b) { return key_of(a) < key_of(b); };
    std::sort(sorted.begin(), sorted.end(), by_key);
    const size_t n = v.size();
    std::vector<size_t> some;
    for (size_t rank = 0; rank < n; rank += n <= 300 ? 1 : n / 37) some.push_back(rank);
    for (size_t rank : {(size_t)1, n / 2, n - 2, n - 1})
        if (rank < n) some.push_back(rank);
    for (size_t rank : some) {
        int passes = 0;
        const T got = radix_select(v, rank, &passes);
        std::vector<T> w(v);
        std::nth_element(w.begin(), w.begin() + (long)rank, w.end(), by_key);
        const T nth = canonical(w[rank]), srt = canonical(sorted[rank]);
        CHECK(key_of(got) == key_of(nth) && key_of(got) == key_of(srt), "%s n %zu rank %zu", what, n, rank);
        if (got == got) CHECK(bits_of(got) == bits_of(srt) && bits_of(got) == bits_of(nth), "%s n %zu rank %zu: bits", what, n, rank);
        else CHECK(srt != srt, "%s n %zu rank %zu: a NaN where the order has a number", what, n, rank);
        if (got == (T)0) CHECK(bits_of(got) == 0, "%s: a zero that is not +0", what);
        CHECK(passes >= 1 && passes <= (int)sizeof(T), "%s: %d passes", what, passes);
    }
}

template <typename T> static void selects() {
    const T inf = std::numeric_limits<T>::infinity(), nan = std::numeric_limits<T>::quiet_NaN(), tiny = std::numeric_limits<T>::denorm_min();
    for (size_t n : {1u, 2u, 3u, 63u, 64u, 65u, 255u, 256u, 257u, 4095u, 4096u, 4097u, 20497u}) {
        std::vector<T> v(n);
        for (T &x : v) x = (T)normal();
        check_select(v, "continuous");
        for (T &x : v) x = (T)(double)(next() % 7) - (T)3;  // seven values, zero among them
        check_select(v, "ties");
        for (size_t k = 0; k < n; ++k) v[k] = (k & 1) ? (T)-0.0 : (T)0.0;
        check_select(v, "zeros");
        const T pool[] = {(T)0, (T)-0.0, inf, -inf, tiny, -tiny, (T)1, (T)-1, std::numeric_limits<T>::max(), std::numeric_limits<T>::lowest(), nan, -nan};
        for (T &x : v) x = pool[next() % 12];
        check_select(v, "specials");
        for (T &x : v) x = pool[next() % 10];
        check_select(v, "specials without NaN");
        for (T &x : v) x = (T)7.25;
        check_select(v, "constant");
        int passes = 0;
        radix_select(v, n / 2, &passes);
        CHECK(passes == (n == 1 ? 1 : (int)sizeof(T)), "a constant line of %zu ends after %d passes", n, passes);
        for (T &x : v) x = nan;
        check_select(v, "all NaN");
        for (size_t k = 0; k < n; ++k) v[k] = (T)(1.0 + (double)k * 1e-7 * (sizeof(T) == 4 ? 1.0 : 1e-9));  // differ in the low digits only
        check_select(v, "low digits");
    }
    CHECK(key_of((T)-0.0) == key_of((T)0.0) && key_of(-tiny) < key_of((T)0) && key_of((T)0) < key_of(tiny), "the zeros' keys");
    CHECK(key_of(-inf) < key_of(std::numeric_limits<T>::lowest()) && key_of(std::numeric_limits<T>::max()) < key_of(inf) && key_of(inf) < key_of(nan) &&
              key_of(nan) == key_of(-nan) && key_of(nan) == (KeyOf<T>)~(KeyOf<T>)0,
          "the keys at the ends");
    CHECK(bits_of(quiet_nan<T>()) == (sizeof(T) == 4 ? (KeyOf<T>)0x7fc00000u : (KeyOf<T>)0x7ff8000000000000ull), "the canonical NaN");
}

static void ranks() {
    const double qs[] = {0.0, 1.0 / 3.0, 0.5, 1.0 - ldexp(1.0, -53), 1.0};
    for (int64_t R = 1; R <= 5; ++R)
        for (double q : qs) {
            const double h = (double)(R - 1) * q;
            const long double hl = h;
            const int64_t fl = (int64_t)floorl(hl), ce = (int64_t)ceill(hl);
            const double frac = (double)(hl - (long double)fl);
            CHECK(h >= 0 && h <= (double)(R - 1), "h");
            Rank r = rank_of(R, q, kLinear);
            CHECK(r.j == fl && r.g == frac && r.j1 == (frac != 0 ? fl + 1 : fl) && r.j1 <= R - 1, "linear R %lld q %.17g", (long long)R, q);
            r = rank_of(R, q, kLower);
            CHECK(r.j == fl && r.g == 0 && r.j1 == fl, "lower R %lld q %.17g", (long long)R, q);
            r = rank_of(R, q, kHigher);
            CHECK(r.j == ce && r.g == 0 && r.j1 == ce && ce <= R - 1, "higher R %lld q %.17g", (long long)R, q);
            r = rank_of(R, q, kNearest);
            int64_t near = frac < 0.5 ? fl : frac > 0.5 ? ce : (fl % 2 == 0 ? fl : ce);  // ties to even
            CHECK(r.j == near && r.g == 0 && r.j1 == near, "nearest R %lld q %.17g: %lld", (long long)R, q, (long long)r.j);
            r = rank_of(R, q, kMidpoint);
            CHECK(r.j == fl && r.g == (frac != 0 ? 0.5 : 0.0) && r.j1 == (frac != 0 ? fl + 1 : fl), "midpoint R %lld q %.17g", (long long)R, q);
        }
    // by hand: the median of 2 and of 4 falls halfway, of 3 and 5 on an element; nearest's ties go to the even rank
    CHECK(rank_of(2, 0.5, kLinear).j == 0 && rank_of(2, 0.5, kLinear).g == 0.5, "median of 2");
    CHECK(rank_of(4, 0.5, kLinear).j == 1 && rank_of(4, 0.5, kLinear).g == 0.5 && rank_of(4, 0.5, kLinear).j1 == 2, "median of 4");
    CHECK(rank_of(3, 0.5, kLinear).j == 1 && rank_of(3, 0.5, kLinear).g == 0.0 && rank_of(5, 0.5, kLinear).j == 2, "median of 3 and 5");
    CHECK(rank_of(2, 0.5, kNearest).j == 0 && rank_of(4, 0.5, kNearest).j == 2, "nearest's ties");
    CHECK(rank_of(1, 1.0 / 3.0, kLinear).j == 0 && rank_of(1, 1.0 / 3.0, kLinear).g == 0.0, "a line of one");
    // q just below 1: (R - 1) q rounds to R - 1 for R = 2 (h = 1 - 2^-53 is exact: j = 0) and stays below it there
    CHECK(rank_of(2, 1.0 - ldexp(1.0, -53), kLinear).j == 0 && rank_of(2, 1.0 - ldexp(1.0, -53), kLinear).g == 1.0 - ldexp(1.0, -53), "q below 1 at R = 2");
    CHECK(rank_of(4, 1.0 - ldexp(1.0, -53), kLinear).j1 <= 3, "q below 1 at R = 4");
    CHECK(rank_of(((int64_t)1 << 31) - 1, 1.0, kLinear).j == ((int64_t)1 << 31) - 2 && rank_of(((int64_t)1 << 31) - 1, 1.0, kLinear).g == 0.0, "the longest axis");
}

static void lerps() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const float finf = std::numeric_limits<float>::infinity();
    CHECK(interpolate(3.0, nan, 0.0) == 3.0 && interpolate(3.0, inf, 0.0) == 3.0 && interpolate(-inf, inf, 0.0) == -inf, "g == 0: hi is not consulted");
    CHECK(interpolate(inf, inf, 0.3) == inf && interpolate(-inf, -inf, 0.7) == -inf && interpolate(2.5, 2.5, 0.9) == 2.5, "lo == hi");
    CHECK(bits_of(finish<double>(-inf, inf, 0.25)) == 0x7ff8000000000000ull && bits_of(finish<double>(-inf, inf, 0.75)) == 0x7ff8000000000000ull, "opposite infinities");
    CHECK(bits_of(finish<float>(-finf, finf, 0.5)) == 0x7fc00000u, "opposite infinities, f32");
    CHECK(finish<double>(1.0, inf, 0.25) == inf && bits_of(finish<double>(1.0, inf, 0.75)) == 0x7ff8000000000000ull, "hi = +inf");
    CHECK(finish<double>(-inf, 1.0, 0.75) == -inf && bits_of(finish<double>(-inf, 1.0, 0.25)) == 0x7ff8000000000000ull, "lo = -inf");
    CHECK(interpolate(1.0, 3.0, 0.25) == 1.5 && interpolate(1.0, 3.0, 0.75) == 2.5 && interpolate(1.0, 3.0, 0.5) == 2.0, "both branches");
    const double big = std::numeric_limits<double>::max();
    CHECK(interpolate(-big, big, 0.25) == inf && interpolate(-big, big, 0.75) == -inf, "an fp64 difference that overflows gives what the formula gives");
    CHECK(finish<float>(-std::numeric_limits<float>::max(), std::numeric_limits<float>::max(), 0.5) == 0.0f, "f32 extremes do not overflow in fp64");
    CHECK(bits_of(finish<float>(-1.0f, 1.0f, 0.5)) == 0u, "a zero from the formula is +0");
    // each step one operation: lo + d * g with the product rounded before the sum (a fused multiply-add would give the other neighbour)
    {
        const double lo = 1.0, hi = 1.0 + ldexp(1.0, -52) * 3, g = 1.0 / 3.0 + ldexp(1.0, -54);
        const double d = hi - lo;
        volatile double p = d * g;
        const double want = lo + p;
        CHECK(interpolate(lo, hi, g) == want, "the product is rounded before the sum");
    }
    for (int k = 0; k < 20000; ++k) {
        const double lo = normal() * 100, hi = lo + fabs(normal()), g = uniform();
        const double d = hi - lo;
        volatile double p1 = d * g, r = 1.0 - g;
        volatile double p2 = d * r;
        const double want = g < 0.5 ? lo + p1 : hi - p2;
        CHECK(interpolate(lo, hi, g) == want, "random lerp");
        const float fl = (float)lo, fh = (float)hi >= fl ? (float)hi : fl;
        const double df = (double)fh - (double)fl;
        volatile double q1 = df * g, q2 = df * r;
        const float wantf = fl == fh ? fl : (float)(g < 0.5 ? (double)fl + q1 : (double)fh - q2);
        CHECK(bits_of(finish<float>(fl, fh, g)) == bits_of(wantf), "random lerp, f32: one rounding");
        const long double exact = (long double)fl + ((long double)fh - (long double)fl) * (long double)g;
        const double bound = (ldexp(1.0, -24) + 3 * ldexp(1.0, -53)) * fmax(fabs((double)fl), fabs((double)fh)) + (double)std::numeric_limits<float>::denorm_min();
        CHECK(fabsl((long double)finish<float>(fl, fh, g) - exact) <= bound, "the f32 bound of include/smhip.h");
    }
}

int main() {
    selects<float>();
    selects<double>();
    ranks();
    lerps();
    printf("quantile_host_check: %ld checks, %d failures\n", checks, failures);
    return failures ? 1 : 0;
}
