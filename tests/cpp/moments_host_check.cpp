// moments_host_check.cpp -- the per-line arithmetic of var / std / standardize (csrc/sm_moments.h) on the host against long double.
//
// Lines of many lengths, three scales, offsets up to 1e4 (f32) and 1e9 (f64) times the spread, ddof 0 and 1, each evaluated whole
// ("held") and cut into chunks whose (sum d, sum d^2) pairs are merged in chunk order.  Every VAR, STD and standardized element must
// lie inside the bounds of include/smhip.h; the worst error is printed as a fraction of its bound.  The exact cases: a constant line
// gives exactly +0 (f32 any value; f64 -3.25 and 2^100), a NaN or an infinity in the line gives NaN, f32 values near 1e30 give +inf.
// No GPU library involved.
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <limits>
#include <vector>

#include "sm_moments.h"

using namespace smmoments;

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            if (++failures <= 20) {            \
                printf("FAIL %s: ", #cond);    \
                printf(__VA_ARGS__);           \
                printf("\n");                  \
            }                                  \
        }                                      \
    } while (0)

static uint64_t rng_state = 0x9e3779b97f4a7c15ULL;
static double uniform() {  // (0, 1)
    rng_state = rng_state * 6364136223846793005ULL + 1442695040888963407ULL;
    return ((double)(rng_state >> 11) + 0.5) / 9007199254740992.0;
}
static double normal() { return sqrt(-2.0 * log(uniform())) * cos(6.283185307179586 * uniform()); }

// What the kernels compute for one line: S in index order, then the pairs of chunks of `chunk` elements (0: the line whole) merged
// in chunk order.
template <typename T> struct Got { double S, var; };
template <typename T> static Got<T> evaluate(const std::vector<T> &x, int64_t ddof, size_t chunk) {
    const size_t n = x.size();
    double S = 0.0;
    for (size_t k = 0; k < n; ++k) S = S + (double)x[k];
    const double N = (double)n, mean = mean_of(S, N);
    if (chunk == 0) chunk = n;
    Sums total = zero();
    for (size_t start = 0; start < n; start += chunk) {
        Sums s = zero();
        for (size_t k = start; k < n && k < start + chunk; ++k) add(s, centre(x[k], mean));
        total = merge(total, s);
    }
    return Got<T>{S, variance(total, N, N - (double)ddof)};
}

template <typename T> struct Worst { double var = 0, sd = 0, y = 0; long lines = 0; };

template <typename T> static void check_line(const std::vector<T> &x, int64_t ddof, size_t chunk, double eps, Worst<T> &w) {
    const double u = ldexp(1.0, -53), uT = sizeof(T) == 4 ? ldexp(1.0, -24) : u;
    const long double tiny = std::numeric_limits<T>::denorm_min();
    const size_t n = x.size();
    long double sum = 0, m2 = 0, xmax = 0;
    for (T v : x) sum += (long double)v;
    const long double mean = sum / n;
    for (T v : x) {
        m2 += ((long double)v - mean) * ((long double)v - mean);
        xmax = fmaxl(xmax, fabsl((long double)v));
    }
    const long double var = m2 / (long double)(n - ddof), sd = sqrtl(var), den = sqrtl(var + (long double)eps);
    const Got<T> g = evaluate<T>(x, ddof, chunk);
    const T gv = finish<T>(kVar, g.var), gs = finish<T>(kStd, g.var);
    const long double bv = (uT + (n + 8.0L) * u) * var + tiny, bs = (uT + (n / 2.0L + 8.0L) * u) * sd + tiny;
    const double fv = (double)(fabsl((long double)gv - var) / bv), fs = (double)(fabsl((long double)gs - sd) / bs);
    CHECK(fv <= 1.0, "var n=%zu ddof=%lld chunk=%zu got %.17g want %.17Lg (%.3f of the bound)", n, (long long)ddof, chunk, (double)gv, var, fv);
    CHECK(fs <= 1.0, "std n=%zu ddof=%lld chunk=%zu got %.17g want %.17Lg (%.3f of the bound)", n, (long long)ddof, chunk, (double)gs, sd, fs);
    w.var = fmax(w.var, fv), w.sd = fmax(w.sd, fs);
    if (den > 0) {
        const double gm = mean_of(g.S, (double)n), gd = denominator(g.var, eps);
        for (size_t k = 0; k < n; ++k) {
            const long double y = ((long double)x[k] - mean) / den;
            const T gy = standardized<T>(centre(x[k], gm), gd);
            const long double by = (uT + (n + 10.0L) * u) * fabsl(y) + (n + 2.0L) * u * xmax / den + tiny;
            const double fy = (double)(fabsl((long double)gy - y) / by);
            CHECK(fy <= 1.0, "standardize n=%zu k=%zu got %.17g want %.17Lg (%.3f of the bound)", n, k, (double)gy, y, fy);
            w.y = fmax(w.y, fy);
        }
    }
    ++w.lines;
}

template <typename T> static void exact_cases(const char *name) {
    const size_t lengths[] = {1, 2, 7, 64, 1000, 4099};
    std::vector<double> values;
    if (sizeof(T) == 4) values = {0.1, -3.25, 1e30, 1.17549435e-38, 16777217.0, -7.0e-5};
    else values = {-3.25, ldexp(1.0, 100)};
    for (size_t n : lengths)
        for (double c : values)
            for (size_t chunk : {(size_t)0, (size_t)5}) {
                std::vector<T> x(n, (T)c);
                const Got<T> g = evaluate<T>(x, 0, chunk);
                const T v = finish<T>(kVar, g.var), s = finish<T>(kStd, g.var);
                CHECK(v == 0 && !signbit(v) && s == 0 && !signbit(s), "%s constant %g n=%zu: var %g std %g", name, c, n, (double)v, (double)s);
                CHECK((T)mean_of(g.S, (double)n) == (T)c, "%s constant %g n=%zu: mean %g", name, c, n, mean_of(g.S, (double)n));
                const T y = standardized<T>(centre(x[0], mean_of(g.S, (double)n)), denominator(g.var, 0.0));
                CHECK(y != y, "%s constant line, eps = 0: 0 / 0 is NaN, got %g", name, (double)y);
                const T y5 = standardized<T>(centre(x[0], mean_of(g.S, (double)n)), denominator(g.var, 1e-5));
                CHECK(y5 == 0, "%s constant line, eps = 1e-5: got %g", name, (double)y5);
            }
    for (double bad : {(double)NAN, (double)INFINITY, -(double)INFINITY}) {
        std::vector<T> x(33, (T)1.5);
        x[17] = (T)bad;
        for (size_t chunk : {(size_t)0, (size_t)8}) {
            const Got<T> g = evaluate<T>(x, 1, chunk);
            const T v = finish<T>(kVar, g.var), s = finish<T>(kStd, g.var);
            CHECK(v != v && s != s, "%s line with %g: var %g std %g", name, bad, (double)v, (double)s);
        }
    }
    if (sizeof(T) == 4) {  // the exact variance is about 1e60: above the range
        std::vector<T> x(100);
        for (size_t k = 0; k < x.size(); ++k) x[k] = (T)((k & 1) ? 1e30 : -1e30);
        const Got<T> g = evaluate<T>(x, 0, 0);
        const T v = finish<T>(kVar, g.var), s = finish<T>(kStd, g.var);
        CHECK(isinf(v) && v > 0, "f32 near 1e30: var %g", (double)v);
        CHECK(fabs((double)s / 1e30 - 1.0) < 1e-6, "f32 near 1e30: std %g", (double)s);
    }
}

template <typename T> static void run(const char *name) {
    Worst<T> w;
    const size_t lengths[] = {2, 3, 4, 5, 9, 15, 16, 17, 63, 64, 65, 100, 255, 256, 257, 511, 1023, 1024, 1025, 4097, 20011};
    const double scales[] = {1e-3, 1.0, 1e3};
    const double offsets32[] = {0.0, 1e2, 1e4}, offsets64[] = {0.0, 1e5, 1e9};
    const size_t chunks[] = {0, 7, 64, 1000};
    for (size_t n : lengths)
        for (double scale : scales)
            for (int oi = 0; oi < 3; ++oi)
                for (int64_t ddof = 0; ddof < 2; ++ddof) {
                    const double offset = (sizeof(T) == 4 ? offsets32[oi] : offsets64[oi]) * scale;
                    std::vector<T> x(n);
                    for (size_t k = 0; k < n; ++k) x[k] = (T)(offset + scale * normal());
                    for (size_t chunk : chunks) {
                        if (chunk >= n) continue;
                        check_line<T>(x, ddof, chunk, (w.lines & 1) ? 1e-5 : 0.0, w);
                    }
                }
    exact_cases<T>(name);
    printf("%s var worst %.4f std worst %.4f standardize worst %.4f of the bound over %ld lines\n", name, w.var, w.sd, w.y, w.lines);
    CHECK(w.var > 0 && w.sd > 0 && w.y > 0, "%s: a worst error of 0 means nothing was compared", name);
}

int main() {
    run<float>("f32");
    run<double>("f64");
    printf("moments_host_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
