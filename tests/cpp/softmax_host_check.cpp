// softmax_host_check.cpp -- csrc/sm_softmax.h compiled for the host: the per-line arithmetic of softmax, log_softmax and logsumexp,
// f32 and f64, against long double.  No GPU library involved (g++ only, like unary_host_check.cpp).
//
// A line is evaluated the way the kernels do it: the maximum (line_max), e_r = exp(d_r) by exp_diff_n, S in fp64, the three finishing
// formulas; and a second time cut into chunks whose (m_c, S_c) pairs are combined in order (combine), as the SPLIT routes do.
// Asserted: the error bounds of include/smhip.h ("softmax") on every element of every line, and the exact cases -- a constant line,
// R == 1, every row of the special-value table, d < -104, differences that overflow f32 (3e38 and -3e38), subnormal inputs.
// Prints the worst error as a fraction of its bound per kind and type, and "<n> failures".
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <limits>
#include <type_traits>
#include <vector>

#include "sm_softmax.h"

using namespace smsoftmax;

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            if (++failures <= 20) {           \
                printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                printf(__VA_ARGS__);          \
                printf("\n");                 \
            }                                 \
        }                                     \
    } while (0)

template <typename T> struct Result {
    std::vector<T> soft, logsoft;
    T lse;
};

template <typename T> static void exp_one(double d, T *e) {
    const double dd[1] = {d};
    T ee[1];
    if constexpr (std::is_same<T, float>::value) exp_diff_n<1>(dd, ee);
    else exp_diff_n<1>(dd, ee, smpow64::TabAoS{smpow64::kLogTab, smpow64::kExpTab});
    *e = ee[0];
}

// (m, S) of x[0 .. n): S = 0 when m is not finite, as the kernels store a chunk's pair
template <typename T> static Pair fold(const T *x, size_t n) {
    T mx = -std::numeric_limits<T>::infinity();
    for (size_t r = 0; r < n; ++r) mx = line_max(mx, x[r]);
    Pair p{(double)mx, 0.0};
    if (special(p.m)) return p;
    for (size_t r = 0; r < n; ++r) {
        T e;
        exp_one<T>((double)x[r] - p.m, &e);
        p.S += (double)e;
    }
    return p;
}

// chunk == 0: the line held whole; else cut into chunks of `chunk`, the pairs combined in chunk order
template <typename T> static void evaluate(const std::vector<T> &x, size_t chunk, Result<T> *out) {
    const size_t R = x.size();
    Pair p;
    if (chunk == 0 || chunk >= R) p = fold(x.data(), R);
    else {
        p = fold(x.data(), chunk);
        for (size_t s = chunk; s < R; s += chunk) p = combine(p, fold(x.data() + s, R - s < chunk ? R - s : chunk));
    }
    out->soft.resize(R), out->logsoft.resize(R);
    if (special(p.m)) {
        for (size_t r = 0; r < R; ++r) out->soft[r] = special_value<T>(kSoftmax, (T)p.m), out->logsoft[r] = special_value<T>(kLogSoftmax, (T)p.m);
        out->lse = special_value<T>(kLogSumExp, (T)p.m);
        return;
    }
    const double lnS = log_sum(p.S);
    for (size_t r = 0; r < R; ++r) {
        const double d = (double)x[r] - p.m;
        T e;
        exp_one<T>(d, &e);
        out->soft[r] = finish_softmax<T>(e, p.S);
        out->logsoft[r] = finish_log_softmax<T>(d, lnS);
    }
    out->lse = finish_logsumexp<T>(p.m, lnS);
}

struct Worst { double soft = 0, logsoft = 0, lse = 0; long lines = 0, elements = 0; };

// The bounds of smhip.h on an ordinary line, every element compared.
template <typename T> static void check_bounds(const std::vector<T> &x, const Result<T> &got, Worst *w, const char *what) {
    typedef long double LD;
    const size_t R = x.size();
    const bool f32 = std::is_same<T, float>::value;
    const LD u = f32 ? ldexpl(1, -24) : ldexpl(1, -53), tiny = (LD)std::numeric_limits<T>::denorm_min();
    LD m = -INFINITY, S = 0, D = 0;
    for (size_t r = 0; r < R; ++r) m = (LD)x[r] > m ? (LD)x[r] : m;
    for (size_t r = 0; r < R; ++r) {
        const LD d = (LD)x[r] - m;
        S += expl(d);
        if (-d > D) D = -d;
    }
    if (D > 746) D = 746;
    const LD lnS = logl(S), lnR = logl((LD)R), extra = 2 * u * (lnR > 1 ? lnR : 1);
    for (size_t r = 0; r < R; ++r) {
        const LD d = (LD)x[r] - m, ad = isinf((double)d) ? 0 : -d;
        const LD es = expl(d) / S, el = d - lnS;
        const LD bs = f32 ? 6 * u * es + 2 * tiny : u * ((LD)R + 5 + ad + D) * es + 2 * tiny;
        const LD bl = f32 ? 2.5L * u + u * fabsl(el) : u * ((LD)R + 1 + D + ad + fabsl(el)) + extra;
        const LD errs = fabsl((LD)got.soft[r] - es);
        CHECK(errs <= bs, "%s softmax R=%zu r=%zu got %.17g exact %.17Lg err %.3Lg bound %.3Lg", what, R, r, (double)got.soft[r], es, errs, bs);
        if ((double)(errs / bs) > w->soft) w->soft = (double)(errs / bs);
        if (isinf((double)el)) {
            CHECK((double)got.logsoft[r] == (double)el, "%s log_softmax R=%zu r=%zu got %g for -inf", what, R, r, (double)got.logsoft[r]);
        } else {
            const LD errl = fabsl((LD)got.logsoft[r] - el);
            CHECK(errl <= bl, "%s log_softmax R=%zu r=%zu got %.17g exact %.17Lg err %.3Lg bound %.3Lg", what, R, r, (double)got.logsoft[r], el, errl, bl);
            if ((double)(errl / bl) > w->logsoft) w->logsoft = (double)(errl / bl);
        }
    }
    const LD ee = m + lnS, be = f32 ? 2.5L * u + u * fabsl(ee) : u * ((LD)R + 1 + D + fabsl(ee)) + extra, erre = fabsl((LD)got.lse - ee);
    CHECK(erre <= be, "%s logsumexp R=%zu got %.17g exact %.17Lg err %.3Lg bound %.3Lg", what, R, (double)got.lse, ee, erre, be);
    if ((double)(erre / be) > w->lse) w->lse = (double)(erre / be);
    w->lines += 1, w->elements += (long)R;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
static double uniform() {  // (0, 1)
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return ((double)(rng_state >> 11) + 0.5) * 0x1p-53;
}
static double normal() { return sqrt(-2.0 * log(uniform())) * cos(6.283185307179586 * uniform()); }

template <typename T> static bool same_bits(T a, T b) { return memcmp(&a, &b, sizeof(T)) == 0; }

template <typename T> static void check_equal(const Result<T> &a, const Result<T> &b, const char *what, size_t R) {
    bool same = same_bits(a.lse, b.lse) || (a.lse != a.lse && b.lse != b.lse);
    for (size_t r = 0; r < R && same; ++r)
        same = (same_bits(a.soft[r], b.soft[r]) || (a.soft[r] != a.soft[r] && b.soft[r] != b.soft[r])) &&
               (same_bits(a.logsoft[r], b.logsoft[r]) || (a.logsoft[r] != a.logsoft[r] && b.logsoft[r] != b.logsoft[r]));
    CHECK(same, "%s R=%zu: held and chunked differ", what, R);
}

template <typename T> static void run(const char *name) {
    const bool f32 = std::is_same<T, float>::value;
    const T inf = std::numeric_limits<T>::infinity(), nan = std::numeric_limits<T>::quiet_NaN();
    Worst w;
    Result<T> got, cut;
    // ---- random lines: the bounds, held and chunked
    const size_t lengths[] = {1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16385, 20497, 40977};
    const double scales[3] = {1, 10, f32 ? 40.0 : 300.0};
    for (size_t R : lengths)
        for (double scale : scales)
            for (int rep = 0; rep < 3; ++rep) {
                std::vector<T> x(R);
                const double shift = rep == 2 ? 1000.0 * normal() : 0.0;
                for (size_t r = 0; r < R; ++r) x[r] = (T)(scale * normal() + shift);
                evaluate(x, 0, &got);
                check_bounds(x, got, &w, name);
                for (size_t chunk : {(size_t)7, (size_t)256, (size_t)4096}) {
                    evaluate(x, chunk, &cut);
                    check_bounds(x, cut, &w, name);
                }
            }
    // ---- a constant line: 1 / R exactly, in one rounding; held and chunked agree bit for bit (every chunk factor is exp(0) = 1)
    for (size_t R : {(size_t)1, (size_t)3, (size_t)7, (size_t)1000, (size_t)20497})
        for (double v : {0.0, -3.25, 1e30, f32 ? 1e-45 : 5e-324}) {
            std::vector<T> x(R, (T)v);
            evaluate(x, 0, &got);
            evaluate(x, 256, &cut);
            check_equal(got, cut, name, R);
            const T want = f32 ? (T)(float)(1.0 / (double)R) : (T)(1.0 / (double)R);
            for (size_t r = 0; r < R; ++r) CHECK(same_bits(got.soft[r], want), "%s constant line R=%zu v=%g: %.17g", name, R, v, (double)got.soft[r]);
            check_bounds(x, got, &w, name);
        }
    // ---- R == 1: 1, +0 and x_0
    for (double v : {3.5, -2.0, 1e30, 0.0, f32 ? 1e-45 : 5e-324}) {
        std::vector<T> x(1, (T)v);
        evaluate(x, 0, &got);
        CHECK(same_bits(got.soft[0], (T)1) && same_bits(got.logsoft[0], (T)0) && same_bits(got.lse, x[0]), "%s R=1 v=%g: %g %g %g", name, v, (double)got.soft[0],
              (double)got.logsoft[0], (double)got.lse);
    }
    // ---- the special-value table: a NaN, m = +inf, all -inf; held and chunked (the special chunk first, in the middle, last)
    for (int row = 0; row < 3; ++row)
        for (size_t R : {(size_t)1, (size_t)5, (size_t)300})
            for (size_t at : {(size_t)0, R / 2, R - 1})
                for (size_t chunk : {(size_t)0, (size_t)2, (size_t)64}) {
                    std::vector<T> x(R);
                    for (size_t r = 0; r < R; ++r) x[r] = row == 2 ? -inf : (T)normal();
                    if (row == 0) x[at] = nan;
                    if (row == 1) {
                        x[at] = inf;
                        if (R - 1 - at != at) x[R - 1 - at] = -inf;
                    }
                    evaluate(x, chunk, &got);
                    bool ok = row == 0 ? got.lse != got.lse : got.lse == (row == 1 ? inf : -inf);
                    for (size_t r = 0; r < R; ++r) ok = ok && got.soft[r] != got.soft[r] && got.logsoft[r] != got.logsoft[r];
                    CHECK(ok, "%s special row %d R=%zu at=%zu chunk=%zu", name, row, R, at, chunk);
                }
    // ---- -inf among finite elements is an ordinary line: e = +0, log_softmax = -inf
    {
        std::vector<T> x = {(T)1, -inf, (T)2, -inf, (T)0.5};
        for (size_t chunk : {(size_t)0, (size_t)2}) {
            evaluate(x, chunk, &got);
            check_bounds(x, got, &w, name);
            CHECK(same_bits(got.soft[1], (T)0) && got.logsoft[3] == -inf, "%s -inf element", name);
        }
    }
    // ---- beyond the exp's reach: d < -104 (f32) / d <= -746 (f64) gives e = +0 exactly
    {
        const double far = f32 ? 104.0 : 746.0;
        std::vector<T> x = {(T)0, (T)(-far - 0.5), (T)(-2 * far), (T)(-far + 1), (T)-1};
        evaluate(x, 0, &got);
        check_bounds(x, got, &w, name);
        CHECK(same_bits(got.soft[1], (T)0) && same_bits(got.soft[2], (T)0), "%s far element: %g %g", name, (double)got.soft[1], (double)got.soft[2]);
        CHECK((double)got.logsoft[1] < -far && (double)got.logsoft[1] > -far - 1.0, "%s far log_softmax %g", name, (double)got.logsoft[1]);
    }
    // ---- differences that overflow the type: {big, -big}, d = -2 big is formed in fp64 (f64: it is -inf there, like any far element)
    {
        const T big = f32 ? (T)3e38 : (T)1.5e308;
        std::vector<T> x = {big, -big};
        for (size_t chunk : {(size_t)0, (size_t)1}) {
            evaluate(x, chunk, &got);
            CHECK(same_bits(got.soft[0], (T)1) && same_bits(got.soft[1], (T)0) && same_bits(got.logsoft[0], (T)0) && got.logsoft[1] == -inf && same_bits(got.lse, big),
                  "%s overflowing difference: %g %g %g %g %g", name, (double)got.soft[0], (double)got.soft[1], (double)got.logsoft[0], (double)got.logsoft[1], (double)got.lse);
        }
    }
    // ---- subnormal inputs
    {
        const T s = std::numeric_limits<T>::denorm_min();
        std::vector<T> x = {s, (T)(2 * s), (T)0, (T)-s, (T)(1000 * s), (T)-0.0};
        for (size_t chunk : {(size_t)0, (size_t)4}) {
            evaluate(x, chunk, &got);
            check_bounds(x, got, &w, name);
        }
    }
    printf("%s softmax worst %.3f log_softmax worst %.3f logsumexp worst %.3f of the bound over %ld lines %ld elements\n", name, w.soft, w.logsoft, w.lse, w.lines,
           w.elements);
}

int main() {
    static_assert(std::numeric_limits<long double>::digits >= 64, "the reference needs a long double wider than double");
    run<float>("f32");
    run<double>("f64");
    printf("softmax_host_check: %d failures\n", failures);
    return failures ? 1 : 0;
}
