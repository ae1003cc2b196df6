// test_quantile.cpp -- quantile, percentile and median through the drop-in surface: sm::quantile(a, q, axis, method, keepdims) with one
// probability and with a list, sm::percentile, sm::median, the member forms and the forms without an axis for float and double,
// negative axes, a transposed and a sliced view and a pending operator chain as operands, the results feeding an operator chain (robust
// standardising), what throws std::invalid_argument, NaN, signed zeros and infinities, the `quantiles` counter.
// Expected values: the rules of include/smhip.h ("quantile") applied on the host to std::sort'ed lines, compared bit for bit.
#include <sm.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

static int g_failures = 0, g_checks = 0;
#define CHECK(cond)                                                                   \
    do {                                                                              \
        ++g_checks;                                                                   \
        if (!(cond)) {                                                                \
            ++g_failures;                                                             \
            if (g_failures <= 20) std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); \
        }                                                                             \
    } while (0)

static std::uint64_t g_state = 0x2468ace0ull;
static double unit() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<double>((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

template <typename T>
static sm::SMArray<T> host_array(std::vector<std::size_t> shape, bool ties) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    T *buf = new T[n];
    for (std::size_t i = 0; i < n; ++i) buf[i] = ties ? static_cast<T>(static_cast<int>(unit() * 9) - 4) : static_cast<T>((unit() - 0.5) * 20.0);
    return sm::SMArray<T>(buf, std::move(shape));
}

using Shape = std::vector<std::size_t>;
using M = sm::quantile_method;

// The contract on one line (copied, then ordered): smhip.h, "quantile".
template <typename T>
static T expected(std::vector<T> line, double q, M method) {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (T x : line)
        if (x != x) return static_cast<T>(nan);
    std::sort(line.begin(), line.end());
    const std::size_t R = line.size();
    const double h = static_cast<double>(R - 1) * q;
    double j = std::floor(h), g = h - j;
    if (method == M::lower) g = 0;
    if (method == M::higher) j = std::ceil(h), g = 0;
    if (method == M::nearest) j = std::nearbyint(h), g = 0;
    if (method == M::midpoint) g = g != 0 ? 0.5 : 0.0;
    const std::size_t at = static_cast<std::size_t>(j);
    const double lo = static_cast<double>(line[at]) + 0.0, hi = static_cast<double>(line[std::min(at + 1, R - 1)]) + 0.0;
    if (g == 0 || lo == hi) return static_cast<T>(lo);
    const double d = hi - lo;
    volatile double p = g < 0.5 ? d * g : d * (1.0 - g);  // the product is rounded before the sum
    return static_cast<T>(g < 0.5 ? lo + p : hi - p);
}

template <typename T>
static bool same_bits(T a, T b) {
    if (a != a && b != b) return true;  // (the device's NaN is the canonical one: checked where it matters)
    return std::memcmp(&a, &b, sizeof(T)) == 0;
}

// out[q][i] against the lines of the dense 2-D array `a` along `axis`.
template <typename T>
static int mismatches(const sm::SMArray<T> &a, const sm::SMArray<T> &out, const std::vector<double> &qs, int axis, M method) {
    const sm::SMArray<T> x = a.contiguous(), r = out.contiguous();
    const std::size_t rows = x.shape()[0], cols = x.shape()[1], lines = axis == 0 ? cols : rows, R = axis == 0 ? rows : cols;
    int bad = 0;
    for (std::size_t i = 0; i < lines; ++i) {
        std::vector<T> line(R);
        for (std::size_t k = 0; k < R; ++k) line[k] = axis == 0 ? x.cdata()[k * cols + i] : x.cdata()[i * cols + k];
        for (std::size_t n = 0; n < qs.size(); ++n) bad += !same_bits(r.cdata()[n * lines + i], expected(line, qs[n], method));
    }
    return bad;
}

template <typename T>
static void test_forms() {
    const std::size_t R = 37, Cn = 1030;
    auto a = host_array<T>({R, Cn}, false);
    auto ties = host_array<T>({R, Cn}, true);
    const std::vector<double> qs = {0.0, 0.25, 0.5, 1.0 / 3.0, 0.999, 1.0};
    for (const auto *x : {&a, &ties})
        for (int axis : {0, 1, -1, -2}) {
            const int ax = axis < 0 ? axis + 2 : axis;
            const std::size_t lines = ax == 0 ? Cn : R;
            for (M method : {M::linear, M::lower, M::higher, M::nearest, M::midpoint}) {
                const auto before = sm::fusion_stats();
                auto many = sm::quantile(*x, qs, axis, method);  // one call, one read of the operand
                CHECK(sm::fusion_stats().quantiles - before.quantiles == 1 && sm::fusion_stats().sorts == before.sorts);
                CHECK((many.shape() == Shape{qs.size(), lines}));
                CHECK(mismatches(*x, many, qs, ax, method) == 0);
                auto one = sm::quantile(*x, 0.25, axis, method);
                CHECK((one.shape() == Shape{lines}) && mismatches(*x, one, {0.25}, ax, method) == 0);
                auto kept = x->quantile(0.25, axis, method, true);  // member form, keepdims
                CHECK((kept.shape() == (ax == 0 ? Shape{1, Cn} : Shape{R, 1})) && std::memcmp(kept.cdata(), one.cdata(), lines * sizeof(T)) == 0);
                auto listed = x->quantile({0.25, 0.75}, axis, method, true);
                CHECK((listed.shape() == (ax == 0 ? Shape{2, 1, Cn} : Shape{2, R, 1})) && std::memcmp(listed.cdata(), one.cdata(), lines * sizeof(T)) == 0);
                auto pct = sm::percentile(*x, {25.0, 75.0}, axis, method);
                CHECK(std::memcmp(pct.cdata(), listed.cdata(), 2 * lines * sizeof(T)) == 0);
                CHECK(std::memcmp(x->percentile(25.0, axis, method).cdata(), one.cdata(), lines * sizeof(T)) == 0);
                const std::vector<double> built = {25.0, 75.0};  // a list built at run time
                CHECK(std::memcmp(sm::percentile(*x, built, axis, method).cdata(), pct.cdata(), 2 * lines * sizeof(T)) == 0);
                CHECK(std::memcmp(x->percentile(built, axis, method).cdata(), pct.cdata(), 2 * lines * sizeof(T)) == 0);
            }
            auto med = sm::median(*x, axis);
            CHECK(mismatches(*x, med, {0.5}, ax, M::linear) == 0);
            CHECK(std::memcmp(x->median(axis, true).cdata(), med.cdata(), lines * sizeof(T)) == 0);
            CHECK(std::memcmp(sm::quantile(*x, 0.5, axis).cdata(), med.cdata(), lines * sizeof(T)) == 0);
        }
    // without an axis: the row-major flattening, shape {1} or {Q}
    {
        T *copy = new T[R * Cn];
        std::memcpy(copy, a.cdata(), R * Cn * sizeof(T));
        const sm::SMArray<T> flat(copy, Shape{1, R * Cn});
        const auto before = sm::fusion_stats();
        auto m = sm::median(a);
        auto q3 = sm::quantile(a, {0.1, 0.5, 0.9}, M::midpoint);
        auto p = a.percentile(90.0);
        CHECK(sm::fusion_stats().quantiles - before.quantiles == 3);
        CHECK(m.shape() == Shape{1} && q3.shape() == Shape{3} && p.shape() == Shape{1});
        CHECK(mismatches(flat, m, {0.5}, 1, M::linear) == 0 && mismatches(flat, q3, {0.1, 0.5, 0.9}, 1, M::midpoint) == 0 && mismatches(flat, p, {0.9}, 1, M::linear) == 0);
        CHECK(same_bits(a.median().cdata()[0], m.cdata()[0]) && same_bits(sm::quantile(a, 0.5).cdata()[0], m.cdata()[0]));
        // a transposed view without an axis: its own row-major order holds the same elements
        CHECK(same_bits(sm::median(a.transpose()).cdata()[0], m.cdata()[0]));
    }
    // a transposed and a sliced view as operands
    const auto t = a.transpose();
    for (int axis : {0, 1}) CHECK(mismatches(t.contiguous(), sm::quantile(t, {0.5, 0.9}, axis), {0.5, 0.9}, axis, M::linear) == 0);
    const auto part = a(SLICE(3, 30), SLICE(5, 905));
    CHECK(mismatches(part.contiguous(), sm::median(part, -1), {0.5}, 1, M::linear) == 0);
    CHECK(mismatches(part.contiguous(), part.quantile({0.2, 0.8}, 0, M::higher), {0.2, 0.8}, 0, M::higher) == 0);
    // a long line: the streamed route
    auto wide = host_array<T>({3, 20497}, false);
    CHECK(mismatches(wide, sm::quantile(wide, {0.01, 0.5, 0.99}, -1), {0.01, 0.5, 0.99}, 1, M::linear) == 0);
    // seventeen probabilities: through the sort, the same values
    std::vector<double> many(17);
    for (std::size_t k = 0; k < many.size(); ++k) many[k] = static_cast<double>(k) / 16.0;
    CHECK(mismatches(a, sm::quantile(a, many, 0), many, 0, M::linear) == 0);
    // a result with a zero extent
    auto none = a(SLICE(0, 0), SLICE_ALL);
    CHECK((sm::median(none, 1).shape() == Shape{0}) && (sm::quantile(none, {0.5, 0.6}, 1).shape() == Shape{2, 0}));
}

template <typename F>
static int throws_invalid(F &&f, const char *what) {
    try {
        f();
    } catch (const std::invalid_argument &e) {
        return std::string(e.what()).find(what) != std::string::npos;
    } catch (...) {
    }
    return 0;
}

static void test_refusals() {
    auto a = host_array<float>({5, 7}, false);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    int threw = 0;
    for (int axis : {2, -3}) {
        threw += throws_invalid([&] { (void)sm::quantile(a, 0.5, axis); }, "quantile: axis");
        threw += throws_invalid([&] { (void)a.median(axis); }, "out of range for rank 2");
        threw += throws_invalid([&] { (void)sm::percentile(a, {50.0}, axis); }, "percentile: axis");
    }
    CHECK(threw == 6);
    threw = 0;
    for (double q : {-0.001, 1.001, nan}) {
        threw += throws_invalid([&] { (void)sm::quantile(a, q, 1); }, "quantile: a probability outside [0, 1] or NaN");
        threw += throws_invalid([&] { (void)a.quantile({0.5, q}); }, "outside [0, 1]");
        threw += throws_invalid([&] { (void)sm::percentile(a, q * 100.0, 0); }, "percentile: a probability outside [0, 100] or NaN");
    }
    CHECK(threw == 9);
    threw = throws_invalid([&] { (void)sm::quantile(a, std::vector<double>{}, 1); }, "quantile: no probability given");
    threw += throws_invalid([&] { (void)a.quantile(std::vector<double>{}); }, "no probability given");
    auto none = a(SLICE_ALL, SLICE(0, 0));
    threw += throws_invalid([&] { (void)sm::median(none, 1); }, "median: an empty axis with a result that is not empty");
    threw += throws_invalid([&] { (void)sm::median(none); }, "an empty axis");
    CHECK(threw == 4);
    CHECK((sm::median(none, 0).shape() == Shape{0}));  // an empty result is no refusal
}

static void test_operands_and_consumers() {
    const std::size_t R = 200, Cn = 300;
    auto a = host_array<float>({R, Cn}, false);
    auto b = host_array<float>({R, Cn}, false);
    const auto before = sm::fusion_stats();
    auto m = sm::median(a * 2.0f + b, -1);  // the operand is a pending chain: evaluated first (one chain), then one call
    const auto after = sm::fusion_stats();
    CHECK(after.chains - before.chains == 1 && after.quantiles - before.quantiles == 1 && after.sorts == before.sorts);
    sm::SMArray<float> c = a * 2.0f + b;
    CHECK(mismatches(c, m, {0.5}, 1, M::linear) == 0);
    // robust standardising: the results feed the next chain, broadcast along the axis they were taken from
    const sm::SMArray<float> &x = c;
    auto q25 = sm::quantile(x, 0.25, -1, M::linear, true), q75 = sm::quantile(x, 0.75, -1, M::linear, true);
    const auto mark = sm::fusion_stats();
    sm::SMArray<float> z = (x - sm::median(x, -1, true)) / (q75 - q25);
    CHECK(sm::fusion_stats().quantiles - mark.quantiles == 1);
    CHECK((z.shape() == Shape{R, Cn}));
    const auto med = sm::median(x, -1);
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i)
        for (std::size_t j = 0; j < Cn; ++j) {
            const float want = (x.cdata()[i * Cn + j] - med.cdata()[i]) / (q75.cdata()[i] - q25.cdata()[i]);
            bad += !(std::fabs(z.cdata()[i * Cn + j] - want) <= 1e-6f * std::fabs(want));  // (the quotient's last place is the chain's affair)
        }
    CHECK(bad == 0);
    // clipping at percentiles: the list form's rows are slices like any array's
    auto ends = sm::percentile(x, {1.0, 99.0}, -1);
    CHECK((ends.shape() == Shape{2, R}));
    bad = 0;
    for (std::size_t i = 0; i < R; ++i) bad += !(ends.cdata()[i] <= med.cdata()[i] && med.cdata()[i] <= ends.cdata()[R + i]);
    CHECK(bad == 0);
}

static void test_nan_zeros_and_infinities() {
    const float inf = std::numeric_limits<float>::infinity();
    float *buf = new float[20]{1.0f, -0.0f,  0.0f, -5.0f, /**/ 2.0f, NAN,  9.0f, -NAN, /**/ 0.0f, -0.0f, -0.0f, 0.0f,
                               inf,  inf,    1.0f, 0.0f,  /**/ -inf, inf,  -inf, inf};
    sm::SMArray<float> a(buf, std::vector<std::size_t>{5, 4});
    const auto m = sm::median(a, 1);
    const float *p = m.cdata();
    std::uint32_t bits[5];
    std::memcpy(bits, p, sizeof bits);
    CHECK(p[0] == 0.0f && bits[0] == 0);          // -5, -0, +0, 1: between the two zeros, +0
    CHECK(bits[1] == 0x7fc00000u);                // a NaN in the line: the canonical NaN
    CHECK(bits[2] == 0);                          // zeros of both signs: +0
    CHECK(bits[3] == 0x7fc00000u);                // 0, 1, inf, inf: halfway from 1 to inf the formula gives inf - inf
    CHECK(bits[4] == 0x7fc00000u);                // -inf, -inf, inf, inf: opposite infinities
    const auto hi = sm::quantile(a, {0.75, 1.0, 0.0}, 1, M::lower);
    CHECK(hi.cdata()[3] == inf && hi.cdata()[5 + 3] == inf && hi.cdata()[10 + 3] == 0.0f && hi.cdata()[10 + 4] == -inf);
    const auto up = sm::quantile(a, 0.9, 1);      // between two equal infinities: that infinity
    CHECK(up.cdata()[3] == inf && up.cdata()[4] == inf);
    double *one = new double[1]{-0.0};
    const sm::SMArray<double> single(one, std::vector<std::size_t>{1, 1});
    const auto s = sm::quantile(single, {0.0, 0.3, 1.0}, 1, M::nearest);  // a line of one element: itself, a zero as +0
    CHECK((s.shape() == Shape{3, 1}) && !std::signbit(s.cdata()[0]) && !std::signbit(s.cdata()[1]) && s.cdata()[2] == 0.0);
}

int main() {
    try {
        test_forms<float>();
        test_forms<double>();
        test_refusals();
        test_operands_and_consumers();
        test_nan_zeros_and_infinities();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_quantile: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
