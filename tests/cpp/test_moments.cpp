// test_moments.cpp -- var, stddev, var_mean and standardize through the drop-in surface: the free and the member forms for float and
// double, negative axes, axis lists, keepdims, ddof, the forms without an axis, a transposed and a sliced view and a pending operator
// chain as operands, the result feeding an operator chain ((x - mean) / sd against standardize), the `moments` counter, what throws
// std::runtime_error, constant and NaN lines.
// Expected values: a long double evaluation on the host, with the bounds of smhip.h ("var / std / standardize") on every element.
#include <sm.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
#include <type_traits>
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

static std::uint64_t g_state = 0x13579bdull;
static double unit() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (static_cast<double>((z ^ (z >> 31)) >> 11) + 0.5) / 9007199254740992.0;
}
static double normal() { return std::sqrt(-2.0 * std::log(unit())) * std::cos(6.283185307179586 * unit()); }

using Shape = std::vector<std::size_t>;
typedef long double LD;

template <typename T>
static sm::SMArray<T> host_array(Shape shape, double offset, double scale) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    T *buf = new T[n];
    for (std::size_t i = 0; i < n; ++i) buf[i] = static_cast<T>(offset + scale * normal());
    return sm::SMArray<T>(buf, std::move(shape));
}

template <typename T>
static bool same_bytes(const sm::SMArray<T> &x, const sm::SMArray<T> &y) {
    if (x.shape() != y.shape()) return false;
    const sm::SMArray<T> a = x.contiguous(), b = y.contiguous();
    return std::memcmp(a.cdata(), b.cdata(), a.totalSize * sizeof(T)) == 0;
}

template <typename T> struct Units {
    static constexpr LD u = 1.0L / 9007199254740992.0L;
    static constexpr LD uT = sizeof(T) == 4 ? 1.0L / 16777216.0L : u;
    static LD tiny() { return std::numeric_limits<T>::denorm_min(); }
};

// The lines of the 2-D array x along `axis` (0 or 1): element k of line l.
template <typename T> struct Lines {
    sm::SMArray<T> x;
    std::size_t rows, cols, N, lines;
    int axis;
    Lines(const sm::SMArray<T> &in, int ax) : x(in.contiguous()), rows(x.shape()[0]), cols(x.shape()[1]), N(ax == 0 ? rows : cols), lines(ax == 0 ? cols : rows), axis(ax) {}
    std::size_t at(std::size_t l, std::size_t k) const { return axis == 0 ? k * cols + l : l * cols + k; }
    LD mean(std::size_t l) const {
        LD s = 0;
        for (std::size_t k = 0; k < N; ++k) s += x.cdata()[at(l, k)];
        return s / N;
    }
    LD var(std::size_t l, std::int64_t ddof) const {
        const LD m = mean(l);
        LD s = 0;
        for (std::size_t k = 0; k < N; ++k) s += (x.cdata()[at(l, k)] - m) * (x.cdata()[at(l, k)] - m);
        return s / (LD)(N - ddof);
    }
    LD xmax(std::size_t l) const {
        LD m = 0;
        for (std::size_t k = 0; k < N; ++k) m = std::fmax(m, std::fabs((LD)x.cdata()[at(l, k)]));
        return m;
    }
};

// kind 0: var, 1: stddev.
template <typename T>
static bool moment_within(int kind, const sm::SMArray<T> &x, int axis, std::int64_t ddof, const sm::SMArray<T> &got_in) {
    const Lines<T> ln(x, axis);
    const sm::SMArray<T> got = got_in.contiguous();
    if (got.totalSize != ln.lines) return false;
    for (std::size_t l = 0; l < ln.lines; ++l) {
        const LD var = ln.var(l, ddof), exact = kind ? std::sqrt(var) : var;
        const LD bound = (Units<T>::uT + ((kind ? ln.N / 2.0L : (LD)ln.N) + 8) * Units<T>::u) * exact + Units<T>::tiny();
        if (!(std::fabs((LD)got.cdata()[l] - exact) <= bound)) return false;
    }
    return true;
}

// `got` against the standardized x within `slack` times the header's bound.
template <typename T>
static bool standardized_within(const sm::SMArray<T> &x, int axis, double eps, std::int64_t ddof, const sm::SMArray<T> &got_in, LD extra_rel = 0) {
    const Lines<T> ln(x, axis);
    const sm::SMArray<T> got = got_in.contiguous();
    if (got.shape() != ln.x.shape()) return false;
    for (std::size_t l = 0; l < ln.lines; ++l) {
        const LD m = ln.mean(l), den = std::sqrt(ln.var(l, ddof) + (LD)eps), xm = ln.xmax(l);
        for (std::size_t k = 0; k < ln.N; ++k) {
            const LD y = (ln.x.cdata()[ln.at(l, k)] - m) / den;
            const LD bound = (Units<T>::uT + (ln.N + 10) * Units<T>::u + extra_rel) * std::fabs(y) + ((ln.N + 2) * Units<T>::u + extra_rel) * xm / den + Units<T>::tiny();
            if (!(std::fabs((LD)got.cdata()[ln.at(l, k)] - y) <= bound)) return false;
        }
    }
    return true;
}

template <typename T>
static void test_forms() {
    const std::size_t R = 37, Cn = 1300;  // rows past the held length, columns cut into chunks
    const double offset = sizeof(T) == 4 ? 1e4 : 1e9, scale = sizeof(T) == 4 ? 1e-2 : 1.0;
    auto a = host_array<T>({R, Cn}, offset, scale);
    for (int ax : {0, 1}) {
        for (int axis : {ax, ax - 2}) {  // counted from the front and from the end
            for (std::int64_t ddof : {0, 1}) {
                const auto before = sm::fusion_stats();
                auto v = sm::var(a, axis, ddof);
                auto s = sm::stddev(a, axis, ddof);
                auto vm = sm::var_mean(a, axis, ddof);
                auto y = sm::standardize(a, axis, 1e-5, ddof);
                const auto after = sm::fusion_stats();
                CHECK(after.moments - before.moments == 4 && after.reductions == before.reductions && after.chains == before.chains);
                CHECK((v.shape() == (ax == 0 ? Shape{Cn} : Shape{R})) && s.shape() == v.shape() && vm.second.shape() == v.shape() && y.shape() == a.shape());
                CHECK(moment_within(0, a, ax, ddof, v) && moment_within(1, a, ax, ddof, s) && standardized_within(a, ax, 1e-5, ddof, y));
                CHECK(same_bytes(vm.first, v) && same_bytes(vm.second, sm::mean(a, axis)));  // the mean: bit for bit the reduction's
                auto vk = sm::var(a, axis, ddof, true);
                CHECK((vk.shape() == (ax == 0 ? Shape{1, Cn} : Shape{R, 1})) && std::memcmp(vk.cdata(), v.cdata(), v.totalSize * sizeof(T)) == 0);
                // the member forms do the same calls
                CHECK(same_bytes(a.var(axis, ddof), v) && same_bytes(a.stddev(axis, ddof), s) && same_bytes(a.var_mean(axis, ddof).first, v) &&
                      same_bytes(a.var_mean(axis, ddof, true).second, sm::mean(a, axis, true)) && same_bytes(a.standardize(axis, 1e-5, ddof), y));
            }
        }
    }
    // standardize without arguments: the last axis, eps = 0, ddof = 0
    CHECK(same_bytes(sm::standardize(a), sm::standardize(a, 1, 0.0, 0)) && same_bytes(a.standardize(), a.standardize(-1)));
    CHECK(standardized_within(a, 1, 0.0, 0, sm::standardize(a)));
    // axis lists and the forms without an axis: one line, shape {1}
    auto all = sm::var(a), all2 = sm::var(a, {0, 1}), all3 = a.var({-1, 0}, 0, true);
    CHECK(all.shape() == Shape{1} && all2.shape() == Shape{1} && (all3.shape() == Shape{1, 1}));
    CHECK(all.cdata()[0] == all2.cdata()[0] && all.cdata()[0] == all3.cdata()[0] && same_bytes(a.var(), all));
    {
        sm::SMArray<T> flat(new T[R * Cn], Shape{1, R * Cn});
        std::memcpy(flat.data, a.cdata(), R * Cn * sizeof(T));
        CHECK(moment_within(0, flat, 1, 0, all) && moment_within(1, flat, 1, 0, sm::stddev(a)) && moment_within(1, flat, 1, 1, a.stddev({0, 1}, 1)));
        auto vm = sm::var_mean(a);
        CHECK(vm.first.cdata()[0] == all.cdata()[0] && vm.second.cdata()[0] == sm::mean(a, {0, 1}).cdata()[0] && same_bytes(a.var_mean().second, vm.second));
    }
    // axes of a rank-3 array that do not merge, against the same elements laid out as rows
    {
        auto c = host_array<T>({5, 6, 7}, offset, scale);
        sm::SMArray<T> rows(new T[210], Shape{6, 35});
        for (std::size_t i = 0; i < 5; ++i)
            for (std::size_t j = 0; j < 6; ++j)
                for (std::size_t k = 0; k < 7; ++k) rows.data[j * 35 + i * 7 + k] = c.cdata()[(i * 6 + j) * 7 + k];
        CHECK(moment_within(0, rows, 1, 1, sm::var(c, {0, 2}, 1)) && moment_within(1, rows, 1, 0, c.stddev({2, 0})));
        CHECK((sm::var(c, {0, -1}, 0, true).shape() == Shape{1, 6, 1}));
        auto vm = sm::var_mean(c, {0, 2});
        CHECK(same_bytes(vm.second, sm::mean(c, {0, 2})) && same_bytes(vm.first, sm::var(c, {0, 2})));
    }
    // a transposed view, read in place, and a sliced one
    const auto t = a.transpose();
    for (int axis : {0, 1})
        CHECK(moment_within(0, t, axis, 1, sm::var(t, axis, 1)) && moment_within(1, t, axis, 0, t.stddev(axis)) && standardized_within(t, axis, 0.0, 0, sm::standardize(t, axis)) &&
              same_bytes(t.var_mean(axis).second, t.mean(axis)));
    const auto part = a(SLICE(3, 30), SLICE(5, 405));
    CHECK((sm::standardize(part).shape() == Shape{27, 400}));
    CHECK(moment_within(0, part, 1, 0, sm::var(part, 1)) && moment_within(1, part, 0, 1, sm::stddev(part, 0, 1)) && standardized_within(part, 1, 0.0, 1, part.standardize(-1, 0.0, 1)) &&
          standardized_within(part, 0, 1e-5, 0, sm::standardize(part, 0, 1e-5)));
    // what throws std::runtime_error, before anything runs
    int threw = 0;
    const auto before = sm::fusion_stats();
    for (int axis : {2, -3}) {
        try { (void)sm::var(a, axis); } catch (const std::runtime_error &) { ++threw; }
        try { (void)a.stddev(axis); } catch (const std::runtime_error &) { ++threw; }
        try { (void)sm::var_mean(a, {0, axis}); } catch (const std::runtime_error &) { ++threw; }
        try { (void)a.standardize(axis); } catch (const std::runtime_error &) { ++threw; }
    }
    try { (void)sm::var(a, {1, -1}); } catch (const std::runtime_error &) { ++threw; }                       // repeated
    try { (void)sm::var(a, 1, -1); } catch (const std::runtime_error &) { ++threw; }                         // ddof < 0
    try { (void)sm::stddev(a, 0, (std::int64_t)R); } catch (const std::runtime_error &) { ++threw; }         // N - ddof = 0
    try { (void)a.var_mean({0, 1}, (std::int64_t)(R * Cn) + 1); } catch (const std::runtime_error &) { ++threw; }
    try { (void)sm::standardize(a, 1, -1e-9); } catch (const std::runtime_error &) { ++threw; }              // eps
    try { (void)sm::standardize(a, 1, std::nan("")); } catch (const std::runtime_error &) { ++threw; }
    try { (void)a.standardize(1, INFINITY); } catch (const std::runtime_error &) { ++threw; }
    try { (void)a.standardize(0, 0.0, (std::int64_t)R); } catch (const std::runtime_error &) { ++threw; }
    try { (void)a.standardize(0, 0.0, -2); } catch (const std::runtime_error &) { ++threw; }
    CHECK(threw == 17 && sm::fusion_stats().moments == before.moments);
}

static void test_operands_and_consumers() {
    const std::size_t R = 200, Cn = 300;
    auto a = host_array<float>({R, Cn}, 50.0, 2.0);
    auto b = host_array<float>({R, Cn}, -7.0, 1.0);
    const auto before = sm::fusion_stats();
    auto v = sm::var(a * 2.0f + b, 1);  // the operand is a pending chain: evaluated first (one chain), then one call
    const auto after = sm::fusion_stats();
    CHECK(after.chains - before.chains == 1 && after.moments - before.moments == 1 && after.reductions == before.reductions);
    sm::SMArray<float> c = a * 2.0f + b;
    CHECK(same_bytes(v, sm::var(c, 1)) && moment_within(0, c, 1, 0, v));
    CHECK(same_bytes((a * 2.0f + b).stddev(0, 1), c.stddev(0, 1)) && same_bytes(sm::standardize(a * 2.0f + b, 0), c.standardize(0)));
    // the results feed the next chain: (x - mean) / sd with keepdims against standardize.  The chain rounds the mean, the
    // difference, sd and the quotient to float: three more roundings of 2^-24 on |y|, and 2^-24 |mean| / sd from the rounded mean.
    for (int axis : {0, 1}) {
        auto vm = sm::var_mean(c, axis, 0, true);
        auto sd = sm::stddev(c, axis, 0, true);
        sm::SMArray<float> z = (c - vm.second) / sd;
        CHECK(z.shape() == c.shape());
        CHECK(standardized_within(c, axis, 0.0, 0, sm::standardize(c, axis)));
        CHECK(standardized_within(c, axis, 0.0, 0, z, 4.0L / 16777216.0L));
    }
    // a normalised array has mean 0 and variance 1
    auto y = sm::standardize(c, 1);
    auto ym = y.mean(1), yv = y.var(1);
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i) bad += !(std::fabs(ym.cdata()[i]) <= 1e-6f) + !(std::fabs(yv.cdata()[i] - 1.0f) <= 1e-5f);
    CHECK(bad == 0);
}

static void test_special_lines() {
    double *buf = new double[12]{1.0, NAN, 0.0, -5.0, /**/ 2.0, INFINITY, 9.0, -1.0, /**/ 2.5, 2.5, 2.5, 2.5};
    sm::SMArray<double> a(buf, Shape{3, 4});
    auto v = sm::var(a, 1), s = sm::stddev(a, 1, 1);
    auto y = sm::standardize(a), ye = sm::standardize(a, -1, 1e-5);
    CHECK(std::isnan(v.cdata()[0]) && std::isnan(v.cdata()[1]) && std::isnan(s.cdata()[0]) && std::isnan(s.cdata()[1]));
    CHECK(v.cdata()[2] == 0.0 && !std::signbit(v.cdata()[2]) && s.cdata()[2] == 0.0 && !std::signbit(s.cdata()[2]));  // a constant line: exactly +0
    int nans = 0, zeros = 0;
    for (std::size_t i = 0; i < 12; ++i) nans += std::isnan(y.cdata()[i]);  // the constant line with eps = 0: 0 / 0
    for (std::size_t i = 8; i < 12; ++i) zeros += ye.cdata()[i] == 0.0;
    CHECK(nans == 12 && zeros == 4);
    auto ones = sm::ones<float>(3, 2000);
    auto q = sm::var_mean(ones, {0, 1});
    CHECK(q.first.cdata()[0] == 0.0f && q.second.cdata()[0] == 1.0f);
    float *big = new float[4]{1e30f, -1e30f, 1e30f, -1e30f};
    sm::SMArray<float> g(big, Shape{1, 4});
    CHECK(sm::var(g, 1).cdata()[0] == INFINITY && std::fabs(sm::stddev(g, 1).cdata()[0] / 1e30f - 1.0f) <= 1e-6f);  // above the range; its root is not
}

int main() {
    try {
        test_forms<float>();
        test_forms<double>();
        test_operands_and_consumers();
        test_special_lines();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_moments: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
