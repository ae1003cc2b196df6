// test_softmax.cpp -- softmax, log_softmax and logsumexp through the drop-in surface: the free and the member forms for float and
// double, negative and absent axis, keepdims, a transposed view, a sliced view and a pending operator chain as operands, the result
// feeding argmax, take_along_axis and an operator chain, the `softmaxes` counter, what throws std::runtime_error, a NaN line.
// Expected values: a long double evaluation on the host, with the bounds of smhip.h ("softmax") on every element.
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

static std::uint64_t g_state = 0x2468aceull;
static double unit() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (static_cast<double>((z ^ (z >> 31)) >> 11) + 0.5) / 9007199254740992.0;
}
static double normal() { return std::sqrt(-2.0 * std::log(unit())) * std::cos(6.283185307179586 * unit()); }

template <typename T>
static sm::SMArray<T> host_array(std::vector<std::size_t> shape, double scale) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    T *buf = new T[n];
    for (std::size_t i = 0; i < n; ++i) buf[i] = static_cast<T>(scale * normal());
    return sm::SMArray<T>(buf, std::move(shape));
}

template <typename T>
static bool same_bytes(const sm::SMArray<T> &x, const sm::SMArray<T> &y) {
    if (x.shape() != y.shape()) return false;
    const sm::SMArray<T> a = x.contiguous(), b = y.contiguous();
    return std::memcmp(a.cdata(), b.cdata(), a.totalSize * sizeof(T)) == 0;
}

enum Kind { kSoftmax, kLogSoftmax, kLogSumExp };
using Shape = std::vector<std::size_t>;

// `got` against the long double value of `kind` along `axis` (0 or 1) of the 2-D array x, every element inside its bound.
template <typename T>
static bool within_bounds(Kind kind, const sm::SMArray<T> &x_in, int axis, const sm::SMArray<T> &got_in) {
    typedef long double LD;
    const sm::SMArray<T> x = x_in.contiguous(), got = got_in.contiguous();
    const std::size_t rows = x.shape()[0], cols = x.shape()[1], R = axis == 0 ? rows : cols, lines = axis == 0 ? cols : rows;
    if (got.totalSize != (kind == kLogSumExp ? lines : rows * cols)) return false;
    const bool f32 = std::is_same<T, float>::value;
    const LD u = std::ldexp(1.0L, f32 ? -24 : -53), tiny = std::numeric_limits<T>::denorm_min();
    const LD extra = 2 * u * std::max<LD>(1, std::log(static_cast<LD>(R)));
    int bad = 0;
    for (std::size_t l = 0; l < lines; ++l) {
        auto at = [&](std::size_t r) { return axis == 0 ? r * cols + l : l * cols + r; };
        LD m = -INFINITY, S = 0, D = 0;
        for (std::size_t r = 0; r < R; ++r) m = std::max<LD>(m, x.cdata()[at(r)]);
        for (std::size_t r = 0; r < R; ++r) S += std::exp(x.cdata()[at(r)] - m), D = std::max<LD>(D, m - x.cdata()[at(r)]);
        const LD lnS = std::log(S);
        if (kind == kLogSumExp) {
            const LD e = m + lnS, b = f32 ? 2.5L * u + u * std::fabs(e) : u * (R + 1 + D + std::fabs(e)) + extra;
            bad += !(std::fabs(got.cdata()[l] - e) <= b);
            continue;
        }
        for (std::size_t r = 0; r < R; ++r) {
            const LD d = x.cdata()[at(r)] - m, g = got.cdata()[at(r)];
            if (kind == kSoftmax) {
                const LD e = std::exp(d) / S, b = f32 ? 6 * u * e + 2 * tiny : u * (R + 5 - d + D) * e + 2 * tiny;
                bad += !(std::fabs(g - e) <= b);
            } else {
                const LD e = d - lnS, b = f32 ? 2.5L * u + u * std::fabs(e) : u * (R + 1 + D - d + std::fabs(e)) + extra;
                bad += !(std::fabs(g - e) <= b);
            }
        }
    }
    return bad == 0;
}

template <typename T>
static void test_forms() {
    const std::size_t R = 37, Cn = 530;
    auto a = host_array<T>({R, Cn}, 10.0);
    for (int axis : {0, 1, -1, -2}) {
        const int ax = axis < 0 ? axis + 2 : axis;
        auto before = sm::fusion_stats();
        auto p = sm::softmax(a, axis);
        auto lp = sm::log_softmax(a, axis);
        auto l = sm::logsumexp(a, axis);
        auto after = sm::fusion_stats();
        CHECK(after.softmaxes - before.softmaxes == 3 && after.reductions == before.reductions && after.chains == before.chains);
        CHECK(p.shape() == a.shape() && lp.shape() == a.shape() && (l.shape() == (ax == 0 ? Shape{Cn} : Shape{R})));
        CHECK(within_bounds(kSoftmax, a, ax, p) && within_bounds(kLogSoftmax, a, ax, lp) && within_bounds(kLogSumExp, a, ax, l));
        auto lk = sm::logsumexp(a, axis, true);
        CHECK((lk.shape() == (ax == 0 ? Shape{1, Cn} : Shape{R, 1})) && std::memcmp(lk.cdata(), l.cdata(), l.totalSize * sizeof(T)) == 0);
        // the member forms do the same calls
        CHECK(same_bytes(a.softmax(axis), p) && same_bytes(a.log_softmax(axis), lp) && same_bytes(a.logsumexp(axis), l) && same_bytes(a.logsumexp(axis, true), lk));
    }
    // no axis argument: the last one; logsumexp without an axis: the row-major flattening, shape {1}
    CHECK(same_bytes(sm::softmax(a), sm::softmax(a, 1)) && same_bytes(a.log_softmax(), a.log_softmax(-1)));
    auto all = sm::logsumexp(a);
    CHECK(all.shape() == Shape{1} && same_bytes(a.logsumexp(), all));
    {
        sm::SMArray<T> flat(new T[R * Cn], Shape{1, R * Cn});
        std::memcpy(flat.data, a.cdata(), R * Cn * sizeof(T));
        CHECK(within_bounds(kLogSumExp, flat, 1, all));
    }
    // a transposed view, read in place, and a sliced one
    const auto t = a.transpose();
    for (int axis : {0, 1}) {
        CHECK(within_bounds(kSoftmax, t, axis, sm::softmax(t, axis)) && within_bounds(kLogSoftmax, t, axis, t.log_softmax(axis)) &&
              within_bounds(kLogSumExp, t, axis, sm::logsumexp(t, axis)));
        CHECK(sm::softmax(t, axis).shape() == t.shape());
    }
    const auto part = a(SLICE(3, 30), SLICE(5, 405));
    CHECK((sm::softmax(part).shape() == Shape{27, 400}));
    CHECK(within_bounds(kSoftmax, part, 1, sm::softmax(part)) && within_bounds(kLogSoftmax, part, 0, sm::log_softmax(part, 0)) &&
          within_bounds(kLogSumExp, part, 1, part.logsumexp(-1)));
    // a long line: streamed in chunks
    auto longs = host_array<T>({2, 20497}, 3.0);
    CHECK(within_bounds(kSoftmax, longs, 1, sm::softmax(longs)) && within_bounds(kLogSoftmax, longs, 1, sm::log_softmax(longs)) &&
          within_bounds(kLogSumExp, longs, 1, sm::logsumexp(longs, -1)));
    // an axis out of range throws std::runtime_error, before anything runs
    int threw = 0;
    const auto before = sm::fusion_stats();
    for (int axis : {2, -3}) {
        try { (void)sm::softmax(a, axis); } catch (const std::runtime_error &) { ++threw; }
        try { (void)a.log_softmax(axis); } catch (const std::runtime_error &) { ++threw; }
        try { (void)sm::logsumexp(a, axis); } catch (const std::runtime_error &) { ++threw; }
        try { (void)a.logsumexp(axis, true); } catch (const std::runtime_error &) { ++threw; }
    }
    CHECK(threw == 8 && sm::fusion_stats().softmaxes == before.softmaxes);
}

static void test_operands_and_consumers() {
    const std::size_t R = 200, Cn = 300;
    auto a = host_array<float>({R, Cn}, 2.0);
    auto b = host_array<float>({R, Cn}, 2.0);
    const auto before = sm::fusion_stats();
    auto p = sm::softmax(a * 2.0f + b);  // the operand is a pending chain: evaluated first (one chain), then one softmax
    const auto after = sm::fusion_stats();
    CHECK(after.chains - before.chains == 1 && after.softmaxes - before.softmaxes == 1 && after.reductions == before.reductions);
    sm::SMArray<float> c = a * 2.0f + b;
    CHECK(same_bytes(p, sm::softmax(c)) && within_bounds(kSoftmax, c, 1, p));
    CHECK(same_bytes((a * 2.0f + b).log_softmax(0), c.log_softmax(0)) && same_bytes(sm::logsumexp(a * 2.0f + b, 1), c.logsumexp(1)));
    // the softmax keeps the order: its argmax is the logits'
    CHECK(same_bytes(sm::argmax(p, -1), sm::argmax(c, -1)));
    // a cross-entropy: the log-probabilities picked at the labels
    auto labels = sm::argmax(c, -1, true);  // {R, 1}
    auto logp = sm::log_softmax(c);
    auto picked = sm::take_along_axis(logp, labels, -1);
    auto lse = sm::logsumexp(c, -1, true), top = c.max(-1, true);
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i) {
        const std::size_t j = static_cast<std::size_t>(labels.cdata()[i]);
        bad += picked.cdata()[i] != logp.cdata()[i * Cn + j];
        bad += !(std::fabs(picked.cdata()[i] - (top.cdata()[i] - lse.cdata()[i])) <= 1e-6f * (1.0f + std::fabs(lse.cdata()[i])));
    }
    CHECK(bad == 0);
    // the result feeds the next operator chain, and a reduction: every row sums to 1
    auto doubled = p * 2.0f;
    auto sums = p.sum(-1);
    bad = 0;
    for (std::size_t i = 0; i < R * Cn; ++i) bad += doubled.cdata()[i] != 2.0f * p.cdata()[i];
    for (std::size_t i = 0; i < R; ++i) bad += !(std::fabs(sums.cdata()[i] - 1.0f) <= 1e-6f);
    CHECK(bad == 0);
    // log(softmax) loses what log_softmax keeps: far below the maximum the probability is 0, its logarithm is not
    float *buf = new float[4]{0.0f, -200.0f, 0.0f, -300.0f};
    sm::SMArray<float> far(buf, Shape{2, 2});
    CHECK(sm::softmax(far).cdata()[1] == 0.0f && sm::log_softmax(far).cdata()[1] == -200.0f && sm::log_softmax(far).cdata()[3] == -300.0f);
}

static void test_special_lines() {
    double *buf = new double[12]{1.0, NAN, 0.0, -5.0, /**/ 2.0, INFINITY, 9.0, -1.0, /**/ -INFINITY, -INFINITY, -INFINITY, -INFINITY};
    sm::SMArray<double> a(buf, Shape{3, 4});
    auto p = sm::softmax(a), lp = sm::log_softmax(a), l = sm::logsumexp(a, -1);
    int nans = 0;
    for (std::size_t i = 0; i < 12; ++i) nans += std::isnan(p.cdata()[i]) + std::isnan(lp.cdata()[i]);
    CHECK(nans == 24);
    CHECK(std::isnan(l.cdata()[0]) && l.cdata()[1] == INFINITY && l.cdata()[2] == -INFINITY);
    auto ones = sm::ones<float>(3, 7);
    auto q = sm::softmax(ones);  // a constant line: 1 / R in one rounding
    int bad = 0;
    for (std::size_t i = 0; i < 21; ++i) bad += q.cdata()[i] != static_cast<float>(1.0 / 7.0);
    CHECK(bad == 0);
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
    std::printf("test_softmax: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
