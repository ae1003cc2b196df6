// test_topk.cpp -- topk through the drop-in surface: sm::topk(a, k, axis, largest), the member form, the forms without an axis (the
// last one) and topk_flat for the four element types, negative axis, a transposed and a sliced view and a pending operator chain as
// operands, the results feeding take_along_axis, put_along_axis and an operator chain, what throws std::invalid_argument, NaN and
// signed zeros, the `topks` counter.
// Expected values: slices of sort_with_index on the same operand, compared byte for byte.
#include <sm.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static std::uint64_t g_state = 0x13579bdfull;
static double unit() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<double>((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

// Small integers: many ties along every axis, so the order of the positions has to be kept.
template <typename T>
static sm::SMArray<T> host_array(std::vector<std::size_t> shape, int lo = -9, int hi = 9) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    T *buf = new T[n];
    for (std::size_t i = 0; i < n; ++i) buf[i] = static_cast<T>(lo + static_cast<int>(unit() * (hi - lo + 1)));
    return sm::SMArray<T>(buf, std::move(shape));
}

template <typename T>
static bool same_bytes(const sm::SMArray<T> &x, const sm::SMArray<T> &y) {
    if (x.shape() != y.shape()) return false;
    const sm::SMArray<T> a = x.contiguous(), b = y.contiguous();
    return std::memcmp(a.cdata(), b.cdata(), a.totalSize * sizeof(T)) == 0;
}

using Pair = std::pair<std::size_t, std::size_t>;
// The first k along `axis` of a 2-D array.
template <typename T>
static sm::SMArray<T> first_k(const sm::SMArray<T> &x, std::size_t k, int axis) {
    return axis == 0 ? x(SLICE(0, k), SLICE_ALL) : x(SLICE_ALL, SLICE(0, k));
}

template <typename T>
static void test_forms() {
    const std::size_t R = 37, Cn = 1030;
    using Shape = std::vector<std::size_t>;
    auto a = host_array<T>({R, Cn});
    for (int axis : {0, 1, -1, -2}) {
        const int ax = axis < 0 ? axis + 2 : axis;
        for (bool largest : {false, true}) {
            auto [sv, sw] = sm::sort_with_index(a, axis, largest);
            for (std::size_t k : {std::size_t{1}, std::size_t{5}, ax == 0 ? R : std::size_t{300}}) {
                const auto before = sm::fusion_stats();
                auto [v, w] = sm::topk(a, k, axis, largest);  // one call for both
                CHECK(sm::fusion_stats().topks - before.topks == 1 && sm::fusion_stats().sorts == before.sorts);
                CHECK((v.shape() == (ax == 0 ? Shape{k, Cn} : Shape{R, k})) && w.shape() == v.shape());
                CHECK(same_bytes(v, first_k(sv, k, ax)) && same_bytes(w, first_k(sw, k, ax)));
                auto [v2, w2] = a.topk(k, axis, largest);
                CHECK(same_bytes(v2, v) && same_bytes(w2, w));
            }
        }
    }
    // no axis argument: the last axis, the largest
    auto [sv, sw] = sm::sort_with_index(a, -1, true);
    CHECK(same_bytes(sm::topk(a, 5).first, first_k(sv, 5, 1)) && same_bytes(a.topk(5).second, first_k(sw, 5, 1)));
    // topk_flat: the row-major flattening, shape {k}
    for (bool largest : {false, true}) {
        const auto fv = sm::sort_flat(a, largest);
        const auto fw = sm::argsort_flat(a, largest);
        auto [v, w] = sm::topk_flat(a, 9, largest);
        CHECK(v.shape() == Shape{9} && w.shape() == Shape{9});
        CHECK(same_bytes(v, fv(SLICE(0, 9))) && same_bytes(w, fw(SLICE(0, 9))));
        CHECK(same_bytes(a.topk_flat(9, largest).second, w));
    }
    // a transposed view: along its axis 0 it is the array along axis 1, laid out as the view; and a sliced one
    const auto t = a.transpose();
    for (int axis : {0, 1}) {
        auto [tv, tw] = sm::sort_with_index(t, axis, axis == 0);
        auto [v, w] = sm::topk(t, 7, axis, axis == 0);
        CHECK(same_bytes(v, first_k(tv, 7, axis)) && same_bytes(w, first_k(tw, 7, axis)));
    }
    const auto part = a(SLICE(3, 30), SLICE(5, 905));
    auto [pv, pw] = sm::sort_with_index(part, -1, true);
    auto [v, w] = sm::topk(part, 6);
    CHECK((v.shape() == Shape{27, 6}));
    CHECK(same_bytes(v, first_k(pv, 6, 1)) && same_bytes(w, first_k(pw, 6, 1)));
    // k = 0: arrays with a 0 extent
    auto [zv, zw] = sm::topk(a, 0);
    CHECK((zv.shape() == Shape{R, 0}) && zw.totalSize == 0);
    // a bad axis and a bad k throw std::invalid_argument
    int threw = 0;
    for (int axis : {2, -3}) {
        try {
            (void)sm::topk(a, 5, axis);
        } catch (const std::invalid_argument &e) {
            threw += std::string(e.what()).find("topk: axis") != std::string::npos;
        }
        try {
            (void)a.topk(5, axis, false);
        } catch (const std::invalid_argument &e) {
            threw += std::string(e.what()).find("out of range for rank 2") != std::string::npos;
        }
    }
    try {
        (void)sm::topk(a, Cn + 1);
    } catch (const std::invalid_argument &e) {
        threw += std::string(e.what()).find("topk: k 1031 above the axis' extent 1030") != std::string::npos;
    }
    try {
        (void)a.topk(R + 1, 0);
    } catch (const std::invalid_argument &e) {
        threw += std::string(e.what()).find("topk: k 38 above") != std::string::npos;
    }
    try {
        (void)sm::topk_flat(a, R * Cn + 1);
    } catch (const std::invalid_argument &e) {
        threw += 1;
    }
    CHECK(threw == 7);
}

static void test_operands_and_consumers() {
    const std::size_t R = 200, Cn = 300;
    auto a = host_array<float>({R, Cn}, -40, 40);
    auto b = host_array<float>({R, Cn}, -40, 40);
    const auto before = sm::fusion_stats();
    auto [v, w] = sm::topk(a * 2.0f + b, 5);  // the operand is a pending chain: evaluated first (one chain), then one topk
    const auto after = sm::fusion_stats();
    CHECK(after.chains - before.chains == 1 && after.topks - before.topks == 1 && after.sorts == before.sorts);
    sm::SMArray<float> c = a * 2.0f + b;
    auto [sv, sw] = sm::sort_with_index(c, -1, true);
    CHECK(same_bytes(v, first_k(sv, 5, 1)) && same_bytes(w, first_k(sw, 5, 1)));
    // the positions pick the values back
    CHECK(same_bytes(sm::take_along_axis(c, w, -1), v));
    CHECK(same_bytes(c.take_along_axis(w, 1, sm::index_mode::clip), v));
    // ... and mark them: a mask of the five best of each row (no two positions of a line are the same)
    auto mask = sm::zeros<float>(R, Cn);
    mask.put_along_axis(w, 1.0f, -1, sm::index_mode::checked, true);
    auto ranked = first_k(sw, 5, 1).contiguous();
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i) {
        float sum = 0.0f;
        for (std::size_t j = 0; j < Cn; ++j) sum += mask.cdata()[i * Cn + j];
        bad += sum != 5.0f;
        for (std::size_t j = 0; j < 5; ++j) bad += mask.cdata()[i * Cn + static_cast<std::size_t>(ranked.cdata()[i * 5 + j])] != 1.0f;
    }
    CHECK(bad == 0);
    // the values feed the next operator chain, the positions one of SMArray<std::int64_t>
    auto margin = v(SLICE_ALL, SLICE(0, 1)) - v(SLICE_ALL, SLICE(4, 5));
    auto shifted = w + std::int64_t{1};
    const auto best = first_k(sv, 5, 1).contiguous();
    bad = 0;
    for (std::size_t i = 0; i < R; ++i) {
        bad += margin.cdata()[i] != best.cdata()[i * 5] - best.cdata()[i * 5 + 4];
        for (std::size_t j = 0; j < 5; ++j) bad += shifted.cdata()[i * 5 + j] != ranked.cdata()[i * 5 + j] + 1;
    }
    CHECK(bad == 0);
    // entry 0 of the largest is where argmax points
    const auto first = w(SLICE_ALL, SLICE(0, 1)).contiguous();
    const auto am = sm::argmax(c, -1);
    CHECK(std::memcmp(first.cdata(), am.cdata(), R * sizeof(std::int64_t)) == 0);
}

static void test_nan_and_signed_zero() {
    float *buf = new float[12]{1.0f, -0.0f, 0.0f, -5.0f, /**/ 2.0f, NAN, 9.0f, -NAN, /**/ 0.0f, -0.0f, -1.0f, 0.0f};
    sm::SMArray<float> a(buf, std::vector<std::size_t>{3, 4});
    auto [v, w] = sm::topk(a, 3, 1, false);
    const std::int64_t *p = w.cdata();
    const float *q = v.cdata();
    CHECK(p[0] == 3 && p[1] == 1 && p[2] == 2);  // -5, -0, +0: the zeros in the order they stand
    CHECK(std::signbit(q[1]) && !std::signbit(q[2]));
    CHECK(p[3] == 0 && p[4] == 2 && p[5] == 1);  // 2, 9, NaN: the NaNs last
    CHECK(std::isnan(q[5]) && !std::signbit(q[5]));
    CHECK(p[6] == 2 && p[7] == 0 && p[8] == 1);  // -1, +0, -0
    CHECK(!std::signbit(q[7]) && std::signbit(q[8]));
    auto [dv, dw] = sm::topk(a, 2, 1);
    p = dw.cdata(), q = dv.cdata();
    CHECK(p[0] == 0 && p[1] == 1);  // 1, -0
    CHECK(p[2] == 1 && p[3] == 3);  // NaN, -NaN: the NaNs first, in the order they stand
    CHECK(std::isnan(q[2]) && !std::signbit(q[2]) && std::isnan(q[3]) && std::signbit(q[3]));
    CHECK(p[4] == 0 && p[5] == 1 && !std::signbit(q[4]) && std::signbit(q[5]));  // +0, -0
}

int main() {
    try {
        test_forms<float>();
        test_forms<double>();
        test_forms<int>();
        test_forms<std::int64_t>();
        test_operands_and_consumers();
        test_nan_and_signed_zero();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_topk: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
