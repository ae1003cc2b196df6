// test_astype.cpp -- astype through the drop-in surface: a.astype<U>() / sm::astype<U>(a) on named arrays, on the unevaluated temporary
// of an operator chain, on transposed views and slices, for every pair of float, double, int and std::int64_t; and the result as an
// operand of the next chain, of take and of cumsum.  Expected values: the rules of smhip.h written out on the host (an in-range
// static_cast; the saturating cases spelt out).
#include <sm.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
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

static std::uint64_t g_state = 0x1234567ull;
static double unit() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<double>((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

template <typename T>
static sm::SMArray<T> host_array(std::vector<std::size_t> shape, std::vector<T> &mirror, double lo, double hi) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    T *buf = new T[n];
    mirror.resize(n);
    for (std::size_t i = 0; i < n; ++i) {
        if constexpr (std::is_integral_v<T>) buf[i] = static_cast<T>(static_cast<std::int64_t>(lo + unit() * (hi - lo)));
        else buf[i] = static_cast<T>(lo + unit() * (hi - lo));
        mirror[i] = buf[i];
    }
    return sm::SMArray<T>(buf, std::move(shape));
}

// the contract on the host: every value the tests feed is in range except where `saturating` says otherwise
template <typename U, typename T>
static U expected(T x) {
    if constexpr (std::is_floating_point_v<T> && std::is_integral_v<U>) {
        if (x != x) return 0;
        const double d = std::trunc(static_cast<double>(x)), top = std::ldexp(1.0, 8 * static_cast<int>(sizeof(U)) - 1);
        if (d >= top) return std::numeric_limits<U>::max();
        if (d <= -top) return std::numeric_limits<U>::min();
        return static_cast<U>(d);
    } else if constexpr (std::is_integral_v<T> && std::is_integral_v<U>) {
        std::uint64_t bits = static_cast<std::uint64_t>(static_cast<std::int64_t>(x));
        if constexpr (sizeof(U) == 4) {
            const std::uint32_t lo = static_cast<std::uint32_t>(bits);
            std::int32_t r;
            std::memcpy(&r, &lo, 4);
            return r;
        } else {
            return static_cast<U>(static_cast<std::int64_t>(x));
        }
    } else {
        return static_cast<U>(x);  // integer -> float and float -> float: the language's conversion rounds once to nearest even
    }
}

template <typename A, typename B>
static bool same(A got, B want) {
    static_assert(std::is_same_v<A, B>);
    if constexpr (std::is_floating_point_v<A>) {
        if (want != want) return got != got;
    }
    return std::memcmp(&got, &want, sizeof(A)) == 0;
}

template <typename T, typename U>
static void test_pair() {
    const std::size_t R = 37, Cn = 53;
    std::vector<T> h;
    const double span = std::is_same_v<T, std::int64_t> || std::is_same_v<T, double> ? 3.0e12 : 2.0e6;  // beyond int's range for the wide sources
    auto a = host_array<T>({R, Cn}, h, -span, span);
    // a named array, member and free form
    auto m = a.template astype<U>();
    auto f = sm::astype<U>(a);
    static_assert(std::is_same_v<decltype(m), sm::SMArray<U>>);
    CHECK(m.shape() == a.shape() && f.shape() == a.shape());
    int bad = 0;
    for (std::size_t i = 0; i < h.size(); ++i) bad += !same(m.cdata()[i], expected<U>(h[i])) || !same(f.cdata()[i], m.cdata()[i]);
    CHECK(bad == 0);
    CHECK(a.cdata()[5] == h[5]);  // the operand is untouched
    // a transposed view (staged) and a block (read in place)
    auto t = a.transpose().template astype<U>();
    CHECK(t.shape()[0] == Cn && t.shape()[1] == R);
    bad = 0;
    for (std::size_t j = 0; j < Cn; ++j)
        for (std::size_t i = 0; i < R; ++i) bad += !same(t.cdata()[j * R + i], expected<U>(h[i * Cn + j]));
    CHECK(bad == 0);
    auto block = a(SLICE(2, 9), SLICE(5, 47)).template astype<U>();
    CHECK(block.shape()[0] == 7 && block.shape()[1] == 42);
    bad = 0;
    for (std::size_t i = 0; i < 7; ++i)
        for (std::size_t j = 0; j < 42; ++j) bad += !same(block.cdata()[i * 42 + j], expected<U>(h[(i + 2) * Cn + j + 5]));
    CHECK(bad == 0);
    auto row = a(3, SLICE_ALL).template astype<U>();  // a slice that starts mid-array: dense, not 16-byte aligned for Cn = 53
    bad = 0;
    for (std::size_t j = 0; j < Cn; ++j) bad += !same(row.cdata()[j], expected<U>(h[3 * Cn + j]));
    CHECK(bad == 0);
    // the unevaluated temporary of a chain: evaluated first, then converted
    const T three = static_cast<T>(3);
    auto c = (a * three + a).template astype<U>();
    bad = 0;
    for (std::size_t i = 0; i < h.size(); ++i) {
        T v;
        if constexpr (std::is_integral_v<T>) {
            typedef std::make_unsigned_t<T> UT;
            v = static_cast<T>(static_cast<UT>(h[i]) * static_cast<UT>(3) + static_cast<UT>(h[i]));
        } else {
            const T p = h[i] * three;  // two rounded operations, as the chain rounds them
            v = p + h[i];
        }
        bad += !same(c.cdata()[i], expected<U>(v));
    }
    CHECK(bad == 0);
    // the result feeds the next chain
    const U two = static_cast<U>(2);
    auto next = m * two - m;
    bad = 0;
    for (std::size_t i = 0; i < h.size(); ++i) {
        const U e = expected<U>(h[i]);
        if constexpr (std::is_integral_v<U>) {
            typedef std::make_unsigned_t<U> UU;
            bad += next.cdata()[i] != static_cast<U>(static_cast<UU>(e) * static_cast<UU>(2) - static_cast<UU>(e));
        } else {
            const U p = e * two;
            bad += !same(next.cdata()[i], static_cast<U>(p - e));
        }
    }
    CHECK(bad == 0);
}

template <typename T>
static void test_same_type_is_a_copy() {
    std::vector<T> h;
    auto a = host_array<T>({41, 30}, h, -1000, 1000);
    auto c = a.template astype<T>();
    auto ct = a.transpose().template astype<T>();
    int bad = 0;
    for (std::size_t i = 0; i < h.size(); ++i) bad += c.cdata()[i] != h[i];
    for (std::size_t j = 0; j < 30; ++j)
        for (std::size_t i = 0; i < 41; ++i) bad += ct.cdata()[j * 41 + i] != h[i * 30 + j];
    CHECK(bad == 0);
    a.assign_where(a == a, static_cast<T>(7));  // the copy does not alias
    CHECK(c.cdata()[7] == h[7] && a.cdata()[7] == static_cast<T>(7));
}

static void test_saturation_and_rounding() {
    const float fin[] = {NAN, -0.0f, -0.9f, 0.9f, 1.5f, -1.5f, INFINITY, -INFINITY, 2147483648.0f, 2147483520.0f, -2147483904.0f, 9223372036854775808.0f, 3e38f, -3e38f};
    auto f = sm::zeros<float>(sizeof fin / sizeof fin[0]);
    for (std::size_t i = 0; i < f.totalSize; ++i) f.data[i] = fin[i];
    auto i32 = f.astype<int>();
    auto i64 = f.astype<std::int64_t>();
    const int want32[] = {0, 0, 0, 0, 1, -1, INT32_MAX, INT32_MIN, INT32_MAX, 2147483520, INT32_MIN, INT32_MAX, INT32_MAX, INT32_MIN};
    const std::int64_t want64[] = {0, 0, 0, 0, 1, -1, INT64_MAX, INT64_MIN, 2147483648LL, 2147483520LL, -2147483904LL, INT64_MAX, INT64_MAX, INT64_MIN};
    int bad = 0;
    for (std::size_t i = 0; i < f.totalSize; ++i) bad += i32(i) != want32[i] || i64(i) != want64[i];
    CHECK(bad == 0);
    // i64 -> f32 is rounded once
    auto big = sm::zeros<std::int64_t>(4);
    const std::int64_t v = (std::int64_t{1} << 60) + (std::int64_t{1} << 36) + 1;
    big.data[0] = v, big.data[1] = -v, big.data[2] = INT64_MAX, big.data[3] = INT64_MIN;
    auto bf = big.astype<float>();
    CHECK(bf(0) == 0x1.000002p+60f && bf(1) == -0x1.000002p+60f && bf(2) == 0x1p+63f && bf(3) == -0x1p+63f);
    auto low = big.astype<int>();
    CHECK(low(0) == 1 && low(1) == -1 && low(2) == -1 && low(3) == 0);  // the low 32 bits
    // f64 -> f32: overflow, subnormals
    auto d = sm::zeros<double>(4);
    d.data[0] = 1e39, d.data[1] = 1e-40, d.data[2] = 1e-46, d.data[3] = -0.0;
    auto df = d.astype<float>();
    CHECK(std::isinf(df(0)) && df(1) == static_cast<float>(1e-40) && df(1) != 0.0f && df(2) == 0.0f && std::signbit(df(3)));
}

static void test_results_as_operands() {
    // take by widened int keys
    std::vector<float> ht;
    std::vector<int> hk;
    auto table = host_array<float>({300}, ht, -5.0, 5.0);
    auto keys = host_array<int>({70001}, hk, 0, 300);
    auto picked = table.take(keys.astype<std::int64_t>(), 0);
    int bad = 0;
    for (std::size_t i = 0; i < hk.size(); ++i) bad += picked.cdata()[i] != ht[static_cast<std::size_t>(hk[i])];
    CHECK(bad == 0);
    // cumsum of float data carried in double: exact for these integers-as-floats
    std::vector<float> hx;
    auto x = host_array<float>({4097}, hx, -100.0, 100.0);
    for (std::size_t i = 0; i < hx.size(); ++i) x.data[i] = hx[i] = std::floor(hx[i]);
    auto run = x.astype<double>().cumsum(0);
    double acc = 0;
    bad = 0;
    for (std::size_t i = 0; i < hx.size(); ++i) {
        acc += static_cast<double>(hx[i]);
        bad += run.cdata()[i] != acc;
    }
    CHECK(bad == 0);
    // argmax against labels: a mask converted and averaged
    std::vector<float> hl;
    auto logits = host_array<float>({512, 10}, hl, -1.0, 1.0);
    auto labels = sm::zeros<std::int64_t>(512);
    std::size_t right = 0;
    for (std::size_t i = 0; i < 512; ++i) {
        std::size_t best = 0;
        for (std::size_t j = 1; j < 10; ++j)
            if (hl[i * 10 + j] > hl[i * 10 + best]) best = j;
        labels.data[i] = static_cast<std::int64_t>(i % 3 ? best : (best + 1) % 10);
        right += i % 3 != 0;
    }
    auto acc_dev = sm::mask(sm::argmax(logits, -1) == labels).astype<double>().mean(0);
    CHECK(acc_dev(0) == static_cast<double>(right) / 512.0);
    // tiny arrays: the conversion of a recorded operator's result, no synchronise in between
    std::vector<float> ha, hb;
    auto a = host_array<float>({5, 5}, ha, -20.0, 20.0);
    auto b = host_array<float>({5, 5}, hb, -20.0, 20.0);
    auto s = a + b;
    auto si = s.astype<int>();
    bad = 0;
    for (std::size_t i = 0; i < 25; ++i) bad += si.cdata()[i] != static_cast<int>(ha[i] + hb[i]);
    CHECK(bad == 0);
    // an empty array
    auto e = sm::zeros<float>(0).astype<std::int64_t>();
    CHECK(e.totalSize == 0);
}

template <typename T>
static void test_from() {
    if constexpr (!std::is_same_v<T, float>) test_pair<T, float>();
    if constexpr (!std::is_same_v<T, double>) test_pair<T, double>();
    if constexpr (!std::is_same_v<T, int>) test_pair<T, int>();
    if constexpr (!std::is_same_v<T, std::int64_t>) test_pair<T, std::int64_t>();
    test_same_type_is_a_copy<T>();
}

int main() {
    try {
        test_from<float>();
        test_from<double>();
        test_from<int>();
        test_from<std::int64_t>();
        test_saturation_and_rounding();
        test_results_as_operands();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_astype: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
