// test_axis_reduce.cpp -- reductions along axes through the drop-in surface: sm::sum / mean / max / min(a, axis, keepdims)
// and the member forms, negative and listed axes, a pending operator chain and a just-recorded tiny operator as the operand,
// and the normalisation `(n - mean(n, 0, true)) / max(n, 0, true)` as one reduction per statistic plus ONE chain launch.
// Expected values: loops on the host over the same elements (fp64 sums rounded once, as the contract in smhip.h says).
#include <sm.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <stdexcept>
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
static sm::SMArray<T> host_array(std::vector<std::size_t> shape, std::vector<T> &mirror) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    T *buf = new T[n];
    mirror.resize(n);
    for (std::size_t i = 0; i < n; ++i) {
        if constexpr (std::is_integral_v<T>) buf[i] = static_cast<T>(static_cast<std::int64_t>(unit() * 2000.0) - 1000);
        else buf[i] = static_cast<T>(unit() * 8.0 - 4.0);
        mirror[i] = buf[i];
    }
    return sm::SMArray<T>(buf, std::move(shape));
}

// rows x cols, reduce axis 0 (per column) or 1 (per row) on the host
template <typename T>
static std::vector<double> host_sum(const std::vector<T> &x, std::size_t rows, std::size_t cols, int axis) {
    std::vector<double> r(axis == 0 ? cols : rows, 0.0);
    for (std::size_t i = 0; i < rows; ++i)
        for (std::size_t j = 0; j < cols; ++j) r[axis == 0 ? j : i] += static_cast<double>(x[i * cols + j]);
    return r;
}
template <typename T>
static std::vector<T> host_ext(const std::vector<T> &x, std::size_t rows, std::size_t cols, int axis, bool want_max) {
    std::vector<T> r(axis == 0 ? cols : rows, want_max ? std::numeric_limits<T>::lowest() : std::numeric_limits<T>::max());
    for (std::size_t i = 0; i < rows; ++i)
        for (std::size_t j = 0; j < cols; ++j) {
            T &v = r[axis == 0 ? j : i];
            const T e = x[i * cols + j];
            v = want_max ? (e > v ? e : v) : (e < v ? e : v);
        }
    return r;
}

static void test_forms_float() {
    const std::size_t R = 300, Cn = 517;
    std::vector<float> h;
    auto a = host_array<float>({R, Cn}, h);
    for (int axis : {0, 1, -1, -2}) {
        const int ax = axis < 0 ? axis + 2 : axis;
        const auto want = host_sum(h, R, Cn, ax);
        const std::size_t n = want.size();
        auto s1 = sm::sum(a, axis);
        auto s2 = a.sum(axis);
        auto m1 = sm::mean(a, axis, true);
        auto mx = sm::max(a, axis);
        auto mn = a.min(axis, true);
        const auto wmx = host_ext(h, R, Cn, ax, true), wmn = host_ext(h, R, Cn, ax, false);
        CHECK(s1.shape() == std::vector<std::size_t>{n});
        CHECK(m1.shape() == (ax == 0 ? std::vector<std::size_t>{1, Cn} : std::vector<std::size_t>{R, 1}));
        const float *p1 = s1.cdata(), *p2 = s2.cdata(), *pm = m1.cdata(), *px = mx.cdata(), *pn = mn.cdata();
        int bad = 0;
        for (std::size_t k = 0; k < n; ++k) {
            bad += p1[k] != static_cast<float>(want[k]) || p2[k] != p1[k];
            bad += pm[k] != static_cast<float>(want[k] / static_cast<double>(ax == 0 ? R : Cn));
            bad += px[k] != wmx[k] || pn[k] != wmn[k];
        }
        CHECK(bad == 0);
    }
    // a list of axes: everything -> shape {1}; with keepdims -> {1, 1}
    auto all = sm::sum(a, {0, 1});
    CHECK(all.shape() == std::vector<std::size_t>{1});
    double tot = 0;
    for (float v : h) tot += v;
    CHECK(all.cdata()[0] == static_cast<float>(tot));
    auto all_k = a.max({-1, 0}, true);
    CHECK((all_k.shape() == std::vector<std::size_t>{1, 1}));
    float m = h[0];
    for (float v : h) m = v > m ? v : m;
    CHECK(all_k.cdata()[0] == m);
    // a transposed view: no copy needed, the same values as the row reduction
    auto t = a.transpose();
    auto ts = sm::sum(t, 0), rs = sm::sum(a, 1);
    int bad = 0;
    for (std::size_t k = 0; k < R; ++k) bad += ts.cdata()[k] != rs.cdata()[k];
    CHECK(bad == 0);
    // bad axes throw
    bool threw = false;
    try { (void)sm::sum(a, 2); } catch (const std::runtime_error &) { threw = true; }
    CHECK(threw);
    threw = false;
    try { (void)a.max({1, -1}); } catch (const std::runtime_error &) { threw = true; }
    CHECK(threw);
}

static void test_integers() {
    const std::size_t R = 65, Cn = 4097;
    std::vector<std::int32_t> h;
    auto a = host_array<std::int32_t>({R, Cn}, h);
    auto s = sm::sum(a, 0);
    auto mx = sm::max(a, {1});
    int bad = 0;
    for (std::size_t j = 0; j < Cn; ++j) {
        std::uint32_t acc = 0;
        for (std::size_t i = 0; i < R; ++i) acc += static_cast<std::uint32_t>(h[i * Cn + j]);
        bad += s.cdata()[j] != static_cast<std::int32_t>(acc);
    }
    const auto wmx = host_ext(h, R, Cn, 1, true);
    for (std::size_t i = 0; i < R; ++i) bad += mx.cdata()[i] != wmx[i];
    CHECK(bad == 0);
}

static void test_pending_chain_and_tiny_operand() {
    const std::size_t R = 200, Cn = 300;
    std::vector<float> ha, hb, hr;
    auto a = host_array<float>({R, Cn}, ha);
    auto b = host_array<float>({R, Cn}, hb);
    auto row = host_array<float>({1, Cn}, hr);
    // the operand is a pending chain: evaluated first (one chain), then one reduction
    const auto before = sm::fusion_stats();
    auto s = sm::sum(a * row + b, 1);
    const auto after = sm::fusion_stats();
    CHECK(after.chains - before.chains == 1);
    CHECK(after.reductions - before.reductions == 1);
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i) {
        double acc = 0;
        for (std::size_t j = 0; j < Cn; ++j) acc += static_cast<double>(ha[i * Cn + j] * hr[j] + hb[i * Cn + j]);
        bad += s.cdata()[i] != static_cast<float>(acc);
    }
    CHECK(bad == 0);
    // a tiny operator (recorded, not yet launched) produces the operand just before the reduction
    std::vector<float> hs;
    auto small = host_array<float>({6, 5}, hs);
    auto small2 = small * 3.0f;
    auto cs = sm::sum(small2, 0);
    auto cm = sm::min(small2, -1, true);
    bad = 0;
    for (std::size_t j = 0; j < 5; ++j) {
        double acc = 0;
        for (std::size_t i = 0; i < 6; ++i) acc += static_cast<double>(hs[i * 5 + j] * 3.0f);
        bad += cs.cdata()[j] != static_cast<float>(acc);
    }
    for (std::size_t i = 0; i < 6; ++i) {
        float m = hs[i * 5] * 3.0f;
        for (std::size_t j = 1; j < 5; ++j) m = std::fmin(m, hs[i * 5 + j] * 3.0f);
        bad += cm.cdata()[i] != m;
    }
    CHECK(bad == 0);
}

static void test_normalisation() {
    const std::size_t R = 4096, Cn = 512;
    std::vector<float> h;
    auto n = host_array<float>({R, Cn}, h);
    for (auto &v : h) v = std::fabs(v) + 1.0f;  // positive maxima
    {
        float *w = n.data;  // host write: the device copy is refreshed before the next operator
        for (std::size_t i = 0; i < h.size(); ++i) w[i] = h[i];
    }
    auto mean = host_sum(h, R, Cn, 0);
    auto mx = host_ext(h, R, Cn, 0, true);
    for (auto &m : mean) m = static_cast<double>(static_cast<float>(m / static_cast<double>(R)));
    const auto before = sm::fusion_stats();
    n = (n - sm::mean(n, 0, true)) / sm::max(n, 0, true);
    const auto after = sm::fusion_stats();
    CHECK(after.reductions - before.reductions == 2);
    CHECK(after.chains - before.chains == 1);
    CHECK(after.single_ops == before.single_ops);
    const float *p = n.cdata();
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i)
        for (std::size_t j = 0; j < Cn; ++j) bad += p[i * Cn + j] != (h[i * Cn + j] - static_cast<float>(mean[j])) / mx[j];
    CHECK(bad == 0);
    // the README's form: one reduction plus one chain launch
    auto s = sm::ones<float>(1, Cn) * 4.0f;
    const auto b2 = sm::fusion_stats();
    n = (n - sm::mean(n, 0, true)) / s;
    const auto a2 = sm::fusion_stats();
    CHECK(a2.reductions - b2.reductions == 1);
    CHECK(a2.chains - b2.chains == 1);
}

int main() {
    try {
        test_forms_float();
        test_integers();
        test_pending_chain_and_tiny_operand();
        test_normalisation();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_axis_reduce: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
