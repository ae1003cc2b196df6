// test_unary.cpp -- functions of one argument through the drop-in surface: sm::exp / log / sqrt / abs and unary minus on
// named arrays, temporaries and views; the README's softmax, log-sum-exp and standard deviation; and the fusion counters
// (sm::fusion_stats()): a function of an expression's temporary is one more stage of that expression's chain.
// Expected values: the same functions on the host in fp64 (exp / log within 1 ULP of that, sqrt / abs / negation exact).
#include <sm.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
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

static std::uint64_t g_state = 0x7654321ull;
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

// |got - want| <= one spacing of T at want
template <typename T>
static bool within_one_ulp(T got, double want) {
    if (std::isnan(want)) return std::isnan(got);
    if (std::isinf(want)) return static_cast<double>(got) == want;
    int e;
    std::frexp(want, &e);
    const int min_e = std::numeric_limits<T>::min_exponent;
    if (e < min_e || want == 0) e = min_e;
    const double ulp = std::ldexp(1.0, e - std::numeric_limits<T>::digits);
    return std::fabs(static_cast<double>(got) - want) <= ulp;
}

template <typename T>
static void test_named_arrays_and_views() {
    const std::size_t R = 96, Cn = 130;
    std::vector<T> h;
    auto a = host_array<T>({R, Cn}, h, 0.05, 20.0);
    const auto before = sm::fusion_stats();
    auto e = sm::exp(a), l = sm::log(a), s = sm::sqrt(a), m = -a, ab = sm::abs(m);
    const auto after = sm::fusion_stats();
    CHECK(after.chains == before.chains && after.single_ops == before.single_ops);  // named operands: one launch each, no chain
    int bad = 0;
    for (std::size_t i = 0; i < h.size(); ++i) {
        const double x = static_cast<double>(h[i]);
        bad += !within_one_ulp<T>(e.cdata()[i], std::exp(x));
        bad += !within_one_ulp<T>(l.cdata()[i], std::log(x));
        bad += s.cdata()[i] != std::sqrt(h[i]);
        bad += m.cdata()[i] != -h[i];
        bad += ab.cdata()[i] != h[i];
    }
    CHECK(bad == 0);
    CHECK(a.cdata()[5] == h[5]);  // the operand is untouched
    // views: a transposed matrix and a row are read in place
    auto st = sm::sqrt(a.transpose()), et = sm::exp(a.transpose()), nt = -a.transpose();
    CHECK(st.shape()[0] == Cn && st.shape()[1] == R);
    bad = 0;
    for (std::size_t j = 0; j < Cn; ++j)
        for (std::size_t i = 0; i < R; ++i) {
            bad += st.cdata()[j * R + i] != std::sqrt(h[i * Cn + j]);
            bad += et.cdata()[j * R + i] != e.cdata()[i * Cn + j];  // the same bits as the function of the dense array
            bad += nt.cdata()[j * R + i] != -h[i * Cn + j];
        }
    CHECK(bad == 0);
    auto row = sm::log(a(3, SLICE_ALL));
    bad = 0;
    for (std::size_t j = 0; j < Cn; ++j) bad += row.cdata()[j] != l.cdata()[3 * Cn + j];
    CHECK(bad == 0);
    auto block = sm::abs(m(SLICE(2, 9), SLICE(5, 77)));
    bad = 0;
    for (std::size_t i = 0; i < 7; ++i)
        for (std::size_t j = 0; j < 72; ++j) bad += block.cdata()[i * 72 + j] != h[(i + 2) * Cn + j + 5];
    CHECK(bad == 0);
}

static void test_integers() {
    std::vector<int> h;
    auto a = host_array<int>({300, 41}, h, -1000, 1000);
    a.data[0] = std::numeric_limits<int>::min();
    h[0] = std::numeric_limits<int>::min();
    auto n = -a, ab = sm::abs(a);
    int bad = 0;
    for (std::size_t i = 1; i < h.size(); ++i) {
        bad += n.cdata()[i] != -h[i];
        bad += ab.cdata()[i] != (h[i] < 0 ? -h[i] : h[i]);
    }
    CHECK(bad == 0);
    CHECK(n.cdata()[0] == std::numeric_limits<int>::min() && ab.cdata()[0] == std::numeric_limits<int>::min());  // wrapping, as numpy
    std::vector<std::int64_t> h64;
    auto b = host_array<std::int64_t>({70001}, h64, -5e12, 5e12);
    auto nb = -(b * static_cast<std::int64_t>(3));  // a temporary: one chain
    bad = 0;
    for (std::size_t i = 0; i < h64.size(); ++i) bad += nb.cdata()[i] != -(h64[i] * 3);
    CHECK(bad == 0);
}

// a function of the expression's temporary continues its chain: counters, not timing
static void test_fusion_counters() {
    const std::size_t R = 1024, Cn = 512;
    std::vector<float> hx, ha, hb;
    auto x = host_array<float>({R, Cn}, hx, -4.0, 4.0);
    auto a = host_array<float>({R, Cn}, ha, -3.0, 3.0);
    auto b = host_array<float>({R, Cn}, hb, -3.0, 3.0);
    auto m = sm::max(x, -1, true);
    {
        const auto s0 = sm::fusion_stats();
        auto e = sm::exp(x - m);  // ONE chain: subtract, exp
        const auto s1 = sm::fusion_stats();
        CHECK(s1.chains - s0.chains == 1);
        CHECK(s1.fused_stages - s0.fused_stages == 2);
        CHECK(s1.single_ops == s0.single_ops);
        int bad = 0;
        for (std::size_t i = 0; i < R; ++i)
            for (std::size_t j = 0; j < Cn; ++j)
                bad += !within_one_ulp<float>(e.cdata()[i * Cn + j], std::exp(static_cast<double>(hx[i * Cn + j] - m.cdata()[i])));
        CHECK(bad == 0);
    }
    {
        // a * a is launched when b * b starts a chain of its own (one chain is pending per thread); b * b, the sum and the root are
        // ONE chain of three stages
        const auto s0 = sm::fusion_stats();
        auto r = sm::sqrt(a * a + b * b);
        const auto s1 = sm::fusion_stats();
        CHECK(s1.chains - s0.chains == 1);
        CHECK(s1.fused_stages - s0.fused_stages == 3);
        CHECK(s1.single_ops - s0.single_ops == 1);
        int bad = 0;
        for (std::size_t i = 0; i < ha.size(); ++i) bad += r.cdata()[i] != std::sqrt(ha[i] * ha[i] + hb[i] * hb[i]);
        CHECK(bad == 0);
    }
    {
        const auto s0 = sm::fusion_stats();
        const double total = sm::exp(x - m).sum();  // the chain's sum in the chain's own pass: nothing is written
        const auto s1 = sm::fusion_stats();
        CHECK(s1.chains - s0.chains == 1);
        CHECK(s1.summed_chains - s0.summed_chains == 1);
        CHECK(s1.fused_stages - s0.fused_stages == 2);
        auto e = sm::exp(x - m);
        double want = 0, scale = 0;
        for (std::size_t i = 0; i < hx.size(); ++i) { want += static_cast<double>(e.cdata()[i]); scale += std::fabs(static_cast<double>(e.cdata()[i])); }
        CHECK(std::fabs(total - want) <= 1e-12 * scale);
    }
    {
        const auto s0 = sm::fusion_stats();
        auto l = sm::log(a * a + 1.0f) * 0.5f;  // log cuts the chain inside smhip_chain; for the front end it is still one chain
        auto g = -sm::abs(a - b);
        const auto s1 = sm::fusion_stats();
        CHECK(s1.chains - s0.chains == 2);
        CHECK(s1.fused_stages - s0.fused_stages == 4 + 3);
        int bad = 0;
        for (std::size_t i = 0; i < ha.size(); ++i) {
            bad += g.cdata()[i] != -std::fabs(ha[i] - hb[i]);
            const float arg = ha[i] * ha[i] + 1.0f;
            bad += std::fabs(static_cast<double>(l.cdata()[i]) - 0.5 * std::log(static_cast<double>(arg))) > 1.2e-7 * (1.0 + std::fabs(std::log(static_cast<double>(arg))));
        }
        CHECK(bad == 0);
    }
}

// the README's examples, against fp64 on the host
static void test_readme_examples() {
    const std::size_t R = 512, Cn = 384;
    std::vector<float> hx;
    auto x = host_array<float>({R, Cn}, hx, -6.0, 6.0);
    auto m = sm::max(x, -1, true);
    auto e = sm::exp(x - m);
    auto softmax = e / sm::sum(e, -1, true);
    auto lse = sm::log(sm::sum(e, -1, true)) + m;
    auto sd = sm::sqrt(sm::mean(sm::pow(x - sm::mean(x, 0, true), 2.0f), 0, true));
    CHECK(softmax.shape()[0] == R && softmax.shape()[1] == Cn && lse.shape()[0] == R && lse.shape()[1] == 1 && sd.shape()[0] == 1 && sd.shape()[1] == Cn);
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i) {
        float mxf = hx[i * Cn];
        double den = 0, rowsum = 0;
        for (std::size_t j = 0; j < Cn; ++j) mxf = std::fmax(mxf, hx[i * Cn + j]);
        const double mx = static_cast<double>(mxf);
        // x - m is an f32 subtraction on the device too: the exponent's argument is that rounded difference
        for (std::size_t j = 0; j < Cn; ++j) den += std::exp(static_cast<double>(hx[i * Cn + j] - mxf));
        for (std::size_t j = 0; j < Cn; ++j) {
            const double want = std::exp(static_cast<double>(hx[i * Cn + j] - mxf)) / den;
            const double got = static_cast<double>(softmax.cdata()[i * Cn + j]);
            bad += std::fabs(got - want) > 4e-7 * want + 1e-30;  // exp: 1 ULP, the f32 sum and the division: half an ULP each
            rowsum += got;
        }
        bad += std::fabs(rowsum - 1.0) > static_cast<double>(Cn) * std::ldexp(1.0, -24);  // rows sum to 1 within C * 2^-24
        const double want_lse = std::log(den) + mx;
        bad += std::fabs(static_cast<double>(lse.cdata()[i]) - want_lse) > 4e-7 * std::fabs(want_lse) + 4e-7;
    }
    CHECK(bad == 0);
    bad = 0;
    for (std::size_t j = 0; j < Cn; ++j) {
        double mean = 0;
        for (std::size_t i = 0; i < R; ++i) mean += static_cast<double>(hx[i * Cn + j]);
        const float meanf = static_cast<float>(mean / static_cast<double>(R));
        double var = 0;
        for (std::size_t i = 0; i < R; ++i) {
            const float d = hx[i * Cn + j] - meanf;
            var += static_cast<double>(d * d);
        }
        const float want = std::sqrt(static_cast<float>(var / static_cast<double>(R)));
        bad += !within_one_ulp<float>(sd.cdata()[j], static_cast<double>(want));  // correctly rounded steps; the fp64 sums may differ in their last bit
    }
    CHECK(bad == 0);
}

// tiny arrays: the function of a recorded operator's result, no synchronise in between
static void test_tiny() {
    std::vector<float> ha, hb;
    auto a = host_array<float>({5, 5}, ha, -2.0, 2.0);
    auto b = host_array<float>({5, 5}, hb, -2.0, 2.0);
    auto t = a + b;
    auto e = sm::exp(t);
    auto n = -(a * b);
    int bad = 0;
    for (std::size_t i = 0; i < 25; ++i) {
        bad += !within_one_ulp<float>(e.cdata()[i], std::exp(static_cast<double>(ha[i] + hb[i])));
        bad += n.cdata()[i] != -(ha[i] * hb[i]);
    }
    CHECK(bad == 0);
}

int main() {
    try {
        test_named_arrays_and_views<float>();
        test_named_arrays_and_views<double>();
        test_integers();
        test_fusion_counters();
        test_readme_examples();
        test_tiny();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_unary: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
