// test_random.cpp -- sm::Generator through the drop-in surface: every method, the advance of offset() and seek() reproducing a draw, the
// draws as operands of the next chain (the dropout line is ONE chain launch after the mask), the in-place forms on arrays and dense
// views, a target that is not dense throwing.  Expected values: Philox4x32-10 and the maps of smhip.h written out on the host.
#include <sm.h>

#include <algorithm>
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

// ------------------------------------------------------------------------------------------------ the definition, on the host
struct Block { std::uint32_t w[4]; };
static Block philox(std::uint64_t seed, std::uint64_t stream, std::uint64_t b) {
    std::uint32_t c0 = static_cast<std::uint32_t>(b), c1 = static_cast<std::uint32_t>(b >> 32), c2 = static_cast<std::uint32_t>(stream),
                  c3 = static_cast<std::uint32_t>(stream >> 32), k0 = static_cast<std::uint32_t>(seed), k1 = static_cast<std::uint32_t>(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const std::uint64_t p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const std::uint32_t n0 = static_cast<std::uint32_t>(p1 >> 32) ^ c1 ^ k0, n2 = static_cast<std::uint32_t>(p0 >> 32) ^ c3 ^ k1;
        c1 = static_cast<std::uint32_t>(p1), c3 = static_cast<std::uint32_t>(p0), c0 = n0, c2 = n2;
        k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
    }
    return {{c0, c1, c2, c3}};
}
static std::uint32_t word32(std::uint64_t seed, std::uint64_t stream, std::uint64_t offset, std::size_t i) { return philox(seed, stream, offset + i / 4).w[i % 4]; }
static std::uint64_t word64(std::uint64_t seed, std::uint64_t stream, std::uint64_t offset, std::size_t i) {
    const Block b = philox(seed, stream, offset + i / 2);
    return b.w[2 * (i % 2)] | (static_cast<std::uint64_t>(b.w[2 * (i % 2) + 1]) << 32);
}
static float uniform01(std::uint32_t w) { return static_cast<float>(w >> 8) * 0x1p-24f; }
// the standard normal of element i of an f32 call, in double
static double normal_f32_ref(std::uint64_t seed, std::uint64_t stream, std::uint64_t offset, std::size_t i) {
    const Block b = philox(seed, stream, offset + i / 4);
    const int pair = static_cast<int>(i % 4) / 2;
    const double u1 = (static_cast<double>(b.w[2 * pair] >> 8) + 1.0) * 0x1p-24, t = static_cast<double>(b.w[2 * pair + 1] >> 8) * 0x1p-24;
    const double r = std::sqrt(-2.0 * std::log(u1)), a = 2.0 * 3.14159265358979323846 * t;
    return r * (i % 2 ? std::sin(a) : std::cos(a));
}
static bool within_ulps(float got, double want, double ulps) {
    // near a zero of the cosine / sine the angle 2 pi t itself is rounded in this reference: allow its absolute error as well
    int e;
    std::frexp(want, &e);
    const double ulp = std::ldexp(1.0, std::max(e, -125) - 24);
    return std::fabs(static_cast<double>(got) - want) <= ulps * ulp + 1e-14;
}

// ---------------------------------------------------------------------------------------------------------------- the tests
static void test_every_method_against_the_definition() {
    const std::uint64_t seed = 0x0123456789abcdefull;
    sm::Generator g(seed);
    CHECK(g.seed() == seed && g.stream() == 0 && g.offset() == 0);
    // uniform<float>: 37 x 53 = 1961 elements, 491 blocks
    auto u = g.uniform<float>(37, 53);
    CHECK(u.shape() == (std::vector<std::size_t>{37, 53}) && g.offset() == 491);
    int bad = 0;
    for (std::size_t i = 0; i < u.totalSize; ++i) bad += u.cdata()[i] != uniform01(word32(seed, 0, 0, i));
    CHECK(bad == 0);
    // uniform<double> continues at block 491: 7 elements, 4 blocks
    auto ud = g.uniform<double>(7);
    CHECK(g.offset() == 495);
    bad = 0;
    for (std::size_t i = 0; i < 7; ++i) bad += ud.cdata()[i] != static_cast<double>(word64(seed, 0, 491, i) >> 11) * 0x1p-53;
    CHECK(bad == 0);
    // bits
    auto b64 = g.bits<std::int64_t>(5);
    auto b32 = g.bits<int>(5);
    CHECK(g.offset() == 495 + 3 + 2);
    bad = 0;
    for (std::size_t i = 0; i < 5; ++i) {
        bad += static_cast<std::uint64_t>(b64.cdata()[i]) != word64(seed, 0, 495, i);
        bad += static_cast<std::uint32_t>(b32.cdata()[i]) != word32(seed, 0, 498, i);
    }
    CHECK(bad == 0);
    // integers: 64-bit draws for both types
    auto k64 = g.integers<std::int64_t>(-5, 1000, 513);
    auto k32 = g.integers<int>(0, 10, 513);
    CHECK(g.offset() == 500 + 257 + 257);
    bad = 0;
    for (std::size_t i = 0; i < 513; ++i) {
        const auto hi = [](std::uint64_t x, std::uint64_t r) { return static_cast<std::uint64_t>((static_cast<unsigned __int128>(x) * r) >> 64); };
        bad += k64.cdata()[i] != -5 + static_cast<std::int64_t>(hi(word64(seed, 0, 500, i), 1005));
        bad += k32.cdata()[i] != static_cast<int>(hi(word64(seed, 0, 757, i), 10));
    }
    CHECK(bad == 0);
    // bernoulli in the four types: the same mask
    g.seek(2000);
    auto mf = g.bernoulli<float>(0.9, 64, 9);
    g.seek(2000);
    auto md = g.bernoulli<double>(0.9, 64, 9);
    g.seek(2000);
    auto mi = g.bernoulli<int>(0.9, 64, 9);
    g.seek(2000);
    auto ml = g.bernoulli<std::int64_t>(0.9, 64, 9);
    CHECK(g.offset() == 2000 + 144);
    const std::uint64_t thr = static_cast<std::uint64_t>(std::floor(0.9 * 0x1p32));
    bad = 0;
    std::size_t ones = 0;
    for (std::size_t i = 0; i < 576; ++i) {
        const int want = word32(seed, 0, 2000, i) < thr;
        ones += want;
        bad += mf.cdata()[i] != static_cast<float>(want) || md.cdata()[i] != static_cast<double>(want) || mi.cdata()[i] != want || ml.cdata()[i] != want;
    }
    CHECK(bad == 0 && ones > 480 && ones < 560);
    // normal<float>: within 5 ULP of the formula in double; mean and variance of 2^16 draws
    g.seek(5000);
    auto z = g.normal<float>(1 << 16);
    CHECK(g.offset() == 5000 + (1 << 14));
    bad = 0;
    double s1 = 0, s2 = 0;
    for (std::size_t i = 0; i < z.totalSize; ++i) {
        bad += !within_ulps(z.cdata()[i], normal_f32_ref(seed, 0, 5000, i), 5.0);
        s1 += z.cdata()[i], s2 += static_cast<double>(z.cdata()[i]) * z.cdata()[i];
    }
    CHECK(bad == 0);
    const double n = static_cast<double>(z.totalSize), mean = s1 / n, var = s2 / n - mean * mean;
    CHECK(std::fabs(mean) < 5.0 / 256.0 && std::fabs(var - 1.0) < 5.0 * std::sqrt(2.0 / n));
    auto zd = g.normal<double>(1001);
    CHECK(g.offset() == 5000 + (1 << 14) + 501);
    s1 = 0;
    for (std::size_t i = 0; i < 1001; ++i) s1 += zd.cdata()[i];
    CHECK(std::fabs(s1 / 1001.0) < 5.0 / std::sqrt(1001.0));
    // another stream: other values
    sm::Generator g1(seed, 1);
    auto u1 = g1.uniform<float>(8);
    bad = 0;
    int same = 0;
    for (std::size_t i = 0; i < 8; ++i) {
        bad += u1.cdata()[i] != uniform01(word32(seed, 1, 0, i));
        same += u1.cdata()[i] == u.cdata()[i];
    }
    CHECK(bad == 0 && same < 8);
}

static void test_sequence_and_seek() {
    sm::Generator a(7), b(7);
    auto x1 = a.uniform<float>(1024), x2 = a.uniform<float>(1024);
    auto y = b.uniform<float>(2048);
    CHECK(a.offset() == 512 && b.offset() == 512);
    int bad = 0;
    for (std::size_t i = 0; i < 1024; ++i) bad += x1.cdata()[i] != y.cdata()[i] || x2.cdata()[i] != y.cdata()[1024 + i];
    CHECK(bad == 0);
    // 5 elements use two blocks: the next call starts at block 2, whatever the 5 were
    sm::Generator c(7);
    auto five = c.uniform<float>(5);
    CHECK(c.offset() == 2);
    auto four = c.uniform<float>(4);
    bad = 0;
    for (std::size_t i = 0; i < 4; ++i) bad += four.cdata()[i] != y.cdata()[8 + i] || five.cdata()[i] != y.cdata()[i];
    CHECK(bad == 0 && five.cdata()[4] == y.cdata()[4]);
    // seek reproduces a draw
    const std::uint64_t at = a.offset();
    auto n1 = a.normal<float>(33, 3);
    a.seek(at);
    auto n2 = a.normal<float>(33, 3);
    CHECK(std::memcmp(n1.cdata(), n2.cdata(), 99 * sizeof(float)) == 0);
    // an empty draw consumes nothing
    auto e = a.uniform<float>(0);
    CHECK(e.totalSize == 0 && a.offset() == at + 25);
}

static void test_draws_feed_chains() {
    sm::Generator g(42);
    auto x = g.uniform<float>(512, 1000);
    auto keep = g.bernoulli<float>(0.9, 512, 1000);
    const auto before = sm::fusion_stats();
    auto y = x * keep / 0.9f;  // dropout: the mask feeds one chain launch
    const float y0 = y.cdata()[0];
    const auto after = sm::fusion_stats();
    CHECK(after.chains == before.chains + 1 && after.single_ops == before.single_ops);
    int bad = 0;
    for (std::size_t i = 0; i < y.totalSize; ++i) {
        const float p = x.cdata()[i] * keep.cdata()[i];
        bad += y.cdata()[i] != p / 0.9f;
    }
    CHECK(bad == 0 && y0 == y.cdata()[0]);
    auto w = g.normal<float>(64, 64) * 0.02f;  // the scale is one launch
    double s2 = 0;
    for (std::size_t i = 0; i < w.totalSize; ++i) s2 += static_cast<double>(w.cdata()[i]) * w.cdata()[i];
    CHECK(std::fabs(std::sqrt(s2 / 4096.0) - 0.02) < 0.002);
    auto labels = g.integers<std::int64_t>(0, 1000, 512);
    std::int64_t lo = 1000, hi = -1;
    for (std::size_t i = 0; i < 512; ++i) lo = std::min(lo, labels.cdata()[i]), hi = std::max(hi, labels.cdata()[i]);
    CHECK(lo >= 0 && hi < 1000 && hi > lo);
}

static void test_in_place_forms() {
    sm::Generator g(9), h(9);
    auto a = sm::zeros<float>(100, 33);
    g.fill_uniform(a, -1.0f, 1.0f);
    auto u = h.uniform<float>(100, 33);
    CHECK(g.offset() == h.offset());
    int bad = 0;
    for (std::size_t i = 0; i < a.totalSize; ++i) {
        const float t = u.cdata()[i] * 2.0f;  // lo + u * span, two roundings
        bad += a.cdata()[i] != -1.0f + t;
    }
    CHECK(bad == 0);
    g.fill_normal(a, 0.5f, 0.02f);
    auto z = h.normal<float>(100, 33);
    bad = 0;
    for (std::size_t i = 0; i < a.totalSize; ++i) {
        const float t = 0.02f * z.cdata()[i];
        bad += a.cdata()[i] != 0.5f + t;
    }
    CHECK(bad == 0);
    auto k = sm::zeros<int>(777);
    g.fill_integers(k, 0, 10);
    auto k2 = h.integers<int>(0, 10, 777);
    CHECK(std::memcmp(k.cdata(), k2.cdata(), 777 * sizeof(int)) == 0);
    auto m = sm::zeros<double>(50, 5);
    g.fill_bernoulli(m, 0.5);
    auto m2 = h.bernoulli<double>(0.5, 50, 5);
    CHECK(std::memcmp(m.cdata(), m2.cdata(), 250 * sizeof(double)) == 0 && g.offset() == h.offset());
    // a dense view -- one row of a host-built matrix, starting mid-vector: the row is drawn, the rest stays
    float *buf = new float[7 * 33];
    for (int i = 0; i < 7 * 33; ++i) buf[i] = static_cast<float>(i);
    sm::SMArray<float> mat(buf, {7, 33});
    auto row = mat(3, SLICE_ALL);
    const std::uint64_t at = g.offset();
    g.fill_uniform(row, 0.0f, 1.0f);
    h.seek(at);
    auto r = h.uniform<float>(33);
    bad = 0;
    for (std::size_t i = 0; i < 7; ++i)
        for (std::size_t j = 0; j < 33; ++j) bad += mat.cdata()[i * 33 + j] != (i == 3 ? r.cdata()[j] : static_cast<float>(i * 33 + j));
    CHECK(bad == 0);
    // a pending chain on the target is evaluated first (and then overwritten)
    auto c = a + a;
    g.fill_uniform(c, 0.0f, 1.0f);
    CHECK(c.cdata()[0] >= 0.0f && c.cdata()[0] < 1.0f);
    // not dense: a column, a transposed view
    bool threw = false;
    try {
        auto col = mat(SLICE_ALL, 2);
        g.fill_uniform(col, 0.0f, 1.0f);
    } catch (const std::invalid_argument &) { threw = true; }
    CHECK(threw);
    threw = false;
    const std::uint64_t kept = g.offset();
    try {
        auto t = mat.transpose();
        g.fill_normal(t, 0.0f, 1.0f);
    } catch (const std::invalid_argument &) { threw = true; }
    CHECK(threw && g.offset() == kept);
    // what the library refuses throws and does not advance the generator
    threw = false;
    try { g.fill_normal(a, 0.0f, -1.0f); } catch (const std::runtime_error &) { threw = true; }
    CHECK(threw && g.offset() == kept);
    threw = false;
    try { (void)g.integers<int>(0, 0, 5); } catch (const std::runtime_error &) { threw = true; }
    CHECK(threw && g.offset() == kept);
}

static void test_permutation_and_shuffle() {
    sm::Generator g(3), h(3);
    auto order = g.permutation(512);
    CHECK(order.totalSize == 512 && g.offset() == 256);
    std::vector<std::int64_t> seen(order.cdata(), order.cdata() + 512);
    std::sort(seen.begin(), seen.end());
    int bad = 0;
    for (std::int64_t i = 0; i < 512; ++i) bad += seen[static_cast<std::size_t>(i)] != i;
    CHECK(bad == 0);
    // the stable argsort of the keys the definition gives
    std::vector<std::int64_t> keys(512), want(512);
    for (std::size_t i = 0; i < 512; ++i) keys[i] = static_cast<std::int64_t>(word64(3, 0, 0, i)), want[i] = static_cast<std::int64_t>(i);
    std::stable_sort(want.begin(), want.end(), [&](std::int64_t p, std::int64_t q) { return keys[static_cast<std::size_t>(p)] < keys[static_cast<std::size_t>(q)]; });
    CHECK(std::memcmp(want.data(), order.cdata(), 512 * sizeof(std::int64_t)) == 0);
    // shuffle along either axis
    auto x = h.uniform<float>(40, 6);  // 60 blocks
    auto p0 = sm::Generator(11).permutation(40), p1 = sm::Generator(11).permutation(6);
    auto s0 = sm::Generator(11).shuffle(x, 0), s1 = sm::Generator(11).shuffle(x, -1);
    bad = 0;
    for (std::size_t i = 0; i < 40; ++i)
        for (std::size_t j = 0; j < 6; ++j) {
            bad += s0.cdata()[i * 6 + j] != x.cdata()[static_cast<std::size_t>(p0.cdata()[i]) * 6 + j];
            bad += s1.cdata()[i * 6 + j] != x.cdata()[i * 6 + static_cast<std::size_t>(p1.cdata()[j])];
        }
    CHECK(bad == 0);
    bool threw = false;
    try { (void)g.shuffle(x, 2); } catch (const std::invalid_argument &) { threw = true; }
    CHECK(threw);
}

int main() {
    try {
        test_every_method_against_the_definition();
        test_sequence_and_seek();
        test_draws_feed_chains();
        test_in_place_forms();
        test_permutation_and_shuffle();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_random: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
