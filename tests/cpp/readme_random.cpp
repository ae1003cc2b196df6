// The snippet of README.md, "Random numbers", compiled and run by tests/test_random_cpp.py so it cannot rot, with checks whose answers
// follow from the definition.
#include <sm.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

static int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) ++g_failures, std::printf("FAIL line %d  %s\n", __LINE__, #cond); \
    } while (0)

int main() {
    sm::Generator g(42);                                   // (seed, stream = 0); g.offset() / g.seek(blocks) expose the position
    auto x      = g.uniform<float>(512, 1000);             // [0, 1), dims as in sm::ones
    auto w      = g.normal<float>(64, 64) * 0.02f;         // standard normal; the scale is one chain launch
    auto labels = g.integers<std::int64_t>(0, 1000, 512);  // [lo, hi)
    auto keep   = g.bernoulli<float>(0.9, 512, 1000);
    auto y      = x * keep / 0.9f;                         // dropout: the mask feeds one chain launch
    auto a = sm::zeros<float>(256, 256);
    auto k = sm::zeros<int>(4096);
    auto m = sm::zeros<float>(256, 256);
    g.fill_uniform(a, -1.0f, 1.0f);  g.fill_normal(a, 0.0f, 0.02f);  g.fill_integers(k, 0, 10);  g.fill_bernoulli(m, 0.5);
    auto order  = g.permutation(512);                      // SMArray<std::int64_t>
    auto batch  = g.shuffle(x, 0);                         // take(x, permutation(x.shape[axis]), axis, clip)

    // 128000 + 1024 + 256 + 128000 blocks for the four draws, 16384 * 2 + 2048 + 16384 for the fills, 256 * 2 for the two orders
    CHECK(g.offset() == 128000u + 1024u + 256u + 128000u + 16384u * 3u + 2048u + 512u);
    double mean = 0, kept = 0, s2 = 0;
    int bad = 0;
    for (std::size_t i = 0; i < x.totalSize; ++i) {
        mean += x.cdata()[i], kept += keep.cdata()[i];
        bad += !(x.cdata()[i] >= 0.0f && x.cdata()[i] < 1.0f) || (keep.cdata()[i] != 0.0f && keep.cdata()[i] != 1.0f);
        const float p = x.cdata()[i] * keep.cdata()[i];
        bad += y.cdata()[i] != p / 0.9f;
    }
    CHECK(bad == 0 && std::fabs(mean / 512000.0 - 0.5) < 0.003 && std::fabs(kept / 512000.0 - 0.9) < 0.003);
    for (std::size_t i = 0; i < w.totalSize; ++i) s2 += static_cast<double>(w.cdata()[i]) * w.cdata()[i];
    CHECK(std::fabs(std::sqrt(s2 / 4096.0) - 0.02) < 0.002);
    bad = 0;
    for (std::size_t i = 0; i < 512; ++i) bad += labels.cdata()[i] < 0 || labels.cdata()[i] >= 1000;
    for (std::size_t i = 0; i < 4096; ++i) bad += k.cdata()[i] < 0 || k.cdata()[i] >= 10;
    for (std::size_t i = 0; i < a.totalSize; ++i) bad += !(std::fabs(a.cdata()[i]) < 0.2f) || (m.cdata()[i] != 0.0f && m.cdata()[i] != 1.0f);
    CHECK(bad == 0);
    std::vector<std::int64_t> seen(order.cdata(), order.cdata() + 512);
    std::sort(seen.begin(), seen.end());
    bad = 0;
    for (std::int64_t i = 0; i < 512; ++i) bad += seen[static_cast<std::size_t>(i)] != i;
    CHECK(bad == 0);
    // the batch holds x's rows in the order the same generator position gives
    sm::Generator again(42);
    again.seek(g.offset() - 256);
    auto rows = again.permutation(512);
    bad = 0;
    for (std::size_t i = 0; i < 512; ++i)
        for (std::size_t j = 0; j < 1000; j += 37) bad += batch.cdata()[i * 1000 + j] != x.cdata()[static_cast<std::size_t>(rows.cdata()[i]) * 1000 + j];
    CHECK(bad == 0);
    // the same program gives the same draws
    sm::Generator g2(42);
    auto x2 = g2.uniform<float>(512, 1000);
    bad = 0;
    for (std::size_t i = 0; i < x.totalSize; ++i) bad += x2.cdata()[i] != x.cdata()[i];
    CHECK(bad == 0);
    std::printf("readme_random: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
