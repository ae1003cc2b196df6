// The snippets of README.md, "Changing the element type", compiled and run by tests/test_astype_cpp.py so they cannot rot: each one with
// data for which the answer is known.
#include <sm.h>

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
    // ---- histogram density: integer counts into a float chain
    const std::size_t n = 1 << 16;
    auto x = sm::zeros<float>(n);
    std::vector<float> hx(n);
    for (std::size_t i = 0; i < n; ++i) x.data[i] = hx[i] = -4.0f + 8.0f * (static_cast<float>((i * 7919u) % n) + 0.5f) / static_cast<float>(n);
    auto [counts, edges] = sm::histogram(x, 64, -4.0, 4.0);      // std::int64_t counts
    const float width = 8.0f / 64.0f;
    auto density = counts.astype<float>() / (static_cast<float>(n) * width);   // np.histogram(x, 64, (-4, 4), density=True)
    CHECK(density.totalSize == 64);
    double area = 0;
    int bad = 0;
    for (std::size_t b = 0; b < 64; ++b) {
        bad += density(b) != static_cast<float>(counts(b)) / (static_cast<float>(n) * width);
        area += static_cast<double>(density(b)) * width;
    }
    CHECK(bad == 0 && std::fabs(area - 1.0) < 1e-6);

    // ---- accuracy: argmax gives std::int64_t, mean wants a float type
    const std::size_t rows = 1 << 10, classes = 10;
    auto logits = sm::zeros<float>(rows, classes);
    auto labels = sm::zeros<std::int64_t>(rows);
    std::size_t right = 0;
    for (std::size_t i = 0; i < rows; ++i) {
        logits.data[i * classes + (i * 3) % classes] = 1.0f;                          // the prediction
        labels.data[i] = static_cast<std::int64_t>(i % 4 ? (i * 3) % classes : (i * 3 + 1) % classes);  // every fourth label differs
        right += i % 4 != 0;
    }
    auto pred = sm::argmax(logits, -1);
    auto accuracy = sm::mask(pred == labels).astype<double>().mean(0);          // mean(pred == labels), shape {1}
    CHECK(accuracy.totalSize == 1 && accuracy(0) == static_cast<double>(right) / static_cast<double>(rows));

    // ---- int keys widened for take
    auto table = sm::zeros<float>(1 << 8);
    for (std::size_t i = 0; i < 256; ++i) table.data[i] = static_cast<float>(i) * 0.5f;
    auto keys = sm::zeros<int>(n);
    for (std::size_t i = 0; i < n; ++i) keys.data[i] = static_cast<int>((i * 31) % 256);
    auto picked = table.take(keys.astype<std::int64_t>(), 0);                    // take wants std::int64_t positions
    bad = 0;
    for (std::size_t i = 0; i < n; i += 97) bad += picked(i) != static_cast<float>((i * 31) % 256) * 0.5f;
    CHECK(picked.totalSize == n && bad == 0);

    // ---- float data scanned in double
    auto running = x.astype<double>().cumsum(0);
    double want = 0;
    bad = 0;
    for (std::size_t i = 0; i < n; ++i) {
        want += static_cast<double>(hx[i]);
        bad += std::fabs(running.cdata()[i] - want) > 1e-7;
    }
    CHECK(bad == 0);

    // ---- a quantised float signal into bincount
    auto level = ((x + 4.0f) * 32.0f).astype<int>();                            // toward zero; saturating, NaN -> 0
    auto per_level = sm::bincount(level, 256);
    std::vector<std::int64_t> host_levels(256, 0);
    for (std::size_t i = 0; i < n; ++i) ++host_levels[static_cast<std::size_t>(static_cast<int>((hx[i] + 4.0f) * 32.0f))];
    bad = 0;
    for (std::size_t b = 0; b < 256; ++b) bad += per_level(b) != host_levels[b];
    CHECK(bad == 0);

    std::printf("readme_astype: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
