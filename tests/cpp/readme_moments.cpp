// The snippet of README.md, "Variance and standardising", compiled and run by tests/test_moments_cpp.py so it cannot rot, with data
// for which the answer is known.
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
    auto n = sm::ones<float>(4096, 512);                            // one row per sample, one column per feature
    auto img = sm::ones<float>(4, 8, 8, 3);
    // element (i, j) = 1000 + j + (i mod 4): every column holds 0, 1, 2, 3 equally often on top of its offset
    for (std::size_t i = 0; i < 4096; ++i)
        for (std::size_t j = 0; j < 512; ++j) n.data[i * 512 + j] = 1000.0f + static_cast<float>(j) + static_cast<float>(i % 4);
    for (std::size_t i = 0; i < 4 * 8 * 8; ++i)
        for (std::size_t c = 0; c < 3; ++c) img.data[i * 3 + c] = static_cast<float>(c) * static_cast<float>(i % 2);  // channel c: 0 and c alternating

    auto sd_col = sm::stddev(n, 0, 1, true);                        // per column, ddof = 1, shape {1, 512}: broadcasts straight back
    auto [var_col, mean_col] = sm::var_mean(n, 0, 0, true);         // both statistics from one call
    sm::SMArray<float> z = (n - mean_col) / sd_col;                 // ... into ONE chain launch
    auto layer = sm::standardize(n, -1, 1e-5);                      // each row to mean 0, variance 1: one read, one write
    auto per_channel = sm::var(img, {0, 1, 2});                     // NHWC (N, H, W, 3) -> shape {3}
    auto spread = n.stddev();                                       // member form, every element: shape {1}

    CHECK((sd_col.shape() == std::vector<std::size_t>{1, 512}) && (var_col.shape() == std::vector<std::size_t>{1, 512}) && (mean_col.shape() == std::vector<std::size_t>{1, 512}));
    CHECK(z.shape() == n.shape() && layer.shape() == n.shape() && (per_channel.shape() == std::vector<std::size_t>{3}) && (spread.shape() == std::vector<std::size_t>{1}));
    int bad = 0;
    const double sd1 = std::sqrt(1.25 * 4096.0 / 4095.0);  // 0, 1, 2, 3: variance 1.25
    for (std::size_t j = 0; j < 512; ++j) {
        bad += var_col.cdata()[j] != 1.25f;
        bad += mean_col.cdata()[j] != 1001.5f + static_cast<float>(j);
        bad += !(std::fabs(sd_col.cdata()[j] - sd1) <= 1e-7 * sd1);
        bad += !(std::fabs(z.cdata()[5 * 512 + j] - (-0.5 / sd1)) <= 1e-6);  // row 5: i mod 4 = 1
    }
    CHECK(bad == 0);
    // a row is 1000 + (i mod 4) + 0 .. 511: mean 1255.5 + (i mod 4), variance (512^2 - 1) / 12
    const double row_var = (512.0 * 512.0 - 1.0) / 12.0;
    for (std::size_t i = 0; i < 4096; i += 97)
        for (std::size_t j = 0; j < 512; j += 31) bad += !(std::fabs(layer.cdata()[i * 512 + j] - (static_cast<double>(j) - 255.5) / std::sqrt(row_var + 1e-5)) <= 1e-6);
    CHECK(bad == 0);
    for (std::size_t c = 0; c < 3; ++c) bad += per_channel.cdata()[c] != static_cast<float>(c * c) / 4.0f;  // 0 and c equally often
    CHECK(bad == 0);
    CHECK(std::fabs(spread.cdata()[0] - std::sqrt(row_var + 1.25)) <= 1e-5 * std::sqrt(row_var));
    std::printf("readme_moments: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
