// The snippet of README.md, "Medians and quantiles", compiled and run by tests/test_quantile_cpp.py so it cannot rot, with data for
// which the answer is known.
#include <sm.h>

#include <cmath>
#include <cstdio>
#include <vector>

static int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) ++g_failures, std::printf("FAIL line %d  %s\n", __LINE__, #cond); \
    } while (0)

int main() {
    auto x = sm::ones<float>(512, 1001);                          // one row per sample
    for (std::size_t i = 0; i < 512; ++i)
        for (std::size_t j = 0; j < 1001; ++j) x.data[i * 1001 + (j * 10 + i) % 1001] = static_cast<float>(j) + static_cast<float>(i);  // row i: i .. i + 1000, shuffled

    using sm::quantile_method;
    auto med = sm::median(x, -1);                                 // shape {512}: the median of each row, no sort
    auto box = sm::quantile(x, {0.25, 0.5, 0.75}, -1);            // shape {3, 512}: the quartiles from ONE read of x
    auto q25 = sm::quantile(x, 0.25, -1, quantile_method::linear, /*keepdims=*/true);   // shape {512, 1}: broadcasts against x
    auto q75 = sm::quantile(x, 0.75, -1, quantile_method::linear, true);
    sm::SMArray<float> robust = (x - sm::median(x, -1, true)) / (q75 - q25);  // robust standardising: the results feed the chain
    auto ends = sm::percentile(x, {1.0, 99.0}, -1, quantile_method::nearest);  // clipping bounds that are elements of the row
    auto by_column = x.median(0);                                 // member form, along the first axis: shape {1001}
    auto overall = sm::quantile(x, 0.9);                          // no axis: the row-major flattening, shape {1}

    CHECK((med.shape() == std::vector<std::size_t>{512}) && (box.shape() == std::vector<std::size_t>{3, 512}));
    CHECK((q25.shape() == std::vector<std::size_t>{512, 1}) && (robust.shape() == std::vector<std::size_t>{512, 1001}));
    CHECK((ends.shape() == std::vector<std::size_t>{2, 512}) && (by_column.shape() == std::vector<std::size_t>{1001}) && overall.totalSize == 1);
    int bad_box = 0, bad_kept = 0, bad_ends = 0, bad_robust = 0, bad_column = 0;
    for (std::size_t i = 0; i < 512; ++i) {
        const float base = static_cast<float>(i);
        bad_box += med.cdata()[i] != base + 500.0f || box.cdata()[i] != base + 250.0f || box.cdata()[512 + i] != base + 500.0f || box.cdata()[1024 + i] != base + 750.0f;
        bad_kept += q25.cdata()[i] != base + 250.0f || q75.cdata()[i] != base + 750.0f;
        bad_ends += ends.cdata()[i] != base + 10.0f || ends.cdata()[512 + i] != base + 990.0f;
        for (std::size_t j = 0; j < 1001; j += 100) {
            const float want = (x.cdata()[i * 1001 + j] - (base + 500.0f)) / 500.0f;
            bad_robust += !(std::fabs(robust.cdata()[i * 1001 + j] - want) <= 1e-6f * std::fabs(want));  // (the quotient's last place is the chain's affair)
        }
    }
    for (std::size_t j = 0; j < 1001; ++j) bad_column += !(by_column.cdata()[j] >= 0.0f && by_column.cdata()[j] <= 1511.0f);
    CHECK(bad_box == 0);
    CHECK(bad_kept == 0);
    CHECK(bad_ends == 0);
    CHECK(bad_robust == 0);
    CHECK(bad_column == 0 && overall.cdata()[0] >= 1100.0f && overall.cdata()[0] <= 1300.0f);
    std::printf("readme_quantile: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
