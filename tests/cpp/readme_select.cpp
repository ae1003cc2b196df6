// The snippets of README.md, "Choosing by condition", compiled and run by tests/test_select_cpp.py so they cannot rot: each one with
// data for which the answer is known.
#include <sm.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

static int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) ++g_failures, std::printf("FAIL line %d  %s\n", __LINE__, #cond); \
    } while (0)

int main() {
    const std::size_t n = 1 << 16;
    auto x = sm::zeros<float>(n);
    auto keys = sm::zeros<int>(n);
    auto y = sm::zeros<float>(n);
    std::size_t positive = 0, nans = 0, large_keys = 0, above_one = 0;
    for (std::size_t i = 0; i < n; ++i) {
        const float v = static_cast<float>(static_cast<int>(i % 13) - 6);   // -6 .. 6
        x.data[i] = i % 97 == 0 ? std::numeric_limits<float>::quiet_NaN() : v;
        keys.data[i] = static_cast<int>(i % 7);
        y.data[i] = static_cast<float>(i);
        nans += i % 97 == 0;
        positive += i % 97 != 0 && v > 0.0f;
        above_one += i % 97 != 0 && v > 1.0f;
        large_keys += i % 7 > 3;
    }
    auto relu = sm::where(x > 0.0f, x, 0.0f);                     // one pass, 8 bytes per element
    CHECK(sm::count_nonzero(relu) == static_cast<std::int64_t>(positive) && relu(5) == 0.0f && relu(12) == 6.0f && relu(0) == 0.0f);
    auto clean = x.select(x == x);                                // x[~isnan(x)]
    CHECK(clean.totalSize == n - nans && sm::count_nonzero(clean != clean) == 0);
    auto large = x.select(keys > 3);                              // values[keys > t]: another element type than the condition's
    CHECK(large.totalSize == large_keys && large(0) == x(4));
    auto table = sm::zeros<float>(1 << 8, 1 << 8);                // ... a row per record ...
    auto labels = sm::zeros<std::int64_t>(1 << 8);                // ... a label per row ...
    for (std::size_t r = 0; r < 256; ++r) {
        labels.data[r] = static_cast<std::int64_t>(r % 3);
        for (std::size_t c = 0; c < 256; ++c) table.data[r * 256 + c] = static_cast<float>(r);
    }
    auto rows_of_2 = sm::compress(labels == 2, table, 0);         // the rows whose label is 2
    CHECK((rows_of_2.shape() == std::vector<std::size_t>{85, 256}) && rows_of_2(0, 0) == 2.0f && rows_of_2(84, 255) == 254.0f);
    auto at = sm::flatnonzero(x > 1.0f);                          // the positions once ...
    auto xs = x.take_flat(at), ys = y.take_flat(at);              // ... for two arrays
    CHECK(at.totalSize == above_one && xs.totalSize == above_one && ys(0) == 8.0f && xs(0) == 2.0f);
    x.assign_where(x > 4.0f, 4.0f);                               // clip from above, in place
    CHECK(sm::count_nonzero(x > 4.0f) == 0 && x(12) == 4.0f && x(3) == -3.0f);
    auto inside = sm::mask(x > -1.0f) * sm::mask(x < 1.0f);       // and
    CHECK(inside(6) == 1.0f && inside(5) == 0.0f && inside(7) == 0.0f && inside(0) == 0.0f);
    auto m = sm::mask(x > 0.0f);
    auto either = m + inside - m * inside, neither = -either + 1.0f;   // or, not
    CHECK(either(6) == 1.0f && either(9) == 1.0f && either(2) == 0.0f && neither(2) == 1.0f && neither(6) == 0.0f);
    std::printf("readme_select: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
