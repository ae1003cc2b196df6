// The snippets of README.md, "The distinct values", compiled and run by tests/test_unique_cpp.py so they cannot rot: each one with data
// for which the answer is known.
#include <sm.h>

#include <cstdint>
#include <cstdio>
#include <vector>

static int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) ++g_failures, std::printf("FAIL line %d  %s\n", __LINE__, #cond); \
    } while (0)

int main() {
    // ---- a group-by: the sum of v per key, keys of any range
    const std::size_t n = 1 << 16;
    auto k = sm::zeros<std::int64_t>(n);
    auto v = sm::zeros<float>(n);
    for (std::size_t i = 0; i < n; ++i) {
        k.data[i] = (static_cast<std::int64_t>(i % 5) - 2) * (std::int64_t{1} << 40);   // -2^41, -2^40, 0, 2^40, 2^41: no bincount reaches these
        v.data[i] = static_cast<float>(i % 5);
    }
    auto [keys, inverse] = sm::unique_inverse(k);                 // the distinct keys, and the group of every element
    auto sums = sm::zeros<float>(keys.totalSize);
    sums.index_add(inverse, v, 0);                                // one sum per key; nothing left HBM
    CHECK(keys.totalSize == 5 && keys(0) == -(std::int64_t{1} << 41) && keys(4) == std::int64_t{1} << 41);
    CHECK(inverse.totalSize == n && inverse(0) == 0 && inverse(7) == 2);
    const float per_key = static_cast<float>(n / 5);
    CHECK(sums(0) == 0.0f && sums(1) == per_key && sums(4) == 4.0f * per_key);
    auto [values, counts] = sm::unique_counts(k);                 // np.unique(k, return_counts=True)
    CHECK(values.totalSize == 5 && counts(0) == static_cast<std::int64_t>(n / 5 + 1) && counts(4) == static_cast<std::int64_t>(n / 5));

    // ---- run-length encoding: no sort, the order of the data is kept
    auto signal = sm::zeros<int>(12);
    const int samples[12] = {7, 7, 7, 2, 2, 7, 9, 9, 9, 9, 2, 2};
    for (std::size_t i = 0; i < 12; ++i) signal.data[i] = samples[i];
    auto [symbols, lengths] = sm::run_lengths(signal);            // {7, 2, 7, 9, 2} and {3, 2, 1, 4, 2}
    CHECK(symbols.totalSize == 5 && symbols(0) == 7 && symbols(1) == 2 && symbols(2) == 7 && symbols(3) == 9 && symbols(4) == 2);
    CHECK(lengths(0) == 3 && lengths(1) == 2 && lengths(2) == 1 && lengths(3) == 4 && lengths(4) == 2);
    auto changes = sm::unique_consecutive(signal);                // the symbols alone
    CHECK(changes.totalSize == 5 && changes(3) == 9);
    std::printf("readme_unique: %d failures\n", g_failures);
    return g_failures ? 1 : 0;
}
