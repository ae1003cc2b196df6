// test_count.cpp -- searchsorted / bincount / histogram through the drop-in surface: the member and the sm:: forms for the four
// element types, what throws std::invalid_argument and std::out_of_range, a view and a pending operator chain as operands,
// bincount of an argmax, the result feeding a chain, the `counts` counter and the README's snippets.
// Expected values: the same searches and counts done one by one on the host, in the order of the contract (NaNs last).
#include <sm.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>
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

static std::uint64_t g_state = 0x13579bdfull;
static std::uint64_t next() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

using Shape = std::vector<std::size_t>;
using I64 = std::int64_t;

template <typename T>
static sm::SMArray<T> from_host(const std::vector<T> &h, Shape shape) {
    T *buf = new T[h.size() ? h.size() : 1];
    std::copy(h.begin(), h.end(), buf);
    return sm::SMArray<T>(buf, std::move(shape));
}

template <typename T>
static int differences(const sm::SMArray<T> &got, const std::vector<T> &want) {
    if (got.totalSize != want.size()) return -1;
    std::vector<T> dense(want.size());
    got.copy_dense_out(dense.data());
    return std::memcmp(dense.data(), want.data(), want.size() * sizeof(T)) != 0;
}

// a before b in the contract's order
template <typename T>
static bool before(T a, T b) {
    if constexpr (std::is_floating_point_v<T>) return a < b || (b != b && a == a);
    else return a < b;
}
template <typename T>
static I64 host_search(const std::vector<T> &edges, T x, bool right) {
    I64 i = 0;
    const I64 n = static_cast<I64>(edges.size());
    if (right) while (i < n && !before(x, edges[static_cast<std::size_t>(i)])) ++i;
    else while (i < n && before(edges[static_cast<std::size_t>(i)], x)) ++i;
    return i;
}
template <typename T>
static std::vector<I64> host_histogram(const std::vector<T> &x, const std::vector<T> &edges) {
    const I64 bins = static_cast<I64>(edges.size()) - 1;
    std::vector<I64> counts(static_cast<std::size_t>(bins), 0);
    for (T v : x) {
        I64 at = host_search(edges, v, true) - 1;
        if (v == edges.back()) at = bins - 1;
        if (at >= 0 && at < bins && v == v) ++counts[static_cast<std::size_t>(at)];
    }
    return counts;
}

template <typename Fn>
static bool throws_invalid_argument(Fn fn) {
    try {
        fn();
    } catch (const std::invalid_argument &) {
        return true;
    } catch (...) {
    }
    return false;
}
template <typename Fn>
static bool throws_out_of_range(Fn fn) {
    try {
        fn();
    } catch (const std::out_of_range &) {
        return true;
    } catch (...) {
    }
    return false;
}

// values in [-span / 2, span / 2), every fourth one a multiple of 8 (where the edges below stand)
template <typename T>
static std::vector<T> values(std::size_t n, int span) {
    std::vector<T> v(n);
    for (std::size_t i = 0; i < n; ++i) {
        int k = static_cast<int>(next() % static_cast<std::uint64_t>(span)) - span / 2;
        if (i % 4 == 0) k = k / 8 * 8;
        v[i] = static_cast<T>(k);
        if constexpr (std::is_floating_point_v<T>)
            if (i % 4 == 1) v[i] += static_cast<T>(0.5);
    }
    return v;
}

template <typename T>
static void test_forms() {
    // edges with a repeat; floats end in a NaN
    std::vector<T> edges;
    for (int k = -64; k <= 64; k += 8) edges.push_back(static_cast<T>(k));
    const T repeated = edges[5];
    edges.insert(edges.begin() + 5, repeated);
    if constexpr (std::is_floating_point_v<T>) edges.push_back(std::numeric_limits<T>::quiet_NaN());
    std::vector<T> hx = values<T>(3 * 1001, 200);
    if constexpr (std::is_floating_point_v<T>) {
        hx[7] = std::numeric_limits<T>::quiet_NaN(), hx[8] = std::numeric_limits<T>::infinity(), hx[9] = -std::numeric_limits<T>::infinity();
        hx[10] = static_cast<T>(-0.0);
    } else {
        hx[7] = std::numeric_limits<T>::min(), hx[8] = std::numeric_limits<T>::max();
    }
    auto e = from_host(edges, {edges.size()});
    auto x = from_host(hx, {3, 1001});
    for (bool right : {false, true}) {
        std::vector<I64> want(hx.size());
        for (std::size_t i = 0; i < hx.size(); ++i) want[i] = host_search(edges, hx[i], right);
        const sm::side s = right ? sm::side::right : sm::side::left;
        auto member = e.searchsorted(x, s);
        auto free_form = sm::searchsorted(e, x, s);
        CHECK(member.shape() == x.shape());
        CHECK(differences(member, want) == 0);
        CHECK(differences(free_form, want) == 0);
        // a transposed view of x: the result has the view's shape and order
        auto xt = x.transpose();  // {1001, 3}
        std::vector<I64> want_t(hx.size());
        for (std::size_t i = 0; i < 3; ++i)
            for (std::size_t j = 0; j < 1001; ++j) want_t[j * 3 + i] = want[i * 1001 + j];
        auto of_view = sm::searchsorted(e, xt, s);
        CHECK(of_view.shape() == xt.shape());
        CHECK(differences(of_view, want_t) == 0);
    }
    {
        std::vector<I64> want(hx.size());
        for (std::size_t i = 0; i < hx.size(); ++i) want[i] = host_search(edges, hx[i], false);
        CHECK(differences(e.searchsorted(x), want) == 0);  // left is the default
    }
    CHECK(throws_invalid_argument([&] { x.searchsorted(x); }));  // a table that is not 1-D

    // histogram with explicit edges (no NaN among them)
    std::vector<T> table(edges.begin(), edges.begin() + 18);
    auto t = from_host(table, {table.size()});
    const std::vector<I64> want = host_histogram(hx, table);
    CHECK(differences(x.histogram(t), want) == 0);
    CHECK(differences(sm::histogram(x, t), want) == 0);
    CHECK(differences(sm::histogram(x.transpose(), t), want) == 0);
    CHECK(differences(sm::histogram(x(SLICE(1, 3), SLICE_ALL), t), host_histogram(std::vector<T>(hx.begin() + 1001, hx.end()), table)) == 0);
    CHECK(throws_invalid_argument([&] { x.histogram(x); }));
    CHECK(throws_invalid_argument([&] { x.histogram(from_host(std::vector<T>{T(1)}, {1})); }));
    // a pending chain as the operand: (x + x) is evaluated first
    if constexpr (!std::is_floating_point_v<T>) {
        std::vector<T> twice(hx.size());
        for (std::size_t i = 0; i < hx.size(); ++i) twice[i] = static_cast<T>(static_cast<std::make_unsigned_t<T>>(hx[i]) * 2u);
        CHECK(differences(sm::histogram(x + x, t), host_histogram(twice, table)) == 0);
    } else {
        std::vector<T> twice(hx.size());
        for (std::size_t i = 0; i < hx.size(); ++i) twice[i] = hx[i] + hx[i];
        CHECK(differences(sm::histogram(x + x, t), host_histogram(twice, table)) == 0);
        CHECK(differences(sm::searchsorted(t, x + x, sm::side::right), [&] {
                  std::vector<I64> w(twice.size());
                  for (std::size_t i = 0; i < twice.size(); ++i) w[i] = host_search(table, twice[i], true);
                  return w;
              }()) == 0);
    }
}

template <typename T>
static void test_uniform() {
    std::vector<T> hx(40003);
    for (std::size_t i = 0; i < hx.size(); ++i) hx[i] = static_cast<T>(static_cast<double>(next() % 2000001) / 1e6 * 10.0 - 10.0);  // [-10, 10]
    hx[0] = T(-3), hx[1] = T(5), hx[2] = std::numeric_limits<T>::quiet_NaN(), hx[3] = std::numeric_limits<T>::infinity();
    auto x = from_host(hx, {hx.size()});
    for (I64 bins : {I64{1}, I64{7}, I64{256}, I64{9000}}) {
        auto [counts, edges] = sm::histogram(x, bins, -3.0, 5.0);
        CHECK(edges.totalSize == static_cast<std::size_t>(bins) + 1 && counts.totalSize == static_cast<std::size_t>(bins));
        std::vector<T> table(edges.totalSize);
        edges.copy_dense_out(table.data());
        bool linspace = table.front() == T(-3) && table.back() == T(5);
        const double step = 8.0 / static_cast<double>(bins);
        for (I64 i = 0; i < bins; ++i) {
            volatile double prod = static_cast<double>(i) * step;
            linspace = linspace && table[static_cast<std::size_t>(i)] == static_cast<T>(prod + -3.0);
        }
        CHECK(linspace);
        CHECK(differences(counts, host_histogram(hx, table)) == 0);
        auto [member_counts, member_edges] = x.histogram(bins, -3.0, 5.0);
        CHECK(differences(member_counts, host_histogram(hx, table)) == 0 && differences(member_edges, table) == 0);
        CHECK(differences(sm::histogram(x, edges), host_histogram(hx, table)) == 0);  // the explicit form of the same table
    }
    {   // a range of one point is (lo - 0.5, hi + 0.5)
        auto [counts, edges] = sm::histogram(x, 4, 2.0, 2.0);
        CHECK(differences(edges, std::vector<T>{T(1.5), T(1.75), T(2), T(2.25), T(2.5)}) == 0);
        std::vector<T> table{T(1.5), T(1.75), T(2), T(2.25), T(2.5)};
        CHECK(differences(counts, host_histogram(hx, table)) == 0);
    }
    CHECK(throws_invalid_argument([&] { sm::histogram(x, 0, 0.0, 1.0); }));
    CHECK(throws_invalid_argument([&] { sm::histogram(x, -2, 0.0, 1.0); }));
    CHECK(throws_invalid_argument([&] { sm::histogram(x, 4, 1.0, 0.0); }));
    CHECK(throws_invalid_argument([&] { sm::histogram(x, 4, 0.0, std::numeric_limits<double>::infinity()); }));
    CHECK(throws_invalid_argument([&] { sm::histogram(x, 4, std::nan(""), 1.0); }));
    if constexpr (std::is_same_v<T, float>) CHECK(throws_invalid_argument([&] { sm::histogram(x, 64, 1.0, 1.0 + std::ldexp(1.0, -20)); }));
    else CHECK(!throws_invalid_argument([&] { sm::histogram(x, 64, 1.0, 1.0 + std::ldexp(1.0, -20)); }));
}

template <typename I>
static void test_bincount() {
    const I64 R = 300;
    std::vector<I> hids(50001);
    std::vector<I64> plain(R, 0), wrapped(R, 0), clipped(R, 0);
    for (std::size_t i = 0; i < hids.size(); ++i) {
        const I64 id = static_cast<I64>(next() % (2 * R)) - R;  // [-R, R)
        hids[i] = static_cast<I>(id);
        ++plain[static_cast<std::size_t>(id < 0 ? id + R : id)];
    }
    auto ids = from_host(hids, {hids.size()});
    CHECK(differences(ids.bincount(R), plain) == 0);
    CHECK(differences(sm::bincount(ids, R), plain) == 0);
    CHECK(differences(sm::bincount(ids, R, sm::index_mode::wrap), plain) == 0);
    // ids outside [-R, R): clip and wrap count them somewhere, checked drops them and throws
    std::vector<I> bad(hids);
    bad[5] = static_cast<I>(R), bad[6] = static_cast<I>(-R - 1), bad[7] = std::numeric_limits<I>::max(), bad[8] = std::numeric_limits<I>::min();
    for (I v : bad) {
        const I64 id = static_cast<I64>(v);
        ++clipped[static_cast<std::size_t>(std::min<I64>(std::max<I64>(id, 0), R - 1))];
        ++wrapped[static_cast<std::size_t>(((id % R) + R) % R)];
    }
    auto with_bad = from_host(bad, {bad.size()});
    CHECK(differences(sm::bincount(with_bad, R, sm::index_mode::clip), clipped) == 0);
    CHECK(differences(sm::bincount(with_bad, R, sm::index_mode::wrap), wrapped) == 0);
    CHECK(throws_out_of_range([&] { sm::bincount(with_bad, R); }));
    CHECK(throws_invalid_argument([&] { sm::bincount(ids, 0); }));
    CHECK(throws_invalid_argument([&] { sm::bincount(ids, -1); }));
    // the contract: the same bits as index_add of ones onto zeros
    if constexpr (std::is_same_v<I, I64>) {
        for (sm::index_mode mode : {sm::index_mode::clip, sm::index_mode::wrap}) {
            auto target = sm::zeros<I64>(static_cast<std::size_t>(R));
            sm::index_add(target, with_bad, I64{1}, 0, mode);
            std::vector<I64> want(static_cast<std::size_t>(R));
            target.copy_dense_out(want.data());
            CHECK(differences(sm::bincount(with_bad, R, mode), want) == 0);
        }
    }
    // a 2-D view is read row-major; more bins than LDS holds take the other route
    auto grid = from_host(hids, {167, 299});  // 49933 of the ids
    std::vector<I64> of_view(20000, 0);
    for (std::size_t j = 0; j < 150; ++j)
        for (std::size_t i = 0; i < 167; ++i) {
            const I64 id = static_cast<I64>(hids[i * 299 + j]);
            ++of_view[static_cast<std::size_t>(id < 0 ? id + 20000 : id)];
        }
    CHECK(differences(sm::bincount(grid(SLICE_ALL, SLICE(0, 150)), 20000), of_view) == 0);
    // four ids, one of them out of range: checked throws (the counts go with the exception), and the next calls on this thread work --
    // the same ids with the bad one clipped, then checked again without it
    auto four = from_host(std::vector<I>{I(1), I(4), I(-1), I(1)}, {4});
    const auto before = sm::fusion_stats();
    CHECK(throws_out_of_range([&] { four.bincount(4); }));
    CHECK(sm::fusion_stats().counts - before.counts == 1);
    CHECK(differences(four.bincount(4, sm::index_mode::clip), std::vector<I64>{1, 2, 0, 1}) == 0);
    CHECK(differences(four(SLICE(2, 4)).bincount(4), std::vector<I64>{0, 1, 0, 1}) == 0);
}

static void test_chains_and_counter() {
    // bincount(argmax(x, -1), classes): how often each class wins
    const std::size_t rows = 4096, classes = 10;
    std::vector<float> hs(rows * classes);
    std::vector<I64> wins(classes, 0);
    for (std::size_t i = 0; i < rows; ++i) {
        std::size_t best = 0;
        for (std::size_t c = 0; c < classes; ++c) {
            hs[i * classes + c] = static_cast<float>(next() % 100003);
            if (hs[i * classes + c] > hs[i * classes + best]) best = c;
        }
        ++wins[best];
    }
    auto scores = from_host(hs, {rows, classes});
    const auto before = sm::fusion_stats();
    auto tally = sm::bincount(sm::argmax(scores, -1), static_cast<I64>(classes));
    CHECK(sm::fusion_stats().counts == before.counts + 1);
    CHECK(differences(tally, wins) == 0);
    // the result feeds a chain: a running total and its end, as written in the README
    auto running = tally.cumsum(0);
    auto total = tally.sum(0, true);
    std::vector<I64> acc(classes);
    I64 sum = 0;
    for (std::size_t c = 0; c < classes; ++c) acc[c] = sum += wins[c];
    CHECK(differences(running, acc) == 0);
    CHECK(differences(total, std::vector<I64>{static_cast<I64>(rows)}) == 0);
    auto twice = tally + tally;
    for (auto &w : wins) w *= 2;
    CHECK(differences(twice, wins) == 0);
}

static void test_readme_snippets() {
    // a histogram, its running total and its CDF
    auto x = sm::zeros<float>(1 << 16);  // ... samples ...
    for (std::size_t i = 0; i < x.totalSize; ++i) x.data[i] = static_cast<float>(static_cast<double>(next() % 1000001) / 1e6 * 9.0 - 4.5);
    auto [counts, edges] = sm::histogram(x, 64, -4.0, 4.0);      // np.histogram(x, 64, range=(-4, 4))
    auto running = counts.cumsum(0);                              // exact, std::int64_t
    auto inside = counts.sum(0, true);                            // how many samples fell inside the range
    auto cdf = sm::zeros<double>(64);
    for (std::size_t b = 0; b < 64; ++b) cdf.data[b] = static_cast<double>(running.cdata()[b]) / static_cast<double>(inside.cdata()[0]);
    std::vector<float> hx(x.totalSize), table(65);
    x.copy_dense_out(hx.data());
    edges.copy_dense_out(table.data());
    const std::vector<I64> want = host_histogram(hx, table);
    CHECK(differences(counts, want) == 0);
    I64 sum = 0;
    for (I64 w : want) sum += w;
    CHECK(running.cdata()[63] == sum && inside.cdata()[0] == sum && cdf.cdata()[63] == 1.0);
    // the bin of every sample, and the samples of one bin counted again
    auto bin = sm::searchsorted(edges, x, sm::side::right);       // 0: below the range, 65: above it (or NaN)
    int bad = 0;
    for (std::size_t i = 0; i < hx.size(); ++i) bad += bin.cdata()[i] != host_search(table, hx[i], true);
    CHECK(bad == 0);
    auto again = sm::bincount(bin, 66);                           // positions 1 .. 64 are the histogram's bins
    std::vector<I64> shifted(66);
    again.copy_dense_out(shifted.data());
    bad = 0;
    for (std::size_t b = 0; b + 1 < 64; ++b) bad += shifted[b + 1] != want[b];
    CHECK(bad == 0);
    // bincount replaces the index_add spelling
    auto samples = sm::zeros<std::int64_t>(70001);                // ... values in [0, 256) ...
    for (std::size_t i = 0; i < 70001; ++i) samples.data[i] = static_cast<I64>(next() % 256);
    auto per_value = sm::bincount(samples, 256);
    auto spelled = sm::zeros<std::int64_t>(256);
    sm::index_add(spelled, samples, std::int64_t{1}, 0);
    std::vector<I64> w(256);
    spelled.copy_dense_out(w.data());
    CHECK(differences(per_value, w) == 0);
    // explicit edges: quartile-like bins
    auto cuts = sm::zeros<float>(5);
    for (std::size_t i = 0; i < 5; ++i) cuts.data[i] = -4.0f + 2.0f * static_cast<float>(i);
    auto quarters = sm::histogram(x, cuts);
    std::vector<float> hc{-4.0f, -2.0f, 0.0f, 2.0f, 4.0f};
    CHECK(differences(quarters, host_histogram(hx, hc)) == 0);
}

int main() {
    try {
        test_forms<float>();
        test_forms<double>();
        test_forms<int>();
        test_forms<std::int64_t>();
        test_uniform<float>();
        test_uniform<double>();
        test_bincount<int>();
        test_bincount<std::int64_t>();
        test_chains_and_counter();
        test_readme_snippets();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_count: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
