// test_unique.cpp -- the distinct values through the drop-in surface: unique_values / unique / unique_counts / unique_inverse /
// unique_all / unique_consecutive / run_lengths, free and member forms, for the four element types, both settings of equal_nan, views
// and pending operator chains as operands, empty operands, values.take_flat(inverse) rebuilding the operand, unique_counts against
// bincount, the group-by through index_add, and the `uniques` and `sorts` counters.
// Expected values: a stable sort on the host under the library's order (a before b when a < b, or when b is a NaN and a is not), then
// the runs of its result one by one.  Nothing here throws below the sort's limit of 2^31 elements, which is the sort's own refusal
// (tests/test_sort_*.py) and which no test allocates.
#include <sm.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>
#include <type_traits>
#include <utility>
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
static std::vector<T> to_host(const sm::SMArray<T> &a) {
    std::vector<T> dense(a.totalSize);
    if (a.totalSize) a.copy_dense_out(dense.data());
    return dense;
}

template <typename T>
static bool same_bytes(const sm::SMArray<T> &got, const std::vector<T> &want) {
    if (got.totalSize != want.size() || got.shape() != Shape{want.size()}) return false;
    const std::vector<T> dense = to_host(got);
    return want.empty() || std::memcmp(dense.data(), want.data(), want.size() * sizeof(T)) == 0;
}

template <typename T>
static bool is_nan(T x) {
    if constexpr (std::is_floating_point_v<T>) return std::isnan(x);
    else return false;
}
template <typename T>
static bool before(T a, T b) { return a < b || (is_nan(b) && !is_nan(a)); }
template <typename T>
static bool same(T a, T b, bool equal_nan) { return a == b || (equal_nan && is_nan(a) && is_nan(b)); }

template <typename T>
struct Model {
    std::vector<T> values;
    std::vector<I64> index, inverse, counts;
};
// sorted: np.unique; otherwise the runs of x as it stands.
template <typename T>
static Model<T> model(const std::vector<T> &x, bool sorted, bool equal_nan) {
    std::vector<I64> order(x.size());
    std::iota(order.begin(), order.end(), I64{0});
    if (sorted) std::stable_sort(order.begin(), order.end(), [&](I64 a, I64 b) { return before(x[a], x[b]); });
    Model<T> m;
    m.inverse.resize(x.size());
    for (std::size_t i = 0; i < x.size(); ++i) {
        if (i == 0 || !same(x[order[i - 1]], x[order[i]], equal_nan)) m.values.push_back(x[order[i]]), m.index.push_back(order[i]), m.counts.push_back(0);
        ++m.counts.back();
        m.inverse[order[i]] = static_cast<I64>(m.values.size()) - 1;
    }
    return m;
}

// few distinct whole numbers, and for the floats NaNs of both signs, both zeros and the infinities
template <typename T>
static std::vector<T> keys(std::size_t n, int distinct) {
    std::vector<T> v(n);
    for (std::size_t i = 0; i < n; ++i) v[i] = static_cast<T>(static_cast<int>(next() % distinct) - distinct / 2);
    if constexpr (std::is_floating_point_v<T>) {
        const T nan = std::numeric_limits<T>::quiet_NaN(), inf = std::numeric_limits<T>::infinity();
        const T special[] = {nan, -nan, T(-0.0), T(0.0), inf, -inf, nan, T(-0.0)};
        for (std::size_t k = 0; k < 8 && n; ++k) v[next() % n] = special[k];
    } else if (n > 2) {
        v[next() % n] = std::numeric_limits<T>::min(), v[next() % n] = std::numeric_limits<T>::max();
    }
    return v;
}

// every form over one operand whose row-major flattening is `flat`
template <typename T>
static void check_forms(const sm::SMArray<T> &a, const std::vector<T> &flat) {
    for (const bool equal_nan : {true, false}) {
        const Model<T> u = model(flat, true, equal_nan), r = model(flat, false, equal_nan);
        CHECK(same_bytes(sm::unique_values(a, equal_nan), u.values));
        CHECK(same_bytes(sm::unique(a, equal_nan), u.values));
        CHECK(same_bytes(a.unique_values(equal_nan), u.values));
        CHECK(same_bytes(a.unique(equal_nan), u.values));
        {
            auto [values, counts] = sm::unique_counts(a, equal_nan);
            CHECK(same_bytes(values, u.values) && same_bytes(counts, u.counts));
            auto member = a.unique_counts(equal_nan);
            CHECK(same_bytes(member.first, u.values) && same_bytes(member.second, u.counts));
        }
        {
            auto [values, inverse] = sm::unique_inverse(a, equal_nan);
            CHECK(same_bytes(values, u.values) && same_bytes(inverse, u.inverse));
            auto member = a.unique_inverse(equal_nan);
            CHECK(same_bytes(member.first, u.values) && same_bytes(member.second, u.inverse));
            // values.take_flat(inverse) rebuilds the flattening, up to which zero and which NaN
            const std::vector<T> back = to_host(values.take_flat(inverse, sm::index_mode::clip));
            bool rebuilt = back.size() == flat.size();
            for (std::size_t i = 0; rebuilt && i < flat.size(); ++i) rebuilt = same(back[i], flat[i], true) && (equal_nan || !is_nan(flat[i]) || std::memcmp(&back[i], &flat[i], sizeof(T)) == 0);
            CHECK(rebuilt);
        }
        {
            const sm::UniqueAll<T> all = sm::unique_all(a, equal_nan), member = a.unique_all(equal_nan);
            CHECK(same_bytes(all.values, u.values) && same_bytes(all.index, u.index) && same_bytes(all.inverse, u.inverse) && same_bytes(all.counts, u.counts));
            CHECK(same_bytes(member.values, u.values) && same_bytes(member.index, u.index) && same_bytes(member.inverse, u.inverse) && same_bytes(member.counts, u.counts));
        }
        CHECK(same_bytes(sm::unique_consecutive(a, equal_nan), r.values));
        CHECK(same_bytes(a.unique_consecutive(equal_nan), r.values));
        {
            auto [values, lengths] = sm::run_lengths(a, equal_nan);
            CHECK(same_bytes(values, r.values) && same_bytes(lengths, r.counts));
            auto member = a.run_lengths(equal_nan);
            CHECK(same_bytes(member.first, r.values) && same_bytes(member.second, r.counts));
        }
    }
}

template <typename T>
static void test_type() {
    // sizes on both sides of a tile and of the one-workgroup route (the C ABI's tests walk them all), few and many distinct values
    for (const std::size_t n : {std::size_t{1}, std::size_t{2}, std::size_t{257}, std::size_t{8193}, std::size_t{70001}}) {
        const std::vector<T> h = keys<T>(n, n < 1000 ? 5 : 1000);
        check_forms(from_host(h, Shape{n}), h);
    }
    // runs: sorted blocks make long ones
    {
        std::vector<T> h = keys<T>(5000, 9);
        std::sort(h.begin(), h.begin() + 2500, [](T a, T b) { return before(a, b); });
        check_forms(from_host(h, Shape{5000}), h);
    }
    // a 2-D operand, its transpose and a stepped slice: the flattening is row-major over the VIEW
    {
        const std::size_t rows = 37, cols = 53;
        const std::vector<T> h = keys<T>(rows * cols, 11);
        const sm::SMArray<T> a = from_host(h, Shape{rows, cols});
        check_forms(a, h);
        std::vector<T> t(rows * cols), s;
        for (std::size_t r = 0; r < rows; ++r)
            for (std::size_t c = 0; c < cols; ++c) t[c * rows + r] = h[r * cols + c];
        check_forms(a.transpose(), t);
        for (std::size_t r = 3; r < 30; ++r)
            for (std::size_t c = 1; c < 50; ++c) s.push_back(h[r * cols + c]);
        check_forms(a(SLICE(3, 30), SLICE(1, 50)), s);
    }
    // a pending chain as the operand: evaluated first
    {
        const std::size_t n = 3001;
        const std::vector<T> x = keys<T>(n, 4), y = keys<T>(n, 3);
        std::vector<T> sum(n);
        for (std::size_t i = 0; i < n; ++i) {
            if constexpr (std::is_floating_point_v<T>) sum[i] = x[i] + y[i];
            else sum[i] = static_cast<T>(static_cast<std::make_unsigned_t<T>>(x[i]) + static_cast<std::make_unsigned_t<T>>(y[i]));
        }
        const sm::SMArray<T> ax = from_host(x, Shape{n}), ay = from_host(y, Shape{n});
        const Model<T> u = model(sum, true, true), r = model(sum, false, true);
        bool nan_free = true;
        for (T v : sum) nan_free = nan_free && !is_nan(v);
        if (nan_free) {  // (inf + -inf makes a NaN whose sign the host and the device need not agree on)
            CHECK(same_bytes(sm::unique_values(ax + ay), u.values));
            CHECK(same_bytes((ax + ay).unique_counts().second, u.counts));
            CHECK(same_bytes(sm::run_lengths(ax + ay).second, r.counts));
        } else {
            CHECK(sm::unique_values(ax + ay).totalSize == u.values.size());
            CHECK(same_bytes((ax + ay).unique_counts().second, u.counts));
            CHECK(same_bytes(sm::run_lengths(ax + ay).second, r.counts));
        }
    }
    // an empty operand: shape {0} everywhere
    {
        const sm::SMArray<T> none = from_host(std::vector<T>{}, Shape{0}), none2 = from_host(std::vector<T>{}, Shape{4, 0});
        for (const sm::SMArray<T> *e : {&none, &none2}) {
            const sm::UniqueAll<T> all = sm::unique_all(*e);
            CHECK(all.values.shape() == Shape{0} && all.index.shape() == Shape{0} && all.inverse.shape() == Shape{0} && all.counts.shape() == Shape{0});
            CHECK(sm::unique_values(*e).shape() == Shape{0} && sm::unique_consecutive(*e).shape() == Shape{0} && sm::run_lengths(*e).second.shape() == Shape{0});
        }
    }
}

int main() {
    test_type<float>();
    test_type<double>();
    test_type<int>();
    test_type<I64>();

    // the counters: a unique is ONE sort call and two run calls (the count, then the runs); unique_consecutive has no sort
    {
        const sm::SMArray<int> x = from_host(std::vector<int>{3, 1, 3, 3, 2, 1}, Shape{6});
        auto before = sm::fusion_stats();
        const sm::UniqueAll<int> all = sm::unique_all(x);
        auto after = sm::fusion_stats();
        CHECK(after.sorts == before.sorts + 1 && after.uniques == before.uniques + 2);
        CHECK(same_bytes(all.values, std::vector<int>{1, 2, 3}) && same_bytes(all.index, std::vector<I64>{1, 4, 0}) &&
              same_bytes(all.inverse, std::vector<I64>{2, 0, 2, 2, 1, 0}) && same_bytes(all.counts, std::vector<I64>{2, 1, 3}));
        before = after;
        CHECK(same_bytes(sm::run_lengths(x).second, std::vector<I64>{1, 1, 2, 1, 1}));
        after = sm::fusion_stats();
        CHECK(after.sorts == before.sorts && after.uniques == before.uniques + 2);
        before = after;
        CHECK(sm::unique_values(from_host(std::vector<int>{}, Shape{0})).totalSize == 0);
        after = sm::fusion_stats();
        CHECK(after.sorts == before.sorts && after.uniques == before.uniques);  // nothing to sort, nothing to count
    }
    // unique_counts against bincount on small ids, and the group-by against a loop
    {
        const std::size_t n = 50001, groups = 37;
        std::vector<I64> ids(n);
        std::vector<float> v(n);
        std::vector<double> want(groups, 0.0);
        for (std::size_t i = 0; i < n; ++i) ids[i] = static_cast<I64>(next() % groups), v[i] = static_cast<float>(next() % 17), want[static_cast<std::size_t>(ids[i])] += v[i];
        const sm::SMArray<I64> k = from_host(ids, Shape{n});
        const sm::SMArray<float> values = from_host(v, Shape{n});
        auto [present, counts] = sm::unique_counts(k);
        CHECK(present.totalSize == groups && same_bytes(counts, to_host(k.bincount(static_cast<I64>(groups)))));
        auto [key, inverse] = sm::unique_inverse(k);
        auto sums = sm::zeros<float>(key.totalSize);
        sums.index_add(inverse, values, 0);
        const std::vector<float> got = to_host(sums);
        bool equal = got.size() == groups;
        for (std::size_t g = 0; equal && g < groups; ++g) equal = got[g] == static_cast<float>(want[g]);
        CHECK(equal);
    }
    std::printf("test_unique: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
