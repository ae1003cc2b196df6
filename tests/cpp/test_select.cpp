// test_select.cpp -- choosing by condition through the drop-in surface: every comparison operator form (array / array, array / scalar,
// scalar / array), sm::where, assign_where, mask, count_nonzero, flatnonzero, nonzero, select and compress for the four element types,
// views and pending operator chains as operands, empty results, what throws std::invalid_argument, flatnonzero feeding take_flat and
// put_flat, and the `selects` counter.
// Expected values: the same comparisons done one by one on the host (C++'s operators on float are IEEE's, which are numpy's).
#include <sm.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <stdexcept>
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

static std::uint64_t g_state = 0x2468ace0ull;
static std::uint64_t next() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

using Shape = std::vector<std::size_t>;
using I64 = std::int64_t;

// ---- what must (not) compile
static_assert(!std::is_convertible_v<sm::Cond<float>, bool>, "a condition is not a truth value");
static_assert(!std::is_constructible_v<bool, sm::Cond<float>>, "... not even explicitly");
static_assert(std::is_same_v<decltype(std::declval<sm::SMArray<float> &>() > 1.0f), sm::Cond<float>>, "array > scalar is a condition, not an array");
static_assert(!std::is_same_v<decltype(std::declval<sm::SMArray<float> &>() > 1.0f), sm::SMArray<float>>);
static_assert(std::is_same_v<decltype(1.0f <= std::declval<sm::SMArray<float> &>()), sm::Cond<float>>);
static_assert(std::is_same_v<decltype(std::declval<sm::SMArray<double> &>() == std::declval<sm::SMArray<double> &>()), sm::Cond<double>>);
static_assert(std::is_same_v<decltype(std::declval<sm::SMArray<I64> &>() != 3), sm::Cond<I64>>);
// the buffer's comparison with nullptr keeps its meaning
static_assert(std::is_same_v<decltype(std::declval<sm::SMArray<float> &>().data == nullptr), bool>);
static_assert(std::is_same_v<decltype(std::declval<sm::SMArray<float> &>().data != nullptr), bool>);

template <typename T>
static sm::SMArray<T> from_host(const std::vector<T> &h, Shape shape) {
    T *buf = new T[h.size() ? h.size() : 1];
    std::copy(h.begin(), h.end(), buf);
    return sm::SMArray<T>(buf, std::move(shape));
}

template <typename T>
static int differences(const sm::SMArray<T> &got, const std::vector<T> &want) {
    if (got.totalSize != want.size()) return -1;
    if (want.empty()) return 0;
    std::vector<T> dense(want.size());
    got.copy_dense_out(dense.data());
    return std::memcmp(dense.data(), want.data(), want.size() * sizeof(T)) != 0;
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

// what no element is greater than
template <typename T>
static T top() {
    if constexpr (std::is_floating_point_v<T>) return std::numeric_limits<T>::infinity();
    else return std::numeric_limits<T>::max();
}

// small whole numbers, and for the floats NaN, both zeros and the infinities
template <typename T>
static std::vector<T> values(std::size_t n) {
    std::vector<T> v(n);
    for (std::size_t i = 0; i < n; ++i) v[i] = static_cast<T>(static_cast<int>(next() % 7) - 3);
    if constexpr (std::is_floating_point_v<T>) {
        const T special[] = {std::numeric_limits<T>::quiet_NaN(), T(-0.0), T(0.0), std::numeric_limits<T>::infinity(), -std::numeric_limits<T>::infinity()};
        for (std::size_t k = 0; k < 5 && n; ++k) v[next() % n] = special[k];
    } else {
        if (n > 2) v[next() % n] = std::numeric_limits<T>::min(), v[next() % n] = std::numeric_limits<T>::max();
    }
    return v;
}

enum { EQ, NE, LT, LE, GT, GE };
template <typename T>
static bool host_cmp(int op, T x, T y) {
    switch (op) {
        case EQ: return x == y;
        case NE: return x != y;
        case LT: return x < y;
        case LE: return x <= y;
        case GT: return x > y;
    }
    return x >= y;
}
template <typename T>
static sm::Cond<T> cond_aa(int op, const sm::SMArray<T> &x, const sm::SMArray<T> &y) {
    switch (op) {
        case EQ: return x == y;
        case NE: return x != y;
        case LT: return x < y;
        case LE: return x <= y;
        case GT: return x > y;
    }
    return x >= y;
}
template <typename T>
static sm::Cond<T> cond_as(int op, const sm::SMArray<T> &x, T s) {
    switch (op) {
        case EQ: return x == s;
        case NE: return x != s;
        case LT: return x < s;
        case LE: return x <= s;
        case GT: return x > s;
    }
    return x >= s;
}
template <typename T>
static sm::Cond<T> cond_sa(int op, T s, const sm::SMArray<T> &x) {
    switch (op) {
        case EQ: return s == x;
        case NE: return s != x;
        case LT: return s < x;
        case LE: return s <= x;
        case GT: return s > x;
    }
    return s >= x;
}

// Everything a condition can be asked, against the host mask (row-major over `shape`).
template <typename T>
static void check_condition(const sm::Cond<T> &c, const std::vector<bool> &mask, const Shape &shape) {
    const std::size_t n = mask.size();
    std::vector<I64> flat;
    std::vector<std::vector<I64>> coords(shape.size());
    std::vector<T> ones(n);
    for (std::size_t i = 0; i < n; ++i) {
        ones[i] = mask[i] ? T(1) : T(0);
        if (!mask[i]) continue;
        flat.push_back(static_cast<I64>(i));
        std::size_t rest = i;
        for (std::size_t d = shape.size(); d-- > 0;) coords[d].push_back(static_cast<I64>(rest % shape[d])), rest /= shape[d];
    }
    CHECK(sm::count_nonzero(c) == static_cast<I64>(flat.size()));
    const auto got_flat = sm::flatnonzero(c);
    CHECK(got_flat.shape() == Shape{flat.size()} && differences(got_flat, flat) == 0);
    const auto got = sm::nonzero(c);
    CHECK(got.size() == shape.size());
    for (std::size_t d = 0; d < got.size() && d < shape.size(); ++d) CHECK(got[d].shape() == Shape{flat.size()} && differences(got[d], coords[d]) == 0);
    const auto m = sm::mask(c);
    CHECK(m.shape() == shape && differences(m, ones) == 0);
}

template <typename T>
static void test_type() {
    const Shape shape{37, 29};
    const std::size_t n = 37 * 29;
    const std::vector<T> hx = values<T>(n), hy = values<T>(n), ha = values<T>(n), hb = values<T>(n);
    const auto x = from_host(hx, shape), y = from_host(hy, shape), a = from_host(ha, shape), b = from_host(hb, shape);
    const T s = T(1);
    for (int op = EQ; op <= GE; ++op) {
        std::vector<bool> aa(n), as(n), sa(n);
        std::vector<T> w_aa(n), w_as(n), w_sa(n), sel;
        for (std::size_t i = 0; i < n; ++i) {
            aa[i] = host_cmp(op, hx[i], hy[i]), as[i] = host_cmp(op, hx[i], s), sa[i] = host_cmp(op, s, hx[i]);
            w_aa[i] = aa[i] ? ha[i] : hb[i], w_as[i] = as[i] ? ha[i] : T(-7), w_sa[i] = sa[i] ? T(5) : hb[i];
            if (as[i]) sel.push_back(ha[i]);
        }
        check_condition(cond_aa(op, x, y), aa, shape);
        check_condition(cond_as(op, x, s), as, shape);
        check_condition(cond_sa(op, s, x), sa, shape);
        CHECK(differences(sm::where(cond_aa(op, x, y), a, b), w_aa) == 0);
        CHECK(differences(sm::where(cond_as(op, x, s), a, T(-7)), w_as) == 0);
        CHECK(differences(sm::where(cond_sa(op, s, x), T(5), b), w_sa) == 0);
        CHECK(differences(a.select(cond_as(op, x, s)), sel) == 0);          // member and free form
        CHECK(differences(sm::select(a, cond_as(op, x, s)), sel) == 0);
    }
    // an array where a condition is expected stands for "nonzero": NaN counts, -0.0 does not
    std::vector<bool> nz(n);
    std::vector<T> w(n), sel;
    for (std::size_t i = 0; i < n; ++i) {
        nz[i] = hx[i] != T(0), w[i] = nz[i] ? T(2) : T(3);
        if (nz[i]) sel.push_back(hb[i]);
    }
    check_condition(sm::Cond<T>(x), nz, shape);
    CHECK(sm::count_nonzero(x) == static_cast<I64>(sel.size()));
    CHECK(differences(sm::where(x, T(2), T(3)), w) == 0);
    CHECK(differences(b.select(x), sel) == 0 && differences(sm::select(b, x), sel) == 0);
    CHECK(sm::flatnonzero(x).totalSize == sel.size() && sm::nonzero(x).size() == 2 && sm::mask(x).shape() == shape);

    // broadcasting: a row and a column against the condition; a condition between a matrix and a row
    const std::vector<T> hrow = values<T>(29), hcol = values<T>(37);
    const auto row = from_host(hrow, {29}), col = from_host(hcol, {37, 1});
    std::vector<T> w_rc(n), w_xr(n);
    for (std::size_t i = 0; i < n; ++i) {
        w_rc[i] = hx[i] > s ? hrow[i % 29] : hcol[i / 29];
        w_xr[i] = hx[i] <= hrow[i % 29] ? hx[i] : hrow[i % 29];
    }
    CHECK(differences(sm::where(x > s, row, col), w_rc) == 0);
    const auto min_xr = sm::where(x <= row, x, row);
    CHECK(min_xr.shape() == shape && differences(min_xr, w_xr) == 0);

    // a view (the transpose) and a pending chain as the condition's operand and as the source
    const auto xt = x.transpose();
    if constexpr (std::is_floating_point_v<T>) {   // (the integer extremes would overflow in the host's sums and products)
        std::vector<bool> mt(n);
        std::vector<T> sel_t, sel_chain;
        std::vector<I64> flat_chain;
        for (std::size_t i = 0; i < n; ++i) {
            const std::size_t r = i / 37, c = i % 37;   // element (r, c) of the (29, 37) transpose
            mt[i] = hx[c * 29 + r] < s;
            if (mt[i]) sel_t.push_back(ha[c * 29 + r]);
            if (hx[i] + hy[i] > s) flat_chain.push_back(static_cast<I64>(i)), sel_chain.push_back(ha[i] * T(2));
        }
        check_condition(xt < s, mt, {29, 37});
        CHECK(differences(a.transpose().select(xt < s), sel_t) == 0);
        CHECK(differences(sm::flatnonzero(x + y > s), flat_chain) == 0);
        CHECK(differences((a * T(2)).select(x + y > s), sel_chain) == 0);
        CHECK(differences(sm::select(a * T(2), x + y > s), sel_chain) == 0);
        auto kept = x + y > s;   // a named condition keeps its operands alive
        CHECK(sm::count_nonzero(kept) == static_cast<I64>(flat_chain.size()));
    } else {
        std::vector<bool> mt(n);
        std::vector<T> sel_t;
        for (std::size_t i = 0; i < n; ++i) {
            const std::size_t r = i / 37, c = i % 37;
            mt[i] = hx[c * 29 + r] < s;
            if (mt[i]) sel_t.push_back(ha[c * 29 + r]);
        }
        check_condition(xt < s, mt, {29, 37});
        CHECK(differences(a.transpose().select(xt < s), sel_t) == 0);
    }

    // a source of another element type and width
    using Other = std::conditional_t<sizeof(T) == 4, double, float>;
    std::vector<Other> ho(n), sel_o;
    for (std::size_t i = 0; i < n; ++i) {
        ho[i] = static_cast<Other>(i) * Other(0.5);
        if (host_cmp(GE, hx[i], s)) sel_o.push_back(ho[i]);
    }
    CHECK(differences(from_host(ho, shape).select(x >= s), sel_o) == 0);

    // assign_where: on a dense array, with a scalar and with an array; on a slice (staged)
    {
        auto t = from_host(ha, shape);
        std::vector<T> want(ha);
        for (std::size_t i = 0; i < n; ++i)
            if (hx[i] < s) want[i] = T(9);
        CHECK(&t.assign_where(x < s, T(9)) == &t && differences(t, want) == 0);
        for (std::size_t i = 0; i < n; ++i)
            if (want[i] == T(9)) want[i] = hb[i];
        t.assign_where(t == T(9), b);   // the condition reads the target itself: np.putmask(t, t == 9, b)
        CHECK(differences(t, want) == 0);
        t.assign_where(y != y, row);    // a broadcast value
        for (std::size_t i = 0; i < n; ++i)
            if (hy[i] != hy[i]) want[i] = hrow[i % 29];
        CHECK(differences(t, want) == 0);
    }
    {
        auto t = from_host(ha, shape);
        std::vector<T> want(ha);
        for (std::size_t r = 5; r < 30; ++r)
            for (std::size_t c = 3; c < 20; ++c)
                if (ha[r * 29 + c] > T(0)) want[r * 29 + c] = T(0);
        auto slice = t(SLICE(5, 30), SLICE(3, 20));
        slice.assign_where(t(SLICE(5, 30), SLICE(3, 20)) > T(0), T(0));
        CHECK(differences(t, want) == 0);
    }

    // flatnonzero feeds take_flat and put_flat
    {
        const auto at = sm::flatnonzero(x > s);
        std::vector<T> taken, put(hb);
        for (std::size_t i = 0; i < n; ++i)
            if (hx[i] > s) taken.push_back(ha[i]), put[i] = T(4);
        CHECK(differences(a.take_flat(at), taken) == 0);
        auto t = from_host(hb, shape);
        t.put_flat(at, T(4), sm::index_mode::checked, true);
        CHECK(differences(t, put) == 0);
    }

    // empty results: shape {0}; and conditions over no elements
    {
        const auto none = sm::flatnonzero(x > top<T>());
        CHECK(none.shape() == Shape{0} && none.totalSize == 0);
        CHECK(a.select(x > top<T>()).shape() == Shape{0});
        const auto nowhere = sm::nonzero(x > top<T>());
        CHECK(nowhere.size() == 2 && nowhere[0].shape() == Shape{0} && nowhere[1].shape() == Shape{0});
        CHECK(sm::count_nonzero(x > top<T>()) == 0);
        const auto e = from_host(std::vector<T>{}, {0, 5});
        CHECK(sm::count_nonzero(e > s) == 0 && sm::flatnonzero(e).shape() == Shape{0} && sm::nonzero(e == e).size() == 2);
        CHECK(sm::where(e > s, e, s).shape() == (Shape{0, 5}) && e.select(e > s).shape() == Shape{0});
    }

    // compress along both axes of a table
    {
        std::vector<T> hl(37), hk(29);
        for (auto &v : hl) v = static_cast<T>(next() % 3);
        for (auto &v : hk) v = static_cast<T>(next() % 2);
        const auto labels = from_host(hl, {37}), keep = from_host(hk, {29});
        std::vector<T> rows, cols;
        for (std::size_t r = 0; r < 37; ++r)
            if (hl[r] == T(2)) rows.insert(rows.end(), ha.begin() + static_cast<long>(r * 29), ha.begin() + static_cast<long>(r * 29 + 29));
        for (std::size_t r = 0; r < 37; ++r)
            for (std::size_t c = 0; c < 29; ++c)
                if (hk[c] != T(0)) cols.push_back(ha[r * 29 + c]);
        const auto by_row = sm::compress(labels == T(2), a, 0);
        CHECK(by_row.shape() == (Shape{rows.size() / 29, 29}) && differences(by_row, rows) == 0);
        const auto by_col = sm::compress(keep, a, 1);
        CHECK(by_col.shape() == (Shape{37, cols.size() / 37}) && differences(by_col, cols) == 0);
        CHECK(differences(sm::compress(keep, a, -1), cols) == 0);
        CHECK(throws_invalid_argument([&] { sm::compress(keep, a, 0); }));       // 29 against an axis of 37
        CHECK(throws_invalid_argument([&] { sm::compress(x > s, a, 0); }));      // not 1-D
        CHECK(throws_invalid_argument([&] { sm::compress(keep, a, 2); }));
    }

    // what throws
    const auto odd = from_host(values<T>(30), {30});
    CHECK(throws_invalid_argument([&] { sm::where(x > odd, a, b); }));           // the condition's own operands
    CHECK(throws_invalid_argument([&] { sm::where(x > s, odd, b); }));
    CHECK(throws_invalid_argument([&] { sm::where(x > s, a, odd); }));
    CHECK(throws_invalid_argument([&] { sm::count_nonzero(x == odd); }));
    CHECK(throws_invalid_argument([&] { a.select(odd > s); }));                  // equal shapes, not broadcasting ones
    CHECK(throws_invalid_argument([&] { a.select(row > s); }));
    CHECK(throws_invalid_argument([&] { sm::select(odd, x > s); }));
    {
        auto t = from_host(ha, shape);
        CHECK(throws_invalid_argument([&] { t.assign_where(odd > s, s); }));
        CHECK(throws_invalid_argument([&] { t.assign_where(x > s, odd); }));
        CHECK(differences(t, ha) == 0);
    }
}

int main() {
    const auto before = sm::fusion_stats().selects;
    test_type<float>();
    test_type<double>();
    test_type<int>();
    test_type<std::int64_t>();
    CHECK(sm::fusion_stats().selects > before);

    // where(x > 0, x, 0) is one library call; count_nonzero one; flatnonzero two (count, select)
    const auto x = from_host(std::vector<float>{1.f, -2.f, 0.f, 3.f}, {4});
    auto calls = sm::fusion_stats().selects;
    const auto relu = sm::where(x > 0.0f, x, 0.0f);
    CHECK(sm::fusion_stats().selects == calls + 1 && differences(relu, std::vector<float>{1.f, 0.f, 0.f, 3.f}) == 0);
    calls = sm::fusion_stats().selects;
    CHECK(sm::count_nonzero(x) == 3 && sm::fusion_stats().selects == calls + 1);
    calls = sm::fusion_stats().selects;
    CHECK(differences(sm::flatnonzero(x < 1), std::vector<I64>{1, 2}) == 0 && sm::fusion_stats().selects == calls + 2);
    // the mask recipe: and, or, not
    const auto m1 = sm::mask(x > 0.0f), m2 = sm::mask(x < 2.0f);
    CHECK(differences(m1 * m2, std::vector<float>{1.f, 0.f, 0.f, 0.f}) == 0);
    CHECK(differences(m1 + m2 - m1 * m2, std::vector<float>{1.f, 1.f, 1.f, 1.f}) == 0);
    CHECK(differences(-m1 + 1.0f, std::vector<float>{0.f, 1.f, 1.f, 0.f}) == 0);
    CHECK(x.data != nullptr);

    std::printf("test_select: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
