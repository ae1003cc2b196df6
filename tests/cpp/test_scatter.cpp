// test_scatter.cpp -- put_along_axis / put / put_flat / scatter_add / index_add through the drop-in surface: the member and the
// sm:: forms for the four element types, negative and absent axis, the scalar overloads, what throws std::invalid_argument and
// std::out_of_range (the valid entries applied by then), a sliced and a transposed target, a pending operator chain as the values,
// the result feeding a chain, the `scatters` counter and the README's snippets.
// Expected values: the same entries placed one by one, in ascending position along the index array, on the host.
#include <sm.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
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

static std::uint64_t g_state = 0x2468ace1ull;
static std::uint64_t next() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

using Shape = std::vector<std::size_t>;

static std::size_t count_of(const Shape &shape) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    return n;
}

// Small whole numbers, so that sums are exact in every element type and the order of a PUT shows.
template <typename T>
static sm::SMArray<T> host_array(Shape shape, std::vector<T> &mirror, int span = 1000) {
    const std::size_t n = count_of(shape);
    T *buf = new T[n ? n : 1];
    mirror.resize(n);
    for (std::size_t i = 0; i < n; ++i) mirror[i] = buf[i] = static_cast<T>(static_cast<int>(next() % static_cast<std::uint64_t>(span)) - span / 2);
    return sm::SMArray<T>(buf, std::move(shape));
}

// Positions in [lo, hi).
static sm::SMArray<std::int64_t> host_index(Shape shape, std::vector<std::int64_t> &mirror, std::int64_t lo, std::int64_t hi) {
    const std::size_t n = count_of(shape);
    std::int64_t *buf = new std::int64_t[n ? n : 1];
    mirror.resize(n);
    for (std::size_t i = 0; i < n; ++i) mirror[i] = buf[i] = lo + static_cast<std::int64_t>(next() % static_cast<std::uint64_t>(hi - lo));
    return sm::SMArray<std::int64_t>(buf, std::move(shape));
}

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

// The reference on a (rows, cols) target: entry (i, j) of the walk goes to position pos along `axis`; bad entries are dropped.
template <typename T>
static void place(std::vector<T> &t, std::size_t cols, int axis, bool add, std::size_t i, std::size_t j, std::int64_t index, T v) {
    const std::int64_t R = static_cast<std::int64_t>(axis == 0 ? t.size() / cols : cols);
    if (index < -R || index >= R) return;
    const std::size_t p = static_cast<std::size_t>(index < 0 ? index + R : index);
    T &dst = axis == 0 ? t[p * cols + j] : t[i * cols + p];
    dst = add ? static_cast<T>(dst + v) : v;
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

template <typename T>
static void test_forms() {
    const std::size_t R = 37, Cn = 130;
    std::vector<T> h, hv, want;
    std::vector<std::int64_t> hi;
    // put_along_axis / scatter_add along each axis, negative axes, member and sm:: forms, duplicates among the entries
    for (int axis : {0, 1, -1, -2}) {
        const int ax = axis < 0 ? axis + 2 : axis;
        const std::size_t J = ax == 0 ? 90 : 300, rows = ax == 0 ? J : R, cols = ax == 0 ? Cn : J;
        const std::int64_t extent = static_cast<std::int64_t>(ax == 0 ? R : Cn);
        for (bool add : {false, true}) {
            auto a = host_array<T>({R, Cn}, h);
            auto b = from_host(h, {R, Cn});
            auto idx = host_index({rows, cols}, hi, -extent, extent);
            auto v = host_array<T>({rows, cols}, hv);
            want = h;
            for (std::size_t i = 0; i < rows; ++i)
                for (std::size_t j = 0; j < cols; ++j) place(want, Cn, ax, add, i, j, hi[i * cols + j], hv[i * cols + j]);
            const auto before = sm::fusion_stats();
            auto &r = add ? a.scatter_add(idx, v, axis) : a.put_along_axis(idx, v, axis);
            CHECK(sm::fusion_stats().scatters - before.scatters == 1);
            CHECK(&r == &a);
            CHECK(differences(a, want) == 0);
            auto &s = add ? sm::scatter_add(b, idx, v, axis) : sm::put_along_axis(b, idx, v, axis);
            CHECK(&s == &b && differences(b, want) == 0);
        }
    }
    // the scalar overloads, and idx / values broadcast: one line of positions for every row, one value per row
    {
        auto a = host_array<T>({R, Cn}, h);
        auto line = host_index({1, 60}, hi, 0, static_cast<std::int64_t>(Cn));
        want = h;
        for (std::size_t i = 0; i < R; ++i)
            for (std::size_t j = 0; j < 60; ++j) place(want, Cn, 1, false, i, j, hi[j], static_cast<T>(7));
        a.put_along_axis(line, static_cast<T>(7), 1);
        CHECK(differences(a, want) == 0);
        for (std::size_t i = 0; i < R; ++i)
            for (std::size_t j = 0; j < 60; ++j) place(want, Cn, 1, true, i, j, hi[j], static_cast<T>(3));
        sm::scatter_add(a, line, static_cast<T>(3), -1);
        CHECK(differences(a, want) == 0);
        auto column = host_array<T>({R, 1}, hv);
        for (std::size_t i = 0; i < R; ++i)
            for (std::size_t j = 0; j < 60; ++j) place(want, Cn, 1, true, i, j, hi[j], hv[i]);
        a.scatter_add(line, column, 1);
        CHECK(differences(a, want) == 0);
    }
    // put / index_add: a 1-D index array along either axis; values full, broadcast and scalar
    for (int axis : {0, 1, -1}) {
        const int ax = axis < 0 ? axis + 2 : axis;
        const std::int64_t extent = static_cast<std::int64_t>(ax == 0 ? R : Cn);
        const std::size_t n = 77, rows = ax == 0 ? n : R, cols = ax == 0 ? Cn : n;
        for (bool add : {false, true}) {
            auto a = host_array<T>({R, Cn}, h);
            auto ids = host_index({n}, hi, -extent, extent);
            auto v = host_array<T>({rows, cols}, hv);
            want = h;
            for (std::size_t i = 0; i < rows; ++i)
                for (std::size_t j = 0; j < cols; ++j) place(want, Cn, ax, add, i, j, hi[ax == 0 ? i : j], hv[i * cols + j]);
            if (add) sm::index_add(a, ids, v, axis);
            else a.put(ids, v, axis);
            CHECK(differences(a, want) == 0);
            for (std::size_t i = 0; i < rows; ++i)
                for (std::size_t j = 0; j < cols; ++j) place(want, Cn, ax, add, i, j, hi[ax == 0 ? i : j], static_cast<T>(5));
            if (add) a.index_add(ids, static_cast<T>(5), axis);
            else sm::put(a, ids, static_cast<T>(5), axis);
            CHECK(differences(a, want) == 0);
        }
    }
    // no axis: the target and idx flattened row-major; put_flat
    {
        auto a = host_array<T>({R, Cn}, h);
        const std::int64_t total = static_cast<std::int64_t>(R * Cn);
        auto idx = host_index({5, 11}, hi, -total, total);
        auto v = host_array<T>({5, 11}, hv);
        want = h;
        for (std::size_t k = 0; k < 55; ++k) place(want, R * Cn, 1, false, 0, k, hi[k], hv[k]);
        sm::put_along_axis(a, idx, v);
        CHECK(differences(a, want) == 0);
        auto ids = host_index({55}, hi, 0, total);
        for (std::size_t k = 0; k < 55; ++k) place(want, R * Cn, 1, false, 0, k, hi[k], static_cast<T>(9));
        a.put_flat(ids, static_cast<T>(9));
        CHECK(differences(a, want) == 0);
        auto w = host_array<T>({55}, hv);
        for (std::size_t k = 0; k < 55; ++k) place(want, R * Cn, 1, false, 0, k, hi[k], hv[k]);
        sm::put_flat(a, ids, w);
        CHECK(differences(a, want) == 0);
    }
    // what throws std::invalid_argument
    {
        auto a = host_array<T>({R, Cn}, h);
        auto idx = host_index({R, 5}, hi, 0, 5);
        auto v = host_array<T>({R, 5}, hv);
        auto ids = host_index({5}, hi, 0, 5);
        CHECK(throws_invalid_argument([&] { a.put_along_axis(idx, v, 2); }));
        CHECK(throws_invalid_argument([&] { a.scatter_add(idx, v, -3); }));
        CHECK(throws_invalid_argument([&] { a.put_along_axis(ids, v, 0); }));                               // rank
        CHECK(throws_invalid_argument([&] { a.put_along_axis(host_index({R - 1, 5}, hi, 0, 5), v, 1); }));  // 37 against 36
        CHECK(throws_invalid_argument([&] { a.put_along_axis(idx, host_array<T>({R, 4}, hv), 1); }));       // values against idx
        CHECK(throws_invalid_argument([&] { a.put(idx, v, 1); }));                                          // ids must be 1-D
        CHECK(throws_invalid_argument([&] { a.index_add(ids, v, 5); }));
        CHECK(throws_invalid_argument([&] { a.put_flat(idx, v); }));
        CHECK(differences(a, h) == 0);
    }
}

static void test_index_modes() {
    std::vector<float> h, hv, want;
    std::vector<std::int64_t> hi;
    const std::int64_t R = 9;
    for (bool unique : {false, true}) {
        const std::vector<std::int64_t> raw = unique ? std::vector<std::int64_t>{0, 12, -8, 4, -20, 8} : std::vector<std::int64_t>{0, 12, -9, 4, -20, 4};
        auto ids = from_host(raw, {raw.size()});
        // checked: the bad entries are dropped, the valid ones applied, then std::out_of_range
        auto a = host_array<float>({9, 8}, h);
        auto v = host_array<float>({raw.size(), 8}, hv);
        want = h;
        for (std::size_t i = 0; i < raw.size(); ++i)
            for (std::size_t j = 0; j < 8; ++j) place(want, 8, 0, true, i, j, raw[i], hv[i * 8 + j]);
        CHECK(throws_out_of_range([&] { a.index_add(ids, v, 0, sm::index_mode::checked, unique); }));
        CHECK(differences(a, want) == 0);
        if (unique) continue;
        // clip and wrap never throw
        for (auto mode : {sm::index_mode::clip, sm::index_mode::wrap}) {
            auto b = from_host(h, {9, 8});
            want = h;
            for (std::size_t i = 0; i < raw.size(); ++i) {
                const std::int64_t p = mode == sm::index_mode::clip ? std::min<std::int64_t>(std::max<std::int64_t>(raw[i], 0), R - 1) : ((raw[i] % R) + R) % R;
                for (std::size_t j = 0; j < 8; ++j) place(want, 8, 0, false, i, j, p, hv[i * 8 + j]);
            }
            b.put(ids, v, 0, mode);
            CHECK(differences(b, want) == 0);
        }
    }
    // an axis of 0 elements with entries to place
    auto hollow = sm::zeros<float>(4, 0);
    auto two = sm::zeros<std::int64_t>(4, 2);
    CHECK(throws_out_of_range([&] { hollow.put_along_axis(two, 1.0f, 1); }));
    // no entries: nothing happens, whatever the mode
    auto a = host_array<float>({4, 5}, h);
    auto none = sm::zeros<std::int64_t>(4, 0);
    a.put_along_axis(none, 1.0f, 1);
    a.index_add(sm::zeros<std::int64_t>(0), 2.0f, 0);
    CHECK(differences(a, h) == 0);
}

static void test_views_chains_and_counter() {
    std::vector<float> h, hv, want;
    std::vector<std::int64_t> hi;
    const std::size_t R = 20, Cn = 48;
    // a sliced target: rows 4..11 and columns 8..31 of a -- staged, and the rest of a untouched
    {
        auto a = host_array<float>({R, Cn}, h);
        auto view = a(SLICE(4, 12), SLICE(8, 32));  // {8, 24}
        auto idx = host_index({8, 40}, hi, -24, 24);
        auto v = host_array<float>({8, 40}, hv);
        want = h;
        for (std::size_t i = 0; i < 8; ++i)
            for (std::size_t j = 0; j < 40; ++j) {
                const std::int64_t p = hi[i * 40 + j] < 0 ? hi[i * 40 + j] + 24 : hi[i * 40 + j];
                want[(i + 4) * Cn + 8 + static_cast<std::size_t>(p)] += hv[i * 40 + j];
            }
        const auto before = sm::fusion_stats();
        view.scatter_add(idx, v, 1);
        CHECK(sm::fusion_stats().scatters - before.scatters == 1);
        CHECK(differences(a, want) == 0);
        // a dense slice (whole rows) is updated in place
        auto rows = a(SLICE(2, 5), SLICE_ALL);
        auto ids = from_host(std::vector<std::int64_t>{2, 0, 2}, {3});
        auto w = host_array<float>({3, Cn}, hv);
        for (std::size_t i = 0; i < 3; ++i)
            for (std::size_t j = 0; j < Cn; ++j) want[(2 + (i == 1 ? 0 : 2)) * Cn + j] = hv[i * Cn + j];
        rows.put(ids, w, 0);
        CHECK(differences(a, want) == 0);
    }
    // a transposed target: index_add along axis 0 of A.T adds into columns of A
    {
        auto a = host_array<float>({R, Cn}, h);
        auto tr = a.transpose();  // {Cn, R}
        auto ids = host_index({33}, hi, 0, static_cast<std::int64_t>(Cn));
        auto v = host_array<float>({33, R}, hv);
        want = h;
        for (std::size_t i = 0; i < 33; ++i)
            for (std::size_t j = 0; j < R; ++j) want[j * Cn + static_cast<std::size_t>(hi[i])] += hv[i * R + j];
        tr.index_add(ids, v, 0);
        CHECK(differences(a, want) == 0);
    }
    // a pending chain as the values, a transposed view as the index array, and the result feeding a chain
    {
        auto a = host_array<float>({R, Cn}, h);
        auto x = host_array<float>({R, 30}, hv);
        std::vector<float> hy;
        auto y = host_array<float>({R, 30}, hy);
        auto base = host_index({30, R}, hi, 0, static_cast<std::int64_t>(Cn));
        want = h;
        for (std::size_t i = 0; i < R; ++i)
            for (std::size_t j = 0; j < 30; ++j) place(want, Cn, 1, false, i, j, hi[j * R + i], (hv[i * 30 + j] + hy[i * 30 + j]) * 2.0f);
        a.put_along_axis(base.transpose(), (x + y) * 2.0f, 1);
        CHECK(differences(a, want) == 0);
        auto next_chain = a * 0.5f + 1.0f;
        for (auto &e : want) e = e * 0.5f + 1.0f;
        CHECK(differences(next_chain, want) == 0);
        // values that are a view of the target itself are copied first
        auto c = host_array<float>({6, 8}, h);
        auto ids = from_host(std::vector<std::int64_t>{5, 4, 3}, {3});
        want = h;
        for (std::size_t i = 0; i < 3; ++i)
            for (std::size_t j = 0; j < 8; ++j) want[(5 - i) * 8 + j] = h[i * 8 + j];
        c.put(ids, c(SLICE(0, 3), SLICE_ALL), 0);
        CHECK(differences(c, want) == 0);
    }
    // the counter: one call each
    {
        auto a = host_array<float>({R, Cn}, h);
        auto idx = host_index({R, 3}, hi, 0, static_cast<std::int64_t>(Cn));
        auto ids = host_index({3}, hi, 0, static_cast<std::int64_t>(R));
        const auto before = sm::fusion_stats();
        a.put_along_axis(idx, 1.0f, 1);
        a.scatter_add(idx, 1.0f, 1);
        a.put(ids, 1.0f, 0);
        a.index_add(ids, 1.0f, 0);
        a.put_flat(ids, 1.0f);
        CHECK(sm::fusion_stats().scatters - before.scatters == 5);
    }
}

static void test_nan_payload_and_signed_zero() {
    // PUT moves bits: which zero, which NaN
    const std::uint32_t bits[4] = {0x7fc01234u, 0xffc00001u, 0x80000000u, 0x00000000u};
    std::vector<float> v(4), zero(8, 1.0f);
    std::memcpy(v.data(), bits, sizeof bits);
    auto a = from_host(zero, {8});
    auto ids = from_host(std::vector<std::int64_t>{7, 0, 3, 3}, {4});
    a.put(ids, from_host(v, {4}), 0);
    std::uint32_t got[8];
    std::memcpy(got, a.cdata(), sizeof got);
    CHECK(got[7] == bits[0] && got[0] == bits[1] && got[3] == bits[3] && got[1] == 0x3f800000u);  // the later of the two entries on position 3 wins
}

static void test_readme_snippets() {
    // one-hot
    auto labels = sm::zeros<std::int64_t>(512, 1);  // ... the class of each sample ...
    for (std::size_t i = 0; i < 512; ++i) labels.data[i] = static_cast<std::int64_t>((i * 7) % 1000);
    auto onehot = sm::zeros<float>(512, 1000);
    sm::put_along_axis(onehot, labels, 1.0f, -1);  // one entry per line: unique by construction, one launch
    int bad = 0;
    for (std::size_t i = 0; i < 512; ++i)
        for (std::size_t j = 0; j < 1000; ++j) bad += onehot.cdata()[i * 1000 + j] != (j == (i * 7) % 1000 ? 1.0f : 0.0f);
    CHECK(bad == 0);
    // bincount via index_add
    auto samples = sm::zeros<std::int64_t>(70001);  // ... values in [0, 256) ...
    std::vector<std::int64_t> expect(256, 0);
    for (std::size_t i = 0; i < 70001; ++i) {
        const std::int64_t bin = static_cast<std::int64_t>(next() % 256);
        samples.data[i] = bin, ++expect[static_cast<std::size_t>(bin)];
    }
    auto counts = sm::zeros<std::int64_t>(256);
    sm::index_add(counts, samples, std::int64_t{1}, 0);
    CHECK(differences(counts, expect) == 0);
    // un-sort via argsort
    std::vector<float> hx;
    auto x = host_array<float>({512, 1000}, hx, 1 << 20);
    auto order = sm::argsort(x, -1);
    auto sorted = sm::take_along_axis(x, order, -1, sm::index_mode::clip);
    auto restored = sm::zeros<float>(512, 1000);
    sm::put_along_axis(restored, order, sorted, -1, sm::index_mode::clip, true);  // a permutation per row: unique
    CHECK(differences(restored, hx) == 0);
    // embedding gradient: table_grad[ids[j], :] += g[j, :], the transpose of take(table, ids, 0)
    std::vector<std::int64_t> hids;
    std::vector<float> hg;
    auto ids = host_index({2048}, hids, 0, 50000);
    for (std::size_t j = 0; j < 2048; j += 3) hids[j] = ids.data[j] = 17;  // a popular row
    auto g = host_array<float>({2048, 64}, hg);
    auto table_grad = sm::zeros<float>(50000, 64);
    sm::index_add(table_grad, ids, g, 0);
    std::vector<double> acc(50000 * 64, 0.0);
    for (std::size_t j = 0; j < 2048; ++j)
        for (std::size_t c = 0; c < 64; ++c) acc[static_cast<std::size_t>(hids[j]) * 64 + c] += hg[j * 64 + c];
    bad = 0;
    for (std::size_t k = 0; k < acc.size(); ++k) bad += table_grad.cdata()[k] != static_cast<float>(acc[k]);
    CHECK(bad == 0);
    // top-5 mask
    auto ranked = sm::argsort(x, -1, true);
    auto mask = sm::zeros<float>(512, 1000);
    mask.put_along_axis(ranked(SLICE_ALL, SLICE(0, 5)), 1.0f, -1, sm::index_mode::clip, true);  // five distinct positions per row
    bad = 0;
    for (std::size_t i = 0; i < 512; ++i) {
        int ones = 0;
        for (std::size_t j = 0; j < 1000; ++j) ones += mask.cdata()[i * 1000 + j] == 1.0f;
        bad += ones != 5;
        for (std::size_t k = 0; k < 5; ++k) bad += mask.cdata()[i * 1000 + static_cast<std::size_t>(ranked.cdata()[i * 1000 + k])] != 1.0f;
    }
    CHECK(bad == 0);
}

// The flat forms on operands that are not dense -- a transposed 3 x 5 target, a transposed index array -- against the same call on
// their contiguous copies; and one checked-mode bad index on a 1-D target of 4 elements.
template <typename T>
static void test_flat_views_and_small_checked() {
    std::vector<T> h, hv;
    std::vector<std::int64_t> hi;
    for (bool flat_ids : {false, true}) {
        auto a = host_array<T>({3, 5}, h);
        auto b = from_host(h, {3, 5});
        auto tr = a.transpose();                   // {5, 3}, not dense
        auto dense = b.transpose().contiguous();   // the same elements, dense
        auto idx = host_index({2, 4}, hi, -15, 15);
        auto idx_t = host_index({4, 2}, hi, -15, 15);
        auto v = host_array<T>({8}, hv);
        const auto before = sm::fusion_stats();
        if (flat_ids) {
            tr.put_flat(from_host(std::vector<std::int64_t>(hi.begin(), hi.end()), {8}), v);
            dense.put_flat(from_host(std::vector<std::int64_t>(hi.begin(), hi.end()), {8}), v);
        } else {
            tr.put_along_axis(idx, v);
            dense.put_along_axis(idx, v);
            tr.put_along_axis(idx_t.transpose(), T(7));  // the index array a view as well
            dense.put_along_axis(idx_t.transpose().contiguous(), T(7));
        }
        CHECK(sm::fusion_stats().scatters - before.scatters == (flat_ids ? 2u : 4u));
        std::vector<T> want(15);
        dense.copy_dense_out(want.data());
        CHECK(differences(tr, want) == 0);
        // ... and a is its transpose
        std::vector<T> back(15);
        for (std::size_t i = 0; i < 3; ++i)
            for (std::size_t j = 0; j < 5; ++j) back[i * 5 + j] = want[j * 3 + i];
        CHECK(differences(a, back) == 0);
    }
    // checked: index 4 of 4 elements is dropped, the valid entries are applied, std::out_of_range; the next call works
    const auto ids = from_host(std::vector<std::int64_t>{1, 4, -1}, {3});
    const auto v = from_host(std::vector<T>{T(10), T(20), T(30)}, {3});
    auto p = from_host(std::vector<T>{T(1), T(2), T(3), T(4)}, {4});
    CHECK(throws_out_of_range([&] { p.put(ids, v, 0); }));
    CHECK(differences(p, std::vector<T>{T(1), T(10), T(3), T(30)}) == 0);
    CHECK(throws_out_of_range([&] { p.scatter_add(ids, v, 0); }));
    CHECK(differences(p, std::vector<T>{T(1), T(20), T(3), T(60)}) == 0);
    CHECK(throws_out_of_range([&] { p.put_flat(ids, T(5)); }));
    CHECK(differences(p, std::vector<T>{T(1), T(5), T(3), T(5)}) == 0);
    p.index_add(ids, v, 0, sm::index_mode::clip);
    CHECK(differences(p, std::vector<T>{T(31), T(15), T(3), T(25)}) == 0);  // clip: 4 names the last position, -1 the first
}

int main() {
    try {
        test_forms<float>();
        test_forms<double>();
        test_forms<int>();
        test_forms<std::int64_t>();
        test_flat_views_and_small_checked<float>();
        test_flat_views_and_small_checked<double>();
        test_flat_views_and_small_checked<int>();
        test_flat_views_and_small_checked<std::int64_t>();
        test_index_modes();
        test_views_chains_and_counter();
        test_nan_payload_and_signed_zero();
        test_readme_snippets();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_scatter: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
