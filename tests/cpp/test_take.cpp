// test_take.cpp -- take / take_along_axis through the drop-in surface: sm::take_along_axis / take / take_flat and the member
// forms for the four element types, negative and absent axis, a bad axis, a rank mismatch and a non-broadcastable index
// (std::invalid_argument), an out-of-range index under the three modes, a transposed view, a slice of an argsort result and a
// pending operator chain as operands, the result feeding an operator chain, NaN payloads and signed zeros, the `takes` counter
// and the README's snippets.
// Expected values: the same picks made on the host.
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

static std::uint64_t g_state = 0x13579bdfull;
static std::uint64_t next() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

using Shape = std::vector<std::size_t>;

// Every element another value, so that a wrong address shows.
template <typename T>
static sm::SMArray<T> host_array(Shape shape, std::vector<T> &mirror) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    T *buf = new T[n];
    mirror.resize(n);
    for (std::size_t i = 0; i < n; ++i) mirror[i] = buf[i] = static_cast<T>(i + 1);
    return sm::SMArray<T>(buf, std::move(shape));
}

// Positions in [lo, hi).
static sm::SMArray<std::int64_t> host_index(Shape shape, std::vector<std::int64_t> &mirror, std::int64_t lo, std::int64_t hi) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    std::int64_t *buf = new std::int64_t[n];
    mirror.resize(n);
    for (std::size_t i = 0; i < n; ++i) mirror[i] = buf[i] = lo + static_cast<std::int64_t>(next() % static_cast<std::uint64_t>(hi - lo));
    return sm::SMArray<std::int64_t>(buf, std::move(shape));
}

template <typename T>
static int differences(const sm::SMArray<T> &got, const std::vector<T> &want) {
    if (got.totalSize != want.size()) return -1;
    return std::memcmp(got.cdata(), want.data(), want.size() * sizeof(T)) != 0;
}

static std::int64_t checked_position(std::int64_t i, std::int64_t R) { return i < 0 ? i + R : i; }

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

template <typename T>
static void test_forms() {
    const std::size_t R = 37, Cn = 130;
    std::vector<T> h, want;
    std::vector<std::int64_t> hi;
    auto a = host_array<T>({R, Cn}, h);
    // take_along_axis along each axis, negative axes, sm:: and member forms; negative positions count from the end
    for (int axis : {0, 1, -1, -2}) {
        const int ax = axis < 0 ? axis + 2 : axis;
        const std::size_t J = ax == 0 ? 50 : 200, rows = ax == 0 ? J : R, cols = ax == 0 ? Cn : J;
        const std::int64_t extent = static_cast<std::int64_t>(ax == 0 ? R : Cn);
        auto idx = host_index({rows, cols}, hi, -extent, extent);
        want.resize(rows * cols);
        for (std::size_t i = 0; i < rows; ++i)
            for (std::size_t j = 0; j < cols; ++j) {
                const std::size_t p = static_cast<std::size_t>(checked_position(hi[i * cols + j], extent));
                want[i * cols + j] = ax == 0 ? h[p * Cn + j] : h[i * Cn + p];
            }
        const auto before = sm::fusion_stats();
        const auto t = sm::take_along_axis(a, idx, axis);
        CHECK(sm::fusion_stats().takes - before.takes == 1);
        CHECK((t.shape() == Shape{rows, cols}));
        CHECK(differences(t, want) == 0);
        CHECK(differences(a.take_along_axis(idx, axis), want) == 0);
    }
    // the index array broadcast against the operand: one line of positions for every row
    {
        auto line = host_index({1, 60}, hi, 0, static_cast<std::int64_t>(Cn));
        want.resize(R * 60);
        for (std::size_t i = 0; i < R; ++i)
            for (std::size_t j = 0; j < 60; ++j) want[i * 60 + j] = h[i * Cn + static_cast<std::size_t>(hi[j])];
        const auto t = sm::take_along_axis(a, line, 1);
        CHECK((t.shape() == Shape{R, 60}));
        CHECK(differences(t, want) == 0);
    }
    // take: a 1-D index array along either axis
    for (int axis : {0, 1, -1}) {
        const int ax = axis < 0 ? axis + 2 : axis;
        const std::int64_t extent = static_cast<std::int64_t>(ax == 0 ? R : Cn);
        const std::size_t n = 77;
        auto ids = host_index({n}, hi, -extent, extent);
        const std::size_t rows = ax == 0 ? n : R, cols = ax == 0 ? Cn : n;
        want.resize(rows * cols);
        for (std::size_t i = 0; i < rows; ++i)
            for (std::size_t j = 0; j < cols; ++j)
                want[i * cols + j] = ax == 0 ? h[static_cast<std::size_t>(checked_position(hi[i], extent)) * Cn + j]
                                             : h[i * Cn + static_cast<std::size_t>(checked_position(hi[j], extent))];
        const auto t = sm::take(a, ids, axis);
        CHECK((t.shape() == Shape{rows, cols}));
        CHECK(differences(t, want) == 0);
        CHECK(differences(a.take(ids, axis), want) == 0);
    }
    // no axis: both flattened row-major; take_flat
    {
        const std::int64_t total = static_cast<std::int64_t>(R * Cn);
        auto idx = host_index({5, 11}, hi, -total, total);
        want.resize(55);
        for (std::size_t k = 0; k < 55; ++k) want[k] = h[static_cast<std::size_t>(checked_position(hi[k], total))];
        const auto t = sm::take_along_axis(a, idx);
        CHECK((t.shape() == Shape{55}));
        CHECK(differences(t, want) == 0 && differences(a.take_along_axis(idx), want) == 0);
        auto ids = host_index({55}, hi, 0, total);
        for (std::size_t k = 0; k < 55; ++k) want[k] = h[static_cast<std::size_t>(hi[k])];
        const auto f = sm::take_flat(a, ids);
        CHECK((f.shape() == Shape{55}));
        CHECK(differences(f, want) == 0 && differences(a.take_flat(ids), want) == 0);
        // of a view the flattening is the view's own row-major order
        const auto tr = a.transpose();
        for (std::size_t k = 0; k < 55; ++k) {
            const std::size_t at = static_cast<std::size_t>(hi[k]);
            want[k] = h[(at % R) * Cn + at / R];
        }
        CHECK(differences(sm::take_flat(tr, ids), want) == 0);
    }
    // a transposed view is read in place: take(A.T, ids, 0) picks columns of A
    {
        const auto tr = a.transpose();  // {Cn, R}
        auto ids = host_index({40}, hi, 0, static_cast<std::int64_t>(Cn));
        want.resize(40 * R);
        for (std::size_t j = 0; j < 40; ++j)
            for (std::size_t i = 0; i < R; ++i) want[j * R + i] = h[i * Cn + static_cast<std::size_t>(hi[j])];
        const auto t = sm::take(tr, ids, 0);
        CHECK((t.shape() == Shape{40, R}));
        CHECK(differences(t, want) == 0);
    }
    // what does not fit throws std::invalid_argument
    auto idx2 = host_index({R, 5}, hi, 0, 5);
    auto ids = host_index({5}, hi, 0, 5);
    for (int axis : {2, -3}) {
        CHECK(throws_invalid_argument([&] { (void)sm::take_along_axis(a, idx2, axis); }));
        CHECK(throws_invalid_argument([&] { (void)a.take(ids, axis); }));
    }
    CHECK(throws_invalid_argument([&] { (void)sm::take_along_axis(a, ids, 1); }));                         // rank 1 against rank 2
    auto wrong = host_index({R - 1, 5}, hi, 0, 5);
    CHECK(throws_invalid_argument([&] { (void)sm::take_along_axis(a, wrong, 1); }));                       // 36 rows against 37
    CHECK(throws_invalid_argument([&] { (void)sm::take(a, idx2, 0); }));                                   // take wants a 1-D index array
    CHECK(throws_invalid_argument([&] { (void)sm::take_flat(a, idx2); }));
}

// The flat forms with BOTH operands not dense -- a transposed 3 x 5 array, a transposed index array -- against the same call on
// their contiguous copies; and one checked-mode bad index on a 1-D array of 4 elements.
template <typename T>
static void test_flat_views_and_small_checked() {
    std::vector<T> h;
    std::vector<std::int64_t> hi;
    auto a = host_array<T>({3, 5}, h);
    auto idx = host_index({4, 2}, hi, -15, 15);
    const auto tr = a.transpose();      // {5, 3}
    const auto ix = idx.transpose();    // {2, 4}
    const auto dense = tr.contiguous();
    const auto dense_ix = ix.contiguous();
    const auto before = sm::fusion_stats();
    const auto want = dense.take_along_axis(dense_ix);
    const auto got = tr.take_along_axis(ix);
    CHECK(sm::fusion_stats().takes - before.takes == 2);
    CHECK((got.shape() == Shape{8}));
    CHECK(std::memcmp(got.cdata(), want.cdata(), 8 * sizeof(T)) == 0);
    std::vector<T> by_hand(8);
    for (std::size_t k = 0; k < 8; ++k) {
        const std::size_t at = static_cast<std::size_t>(checked_position(hi[(k % 4) * 2 + k / 4], 15));  // ix[k / 4][k % 4] = idx[k % 4][k / 4]
        by_hand[k] = h[(at % 3) * 5 + at / 3];                                                            // tr's flattening: tr[at / 3][at % 3]
    }
    CHECK(differences(got, by_hand) == 0);
    // checked: index 4 of 4 elements throws std::out_of_range; the next call on this thread works
    auto four = host_array<T>({4}, h);
    sm::SMArray<std::int64_t> ids(new std::int64_t[3]{1, 4, -1}, Shape{3});
    int threw = 0;
    try {
        (void)four.take(ids, 0);
    } catch (const std::out_of_range &) {
        ++threw;
    }
    try {
        (void)four.take_flat(ids);
    } catch (const std::out_of_range &) {
        ++threw;
    }
    CHECK(threw == 2);
    CHECK(differences(four.take(ids, 0, sm::index_mode::clip), std::vector<T>{h[1], h[3], h[0]}) == 0);
    CHECK(differences(four.take(ids(SLICE(0, 1)), 0), std::vector<T>{h[1]}) == 0);
}

static void test_index_modes() {
    std::vector<float> h;
    auto a = host_array<float>({9, 300}, h);
    const std::int64_t R = 300, trouble[] = {R, -R - 1, INT64_MIN, INT64_MAX, std::int64_t{1} << 32, (std::int64_t{1} << 32) + 1};
    for (std::int64_t t : trouble) {
        std::int64_t *buf = new std::int64_t[4]{0, t, R - 1, -1};
        sm::SMArray<std::int64_t> ids(buf, Shape{4});
        int threw = 0;
        try {
            (void)sm::take(a, ids, 1);  // checked is the default
        } catch (const std::out_of_range &) {
            ++threw;
        }
        try {
            (void)a.take_along_axis(sm::SMArray<std::int64_t>(new std::int64_t[4]{0, t, R - 1, -1}, Shape{1, 4}), 1, sm::index_mode::checked);
        } catch (const std::out_of_range &) {
            ++threw;
        }
        CHECK(threw == 2);
        const auto c = sm::take(a, ids, 1, sm::index_mode::clip);   // numpy: negatives go to 0
        const auto w = sm::take(a, ids, 1, sm::index_mode::wrap);   // numpy: the non-negative remainder
        const std::size_t ct = t < 0 ? 0 : static_cast<std::size_t>(R - 1), wt = static_cast<std::size_t>(((t % R) + R) % R);
        int bad = 0;
        for (std::size_t i = 0; i < 9; ++i) {
            bad += c.cdata()[i * 4] != h[i * 300] || c.cdata()[i * 4 + 1] != h[i * 300 + ct] || c.cdata()[i * 4 + 2] != h[i * 300 + 299] || c.cdata()[i * 4 + 3] != h[i * 300];
            bad += w.cdata()[i * 4] != h[i * 300] || w.cdata()[i * 4 + 1] != h[i * 300 + wt] || w.cdata()[i * 4 + 2] != h[i * 300 + 299] || w.cdata()[i * 4 + 3] != h[i * 300 + 299];
        }
        CHECK(bad == 0);
    }
    // every position of [-R, R) is valid under checked
    std::int64_t *all = new std::int64_t[600];
    for (int k = 0; k < 600; ++k) all[k] = k - 300;
    const auto t = sm::take(a, sm::SMArray<std::int64_t>(all, Shape{600}), 1);
    int bad = 0;
    for (std::size_t k = 0; k < 600; ++k) bad += t.cdata()[k] != h[k % 300];
    CHECK(bad == 0);
}

static void test_views_chains_and_counter() {
    const std::size_t R = 200, Cn = 300;
    std::vector<float> ha, hb;
    std::vector<std::int64_t> hi;
    auto a = host_array<float>({R, Cn}, ha);
    auto b = host_array<float>({R, Cn}, hb);
    auto idx = host_index({R, Cn}, hi, 0, static_cast<std::int64_t>(Cn));
    const auto before = sm::fusion_stats();
    auto t = sm::take_along_axis(a * 2.0f + b, idx, -1);  // the operand is a pending chain: evaluated first (one chain), then one take
    const auto after = sm::fusion_stats();
    CHECK(after.chains - before.chains == 1);
    CHECK(after.takes - before.takes == 1);
    CHECK(after.sorts == before.sorts && after.arg_reductions == before.arg_reductions && after.reductions == before.reductions);
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i)
        for (std::size_t j = 0; j < Cn; ++j) {
            const std::size_t p = i * Cn + static_cast<std::size_t>(hi[i * Cn + j]);
            bad += t.cdata()[i * Cn + j] != ha[p] * 2.0f + hb[p];
        }
    CHECK(bad == 0);
    // a pending chain as the INDEX operand
    auto shifted = sm::take_along_axis(a, idx + std::int64_t{-300}, -1);  // every position counted from the end instead
    bad = 0;
    for (std::size_t k = 0; k < R * Cn; ++k) bad += shifted.cdata()[k] != ha[k / Cn * Cn + static_cast<std::size_t>(hi[k])];
    CHECK(bad == 0);
    // the result feeds the next chain
    auto lifted = sm::take_along_axis(a, idx, -1) + 1.0f;
    bad = 0;
    for (std::size_t k = 0; k < R * Cn; ++k) bad += lifted.cdata()[k] != ha[k / Cn * Cn + static_cast<std::size_t>(hi[k])] + 1.0f;
    CHECK(bad == 0);
    // a slice of an argsort result as the index operand: the five largest of each row are the head of the descending sort
    auto keys = sm::take_along_axis(b, idx, -1);  // values with duplicates
    auto [sorted, order] = sm::sort_with_index(keys, -1, true);
    auto top5 = sm::take_along_axis(keys, order(SLICE_ALL, SLICE(0, 5)), -1, sm::index_mode::clip);
    CHECK((top5.shape() == Shape{R, 5}));
    bad = 0;
    for (std::size_t i = 0; i < R; ++i)
        for (std::size_t j = 0; j < 5; ++j) bad += top5.cdata()[i * 5 + j] != sorted.cdata()[i * Cn + j];
    CHECK(bad == 0);
    // applying the whole permutation gives the sorted array, bit for bit
    CHECK(std::memcmp(sm::take_along_axis(keys, order, -1).cdata(), sorted.cdata(), R * Cn * sizeof(float)) == 0);
    // argmax with keepdims picks the maxima
    auto [best, where] = sm::max_with_index(keys, -1, true);
    CHECK(std::memcmp(sm::take_along_axis(keys, where, -1).cdata(), best.cdata(), R * sizeof(float)) == 0);
    const auto b2 = sm::fusion_stats();
    (void)a.take_along_axis(idx, 1);
    (void)sm::take_along_axis(a, idx);
    (void)sm::take(a, order(0, SLICE_ALL), 1, sm::index_mode::wrap);
    (void)a.take_flat(order(0, SLICE_ALL));
    CHECK(sm::fusion_stats().takes - b2.takes == 4);
}

static void test_nan_payload_and_signed_zero() {
    const std::uint32_t bits[8] = {0x7fc00001u, 0xffc00002u, 0x7f800123u, 0x80000000u, 0x00000000u, 0x80000001u, 0xff800000u, 0x3f800000u};
    float *buf = new float[8];
    std::memcpy(buf, bits, sizeof bits);
    sm::SMArray<float> a(buf, Shape{2, 4});
    sm::SMArray<std::int64_t> idx(new std::int64_t[8]{3, 0, 1, 2, -1, 2, 0, 1}, Shape{2, 4});
    const std::uint32_t want[8] = {bits[3], bits[0], bits[1], bits[2], bits[7], bits[6], bits[4], bits[5]};
    for (auto mode : {sm::index_mode::checked, sm::index_mode::wrap}) {
        const auto t = sm::take_along_axis(a, idx, 1, mode);
        CHECK(std::memcmp(t.cdata(), want, sizeof want) == 0);
    }
    const double dbits_src[3] = {-0.0, std::nan("0x5"), 0.0};
    sm::SMArray<double> d(new double[3]{dbits_src[0], dbits_src[1], dbits_src[2]}, Shape{3});
    const auto r = sm::take(d, sm::SMArray<std::int64_t>(new std::int64_t[4]{1, 0, 2, 0}, Shape{4}), 0);
    const double want_d[4] = {dbits_src[1], dbits_src[0], dbits_src[2], dbits_src[0]};
    CHECK(std::memcmp(r.cdata(), want_d, sizeof want_d) == 0);
}

// The README's snippets ("Picking by position"), as they stand there.
static void test_readme_snippet() {
    auto keys = sm::ones<float>(512, 1000), values = sm::ones<float>(512, 1000);
    {
        float *k = keys.data, *v = values.data;
        for (std::size_t i = 0; i < 512; ++i)
            for (std::size_t j = 0; j < 1000; ++j) k[i * 1000 + j] = static_cast<float>((j * 7 + i) % 1000), v[i * 1000 + j] = static_cast<float>(j) * 0.001f;
    }
    auto by_key = sm::take_along_axis(values, sm::argsort(keys, -1), -1);   // each row of values in the order of its row of keys
    auto e = sm::exp(values - sm::max(values, -1, true));
    auto softmax = e / sm::sum(e, -1, true);
    auto labels2d = sm::zeros<std::int64_t>(512, 1);                        // ... the class of each sample ...
    {
        std::int64_t *l = labels2d.data;
        for (std::size_t i = 0; i < 512; ++i) l[i] = static_cast<std::int64_t>((i * 13) % 1000);
    }
    auto p_label = sm::take_along_axis(softmax, labels2d, -1);              // shape {512, 1}: each sample's label probability
    auto table = sm::ones<float>(50000, 64);
    auto ids = sm::zeros<std::int64_t>(2048);                               // ... row numbers ...
    {
        float *t = table.data;
        for (std::size_t i = 0; i < 50000 * 64; ++i) t[i] = static_cast<float>(i % 4099);
        std::int64_t *p = ids.data;
        for (std::size_t i = 0; i < 2048; ++i) p[i] = static_cast<std::int64_t>((i * 7919) % 50000);
    }
    auto rows = sm::take(table, ids, 0);                                    // shape {2048, 64}: the embedding lookup
    auto ranked = sm::argsort(values, -1, true);
    auto top5 = sm::take_along_axis(values, ranked(SLICE_ALL, SLICE(0, 5)), -1);  // the five largest of each row: a sliced view as the index operand
    auto clipped = sm::take(table, ids, 0, sm::index_mode::clip);           // ids outside the table go to its first / last row
    auto wrapped = table.take(ids, 0, sm::index_mode::wrap);                // ids modulo the number of rows; member form
    auto checked = sm::take(table, ids, 0);                                 // the default: throws std::out_of_range on a bad id
    CHECK((by_key.shape() == Shape{512, 1000}) && (p_label.shape() == Shape{512, 1}) && (rows.shape() == Shape{2048, 64}) && (top5.shape() == Shape{512, 5}));
    int bad = 0;
    for (std::size_t i = 0; i < 512; ++i) {
        // key (j * 7 + i) % 1000 is a permutation of 0..999 along j: the value that lands at rank r belongs to the j with that key
        for (std::size_t r = 0; r < 1000; r += 37) {
            std::size_t j = 0;
            while ((j * 7 + i) % 1000 != r) ++j;
            bad += by_key.cdata()[i * 1000 + r] != static_cast<float>(j) * 0.001f;
        }
        bad += p_label.cdata()[i] != softmax.cdata()[i * 1000 + (i * 13) % 1000];
        for (std::size_t j = 0; j < 5; ++j) bad += top5.cdata()[i * 5 + j] != static_cast<float>(999 - j) * 0.001f;
    }
    for (std::size_t i = 0; i < 2048; ++i)
        for (std::size_t j = 0; j < 64; j += 9) {
            const float want = static_cast<float>((((i * 7919) % 50000) * 64 + j) % 4099);
            bad += rows.cdata()[i * 64 + j] != want || clipped.cdata()[i * 64 + j] != want || wrapped.cdata()[i * 64 + j] != want || checked.cdata()[i * 64 + j] != want;
        }
    CHECK(bad == 0);
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
        test_readme_snippet();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_take: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
