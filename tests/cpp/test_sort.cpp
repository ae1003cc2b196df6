// test_sort.cpp -- sort / argsort through the drop-in surface: sm::sort / argsort / sort_with_index(a, axis, descending), the
// member forms, the forms without an axis (the last one) and the _flat forms for the four element types, negative axis, a bad
// axis, a transposed view and a pending operator chain as operands, the sorted result feeding an operator chain and a slice,
// NaN and signed zeros, the `sorts` counter and the README's snippets.
// Expected values: std::stable_sort on the host over the same elements.
#include <sm.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <numeric>
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

static std::uint64_t g_state = 0x2468ace0ull;
static double unit() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<double>((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

// Small integers: many ties along every axis, so the order of the positions has to be kept.
template <typename T>
static sm::SMArray<T> host_array(std::vector<std::size_t> shape, std::vector<T> &mirror, int lo = -9, int hi = 9) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    T *buf = new T[n];
    mirror.resize(n);
    for (std::size_t i = 0; i < n; ++i) {
        buf[i] = static_cast<T>(lo + static_cast<int>(unit() * (hi - lo + 1)));
        mirror[i] = buf[i];
    }
    return sm::SMArray<T>(buf, std::move(shape));
}

// The stable order of rows x cols along `axis` on the host: positions and values, laid out like the operand.
template <typename T>
static void host_sort(const std::vector<T> &x, std::size_t rows, std::size_t cols, int axis, bool descending, std::vector<T> &values,
                      std::vector<std::int64_t> &where) {
    const std::size_t lines = axis == 0 ? cols : rows, len = axis == 0 ? rows : cols;
    values.resize(x.size());
    where.resize(x.size());
    std::vector<std::int64_t> order(len);
    for (std::size_t l = 0; l < lines; ++l) {
        auto at = [&](std::size_t r) { return axis == 0 ? r * cols + l : l * cols + r; };
        std::iota(order.begin(), order.end(), 0);
        std::stable_sort(order.begin(), order.end(), [&](std::int64_t p, std::int64_t q) { return descending ? x[at(p)] > x[at(q)] : x[at(p)] < x[at(q)]; });
        for (std::size_t r = 0; r < len; ++r) where[at(r)] = order[r], values[at(r)] = x[at(order[r])];
    }
}

template <typename T>
static int differences(const sm::SMArray<T> &got, const std::vector<T> &want) {
    if (got.totalSize != want.size()) return -1;
    const T *p = got.cdata();
    int bad = 0;
    for (std::size_t k = 0; k < want.size(); ++k) bad += p[k] != want[k];
    return bad;
}

template <typename T>
static void test_forms() {
    const std::size_t R = 37, Cn = 1030;
    using Shape = std::vector<std::size_t>;
    std::vector<T> h, hv;
    std::vector<std::int64_t> hw;
    auto a = host_array<T>({R, Cn}, h);
    for (int axis : {0, 1, -1, -2}) {
        const int ax = axis < 0 ? axis + 2 : axis;
        for (bool desc : {false, true}) {
            host_sort(h, R, Cn, ax, desc, hv, hw);
            const auto s = sm::sort(a, axis, desc);
            CHECK((s.shape() == Shape{R, Cn}));
            CHECK(differences(s, hv) == 0);
            CHECK(differences(a.sort(axis, desc), hv) == 0);
            const auto w = sm::argsort(a, axis, desc);
            CHECK((w.shape() == Shape{R, Cn}));
            CHECK(differences(w, hw) == 0);
            CHECK(differences(a.argsort(axis, desc), hw) == 0);
            const auto before = sm::fusion_stats();
            auto [v2, w2] = sm::sort_with_index(a, axis, desc);  // one call for both
            CHECK(sm::fusion_stats().sorts - before.sorts == 1);
            CHECK(differences(v2, hv) == 0 && differences(w2, hw) == 0);
            auto [v3, w3] = a.sort_with_index(axis, desc);
            CHECK(differences(v3, hv) == 0 && differences(w3, hw) == 0);
        }
    }
    // no axis argument: the last axis, ascending
    host_sort(h, R, Cn, 1, false, hv, hw);
    CHECK(differences(sm::sort(a), hv) == 0 && differences(a.sort(), hv) == 0);
    CHECK(differences(sm::argsort(a), hw) == 0 && differences(a.argsort(), hw) == 0);
    CHECK(differences(sm::sort_with_index(a).second, hw) == 0);
    // the _flat forms: the row-major flattening, shape {size}
    for (bool desc : {false, true}) {
        host_sort(h, 1, R * Cn, 1, desc, hv, hw);
        const auto f = sm::sort_flat(a, desc);
        CHECK(f.shape() == Shape{R * Cn});
        CHECK(differences(f, hv) == 0 && differences(a.sort_flat(desc), hv) == 0);
        CHECK(differences(sm::argsort_flat(a, desc), hw) == 0 && differences(a.argsort_flat(desc), hw) == 0);
        CHECK(sm::argsort_flat(a).shape() == Shape{R * Cn});
    }
    // a transposed view: along its axis 0 it is the array along axis 1, laid out as the view
    const auto t = a.transpose();
    std::vector<T> ht(h.size());
    for (std::size_t i = 0; i < R; ++i)
        for (std::size_t j = 0; j < Cn; ++j) ht[j * R + i] = h[i * Cn + j];
    for (int axis : {0, 1}) {
        host_sort(ht, Cn, R, axis, axis == 1, hv, hw);
        auto [tv, tw] = sm::sort_with_index(t, axis, axis == 1);
        CHECK((tv.shape() == Shape{Cn, R}));
        CHECK(differences(tv, hv) == 0 && differences(tw, hw) == 0);
    }
    // ... and flattened its own row-major order counts (the view is copied dense first)
    host_sort(ht, 1, R * Cn, 1, false, hv, hw);
    CHECK(differences(sm::argsort_flat(t), hw) == 0);
    // a bad axis throws, with the reductions' wording
    for (int axis : {2, -3}) {
        int threw = 0;
        try {
            (void)sm::sort(a, axis);
        } catch (const std::runtime_error &e) {
            threw += std::string(e.what()).find("out of range for rank 2") != std::string::npos;
        }
        try {
            (void)a.argsort(axis, true);
        } catch (const std::runtime_error &e) {
            threw += std::string(e.what()).find("out of range for rank 2") != std::string::npos;
        }
        try {
            (void)sm::sort_with_index(a, axis);
        } catch (const std::runtime_error &e) {
            threw += std::string(e.what()).find("out of range for rank 2") != std::string::npos;
        }
        CHECK(threw == 3);
    }
}

static void test_pending_chain_operand_result_in_a_chain_and_counter() {
    const std::size_t R = 200, Cn = 300;
    std::vector<float> ha, hb, hv;
    std::vector<std::int64_t> hw;
    auto a = host_array<float>({R, Cn}, ha);
    auto b = host_array<float>({R, Cn}, hb);
    const auto before = sm::fusion_stats();
    auto s = sm::sort(a * 2.0f + b, -1);  // the operand is a pending chain: evaluated first (one chain), then one sort
    const auto after = sm::fusion_stats();
    CHECK(after.chains - before.chains == 1);
    CHECK(after.sorts - before.sorts == 1);
    CHECK(after.reductions == before.reductions && after.scans == before.scans && after.arg_reductions == before.arg_reductions);
    std::vector<float> hc(ha.size());
    for (std::size_t i = 0; i < hc.size(); ++i) hc[i] = ha[i] * 2.0f + hb[i];
    host_sort(hc, R, Cn, 1, false, hv, hw);
    CHECK(differences(s, hv) == 0);
    // a slice of the sorted rows is a view, and it feeds the next operator chain
    auto low5 = s(SLICE_ALL, SLICE(0, 5));
    CHECK((low5.shape() == std::vector<std::size_t>{R, 5}));
    auto range = s(SLICE_ALL, SLICE(Cn - 1, Cn)) - s(SLICE_ALL, SLICE(0, 1));  // max - min of each row
    auto lifted = low5 + 1.0f;
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i) {
        bad += range.cdata()[i] != hv[i * Cn + Cn - 1] - hv[i * Cn];
        for (std::size_t j = 0; j < 5; ++j) bad += low5(i, j) != hv[i * Cn + j], bad += lifted.cdata()[i * 5 + j] != hv[i * Cn + j] + 1.0f;
    }
    CHECK(bad == 0);
    // the positions feed an operator chain of SMArray<std::int64_t> like any array
    auto w = sm::argsort(a, -1, true);
    auto shifted = w + std::int64_t{1};
    host_sort(ha, R, Cn, 1, true, hv, hw);
    bad = 0;
    for (std::size_t i = 0; i < hw.size(); ++i) bad += shifted.cdata()[i] != hw[i] + 1;
    CHECK(bad == 0);
    // descending starts where argmax points
    const auto first = w(SLICE_ALL, SLICE(0, 1)).contiguous();
    const auto am = sm::argmax(a, -1);
    CHECK(std::memcmp(first.cdata(), am.cdata(), R * sizeof(std::int64_t)) == 0);
    const auto b2 = sm::fusion_stats();
    (void)a.sort(0);
    (void)sm::argsort(a);
    (void)sm::sort_with_index(a, 1, true);
    (void)sm::sort_flat(a);
    (void)a.argsort_flat(true);
    CHECK(sm::fusion_stats().sorts - b2.sorts == 5);
}

static void test_nan_and_signed_zero() {
    float *buf = new float[12]{1.0f, -0.0f, 0.0f, -5.0f, /**/ 2.0f, NAN, 9.0f, -NAN, /**/ 0.0f, -0.0f, -1.0f, 0.0f};
    sm::SMArray<float> a(buf, std::vector<std::size_t>{3, 4});
    auto [v, w] = sm::sort_with_index(a, 1);
    const std::int64_t *p = w.cdata();
    const float *q = v.cdata();
    CHECK(p[0] == 3 && p[1] == 1 && p[2] == 2 && p[3] == 0);       // -5, -0, +0, 1: the zeros in the order they stand
    CHECK(std::signbit(q[1]) && !std::signbit(q[2]));
    CHECK(p[4] == 0 && p[5] == 2 && p[6] == 1 && p[7] == 3);       // 2, 9, NaN, -NaN: the NaNs last, in the order they stand
    CHECK(std::isnan(q[6]) && !std::signbit(q[6]) && std::isnan(q[7]) && std::signbit(q[7]));
    CHECK(p[8] == 2 && p[9] == 0 && p[10] == 1 && p[11] == 3);     // -1, +0, -0, +0
    CHECK(!std::signbit(q[9]) && std::signbit(q[10]) && !std::signbit(q[11]));
    auto [dv, dw] = sm::sort_with_index(a, 1, true);
    p = dw.cdata(), q = dv.cdata();
    CHECK(p[0] == 0 && p[1] == 1 && p[2] == 2 && p[3] == 3);       // 1, -0, +0, -5: ties still in rising position
    CHECK(p[4] == 1 && p[5] == 3 && p[6] == 2 && p[7] == 0);       // NaN, -NaN, 9, 2: the NaNs first
    CHECK(!std::signbit(q[4]) && std::signbit(q[5]));
    CHECK(p[8] == 0 && p[9] == 1 && p[10] == 3 && p[11] == 2);     // +0, -0, +0, -1
}

// The README's snippets ("The order along an axis"), as they stand there.
static void test_readme_snippet() {
    auto x = sm::ones<float>(512, 1000);                       // logits, one row per sample
    {
        float *p = x.data;
        for (std::size_t i = 0; i < 512; ++i) p[i * 1000 + (i * 7) % 1000] = 3.0f, p[i * 1000 + (i * 7 + 1) % 1000] = 2.0f;
    }
    auto ranked = sm::argsort(x, -1, true);                    // shape {512, 1000}: the classes of each sample, best first
    auto top5 = ranked(SLICE_ALL, SLICE(0, 5));                // a view of it: the five best classes, never leaving HBM
    auto [sorted, order] = sm::sort_with_index(x, -1);         // ascending values and the permutation that sorts them, one call
    auto median = sorted(SLICE_ALL, SLICE(500, 501));          // the (upper) median of each row is a slice of the sorted rows
    auto spread = sorted(SLICE_ALL, SLICE(999, 1000)) - sorted(SLICE_ALL, SLICE(0, 1));  // ... and feeds the next chain
    auto by_column = x.sort(0);                                // member form, along the first axis
    auto everything = sm::sort_flat(x);                        // the row-major flattening, shape {512000}
    CHECK((ranked.shape() == std::vector<std::size_t>{512, 1000}));
    CHECK((top5.shape() == std::vector<std::size_t>{512, 5}));
    int bad = 0;
    for (std::size_t i = 0; i < 512; ++i) {
        const std::int64_t best = static_cast<std::int64_t>((i * 7) % 1000), second = static_cast<std::int64_t>((i * 7 + 1) % 1000);
        bad += top5(i, 0) != best || top5(i, 1) != second;
        bad += top5(i, 2) != (best == 0 || second == 0 ? (best == 1 || second == 1 ? 2 : 1) : 0);  // then the ties, in rising position
        bad += order.cdata()[i * 1000 + 999] != best || order.cdata()[i * 1000 + 998] != second;
        bad += median(i, 0) != 1.0f || spread.cdata()[i] != 2.0f;
    }
    CHECK(bad == 0);
    CHECK(by_column.cdata()[0] == 1.0f && by_column.cdata()[511 * 1000] == 3.0f);
    CHECK((everything.shape() == std::vector<std::size_t>{512000}) && everything.cdata()[0] == 1.0f && everything.cdata()[511999] == 3.0f);
}

int main() {
    try {
        test_forms<float>();
        test_forms<double>();
        test_forms<int>();
        test_forms<std::int64_t>();
        test_pending_chain_operand_result_in_a_chain_and_counter();
        test_nan_and_signed_zero();
        test_readme_snippet();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_sort: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
