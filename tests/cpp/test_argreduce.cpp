// test_argreduce.cpp -- argmax / argmin through the drop-in surface: sm::argmax / argmin(a, axis, keepdims), the member forms
// and the forms without an axis for the four element types, negative axis, keepdims shapes, a bad axis, a pending operator
// chain and a transposed view as operands, sm::max_with_index / min_with_index against sm::max / min and sm::argmax / argmin
// called separately, the result feeding an operator chain of SMArray<std::int64_t>, the `arg_reductions` counter and the
// README's snippets.
// Expected values: loops on the host over the same elements (the first position of the extreme, as np.argmax gives it).
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
static double unit() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<double>((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

// Small integers: many ties along every axis, so the first occurrence has to win.
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

// The first position of the maximum / minimum of rows x cols along `axis`, on the host.
template <typename T>
static std::vector<std::int64_t> host_arg(const std::vector<T> &x, std::size_t rows, std::size_t cols, int axis, bool max) {
    const std::size_t lines = axis == 0 ? cols : rows, len = axis == 0 ? rows : cols;
    std::vector<std::int64_t> out(lines);
    for (std::size_t l = 0; l < lines; ++l) {
        std::size_t best = 0;
        for (std::size_t r = 1; r < len; ++r) {
            const T e = x[axis == 0 ? r * cols + l : l * cols + r], b = x[axis == 0 ? best * cols + l : l * cols + best];
            if (max ? e > b : e < b) best = r;
        }
        out[l] = static_cast<std::int64_t>(best);
    }
    return out;
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
    std::vector<T> h;
    auto a = host_array<T>({R, Cn}, h);
    for (int axis : {0, 1, -1, -2}) {
        const int ax = axis < 0 ? axis + 2 : axis;
        const auto hi = sm::argmax(a, axis);
        CHECK(hi.shape() == Shape{ax == 0 ? Cn : R});
        CHECK(differences(hi, host_arg(h, R, Cn, ax, true)) == 0);
        CHECK(differences(a.argmax(axis), host_arg(h, R, Cn, ax, true)) == 0);
        CHECK(differences(sm::argmin(a, axis), host_arg(h, R, Cn, ax, false)) == 0);
        CHECK(differences(a.argmin(axis), host_arg(h, R, Cn, ax, false)) == 0);
        const auto kept = sm::argmin(a, axis, true);
        CHECK(kept.shape() == (ax == 0 ? Shape{1, Cn} : Shape{R, 1}));
        CHECK(differences(kept, host_arg(h, R, Cn, ax, false)) == 0);
        CHECK(a.argmax(axis, true).shape() == (ax == 0 ? Shape{1, Cn} : Shape{R, 1}));
    }
    // no axis: the row-major index of the whole array, shape {1}
    const auto flat = a.argmax();
    CHECK(flat.shape() == Shape{1});
    CHECK(differences(flat, host_arg(h, 1, R * Cn, 1, true)) == 0);
    CHECK(differences(sm::argmax(a), host_arg(h, 1, R * Cn, 1, true)) == 0);
    CHECK(differences(sm::argmin(a), host_arg(h, 1, R * Cn, 1, false)) == 0);
    CHECK(differences(a.argmin(), host_arg(h, 1, R * Cn, 1, false)) == 0);
    // a transposed view is read in place: along its axis 0 it is the array along axis 1
    const auto t = a.transpose();
    CHECK(differences(t.argmax(0), host_arg(h, R, Cn, 1, true)) == 0);
    CHECK(differences(sm::argmin(t, 1), host_arg(h, R, Cn, 0, false)) == 0);
    // ... and without an axis its own row-major order counts (the view is copied dense first)
    std::vector<T> ht(h.size());
    for (std::size_t i = 0; i < R; ++i)
        for (std::size_t j = 0; j < Cn; ++j) ht[j * R + i] = h[i * Cn + j];
    CHECK(differences(sm::argmax(t), host_arg(ht, 1, R * Cn, 1, true)) == 0);
    // max_with_index: one call, and it agrees with sm::max and sm::argmax called separately
    for (int axis : {0, -1}) {
        for (bool keep : {false, true}) {
            const auto before = sm::fusion_stats();
            auto [mx, at] = sm::max_with_index(a, axis, keep);
            const auto after = sm::fusion_stats();
            CHECK(after.arg_reductions - before.arg_reductions == 1);
            CHECK(after.reductions == before.reductions);
            const auto m2 = sm::max(a, axis, keep);
            const auto a2 = sm::argmax(a, axis, keep);
            CHECK(mx.shape() == m2.shape() && at.shape() == a2.shape());
            CHECK(std::memcmp(mx.cdata(), m2.cdata(), m2.totalSize * sizeof(T)) == 0);
            CHECK(std::memcmp(at.cdata(), a2.cdata(), a2.totalSize * sizeof(std::int64_t)) == 0);
            auto [mn, an] = sm::min_with_index(a, axis, keep);
            const auto n2 = sm::min(a, axis, keep);
            const auto b2 = sm::argmin(a, axis, keep);
            CHECK(mn.shape() == n2.shape() && an.shape() == b2.shape());
            CHECK(std::memcmp(mn.cdata(), n2.cdata(), n2.totalSize * sizeof(T)) == 0);
            CHECK(std::memcmp(an.cdata(), b2.cdata(), b2.totalSize * sizeof(std::int64_t)) == 0);
        }
    }
    // a bad axis throws, with the reductions' wording
    for (int axis : {2, -3}) {
        bool threw = false;
        try {
            (void)sm::argmax(a, axis);
        } catch (const std::runtime_error &e) {
            threw = std::string(e.what()).find("out of range for rank 2") != std::string::npos;
        }
        CHECK(threw);
        threw = false;
        try {
            (void)sm::min_with_index(a, axis);
        } catch (const std::runtime_error &e) {
            threw = std::string(e.what()).find("out of range for rank 2") != std::string::npos;
        }
        CHECK(threw);
    }
}

static void test_pending_chain_operand_result_in_a_chain_and_counter() {
    const std::size_t R = 200, Cn = 300;
    std::vector<float> ha, hb;
    auto a = host_array<float>({R, Cn}, ha);
    auto b = host_array<float>({R, Cn}, hb);
    const auto before = sm::fusion_stats();
    auto w = sm::argmax(a * 2.0f + b, -1);  // the operand is a pending chain: evaluated first (one chain), then one arg-reduction
    const auto after = sm::fusion_stats();
    CHECK(after.chains - before.chains == 1);
    CHECK(after.arg_reductions - before.arg_reductions == 1);
    CHECK(after.reductions == before.reductions && after.scans == before.scans);
    std::vector<float> hc(ha.size());
    for (std::size_t i = 0; i < hc.size(); ++i) hc[i] = ha[i] * 2.0f + hb[i];
    const auto want = host_arg(hc, R, Cn, 1, true);
    CHECK(differences(w, want) == 0);
    // the positions feed an operator chain of SMArray<std::int64_t> like any array
    const std::int64_t cols = static_cast<std::int64_t>(Cn);
    std::vector<std::int64_t> hr;
    auto rows = host_array<std::int64_t>({R}, hr, 0, 0);
    {
        std::int64_t *p = rows.data;
        for (std::size_t i = 0; i < R; ++i) p[i] = static_cast<std::int64_t>(i);
    }
    auto flat_index = rows * cols + w;  // where each row's maximum stands in the flat array
    const std::int64_t *f = flat_index.cdata();
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i) bad += f[i] != static_cast<std::int64_t>(i) * cols + want[i];
    CHECK(bad == 0);
    const auto b2 = sm::fusion_stats();
    (void)a.argmin(0);
    (void)sm::argmax(a);
    (void)sm::min_with_index(a, 1);
    CHECK(sm::fusion_stats().arg_reductions - b2.arg_reductions == 3);
}

static void test_nan_and_signed_zero() {
    float *buf = new float[12]{1.0f, -0.0f, 0.0f, -5.0f, /**/ 2.0f, NAN, 9.0f, NAN, /**/ 0.0f, -0.0f, -1.0f, -2.0f};
    sm::SMArray<float> a(buf, std::vector<std::size_t>{3, 4});
    auto [mx, at] = sm::max_with_index(a, 1);
    const std::int64_t *p = at.cdata();
    CHECK(p[0] == 0 && p[1] == 1 && p[2] == 0);
    CHECK(std::isnan(mx.cdata()[1]) && mx.cdata()[0] == 1.0f && !std::signbit(mx.cdata()[2]));
    auto [mn, an] = sm::min_with_index(a, 1);
    CHECK(an.cdata()[0] == 3 && an.cdata()[1] == 1 && an.cdata()[2] == 3);
    const auto z = sm::argmin(a, 0);  // columns: {1, 2, 0}, {-0, NaN, -0}, {0, 9, -1}, {-5, NaN, -2}
    CHECK(z.cdata()[0] == 2 && z.cdata()[1] == 1 && z.cdata()[2] == 2 && z.cdata()[3] == 1);
}

// The README's snippets ("Where the maximum is"), as they stand there.
static void test_readme_snippet() {
    auto x = sm::ones<float>(512, 1000);                   // logits, one row per sample
    {
        float *p = x.data;
        for (std::size_t i = 0; i < 512; ++i) p[i * 1000 + (i * 7) % 1000] = 3.0f;
    }
    auto e = sm::exp(x - sm::max(x, -1, true));
    auto softmax = e / sm::sum(e, -1, true);
    auto predicted = sm::argmax(softmax, -1);              // shape {512}: the class of each sample, never leaving HBM
    auto [best, where] = sm::max_with_index(softmax, -1);  // the winning probability and its class, one pass
    auto h = sm::ones<float>(256, 8);                      // a histogram per column
    auto peak_bin = sm::argmax(h, 0);                      // shape {8}: the first of the fullest bins of each column
    auto last_filled = sm::argmax(h.cumsum(0), 0);         // where the running total first reaches its end: the last non-empty bin
    auto flat = sm::argmin(h);                             // no axis: the row-major index, shape {1}
    CHECK(predicted.shape() == std::vector<std::size_t>{512});
    int bad = 0;
    for (std::size_t i = 0; i < 512; ++i) {
        bad += predicted.cdata()[i] != static_cast<std::int64_t>((i * 7) % 1000);
        bad += where.cdata()[i] != predicted.cdata()[i];
        bad += best.cdata()[i] != softmax.cdata()[i * 1000 + (i * 7) % 1000];
    }
    CHECK(bad == 0);
    CHECK(peak_bin.shape() == std::vector<std::size_t>{8} && peak_bin.cdata()[5] == 0);
    CHECK(last_filled.cdata()[0] == 255 && last_filled.cdata()[7] == 255);
    CHECK(flat.shape() == std::vector<std::size_t>{1} && flat.cdata()[0] == 0);
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
    std::printf("test_argreduce: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
