// test_scan.cpp -- cumulative scans through the drop-in surface: sm::cumsum / cumprod / cummax / cummin(a, axis) and the member
// forms for the four element types, negative and absent axis, a bad axis, a pending operator chain and a view as the operand,
// the CDF `h.cumsum(0) / h.sum(0, true)`, the `scans` counter and the README's snippet.
// Expected values: loops on the host over the same elements (fp64 running values rounded once, as the contract in smhip.h says).
#include <sm.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
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

static std::uint64_t g_state = 0x2468aceull;
static double unit() {
    std::uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return static_cast<double>((z ^ (z >> 31)) >> 11) / 9007199254740992.0;
}

// Small integers: sums are exact in fp64; products use the factors -2 .. 2 without 0 only for short axes.
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

enum Kind { SUM, PROD, MAX, MIN };

// The scan of rows x cols along `axis` on the host, under the contract: fp64 / wrapping running value, rounded per output.
template <typename T>
static std::vector<T> host_scan(const std::vector<T> &x, std::size_t rows, std::size_t cols, int axis, Kind kind) {
    using A = std::conditional_t<std::is_integral_v<T>, std::uint64_t, double>;
    std::vector<T> out(x.size());
    const std::size_t lines = axis == 0 ? cols : rows, len = axis == 0 ? rows : cols;
    for (std::size_t l = 0; l < lines; ++l) {
        A acc = kind == PROD ? A(1) : A(0);
        T ext = T();
        for (std::size_t r = 0; r < len; ++r) {
            const std::size_t at = axis == 0 ? r * cols + l : l * cols + r;
            const T e = x[at];
            if (kind == SUM) acc += static_cast<A>(static_cast<std::conditional_t<std::is_integral_v<T>, std::int64_t, double>>(e));
            if (kind == PROD) acc *= static_cast<A>(static_cast<std::conditional_t<std::is_integral_v<T>, std::int64_t, double>>(e));
            if (kind == MAX) ext = r == 0 || e > ext ? e : ext;
            if (kind == MIN) ext = r == 0 || e < ext ? e : ext;
            if (kind == SUM || kind == PROD) {
                if constexpr (std::is_integral_v<T>) out[at] = static_cast<T>(static_cast<std::int64_t>(acc));
                else out[at] = static_cast<T>(acc);
            } else {
                out[at] = ext;
            }
        }
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
    const std::size_t R = 37, Cn = 1030;  // axis 0: 37 factors of magnitude <= 2 stay far inside every type's fp64 / wrapping range
    std::vector<T> h;
    auto a = host_array<T>({R, Cn}, h);
    std::vector<T> hp;
    auto p = host_array<T>({R, Cn}, hp, 1, 2);  // factors 1 and 2 ...
    for (std::size_t i = 0; i < hp.size(); i += 3) hp[i] = static_cast<T>(-hp[i]);  // ... some of them negative
    {
        T *w = p.data;
        for (std::size_t i = 0; i < hp.size(); ++i) w[i] = hp[i];
    }
    for (int axis : {0, 1, -1, -2}) {
        const int ax = axis < 0 ? axis + 2 : axis;
        const auto s1 = sm::cumsum(a, axis);
        const auto s2 = a.cumsum(axis);
        CHECK(s1.shape() == (std::vector<std::size_t>{R, Cn}));
        CHECK(differences(s1, host_scan(h, R, Cn, ax, SUM)) == 0);
        CHECK(differences(s2, host_scan(h, R, Cn, ax, SUM)) == 0);
        CHECK(differences(sm::cummax(a, axis), host_scan(h, R, Cn, ax, MAX)) == 0);
        CHECK(differences(a.cummax(axis), host_scan(h, R, Cn, ax, MAX)) == 0);
        CHECK(differences(sm::cummin(a, axis), host_scan(h, R, Cn, ax, MIN)) == 0);
        CHECK(differences(a.cummin(axis), host_scan(h, R, Cn, ax, MIN)) == 0);
    }
    // products along the short axis (2^37 fits every accumulator; int32 wraps, as the host loop does)
    CHECK(differences(sm::cumprod(p, 0), host_scan(hp, R, Cn, 0, PROD)) == 0);
    CHECK(differences(p.cumprod(-2), host_scan(hp, R, Cn, 0, PROD)) == 0);
    // no axis: the elements in row-major order, shape {totalSize}
    const auto flat = a.cumsum();
    CHECK(flat.shape() == std::vector<std::size_t>{R * Cn});
    CHECK(differences(flat, host_scan(h, 1, R * Cn, 1, SUM)) == 0);
    CHECK(differences(sm::cummax(a), host_scan(h, 1, R * Cn, 1, MAX)) == 0);
    CHECK(differences(sm::cummin(a), host_scan(h, 1, R * Cn, 1, MIN)) == 0);
    CHECK(sm::cumsum(a).shape() == std::vector<std::size_t>{R * Cn});
    std::vector<T> hs;
    auto sp = host_array<T>({5, 6}, hs, 1, 2);
    CHECK(differences(sm::cumprod(sp), host_scan(hs, 1, 30, 1, PROD)) == 0);
    CHECK(differences(sp.cumprod(), host_scan(hs, 1, 30, 1, PROD)) == 0);
    // a view operand: the transposed array along axis 0 is the array along axis 1, transposed
    const auto t = a.transpose().cumsum(0);
    CHECK(t.shape() == (std::vector<std::size_t>{Cn, R}));
    const auto want = host_scan(h, R, Cn, 1, SUM);
    const T *tp = t.cdata();
    int bad = 0;
    for (std::size_t i = 0; i < R; ++i)
        for (std::size_t j = 0; j < Cn; ++j) bad += tp[j * R + i] != want[i * Cn + j];
    CHECK(bad == 0);
    // the flattened transposed view: its own row-major order
    const auto tf = sm::cumsum(a.transpose());
    std::vector<T> ht(h.size());
    for (std::size_t i = 0; i < R; ++i)
        for (std::size_t j = 0; j < Cn; ++j) ht[j * R + i] = h[i * Cn + j];
    CHECK(differences(tf, host_scan(ht, 1, R * Cn, 1, SUM)) == 0);
    // a bad axis throws, with the reductions' wording
    for (int axis : {2, -3}) {
        bool threw = false;
        try {
            (void)sm::cumsum(a, axis);
        } catch (const std::runtime_error &e) {
            threw = std::string(e.what()).find("out of range for rank 2") != std::string::npos;
        }
        CHECK(threw);
    }
}

static void test_pending_chain_operand_and_counter() {
    const std::size_t R = 200, Cn = 300;
    std::vector<float> ha, hb;
    auto a = host_array<float>({R, Cn}, ha);
    auto b = host_array<float>({R, Cn}, hb);
    const auto before = sm::fusion_stats();
    auto s = sm::cumsum(a * 2.0f + b, 1);  // the operand is a pending chain: evaluated first (one chain), then one scan
    const auto after = sm::fusion_stats();
    CHECK(after.chains - before.chains == 1);
    CHECK(after.scans - before.scans == 1);
    CHECK(after.reductions == before.reductions);
    std::vector<float> hc(ha.size());
    for (std::size_t i = 0; i < hc.size(); ++i) hc[i] = ha[i] * 2.0f + hb[i];
    CHECK(differences(s, host_scan(hc, R, Cn, 1, SUM)) == 0);
    const auto b2 = sm::fusion_stats();
    (void)a.cummax(0);
    (void)sm::cumprod(a);
    CHECK(sm::fusion_stats().scans - b2.scans == 2);
}

static void test_cdf() {
    // integer-valued counts: the running sum and the total are exact, so the CDF ends at exactly 1 in every column
    const std::size_t R = 513, Cn = 70;
    std::vector<float> h;
    auto hist = host_array<float>({R, Cn}, h, 1, 40);
    const auto before = sm::fusion_stats();
    auto cdf = hist.cumsum(0) / hist.sum(0, true);
    const auto after = sm::fusion_stats();
    CHECK(after.scans - before.scans == 1);
    CHECK(after.reductions - before.reductions == 1);
    CHECK(cdf.shape() == (std::vector<std::size_t>{R, Cn}));
    const float *p = cdf.cdata();
    const auto run = host_scan(h, R, Cn, 0, SUM);
    int bad = 0;
    for (std::size_t j = 0; j < Cn; ++j) {
        bad += p[(R - 1) * Cn + j] != 1.0f;
        for (std::size_t i = 0; i < R; ++i) bad += p[i * Cn + j] != run[i * Cn + j] / run[(R - 1) * Cn + j];
        for (std::size_t i = 1; i < R; ++i) bad += !(p[i * Cn + j] > p[(i - 1) * Cn + j]);
    }
    CHECK(bad == 0);
}

// The README's snippet ("Cumulative scans"), as it stands there.
static void test_readme_snippet() {
    auto h = sm::ones<float>(256, 8);                 // a histogram per column
    auto cdf = h.cumsum(0) / h.sum(0, true);          // one scan, one reduction, one division: rows end at exactly 1
    auto offsets = sm::cumsum(h, 0) - h;              // exclusive prefix: where each bin starts
    auto peak = sm::cummax(h, -1);                    // running maximum along the last axis
    auto growth = sm::cumprod(h * 1.01f, 0);          // cumulative return from per-step factors
    auto flat = sm::cumsum(h);                        // no axis: row-major order, shape {2048}
    CHECK(cdf.cdata()[255 * 8 + 3] == 1.0f && cdf.cdata()[3] == 1.0f / 256.0f);
    CHECK(offsets.cdata()[10 * 8] == 10.0f);
    CHECK(peak.cdata()[77] == 1.0f);
    CHECK(std::fabs(growth.cdata()[255 * 8] - std::pow(1.01f, 256.0)) < 1e-3);
    CHECK(flat.shape() == std::vector<std::size_t>{2048} && flat.cdata()[2047] == 2048.0f);
}

int main() {
    try {
        test_forms<float>();
        test_forms<double>();
        test_forms<int>();
        test_forms<std::int64_t>();
        test_pending_chain_operand_and_counter();
        test_cdf();
        test_readme_snippet();
    } catch (const std::exception &e) {
        std::printf("exception: %s\n", e.what());
        ++g_failures;
    }
    std::printf("test_scan: %d checks, %d failures\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
