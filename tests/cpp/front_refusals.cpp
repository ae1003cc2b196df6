// front_refusals.cpp -- what the C++ front refuses BEFORE anything touches the device: every such call of the axis, index, counting,
// where / select and unique families made once on host-built arrays, one line per call: name, the exception's type as caught
// most-derived first (out_of_range, invalid_argument, runtime_error), and what().  tests/golden/front_refusals.txt is this program's
// output; tests/test_front_refusals_host.py replays it.  No call here may reach the library's device path: the table reads the same
// with and without a GPU.
#include <sm.h>

#include <cstdint>
#include <cstdio>
#include <limits>
#include <stdexcept>
#include <utility>
#include <vector>

using Shape = std::vector<std::size_t>;
using Index = sm::SMArray<std::int64_t>;

// A host-built array of zeros (an extent of 0 is allowed).
template <typename T>
static sm::SMArray<T> zeros(Shape shape) {
    std::size_t n = 1;
    for (auto d : shape) n *= d;
    T *buf = new T[n ? n : 1]();
    return sm::SMArray<T>(buf, std::move(shape));
}

template <typename Fn>
static void refused(const char *name, Fn fn) {
    const char *type = "none";
    std::string what;
    try {
        fn();
    } catch (const std::out_of_range &e) {
        type = "out_of_range", what = e.what();
    } catch (const std::invalid_argument &e) {
        type = "invalid_argument", what = e.what();
    } catch (const std::runtime_error &e) {
        type = "runtime_error", what = e.what();
    } catch (const std::exception &e) {
        type = "exception", what = e.what();
    }
    std::printf("%s\t%s\t%s\n", name, type, what.c_str());
}

int main() {
    auto a = zeros<float>({2, 3});
    auto a3 = zeros<float>({2, 3, 4});
    auto line = zeros<float>({4});
    auto none = zeros<float>({0, 3});
    auto ids = zeros<std::int64_t>({2});
    auto ids2d = zeros<std::int64_t>({2, 2});
    auto idx = zeros<std::int64_t>({2, 3});
    auto idx1d = zeros<std::int64_t>({3});
    auto idx5 = zeros<std::int64_t>({5, 2});
    auto counts = zeros<int>({4});
    const double inf = std::numeric_limits<double>::infinity();

    // ---- reductions: the axis list
    refused("sum axis 2 of rank 2", [&] { (void)a.sum(2); });
    refused("sum axis -3 of rank 2", [&] { (void)a.sum(-3); });
    refused("sum axes {0, -2} repeated", [&] { (void)a.sum({0, -2}); });
    refused("sum no axis", [&] { (void)a.sum(std::initializer_list<int>{}); });
    refused("mean axis 5", [&] { (void)a.mean(5, true); });
    refused("mean axes {1, 1}", [&] { (void)a.mean({1, 1}); });
    refused("max axis -4 of rank 3", [&] { (void)a3.max(-4); });
    refused("min axes {0, 3} of rank 3", [&] { (void)a3.min({0, 3}); });
    refused("sm::sum axis 2", [&] { (void)sm::sum(a, 2); });
    // ---- scans
    refused("cumsum axis 2", [&] { (void)a.cumsum(2); });
    refused("cumprod axis -3", [&] { (void)a.cumprod(-3); });
    refused("cummax axis 1 of rank 1", [&] { (void)line.cummax(1); });
    refused("cummin axis 3 of rank 3", [&] { (void)a3.cummin(3); });
    // ---- argmax / argmin
    refused("argmax axis 2", [&] { (void)a.argmax(2); });
    refused("argmin axis -3 keepdims", [&] { (void)a.argmin(-3, true); });
    refused("max_with_index axis 2", [&] { (void)a.max_with_index(2); });
    refused("min_with_index axis -4 of rank 3", [&] { (void)a3.min_with_index(-4); });
    // ---- sort
    refused("sort axis 2", [&] { (void)a.sort(2); });
    refused("argsort axis -3", [&] { (void)a.argsort(-3, true); });
    refused("sort_with_index axis 1 of rank 1", [&] { (void)line.sort_with_index(1); });
    // ---- take
    refused("take_along_axis rank mismatch", [&] { (void)a.take_along_axis(idx1d, 0); });
    refused("take_along_axis axis 2", [&] { (void)a.take_along_axis(idx, 2); });
    refused("take_along_axis axis -3", [&] { (void)a.take_along_axis(idx, -3); });
    refused("take_along_axis shapes do not broadcast", [&] { (void)a.take_along_axis(idx5, 1); });
    refused("take 2-D ids", [&] { (void)a.take(ids2d, 0); });
    refused("take axis 2", [&] { (void)a.take(ids, 2); });
    refused("take_flat 2-D ids", [&] { (void)a.take_flat(ids2d); });
    refused("sm::take axis -3", [&] { (void)sm::take(a, ids, -3); });
    // ---- scatter
    refused("put_along_axis rank mismatch", [&] { a.put_along_axis(idx1d, 1.0f, 0); });
    refused("put_along_axis axis 2", [&] { a.put_along_axis(idx, 1.0f, 2); });
    refused("put_along_axis idx does not match", [&] { a.put_along_axis(idx5, 1.0f, 1); });
    refused("put_along_axis values of higher rank", [&] { a.put_along_axis(idx, a3, 1); });
    refused("put_along_axis values do not broadcast", [&] { a.put_along_axis(idx, line, 1); });
    refused("put_along_axis flat values do not broadcast", [&] { a.put_along_axis(idx, line); });
    refused("put_along_axis onto an axis of 0 elements", [&] { none.put_along_axis(idx, 1.0f, 0); });
    refused("scatter_add rank mismatch", [&] { a.scatter_add(idx1d, a, 0); });
    refused("scatter_add axis -3", [&] { a.scatter_add(idx, a, -3); });
    refused("put 2-D ids", [&] { a.put(ids2d, 1.0f, 0); });
    refused("put axis 2", [&] { a.put(ids, 1.0f, 2); });
    refused("put values do not broadcast", [&] { a.put(ids, line, 0); });
    refused("put_flat 2-D ids", [&] { a.put_flat(ids2d, 1.0f); });
    refused("put_flat 2-D ids, array values", [&] { a.put_flat(ids2d, line); });
    refused("index_add 2-D ids", [&] { a.index_add(ids2d, a, 0); });
    refused("index_add axis -3", [&] { a.index_add(ids, 1.0f, -3); });
    refused("sm::put_along_axis rank mismatch", [&] { sm::put_along_axis(a, idx1d, 1.0f, 0); });
    // ---- counting
    refused("searchsorted 2-D edges", [&] { (void)a.searchsorted(line); });
    refused("bincount -1 bins", [&] { (void)counts.bincount(-1); });
    refused("bincount 0 bins for 4 ids", [&] { (void)counts.bincount(0); });
    refused("histogram 0 bins", [&] { (void)line.histogram(0, 0.0, 1.0); });
    refused("histogram -2 bins", [&] { (void)line.histogram(-2, 0.0, 1.0); });
    refused("histogram lo above hi", [&] { (void)line.histogram(4, 2.0, 1.0); });
    refused("histogram range not finite", [&] { (void)line.histogram(4, 0.0, inf); });
    refused("histogram too many bins for the range", [&] { (void)line.histogram(8, 1.0, 1.0000001); });
    refused("histogram 2-D edges", [&] { (void)line.histogram(a); });
    refused("histogram one edge", [&] { (void)line.histogram(zeros<float>({1})); });
    // ---- where / assign_where / select / conditions
    refused("where a does not broadcast", [&] { (void)sm::where(a > 0.0f, line, 0.0f); });
    refused("where b does not broadcast", [&] { (void)sm::where(a > 0.0f, 1.0f, line); });
    refused("where condition does not broadcast", [&] { (void)sm::where(a > line, 1.0f, 0.0f); });
    refused("mask condition does not broadcast", [&] { (void)sm::mask(a == line); });
    refused("assign_where condition has more axes", [&] { a.assign_where(a3 > 0.0f, 1.0f); });
    refused("assign_where condition does not broadcast", [&] { a.assign_where(line > 0.0f, 1.0f); });
    refused("assign_where values have more axes", [&] { a.assign_where(a > 0.0f, a3); });
    refused("assign_where values do not broadcast", [&] { a.assign_where(a > 0.0f, line); });
    refused("select shapes differ", [&] { (void)a.select(line > 0.0f); });
    refused("select nonzero array of another shape", [&] { (void)a.select(counts); });
    refused("count_nonzero condition does not broadcast", [&] { (void)sm::count_nonzero(a < line); });
    refused("flatnonzero condition does not broadcast", [&] { (void)sm::flatnonzero(a <= line); });
    refused("nonzero condition does not broadcast", [&] { (void)sm::nonzero(a != line); });
    refused("compress axis 2", [&] { (void)sm::compress(line > 0.0f, a, 2); });
    refused("compress condition not as long as the axis", [&] { (void)sm::compress(line > 0.0f, a, 1); });
    refused("compress 2-D condition", [&] { (void)sm::compress(a > 0.0f, a, 0); });
    // ---- sm::expr_sum
    refused("expr_sum 5 scalars", [&] { (void)sm::expr_sum("a0", {1.0f, 2.0f, 3.0f, 4.0f, 5.0f}, a); });
    return 0;
}
