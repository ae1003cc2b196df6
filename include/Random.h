// Random.h -- sm::Generator: counter-based random draws born in HBM (smhip_random; smhip.h has the definition and the table).
//
//     sm::Generator g(42);                                   // (seed, stream = 0)
//     auto x      = g.uniform<float>(512, 1000);             // [0, 1), dims as in sm::ones
//     auto w      = g.normal<float>(64, 64) * 0.02f;         // standard normal; the scale is one chain launch
//     auto labels = g.integers<std::int64_t>(0, 1000, 512);  // [lo, hi)
//     auto keep   = g.bernoulli<float>(0.9, 512, 1000);
//     auto y      = x * keep / 0.9f;                         // dropout: the mask feeds one chain launch
//
// Element i of a draw is a pure function of (seed, stream, position, i): the bits do not depend on the run, the queue or the grid,
// and tests/random_model.py reproduces them on the CPU.  Each call advances the generator's position by the blocks it consumed
// (smhip_random_blocks), so a program's draws are reproducible and a draw does not depend on how the elements before it were split
// into calls: two calls of 1024 floats equal one call of 2048.  offset() / seek(blocks) expose the position.  Results are device-born
// (no host mirror is touched) and feed the next chain like any array.  The element type is float, double, int or std::int64_t;
// uniform and normal are defined for the two float types, integers and bits for the two integer types, bernoulli for all four.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "SMArray.h"

namespace sm {

class Generator {
public:
    explicit Generator(std::uint64_t seed, std::uint64_t stream = 0) : seed_(seed), stream_(stream) {}

    std::uint64_t seed() const { return seed_; }
    std::uint64_t stream() const { return stream_; }
    // The position: the number of the next Philox block.  seek(p) puts the generator there; a draw made from a position is the same
    // draw every time.
    std::uint64_t offset() const { return offset_; }
    void seek(std::uint64_t blocks) { offset_ = blocks; }

    // New dense arrays of shape {dims...}.
    template <typename T, typename... Dims>
    SMArray<T> uniform(Dims... dims) {  // [0, 1)
        static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "Generator::uniform<T>: T must be float or double");
        return born<T>(SMHIP_RANDOM_UNIFORM, 0.0, 1.0, dims...);
    }
    template <typename T, typename... Dims>
    SMArray<T> normal(Dims... dims) {  // mean 0, standard deviation 1
        static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "Generator::normal<T>: T must be float or double");
        return born<T>(SMHIP_RANDOM_NORMAL, 0.0, 1.0, dims...);
    }
    template <typename T, typename... Dims>
    SMArray<T> integers(std::int64_t lo, std::int64_t hi, Dims... dims) {  // [lo, hi), 1 <= hi - lo <= 2^32
        static_assert(std::is_same_v<T, int> || std::is_same_v<T, std::int64_t>, "Generator::integers<T>: T must be int or std::int64_t");
        return born<T>(SMHIP_RANDOM_INTEGERS, whole(lo), whole(hi), dims...);
    }
    template <typename T, typename... Dims>
    SMArray<T> bernoulli(double p, Dims... dims) {  // 1 with probability p, else 0
        static_assert(four_types<T>, "Generator::bernoulli<T>: T must be float, double, int or std::int64_t");
        return born<T>(SMHIP_RANDOM_BERNOULLI, p, 0.0, dims...);
    }
    template <typename T, typename... Dims>
    SMArray<T> bits(Dims... dims) {  // every bit pattern of T equally likely
        static_assert(std::is_same_v<T, int> || std::is_same_v<T, std::int64_t>, "Generator::bits<T>: T must be int or std::int64_t");
        return born<T>(SMHIP_RANDOM_BITS, 0.0, 0.0, dims...);
    }

    // The same draws written in place into a dense array (a row of a matrix, a whole array), the parameters applied inside the
    // kernel.  A target that is not dense throws std::invalid_argument; a chain still pending on it is evaluated first.
    template <typename T>
    void fill_uniform(SMArray<T> &a, T lo, T hi) {
        static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "Generator::fill_uniform: float or double arrays");
        into(SMHIP_RANDOM_UNIFORM, a, static_cast<double>(lo), static_cast<double>(hi));
    }
    template <typename T>
    void fill_normal(SMArray<T> &a, T mean, T std_dev) {
        static_assert(std::is_same_v<T, float> || std::is_same_v<T, double>, "Generator::fill_normal: float or double arrays");
        into(SMHIP_RANDOM_NORMAL, a, static_cast<double>(mean), static_cast<double>(std_dev));
    }
    template <typename T>
    void fill_integers(SMArray<T> &a, std::int64_t lo, std::int64_t hi) {
        static_assert(std::is_same_v<T, int> || std::is_same_v<T, std::int64_t>, "Generator::fill_integers: int or std::int64_t arrays");
        into(SMHIP_RANDOM_INTEGERS, a, whole(lo), whole(hi));
    }
    template <typename T>
    void fill_bernoulli(SMArray<T> &a, double p) {
        static_assert(four_types<T>, "Generator::fill_bernoulli: float, double, int or std::int64_t arrays");
        into(SMHIP_RANDOM_BERNOULLI, a, p, 0.0);
    }

    // A random order of 0 .. n - 1: the stable argsort of n 64-bit keys, so it is the same order even where two keys tie.  From
    // 2^31 elements on it throws what sort_flat throws.
    SMArray<std::int64_t> permutation(std::size_t n) { return bits<std::int64_t>(n).argsort_flat(); }
    // x with its slices along `axis` in a random order: take(x, permutation(x.shape()[axis]), axis).
    template <typename T>
    SMArray<T> shuffle(const SMArray<T> &x, int axis = 0) {
        const int nd = static_cast<int>(x.shape().size()), ax = axis < 0 ? axis + nd : axis;
        if (ax < 0 || ax >= nd) throw std::invalid_argument("simpleMath/MI355X: shuffle: axis " + std::to_string(axis) + " of an array of rank " + std::to_string(nd));
        return x.take(permutation(x.shape()[static_cast<std::size_t>(ax)]), ax, index_mode::clip);  // the positions are valid by construction
    }

private:
    template <typename T>
    static constexpr bool four_types = std::is_same_v<T, float> || std::is_same_v<T, double> || std::is_same_v<T, int> || std::is_same_v<T, std::int64_t>;

    // smhip_random takes INTEGERS' bounds as doubles that hold whole numbers exactly.
    static double whole(std::int64_t v) {
        const double d = static_cast<double>(v);
        if (d >= 0x1p63 || static_cast<std::int64_t>(d) != v) throw std::invalid_argument("simpleMath/MI355X: Generator: the bound " + std::to_string(v) + " is not a whole number of a double");
        return d;
    }

    template <typename T>
    void run(int kind, T *out, std::size_t n, double a, double b) {
        const double params[2] = {a, b};
        std::uint64_t blocks = 0;
        hip::check(smhip_random_blocks(kind, hip::dtype_of<T>::id, n, &blocks));
        hip::check(smhip_random(kind, hip::dtype_of<T>::id, out, n, seed_, stream_, offset_, params));
        offset_ += blocks;
    }

    template <typename T, typename... Dims>
    SMArray<T> born(int kind, double a, double b, Dims... dims) {
        SMArray<T> out = SMArray<T>::device_empty({static_cast<std::size_t>(dims)...});
        hip::DeviceGuard on(out.device());
        run<T>(kind, out.totalSize ? out.device_data_mut() : nullptr, out.totalSize, a, b);
        return out;
    }

    template <typename T>
    void into(int kind, SMArray<T> &a, double p0, double p1) {
        if (!a.is_dense()) throw std::invalid_argument("simpleMath/MI355X: Generator::fill_*: the target must be dense (fill a dense array and assign it to the view)");
        hip::DeviceGuard on(a.device());
        T *out = nullptr;
        if (a.totalSize) out = a.is_view() ? a.data.storage()->dev_rw() + a.data.offset() : a.device_data_mut();  // a view: the rest of its parent stays
        run<T>(kind, out, a.totalSize, p0, p1);
    }

    std::uint64_t seed_, stream_, offset_ = 0;
};

}  // namespace sm
