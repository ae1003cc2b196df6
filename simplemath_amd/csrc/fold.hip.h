// fold.hip.h -- the folds of reduce_axis.hip (axis reductions) and scan_axis.hip (cumulative scans): the accumulator a fold
// runs in, the fold itself, its identity, and the conversions into and out of the accumulator.
//   sum / prod   f32, f64: fp64;  i32, i64: uint64_t -- wrapping, exact modulo 2^64 and hence modulo the type's width
//   max / min    the element type; a NaN on either side propagates
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <limits>
#include <type_traits>

namespace smhip {
namespace dev {

enum FoldKind { kSum = 0, kProd = 1, kMax = 2, kMin = 3 };  // the reductions' mean = kSum and a divisor at the last launch

template <typename T, int K> struct Acc { typedef T type; };
template <> struct Acc<float, kSum> { typedef double type; };
template <> struct Acc<double, kSum> { typedef double type; };
template <> struct Acc<int32_t, kSum> { typedef uint64_t type; };  // wrapping: exact modulo 2^64, hence modulo 2^32
template <> struct Acc<int64_t, kSum> { typedef uint64_t type; };
template <> struct Acc<float, kProd> { typedef double type; };
template <> struct Acc<double, kProd> { typedef double type; };
template <> struct Acc<int32_t, kProd> { typedef uint64_t type; };
template <> struct Acc<int64_t, kProd> { typedef uint64_t type; };

template <typename A, int K> __device__ __forceinline__ A fold(A x, A y) {
    if constexpr (K == kSum) return x + y;
    else if constexpr (K == kProd) return x * y;
    else if constexpr (K == kMax) {
        if constexpr (std::is_floating_point<A>::value) return (x > y || x != x) ? x : y;  // NaN in either propagates
        else return x > y ? x : y;
    } else {
        if constexpr (std::is_floating_point<A>::value) return (x < y || x != x) ? x : y;
        else return x < y ? x : y;
    }
}
template <typename A, int K> __device__ __forceinline__ A identity() {
    if constexpr (K == kSum) return A(0);
    else if constexpr (K == kProd) return A(1);
    else if constexpr (K == kMax) return std::is_floating_point<A>::value ? -std::numeric_limits<A>::infinity() : std::numeric_limits<A>::lowest();
    else return std::is_floating_point<A>::value ? std::numeric_limits<A>::infinity() : std::numeric_limits<A>::max();
}
template <typename TI, typename A> __device__ __forceinline__ A widen(TI x) {
    if constexpr (std::is_integral<TI>::value && std::is_unsigned<A>::value) return (A)(int64_t)x;  // sign-extended, then wrapping
    else return (A)x;
}
// The accumulator to the launch's output type; `divisor` > 0: the mean's one division (fp64), then one rounding.
template <typename TO, typename A> __device__ __forceinline__ TO finish(A acc, double divisor) {
    if constexpr (std::is_integral<TO>::value) return (TO)(int64_t)acc;  // the wrapped residue
    else if constexpr (std::is_same<A, double>::value) return divisor > 0.0 ? (TO)(acc / divisor) : (TO)acc;
    else return (TO)acc;
}

// Four consecutive elements at any element-aligned address (gfx950 takes 16- and 32-byte accesses there).
template <typename T> struct Quad { typedef T type __attribute__((ext_vector_type(4), aligned(sizeof(T)))); };

}  // namespace dev
}  // namespace smhip
