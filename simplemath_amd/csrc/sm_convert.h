// sm_convert.h -- the element type conversions behind astype, shared by the gfx950 kernels (convert.hip) and, compiled for the
// host by tests/cpp/convert_host_check.cpp, by the CPU check of the rules themselves.
//
// One function per ordered pair of {f32, f64, i32, i64} (smhip.h has the table):
//   integer -> integer   sign extension / the low 32 bits (wraps, as numpy)
//   integer -> float     round to nearest, ties to even, rounded ONCE.  i32 -> f32 / f64 and i64 -> f64 are the language's
//                        conversion (v_cvt_f32_i32, v_cvt_f64_i32, and hi * 2^32 + lo with one rounding in the add);
//                        i64 -> f32 is written out below: through double it would round twice (2^60 + 2^36 + 1 -> 2^60
//                        instead of 2^60 + 2^37).
//   float -> float       f32 -> f64 exact (subnormals and -0 kept); f64 -> f32 round to nearest even, overflow to +-inf,
//                        correct subnormals
//   float -> integer     saturating truncation: toward zero; beyond the target's range its min / max; NaN gives 0 (Rust's
//                        `as`, Java, WebAssembly's trunc_sat -- and what v_cvt_i32_f32 / v_cvt_i32_f64 do).  The range
//                        tests are written out and the cast itself only ever sees a value whose truncation fits: an
//                        out-of-range cast is undefined in C++, and the host and device compilers differ on it.
#pragma once

#include <stdint.h>
#include <string.h>

#include <type_traits>

#if defined(__HIPCC__)
#define SM_CVT_FN __host__ __device__ __forceinline__
#else
#define SM_CVT_FN static inline
#endif

namespace smconvert {

SM_CVT_FN int clz64(uint64_t u) {  // u != 0
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)u);
#else
    return __builtin_clzll(u);
#endif
}

// -------------------------------------------------------------------------------------------------- integer -> integer
SM_CVT_FN int64_t i32_to_i64(int32_t x) { return (int64_t)x; }
SM_CVT_FN int32_t i64_to_i32(int64_t x) {
    const uint32_t lo = (uint32_t)(uint64_t)x;
    int32_t r;
    memcpy(&r, &lo, 4);
    return r;
}

// ---------------------------------------------------------------------------------------------------- integer -> float
SM_CVT_FN double i32_to_f64(int32_t x) { return (double)x; }
SM_CVT_FN float i32_to_f32(int32_t x) { return (float)x; }
SM_CVT_FN double i64_to_f64(int64_t x) { return (double)x; }
// |x| normalised to 64 bits; its top 32 with everything below them folded into bit 0 (a sticky bit: the float keeps 24 bits, so
// the rounding bit is bit 7 and bits 0-6 only say "more below") convert in ONE rounding; the power of two that puts the
// value back is exact.
SM_CVT_FN float i64_to_f32(int64_t x) {
    if (x == 0) return 0.0f;
    const bool neg = x < 0;
    const uint64_t u = neg ? 0ull - (uint64_t)x : (uint64_t)x;
    const int lz = clz64(u);
    const uint64_t norm = u << lz;
    const uint32_t top = (uint32_t)(norm >> 32) | ((uint32_t)norm != 0u ? 1u : 0u);
    const float m = (float)top;  // in [2^31, 2^32]
    const uint32_t scale_bits = (uint32_t)(127 + 32 - lz) << 23;  // 2^(32 - lz), lz in 0..63
    float scale;
    memcpy(&scale, &scale_bits, 4);
    const float r = m * scale;
    return neg ? -r : r;
}

// ------------------------------------------------------------------------------------------------------ float -> float
SM_CVT_FN double f32_to_f64(float x) { return (double)x; }
SM_CVT_FN float f64_to_f32(double x) { return (float)x; }

// ---------------------------------------------------------------------------------------------------- float -> integer
// 2^31 and 2^63 are exact in both float types; x <= -2^31 (-2^63) truncates to the minimum or lies beyond it, so the
// minimum is the answer either way, and what reaches the cast satisfies -2^31 < x < 2^31 (-2^63 < x < 2^63).
SM_CVT_FN int32_t f32_to_i32(float x) {
    if (x != x) return 0;
    if (x >= 2147483648.0f) return INT32_MAX;
    if (x <= -2147483648.0f) return INT32_MIN;
    return (int32_t)x;
}
SM_CVT_FN int32_t f64_to_i32(double x) {
    if (x != x) return 0;
    if (x >= 2147483648.0) return INT32_MAX;
    if (x <= -2147483648.0) return INT32_MIN;
    return (int32_t)x;
}
SM_CVT_FN int64_t f32_to_i64(float x) {
    if (x != x) return 0;
    if (x >= 9223372036854775808.0f) return INT64_MAX;
    if (x <= -9223372036854775808.0f) return INT64_MIN;
    return (int64_t)x;
}
SM_CVT_FN int64_t f64_to_i64(double x) {
    if (x != x) return 0;
    if (x >= 9223372036854775808.0) return INT64_MAX;
    if (x <= -9223372036854775808.0) return INT64_MIN;
    return (int64_t)x;
}

// convert<D>(x): the function of the pair (S, D); the identity for S == D.
template <typename D, typename S>
SM_CVT_FN D convert(S x) {
    if constexpr (std::is_same<S, D>::value) return x;
    else if constexpr (std::is_same<S, int32_t>::value && std::is_same<D, int64_t>::value) return i32_to_i64(x);
    else if constexpr (std::is_same<S, int64_t>::value && std::is_same<D, int32_t>::value) return i64_to_i32(x);
    else if constexpr (std::is_same<S, int32_t>::value && std::is_same<D, float>::value) return i32_to_f32(x);
    else if constexpr (std::is_same<S, int32_t>::value && std::is_same<D, double>::value) return i32_to_f64(x);
    else if constexpr (std::is_same<S, int64_t>::value && std::is_same<D, float>::value) return i64_to_f32(x);
    else if constexpr (std::is_same<S, int64_t>::value && std::is_same<D, double>::value) return i64_to_f64(x);
    else if constexpr (std::is_same<S, float>::value && std::is_same<D, double>::value) return f32_to_f64(x);
    else if constexpr (std::is_same<S, double>::value && std::is_same<D, float>::value) return f64_to_f32(x);
    else if constexpr (std::is_same<S, float>::value && std::is_same<D, int32_t>::value) return f32_to_i32(x);
    else if constexpr (std::is_same<S, float>::value && std::is_same<D, int64_t>::value) return f32_to_i64(x);
    else if constexpr (std::is_same<S, double>::value && std::is_same<D, int32_t>::value) return f64_to_i32(x);
    else {
        static_assert(std::is_same<S, double>::value && std::is_same<D, int64_t>::value, "convert: float, double, int32_t and int64_t");
        return f64_to_i64(x);
    }
}

}  // namespace smconvert
