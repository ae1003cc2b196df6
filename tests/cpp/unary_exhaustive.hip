// tests/cpp/unary_exhaustive.hip -- exp, log or sqrt through smhip_unary for EVERY float bit pattern (2^32: both signs,
// denormals, infinities, NaNs) against the device libm's fp64 exp / log / sqrt of the argument rounded to f32 (the fp64 value
// is within 1 ULP of fp64, i.e. 2^-29 ULP of f32: "0 ULP" below means correctly rounded except possibly at a near-tie).
// A NaN must meet a NaN; zeros must agree in sign.  Prints the ULP-error histogram and the largest error in (real-valued) f32
// ULPs of the fp64 value; exit status 1 when anything is beyond 1 ULP (sqrt: beyond 0).  Usage: unary_exhaustive exp|log|sqrt.
// Built by simplemath_amd/build.py (hipcc) into simplemath_amd/bin/unary_exhaustive; run by tests/test_unary_cpp.py.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "smhip.h"
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)
#define SK(x) do { if ((x) < 0) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, smhip_last_error()); exit(1); } } while (0)

__global__ void fill_bits(float* p, unsigned first, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = __uint_as_float(first + (unsigned)i);
}
// sign-magnitude bits -> a number line on which neighbouring floats differ by one (+0 and -0 are told apart by the caller)
__device__ long long ordered(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? -(long long)(u & 0x7fffffffu) : (long long)u;
}
__global__ void check(const float* x, const float* r, size_t n, int fn, unsigned long long* hist, unsigned* worst_bits, unsigned long long* max_err_bits) {
    unsigned long long h0 = 0, h1 = 0, h2 = 0, h3 = 0;
    double worst_err = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const double xd = (double)x[i];
        const double ref = fn == SMHIP_UNARY_EXP ? exp(xd) : (fn == SMHIP_UNARY_LOG ? log(xd) : sqrt(xd));
        const float rf = (float)ref, got = r[i];
        long long d;
        if (rf != rf || got != got) d = (rf != rf && got != got) ? 0 : 1000;                                            // NaN meets NaN
        else if (rf == 0.0f && got == 0.0f) d = (__float_as_uint(rf) == __float_as_uint(got)) ? 0 : 1000;              // the same zero
        else { d = ordered(got) - ordered(rf); d = d < 0 ? -d : d; }                                                    // (inf is the grid point after FLT_MAX)
        if (rf == rf && got == got && ref != 0.0 && !isinf(ref)) {  // |got - ref| in units of the f32 grid's spacing at ref
            int e = ilogb(ref);
            e = e < -126 ? -126 : e;
            const double g = isinf(got) ? copysign(0x1p128, (double)got) : (double)got, top = 0x1p128;
            const double w = ref > top ? top : (ref < -top ? -top : ref);
            const double err = ldexp(fabs(g - w), 23 - e);
            worst_err = err > worst_err ? err : worst_err;
        }
        if (d == 0) ++h0; else if (d == 1) ++h1; else if (d == 2) ++h2; else { ++h3; atomicMax(worst_bits, __float_as_uint(x[i])); }
    }
    atomicAdd(&hist[0], h0); atomicAdd(&hist[1], h1); atomicAdd(&hist[2], h2); atomicAdd(&hist[3], h3);
    atomicMax(max_err_bits, (unsigned long long)__double_as_longlong(worst_err));  // non-negative doubles are ordered like their bits
}
int main(int argc, char** argv) {
    const char* name = argc > 1 ? argv[1] : "exp";
    const int fn = !strcmp(name, "exp") ? SMHIP_UNARY_EXP : !strcmp(name, "log") ? SMHIP_UNARY_LOG : !strcmp(name, "sqrt") ? SMHIP_UNARY_SQRT : -1;
    if (fn < 0) { fprintf(stderr, "usage: %s exp|log|sqrt\n", argv[0]); return 2; }
    const size_t chunk = (size_t)1 << 28, total = (size_t)1 << 32;
    void *x, *r; SK(smhip_alloc(&x, chunk * 4)); SK(smhip_alloc(&r, chunk * 4));
    unsigned long long* hist; unsigned* worst; CK(hipMalloc(&hist, 32)); CK(hipMalloc(&worst, 4)); CK(hipMemset(hist, 0, 32)); CK(hipMemset(worst, 0, 4));
    unsigned long long* max_err; CK(hipMalloc(&max_err, 8)); CK(hipMemset(max_err, 0, 8));
    const int64_t one = 1, shape = (int64_t)chunk;
    for (size_t lo = 0; lo < total; lo += chunk) {
        fill_bits<<<4096, 256>>>((float*)x, (unsigned)lo, chunk);
        CK(hipDeviceSynchronize());
        SK(smhip_unary(fn, SMHIP_F32, x, &one, &shape, 1, r));
        SK(smhip_synchronize());
        check<<<4096, 256>>>((const float*)x, (const float*)r, chunk, fn, hist, worst, max_err);
        CK(hipDeviceSynchronize());
    }
    unsigned long long h[4]; unsigned w; CK(hipMemcpy(h, hist, 32, hipMemcpyDeviceToHost)); CK(hipMemcpy(&w, worst, 4, hipMemcpyDeviceToHost));
    const double tot = (double)(h[0] + h[1] + h[2] + h[3]);
    printf("%s(x) over all %llu float bit patterns: 0 ULP %llu (%.4f %%)  1 ULP %llu (%.4f %%)  2 ULP %llu  >2 ULP %llu\n", name,
           h[0] + h[1] + h[2] + h[3], h[0], 100.0 * h[0] / tot, h[1], 100.0 * h[1] / tot, h[2], h[3]);
    if (h[3]) printf("largest x bits beyond 2 ULP: 0x%08x\n", w);
    double err; CK(hipMemcpy(&err, max_err, 8, hipMemcpyDeviceToHost));
    printf("largest error against the fp64 value: %.4f ULP\n", err);
    const bool bad = h[2] || h[3] || (fn == SMHIP_UNARY_SQRT && h[1]) || err > 1.0;
    return bad ? 1 : 0;
}
