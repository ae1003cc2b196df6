// tools/sweep_widen.hip -- what limits a 4-byte -> 8-byte conversion stream (astype f32 -> f64, csrc/convert.hip)?  The same 12 bytes per
// element moved five ways over 2^26 and 2^28 floats, workgroups of 256, non-temporal accesses unless said otherwise:
//   A  one 16-byte load, two ADJACENT 16-byte stores per lane (convert.hip's DENSE): a store instruction writes 16 bytes of every 32
//   B  one 8-byte load, one 16-byte store per lane: every store instruction writes 1 KiB without holes; the load side is 8-byte accesses
//   C  B twice per lane, the two halves 64 lanes apart (as much work per lane as A, stores without holes)
//   D  A with the middle vectors of neighbouring lanes exchanged (DPP), so that a store instruction writes 32 bytes of every 64
//   E  A with plain stores
// Development tool: prints time, GB/s and a check of the last elements.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1); } } while (0)
typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef double d2 __attribute__((ext_vector_type(2)));
typedef int i4 __attribute__((ext_vector_type(4)));
constexpr int kBlock = 256;

__global__ __launch_bounds__(kBlock) void kA(const float *__restrict__ a, double *__restrict__ o, size_t n4) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n4) return;
    const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(a) + i);
    d2 *p = reinterpret_cast<d2 *>(o) + 2 * i;
    __builtin_nontemporal_store((d2){(double)v[0], (double)v[1]}, p);
    __builtin_nontemporal_store((d2){(double)v[2], (double)v[3]}, p + 1);
}
__global__ __launch_bounds__(kBlock) void kE(const float *__restrict__ a, double *__restrict__ o, size_t n4) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n4) return;
    const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(a) + i);
    d2 *p = reinterpret_cast<d2 *>(o) + 2 * i;
    p[0] = (d2){(double)v[0], (double)v[1]};
    p[1] = (d2){(double)v[2], (double)v[3]};
}
__global__ __launch_bounds__(kBlock) void kB(const float *__restrict__ a, double *__restrict__ o, size_t n2) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n2) return;
    const f2 v = __builtin_nontemporal_load(reinterpret_cast<const f2 *>(a) + i);
    __builtin_nontemporal_store((d2){(double)v[0], (double)v[1]}, reinterpret_cast<d2 *>(o) + i);
}
__global__ __launch_bounds__(kBlock) void kC(const float *__restrict__ a, double *__restrict__ o, size_t n4) {  // n4 a multiple of 64
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n4) return;
    const size_t j = (i & ~(size_t)63) * 2 + (i & 63);  // this wave's 128 pairs: lane l takes pairs l and 64 + l
    const f2 v0 = __builtin_nontemporal_load(reinterpret_cast<const f2 *>(a) + j), v1 = __builtin_nontemporal_load(reinterpret_cast<const f2 *>(a) + j + 64);
    __builtin_nontemporal_store((d2){(double)v0[0], (double)v0[1]}, reinterpret_cast<d2 *>(o) + j);
    __builtin_nontemporal_store((d2){(double)v1[0], (double)v1[1]}, reinterpret_cast<d2 *>(o) + j + 64);
}
__device__ __forceinline__ d2 swap_neighbour(d2 x) {
    i4 b = __builtin_bit_cast(i4, x);
#pragma unroll
    for (int k = 0; k < 4; ++k) b[k] = __builtin_amdgcn_mov_dpp(b[k], 0xB1, 0xf, 0xf, true);  // quad_perm [1, 0, 3, 2]
    return __builtin_bit_cast(d2, b);
}
__global__ __launch_bounds__(kBlock) void kD(const float *__restrict__ a, double *__restrict__ o, size_t n4) {  // n4 even
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n4) return;
    const f4 v = __builtin_nontemporal_load(reinterpret_cast<const f4 *>(a) + i);
    const d2 w0 = {(double)v[0], (double)v[1]}, w1 = {(double)v[2], (double)v[3]};
    const bool odd = i & 1;
    const d2 got = swap_neighbour(odd ? w0 : w1);
    d2 *p = reinterpret_cast<d2 *>(o) + 4 * (i >> 1) + (odd ? 1 : 0);
    __builtin_nontemporal_store(odd ? got : w0, p);
    __builtin_nontemporal_store(odd ? w1 : got, p + 2);
}
__global__ void init_k(float *p, size_t n) { for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = (float)(i % 100003) * 0.25f; }

int main() {
    for (int log2n : {26, 28}) {
        const size_t n = (size_t)1 << log2n;
        float *A; double *O;
        CK(hipMalloc(&A, n * 4)); CK(hipMalloc(&O, n * 8));
        init_k<<<4096, 256>>>(A, n); CK(hipDeviceSynchronize());
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        struct { const char *name; void (*k)(const float *, double *, size_t); size_t lanes; } rows[] = {
            {"A 16B load, 2 adjacent 16B stores", kA, n / 4}, {"B 8B load, 16B store", kB, n / 2}, {"C 2 x (8B load, 16B store)", kC, n / 4},
            {"D A + neighbour exchange", kD, n / 4}, {"E A with plain stores", kE, n / 4}};
        for (int round = 0; round < 2; ++round)
            for (auto &r : rows) {
                CK(hipMemset(O, 0, n * 8));
                const unsigned grid = (unsigned)(r.lanes / kBlock);
                for (int w = 0; w < 5; ++w) r.k<<<grid, kBlock>>>(A, O, r.lanes);
                CK(hipEventRecord(e0));
                for (int k = 0; k < 20; ++k) r.k<<<grid, kBlock>>>(A, O, r.lanes);
                CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
                float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= 20;
                std::vector<double> h(1024); std::vector<float> ha(1024);
                bool ok = true;
                for (size_t at : {(size_t)0, n / 2 - 512, n - 1024}) {
                    CK(hipMemcpy(h.data(), O + at, 8192, hipMemcpyDeviceToHost)); CK(hipMemcpy(ha.data(), A + at, 4096, hipMemcpyDeviceToHost));
                    for (int k = 0; k < 1024; ++k) ok &= h[k] == (double)ha[k];
                }
                printf("2^%d  %-36s %8.1f us %7.1f GB/s  %s\n", log2n, r.name, ms * 1e3, 12.0 * n / ms * 1e-6, ok ? "ok" : "MISMATCH");
            }
        CK(hipFree(A)); CK(hipFree(O));
    }
    return 0;
}
