// random.hip -- smhip_random: counter-based draws born in HBM (the definition: sm_random.h; the contract: smhip.h).
//
// One lane computes whole Philox blocks and stores 16 bytes at a time; which elements a lane holds follows from its index
// alone, so the values belong to the element index whatever the grid and wherever `out` starts:
//   4-byte results of 32-bit draws   a unit is 4 elements: one block, one 16-byte store
//   8-byte results of 64-bit draws   a unit is 2 elements: one block, one 16-byte store
//   INTEGERS of i32                  a unit is 4 elements: two blocks, one 16-byte store
//   BERNOULLI of f64 / i64           a unit is 2 elements: two neighbouring lanes compute the same block and store half of it each.
//                                    (First built as one block and two adjacent 16-byte stores per lane: 0.36 of smhip_fill's rate,
//                                    the non-temporal stores with 16-byte holes of convert.hip once more; computing the block twice
//                                    costs nothing that shows, the 4-byte Bernoulli kernels being store-bound with room to spare.)
// The stores need only element alignment (ops.hip.h: vec_t), so an `out` that starts at element 1, 2 or 3 of a larger array
// takes the same kernel and the mapping does not shift.  The last unit of a call, when it is short, is written element by
// element by its lane: nothing past element n - 1 is touched.  Indices are 64-bit; the block number offset + block index
// carries from the low counter word into the high one as a 64-bit sum.  Stores follow the launch's streaming policy, as the
// fill kernel's do.  Workgroups of 256; one launch (2^31 - 1 workgroups are 2^41 elements).
#include <math.h>

#include "internal.h"
#include "ops.hip.h"
#include "sm_random.h"

namespace smhip {
namespace {

using namespace dev;
using smrandom::Params;

constexpr int kBlock = 256;

template <int KIND, typename T>
struct Unit {
    static constexpr int per_block = smrandom::PerBlock<KIND, T>::value;
    static constexpr int size = VecTraits<T>::width;                           // elements per lane: ONE 16-byte store
    static constexpr int blocks = size > per_block ? size / per_block : 1;     // blocks a lane computes
    static constexpr int share = per_block > size ? per_block / size : 1;      // lanes that compute the same block and keep a part each
};

template <int KIND, typename T>
__global__ __launch_bounds__(kBlock) void random_kernel(T *__restrict__ out, size_t n, uint64_t seed, uint64_t stream, uint64_t offset,
                                                        Params<T> p, int pol) {
    typedef Unit<KIND, T> U;
    typedef VecTraits<T> TV;
    const size_t lane = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const size_t e0 = lane * U::size;
    if (e0 >= n) return;
    T v[U::blocks * U::per_block];
    const uint64_t b0 = U::share > 1 ? (uint64_t)lane / U::share : (uint64_t)lane * U::blocks;
#pragma unroll
    for (int b = 0; b < U::blocks; ++b) {
        uint32_t w[4];
        smrandom::block_words(seed, stream, offset + (b0 + b), w);
        smrandom::block_values<KIND, T>(w, p, v + b * U::per_block);
    }
    typename TV::full_t r;
#pragma unroll
    for (int k = 0; k < U::size; ++k) r[k] = v[k];
    if constexpr (U::share == 2) {
        if (lane & 1) {
#pragma unroll
            for (int k = 0; k < U::size; ++k) r[k] = v[U::size + k];
        }
    }
    static_assert(U::share <= 2, "a block is at most two 16-byte stores");
    if (n - e0 >= (size_t)U::size) {
        store_stream_if(T, reinterpret_cast<typename TV::vec_t *>(out + e0), r, pol);
    } else {  // the call's last, short unit
        const int rem = (int)(n - e0);
#pragma unroll
        for (int k = 0; k < U::size; ++k)
            if (k < rem) out[e0 + k] = r[k];
    }
}

template <int KIND, typename T>
int run_random(void *out, size_t n, uint64_t seed, uint64_t stream, uint64_t offset, const Params<T> &p, hipStream_t s) {
    constexpr int US = Unit<KIND, T>::size;  // (e0 = lane * US never wraps: lanes <= n / US + 1)
    const size_t lanes = n / US + (n % US ? 1 : 0);
    const size_t grid = (lanes + kBlock - 1) / kBlock;
    if (grid > 0x7fffffffu) return fail(SMHIP_ERR_UNSUPPORTED, "random: too large");
    T *po = static_cast<T *>(out);
    const int pol = stream_policy({}, {po, n * sizeof(T)});
    hipLaunchKernelGGL((random_kernel<KIND, T>), dim3((unsigned)grid), dim3(kBlock), 0, s, po, n, seed, stream, offset, p, pol);
    SMHIP_LAUNCH_CHECK("random");
    return SMHIP_OK;
}

bool float_dtype(int dtype) { return dtype == SMHIP_F32 || dtype == SMHIP_F64; }

bool valid_pair(int kind, int dtype) {
    if (!valid_dtype(dtype)) return false;
    switch (kind) {
        case SMHIP_RANDOM_BITS: case SMHIP_RANDOM_INTEGERS: return !float_dtype(dtype);
        case SMHIP_RANDOM_UNIFORM: case SMHIP_RANDOM_NORMAL: return float_dtype(dtype);
        case SMHIP_RANDOM_BERNOULLI: return true;
    }
    return false;
}

uint64_t blocks_of(int kind, int dtype, size_t n) {
    const uint64_t per = (uint64_t)smrandom::per_block(kind, (int)dtype_size(dtype));
    return (uint64_t)n / per + ((uint64_t)n % per ? 1 : 0);
}

// The call's parameters, checked and in the element type.  Everything here is host arithmetic.
struct Checked {
    double a = 0, b = 0;
    int64_t lo = 0;
    uint64_t u = 0;
};

int check_call(const char *who, int kind, int dtype, size_t n, uint64_t offset, const double *params, Checked *c) {
    if (!valid_pair(kind, dtype)) return fail(SMHIP_ERR_INVALID, "%s: kind %d of dtype %d is not defined", who, kind, dtype);
    const uint64_t blocks = blocks_of(kind, dtype, n);
    if (offset + blocks < offset) return fail(SMHIP_ERR_INVALID, "%s: offset + blocks passes 2^64", who);
    if (kind == SMHIP_RANDOM_BITS) return SMHIP_OK;
    if (!params) return fail(SMHIP_ERR_INVALID, "%s: null params", who);
    const double x = params[0], y = params[1];
    switch (kind) {
        case SMHIP_RANDOM_UNIFORM: {
            if (!isfinite(x) || !isfinite(y)) return fail(SMHIP_ERR_INVALID, "%s: uniform bounds must be finite", who);
            if (y < x) return fail(SMHIP_ERR_INVALID, "%s: uniform hi < lo", who);
            if (dtype == SMHIP_F32) {
                const float lo = (float)x, hi = (float)y, span = hi - lo;
                if (!isfinite(lo) || !isfinite(hi) || !isfinite(span)) return fail(SMHIP_ERR_INVALID, "%s: uniform bounds beyond float", who);
                c->a = lo, c->b = span;
            } else {
                const double span = y - x;
                if (!isfinite(span)) return fail(SMHIP_ERR_INVALID, "%s: uniform span overflows", who);
                c->a = x, c->b = span;
            }
            return SMHIP_OK;
        }
        case SMHIP_RANDOM_NORMAL: {
            if (!isfinite(x) || !isfinite(y)) return fail(SMHIP_ERR_INVALID, "%s: normal mean / std must be finite", who);
            if (y < 0) return fail(SMHIP_ERR_INVALID, "%s: normal std < 0", who);
            if (dtype == SMHIP_F32 && (!isfinite((float)x) || !isfinite((float)y))) return fail(SMHIP_ERR_INVALID, "%s: normal mean / std beyond float", who);
            c->a = dtype == SMHIP_F32 ? (double)(float)x : x;
            c->b = dtype == SMHIP_F32 ? (double)(float)y : y;
            return SMHIP_OK;
        }
        case SMHIP_RANDOM_INTEGERS: {
            if (!isfinite(x) || !isfinite(y) || x != floor(x) || y != floor(y)) return fail(SMHIP_ERR_INVALID, "%s: integer bounds must be whole numbers", who);
            const double most = dtype == SMHIP_I32 ? 0x1p31 : 0x1p63;
            if (x < -most || y > most) return fail(SMHIP_ERR_INVALID, "%s: integer bounds beyond the element type", who);
            const double range = y - x;  // a difference of whole numbers: exact whenever it is below 2^53
            if (range < 1 || range > 0x1p32) return fail(SMHIP_ERR_INVALID, "%s: integers needs 1 <= hi - lo <= 2^32", who);
            c->lo = (int64_t)x;
            c->u = (uint64_t)range;
            return SMHIP_OK;
        }
        default: {  // BERNOULLI
            if (!(x >= 0.0 && x <= 1.0)) return fail(SMHIP_ERR_INVALID, "%s: bernoulli p outside [0, 1]", who);
            c->u = (uint64_t)floor(x * 0x1p32);  // p = 1: 2^32, above every word
            return SMHIP_OK;
        }
    }
}

template <int KIND, typename T>
int run_checked(void *out, size_t n, uint64_t seed, uint64_t stream, uint64_t offset, const Checked &c, hipStream_t s) {
    Params<T> p;
    p.a = (T)c.a, p.b = (T)c.b, p.lo = c.lo, p.u = c.u;
    return run_random<KIND, T>(out, n, seed, stream, offset, p, s);
}

int launch_random(int kind, int dtype, void *out, size_t n, uint64_t seed, uint64_t stream, uint64_t offset, const Checked &c, hipStream_t s) {
#define SMHIP_RANDOM_CASE(K, D, T) \
    if (kind == SMHIP_RANDOM_##K && dtype == D) return run_checked<smrandom::K, T>(out, n, seed, stream, offset, c, s)
    SMHIP_RANDOM_CASE(BITS, SMHIP_I32, int32_t);
    SMHIP_RANDOM_CASE(BITS, SMHIP_I64, int64_t);
    SMHIP_RANDOM_CASE(UNIFORM, SMHIP_F32, float);
    SMHIP_RANDOM_CASE(UNIFORM, SMHIP_F64, double);
    SMHIP_RANDOM_CASE(INTEGERS, SMHIP_I32, int32_t);
    SMHIP_RANDOM_CASE(INTEGERS, SMHIP_I64, int64_t);
    SMHIP_RANDOM_CASE(BERNOULLI, SMHIP_F32, float);
    SMHIP_RANDOM_CASE(BERNOULLI, SMHIP_F64, double);
    SMHIP_RANDOM_CASE(BERNOULLI, SMHIP_I32, int32_t);
    SMHIP_RANDOM_CASE(BERNOULLI, SMHIP_I64, int64_t);
    SMHIP_RANDOM_CASE(NORMAL, SMHIP_F32, float);
    SMHIP_RANDOM_CASE(NORMAL, SMHIP_F64, double);
#undef SMHIP_RANDOM_CASE
    return fail(SMHIP_ERR_INVALID, "random: kind %d of dtype %d is not defined", kind, dtype);
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_random(int kind, int dtype, void *out, size_t n, uint64_t seed, uint64_t stream, uint64_t offset, const double params[2]) {
    Checked c;
    if (int rc = check_call("random", kind, dtype, n, offset, params, &c)) return rc;
    if (n == 0) return SMHIP_OK;
    if (!out) return fail(SMHIP_ERR_INVALID, "random: null buffer");
    hipStream_t s;
    OpScope op_scope;
    if (int rc = op_scope.begin(nullptr, 0, Span{out, n * dtype_size(dtype)}, &s)) return rc;  // recorded tiny operators are flushed first
    return launch_random(kind, dtype, out, n, seed, stream, offset, c, s);
}

int smhip_random_blocks(int kind, int dtype, size_t n, uint64_t *blocks) {
    if (!valid_pair(kind, dtype)) return fail(SMHIP_ERR_INVALID, "random_blocks: kind %d of dtype %d is not defined", kind, dtype);
    if (!blocks) return fail(SMHIP_ERR_INVALID, "random_blocks: null output");
    *blocks = blocks_of(kind, dtype, n);
    return SMHIP_OK;
}
