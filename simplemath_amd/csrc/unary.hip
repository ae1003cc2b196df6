// unary.hip -- functions of one argument: out = f(a), f in {neg, abs, sqrt, exp, log} (smhip_unary).
//
// The reference has none of these (its README's "Important Note" names vector exp / log as wanted and missing).
//
// Dense operands: one 16-byte vector per lane, one read and one write stream -- contiguous.hip's array-scalar kernel with
// the Op's second operand gone: workgroups of 256, the launch's streaming policy (internal.h: stream_policy), arrays above
// 256 MiB in pieces of 256 MiB.  2 * sizeof(T) bytes per element; roofline: HBM.  The three functions that look a table up
// in LDS (f32 log, f64 exp and log) go through pow's tile kernel instead (launch_unary_dense below).
// Views (transposed, stepped, broadcast): NEG / ABS / SQRT go through the broadcast kernels as Ops whose apply(a, b) ignores
// b, exactly as SMHIP_OP_LEFT does -- the view is read in place by the tile / strided-row / gather kernels, 2 * sizeof(T)
// bytes per element.  EXP / LOG of a view run as LEFT into the (dense) output followed by the dense kernel in place,
// 4 * sizeof(T) bytes per element: five more Ops through every broadcast kernel was too much code for the rarer case.
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "internal.h"
#include "ops.hip.h"

namespace smhip {
namespace {

using namespace dev;

constexpr int kBlock = 256;
constexpr size_t kPieceVec = (size_t)1 << 24;  // 256 MiB per operand

template <typename T, typename Op>
__global__ __launch_bounds__(kBlock) void unary_vec_kernel(const T *a, T *out, size_t n_vec, int tail, int pol) {
    typedef typename VecTraits<T>::vec_t V;
    constexpr int W = VecTraits<T>::width;
    OpCtx<Op> ctx;  // (no __restrict__: out may BE a, each element read before it is written by the same lane)
    ctx.init();
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < n_vec) {
        const V va = load_stream_if(T, reinterpret_cast<const V *>(a) + i, pol);
        store_stream_if(T, reinterpret_cast<V *>(out) + i, (apply_vec<Op, T>(ctx, va, va)), pol);
    } else if (i == n_vec) {  // the n % W elements past the last whole vector: the first lane past the body
        for (int k = 0; k < tail; ++k) {
            const T x = a[n_vec * W + k];
            out[n_vec * W + k] = Op::apply(x, x);
        }
    }
}

template <typename T, typename Op>
int run_dense(const void *a, void *out, size_t n, hipStream_t s) {
    constexpr int W = VecTraits<T>::width;
    const T *pa = static_cast<const T *>(a);
    T *po = static_cast<T *>(out);
    const size_t n_vec = n / W;
    const int tail = (int)(n % W);
    const int pol = stream_policy({{pa, n * sizeof(T)}}, {po, n * sizeof(T)});
    size_t piece = piece_for(n_vec, 2);  // honours SMHIP_PIECE_LOG2VEC (tests run the piece loop at small sizes)
    if (piece == 0 || piece > kPieceVec) piece = kPieceVec;
    for (size_t v0 = 0;; v0 += piece) {
        const bool last = v0 + piece >= n_vec;
        const size_t nv = last ? n_vec - v0 : piece;
        const size_t threads = nv + (last && tail ? 1 : 0);
        const size_t grid = (threads + kBlock - 1) / kBlock;  // <= 2^24 / 256 + 1
        if (grid) hipLaunchKernelGGL((unary_vec_kernel<T, Op>), dim3((unsigned)grid), dim3(kBlock), 0, s, pa + v0 * W, po + v0 * W, nv, last ? tail : 0, pol);
        if (last) break;
    }
    SMHIP_LAUNCH_CHECK("unary");
    return SMHIP_OK;
}

template <typename T>
int run_dense_fn(int fn, const void *a, void *out, size_t n, hipStream_t s) {
    switch (fn) {
        case SMHIP_UNARY_NEG: return run_dense<T, NegOp<T>>(a, out, n, s);
        case SMHIP_UNARY_ABS: return run_dense<T, AbsOp<T>>(a, out, n, s);
    }
    if constexpr (std::is_floating_point<T>::value) {
        switch (fn) {
            case SMHIP_UNARY_SQRT: return run_dense<T, SqrtOp<T>>(a, out, n, s);
            case SMHIP_UNARY_EXP: return run_dense<T, ExpOp<T>>(a, out, n, s);
            case SMHIP_UNARY_LOG: return run_dense<T, LogOp<T>>(a, out, n, s);
        }
    }
    return fail(SMHIP_ERR_UNSUPPORTED, "unary: function %d is not defined for an integer element type", fn);
}

}  // namespace

int launch_unary_dense(int fn, int dtype, const void *a, size_t n, void *out, hipStream_t s) {
    if (n == 0) return SMHIP_OK;
    // The functions that look a table up in LDS take pow's tile kernel from 2^16 elements on (contiguous.hip:
    // launch_unary_tiles): with one vector per lane every 4 KiB of data paid for staging 2-5 KiB of table -- the f64 exp / log ran
    // at 57 % of HBM peak, the f32 log at 68 % (profiles/unary_rates.txt has both forms).  The same Op, the same bits.
    const bool table = (dtype == SMHIP_F32 && fn == SMHIP_UNARY_LOG) || (dtype == SMHIP_F64 && (fn == SMHIP_UNARY_EXP || fn == SMHIP_UNARY_LOG));
    if (table && n >= ((size_t)1 << 16)) return launch_unary_tiles(fn, dtype, a, n, out, s);
    switch (dtype) {
        case SMHIP_F32: return run_dense_fn<float>(fn, a, out, n, s);
        case SMHIP_F64: return run_dense_fn<double>(fn, a, out, n, s);
        case SMHIP_I32: return run_dense_fn<int32_t>(fn, a, out, n, s);
        case SMHIP_I64: return run_dense_fn<int64_t>(fn, a, out, n, s);
    }
    return fail(SMHIP_ERR_INVALID, "unary: bad dtype %d", dtype);
}

int launch_unary(int fn, int dtype, const void *a, const int64_t *strides, const int64_t *shape, int ndim, void *out, hipStream_t s) {
    size_t n = 1;
    for (int d = 0; d < ndim; ++d) n *= (size_t)shape[d];
    if (n == 0) return SMHIP_OK;
    if (axis_plan::row_major(shape, strides, ndim)) return launch_unary_dense(fn, dtype, a, n, out, s);
    const int64_t zero[SMHIP_MAX_NDIM] = {};
    if (fn == SMHIP_UNARY_EXP || fn == SMHIP_UNARY_LOG) {
        if (int rc = launch_broadcast(SMHIP_OP_LEFT, dtype, a, strides, a, zero, shape, ndim, out, s)) return rc;
        return launch_unary_dense(fn, dtype, out, n, out, s);
    }
    return launch_broadcast(SMHIP_OP_UNARY_BASE + fn, dtype, a, strides, a, zero, shape, ndim, out, s);
}

}  // namespace smhip

using namespace smhip;

int smhip_unary(int fn, int dtype, const void *a, const int64_t *strides, const int64_t *shape, int ndim, void *out) {
    if (fn < SMHIP_UNARY_NEG || fn > SMHIP_UNARY_LOG || !valid_dtype(dtype)) return fail(SMHIP_ERR_INVALID, "unary: bad function %d / dtype %d", fn, dtype);
    if (ndim < 1 || ndim > SMHIP_MAX_NDIM) return fail(SMHIP_ERR_INVALID, "unary: ndim %d outside 1..%d", ndim, SMHIP_MAX_NDIM);
    if (!strides || !shape) return fail(SMHIP_ERR_INVALID, "unary: null shape/stride");
    int64_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] < 0 || strides[i] < 0) return fail(SMHIP_ERR_INVALID, "unary: negative extent or stride at dim %d", i);
        n *= shape[i];
    }
    if (fn >= SMHIP_UNARY_SQRT && (dtype == SMHIP_I32 || dtype == SMHIP_I64))
        return fail(SMHIP_ERR_UNSUPPORTED, "unary: sqrt / exp / log of an integer element type");
    if (n == 0) return SMHIP_OK;
    if (!a || !out) return fail(SMHIP_ERR_INVALID, "unary: null buffer");
    const size_t esz = dtype_size(dtype);
    const Span read{a, span_bytes(shape, strides, ndim, esz)}, write{out, (size_t)n * esz};
    if (spans_overlap(read, write) && !(a == out && axis_plan::row_major(shape, strides, ndim)))
        return fail(SMHIP_ERR_INVALID, "unary: `out` overlaps the operand (only out == a with a dense operand is in place)");
    hipStream_t s;
    OpScope op_scope;
    if (int rc = op_scope.begin(&read, 1, write, &s)) return rc;  // recorded tiny operators are flushed first
    return launch_unary(fn, dtype, a, strides, shape, ndim, out, s);
}
