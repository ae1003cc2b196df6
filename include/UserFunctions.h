// UserFunctions.h -- free functions of the drop-in surface: sm::empty / ones /
// zeros, sm::pow, operator<< (reference include/UserFunctions.h:8-57), plus
// sm::sum and sm::synchronize for the MI355X side.
//
// Creation happens in HBM: ones/zeros are device fills (smhip_fill), empty
// reserves pooled device memory; a host mirror appears only if host code later
// touches `data` or operator()(i...).
#pragma once

#include <initializer_list>
#include <ostream>
#include <vector>

#include "SMArray.h"

namespace sm {

template <typename T, typename... Args>
SMArray<T> empty(Args... args) {
    return SMArray<T>::device_empty({static_cast<std::size_t>(args)...});
}

template <typename T, typename... Args>
SMArray<T> ones(Args... args) {
    return SMArray<T>::device_full({static_cast<std::size_t>(args)...}, T{1});
}

template <typename T, typename... Args>
SMArray<T> zeros(Args... args) {
    return SMArray<T>::device_full({static_cast<std::size_t>(args)...}, T{0});
}

// Element-wise arr ^ val (reference UserFunctions.h:42-48 -> array_scalar_op<T, PowOp<T>>).
// int32/int64: the reference's square-and-multiply with wrapping products
// (crafted_pow.h:54-103) on every element; float: in-register exp2/log2 chain.
template <typename T>
SMArray<T> pow(const SMArray<T> &arr, T val) {
    return arr.template apply_scalar<PowOp<T>>(val);
}
// ... of a temporary: sm::pow(a - b, 2.0f) continues the expression's operator chain (SMArray::pow_of) instead of reading
// its result back from HBM -- the squared difference is one kernel.
template <typename T>
SMArray<T> pow(SMArray<T> &&arr, T val) {
    return SMArray<T>::pow_of(arr, true, val);
}

// Functions of one argument, elementwise (the reference has none: its README names vector exp / log as wanted and missing):
// e^x, the natural logarithm, the correctly rounded square root, |x|; unary minus is SMArray::operator-.  exp and log are
// within 1 ULP (smhip.h has the contract table and the special values).  Of a named array or a view they launch one kernel
// (views are read in place) and the result lives in HBM; of a temporary -- sm::exp(x - m) -- they continue the expression's
// operator chain like sm::pow(a - b, 2.0f) does, so the difference is never written.
#define SM_UNARY_FUNCTION(NAME, FN, FLOAT_ONLY)                                                                                    \
    template <typename T>                                                                                                          \
    SMArray<T> NAME(const SMArray<T> &arr) {                                                                                       \
        static_assert(!(FLOAT_ONLY) || std::is_floating_point_v<T>, "sm::" #NAME " is defined for float and double arrays only");  \
        return SMArray<T>::unary_of(arr, false, FN);                                                                               \
    }                                                                                                                              \
    template <typename T>                                                                                                          \
    SMArray<T> NAME(SMArray<T> &&arr) {                                                                                            \
        static_assert(!(FLOAT_ONLY) || std::is_floating_point_v<T>, "sm::" #NAME " is defined for float and double arrays only");  \
        return SMArray<T>::unary_of(arr, true, FN);                                                                                \
    }
SM_UNARY_FUNCTION(exp, SMHIP_UNARY_EXP, true)
SM_UNARY_FUNCTION(log, SMHIP_UNARY_LOG, true)
SM_UNARY_FUNCTION(sqrt, SMHIP_UNARY_SQRT, true)
SM_UNARY_FUNCTION(abs, SMHIP_UNARY_ABS, false)
#undef SM_UNARY_FUNCTION

// Fusion hook: (a Op1 b) Op2 c in ONE pass over HBM (the reference makes two passes and a
// temporary).  Dense, equal-shaped operands take the two-Op kernel; operands that broadcast against each other (a row, a
// column, a scalar-like array, the reference tests' (1,224,1,3)) take the chain kernel (smhip_chain) -- what the operators
// themselves do for `(a + b) * c` written as one expression; user-defined Ops and pow are evaluated as the two operator
// calls.  Same values every way.
//   auto r = sm::fused<AddOp<float>, MultiplyOp<float>>(a, b, c);   // (a + b) * c
template <typename Op1, typename Op2, typename T>
SMArray<T> fused(const SMArray<T> &a, const SMArray<T> &b, const SMArray<T> &c) {
    if constexpr (hip::on_device_v<T, Op1> && hip::on_device_v<T, Op2>) {
        const int o1 = hip::device_op<Op1>::id(), o2 = hip::device_op<Op2>::id();
        if (o1 <= SMHIP_OP_DIV && o2 <= SMHIP_OP_DIV && a.shape() == b.shape() && a.shape() == c.shape() && a.is_dense() &&
            b.is_dense() && c.is_dense()) {
            SMArray<T>::common_device(a, c);
            hip::DeviceGuard on(SMArray<T>::common_device(a, b));
            SMArray<T> out = SMArray<T>::device_empty(std::vector<std::size_t>(a.shape()));
            hip::check(smhip_fused_contiguous(o1, o2, hip::dtype_of<T>::id, a.device_data(), b.device_data(), c.device_data(),
                                              nullptr, out.device_data_mut(), a.totalSize));
            return out;
        }
        if (o1 <= SMHIP_OP_DIV && o2 <= SMHIP_OP_DIV) return SMArray<T>::template chain_of<Op1, Op2>(a, b, &c, T{});
    }
    return a.template apply<Op1>(b).template apply<Op2>(c);
}
template <typename Op1, typename Op2, typename T>
SMArray<T> fused(const SMArray<T> &a, const SMArray<T> &b, T c) {
    if constexpr (hip::on_device_v<T, Op1> && hip::on_device_v<T, Op2>) {
        const int o1 = hip::device_op<Op1>::id(), o2 = hip::device_op<Op2>::id();
        if (o1 <= SMHIP_OP_DIV && o2 <= SMHIP_OP_DIV && a.shape() == b.shape() && a.is_dense() && b.is_dense()) {
            hip::DeviceGuard on(SMArray<T>::common_device(a, b));
            SMArray<T> out = SMArray<T>::device_empty(std::vector<std::size_t>(a.shape()));
            hip::check(smhip_fused_contiguous(o1, o2, hip::dtype_of<T>::id, a.device_data(), b.device_data(), nullptr, &c,
                                              out.device_data_mut(), a.totalSize));
            return out;
        }
        if (o1 <= SMHIP_OP_DIV && o2 <= SMHIP_OP_DIV) return SMArray<T>::template chain_of<Op1, Op2>(a, b, nullptr, c);
    }
    return a.template apply<Op1>(b).template apply_scalar<Op2>(c);
}

// A whole expression in ONE pass over HBM: sm::expr("(a0 + a1) * a2 - 3 * a3", a, b, c, d).  The operands appear as
// a0 .. a7 in a HIP expression of the element type and broadcast against each other like the operators' (NumPy rule): a
// row, a column, a per-channel value or a one-element array is read through the caches inside the pass, a transposed or
// stepped view is copied dense first.  Each operation rounds as the separate operators do, so the values equal the operator
// chain's; the traffic is (k + 1) * sizeof(T) bytes per element for k full-size operands instead of 3 * sizeof(T) per
// operator.  Compiled by hipRTC on first use, cached.
// Run-time scalars appear as s0 .. s3 and are passed at launch (changing them does not recompile):
//     sm::expr("a0 * s0 + a1", {alpha}, x, y)        // axpy in one pass
template <typename T, typename... Rest>
SMArray<T> expr(const char *expression, std::initializer_list<T> scalars, const SMArray<T> &first, const Rest &...rest) {
    static_assert(hip::dtype_of<T>::id >= 0, "sm::expr: element type has no kernels");
    static_assert(sizeof...(Rest) <= 7, "sm::expr: at most 8 operands");
    static_assert((std::is_same_v<Rest, SMArray<T>> && ...), "sm::expr: operands must be SMArray<T> of one element type");
    if (scalars.size() > 4) throw std::runtime_error("sm::expr: at most 4 scalars");
    const SMArray<T> *arrays[] = {&first, &rest...};
    constexpr int n = 1 + static_cast<int>(sizeof...(Rest));
    const void *ptrs[8] = {};
    for (int k = 1; k < n; ++k) SMArray<T>::common_device(first, *arrays[k]);  // all operands on one GPU, or it throws
    hip::DeviceGuard on(first.device());
    bool flat = true;
    for (int k = 0; k < n; ++k) flat = flat && arrays[k]->shape() == first.shape() && arrays[k]->is_dense();
    if (flat) {
        for (int k = 0; k < n; ++k) ptrs[k] = arrays[k]->device_data();
        SMArray<T> out = SMArray<T>::device_empty(std::vector<std::size_t>(first.shape()));
        hip::check(smhip_fused_expr(expression, hip::dtype_of<T>::id, ptrs, n, scalars.size() ? scalars.begin() : nullptr,
                                    static_cast<int>(scalars.size()), out.device_data_mut(), first.totalSize));
        return out;
    }
    // the common shape (sm::broadcast throws the reference's "Cannot broadcast shapes" on a mismatch), then every operand's
    // strides against it
    std::vector<std::size_t> shape = first.shape();
    const std::vector<std::size_t> none;
    for (int k = 1; k < n; ++k) shape = sm::broadcast(shape, std::vector<std::size_t>(shape.size(), 0), arrays[k]->shape(), arrays[k]->strides()).resultShape;
    if (shape.size() > MAX_NDIM) throw std::runtime_error("rank exceeds MAX_NDIM");
    if (shape.empty()) throw std::runtime_error("sm::expr: 0-d operands");
    const std::size_t nd = shape.size();
    std::vector<std::int64_t> strides(static_cast<std::size_t>(n) * nd, 0), sh(shape.begin(), shape.end());
    for (int k = 0; k < n; ++k) {
        const auto &ls = arrays[k]->shape();
        const auto &lt = arrays[k]->strides();
        const std::size_t shift = nd - ls.size();
        for (std::size_t i = 0; i < ls.size(); ++i) strides[k * nd + shift + i] = (ls[i] == 1 && shape[shift + i] != 1) ? 0 : static_cast<std::int64_t>(lt[i]);
        ptrs[k] = arrays[k]->device_data();
    }
    SMArray<T> out = SMArray<T>::device_empty(std::move(shape));
    hip::check(smhip_fused_expr_bcast(expression, hip::dtype_of<T>::id, ptrs, strides.data(), n, scalars.size() ? scalars.begin() : nullptr,
                                      static_cast<int>(scalars.size()), sh.data(), static_cast<int>(nd), out.device_data_mut()));
    return out;
}
template <typename T, typename... Rest>
SMArray<T> expr(const char *expression, const SMArray<T> &first, const Rest &...rest) {
    return expr<T>(expression, std::initializer_list<T>{}, first, rest...);
}

// The sum of an expression's results in the same single pass, nothing stored: sm::expr_sum("(a0 - a1) * (a0 - a1)", x, y)
// is a squared distance at 8 bytes per element and no temporary (fp64 accumulation, deterministic).
template <typename T, typename... Rest>
double expr_sum(const char *expression, std::initializer_list<T> scalars, const SMArray<T> &first, const Rest &...rest) {
    static_assert(hip::dtype_of<T>::id >= 0, "sm::expr_sum: element type has no kernels");
    static_assert(sizeof...(Rest) <= 7, "sm::expr_sum: at most 8 operands");
    static_assert((std::is_same_v<Rest, SMArray<T>> && ...), "sm::expr_sum: operands must be SMArray<T> of one element type");
    if (scalars.size() > 4) throw std::runtime_error("sm::expr_sum: at most 4 scalars");
    const SMArray<T> *arrays[] = {&first, &rest...};
    constexpr int n = 1 + static_cast<int>(sizeof...(Rest));
    std::vector<SMArray<T>> dense;
    dense.reserve(n);
    const void *ptrs[8] = {};
    for (int k = 1; k < n; ++k) SMArray<T>::common_device(first, *arrays[k]);
    hip::DeviceGuard on(first.device());
    for (int k = 0; k < n; ++k) {
        if (arrays[k]->shape() != first.shape()) throw std::runtime_error("sm::expr_sum: operands must have the same shape");
        if (arrays[k]->is_dense()) {
            ptrs[k] = arrays[k]->device_data();
        } else {
            dense.push_back(arrays[k]->contiguous());
            ptrs[k] = dense.back().device_data();
        }
    }
    const detail::DeviceWord<double> result;
    hip::check(smhip_fused_expr_sum_async(expression, hip::dtype_of<T>::id, ptrs, n, scalars.size() ? scalars.begin() : nullptr,
                                          static_cast<int>(scalars.size()), nullptr, first.totalSize, result.ptr()));
    return result.read();
}
template <typename T, typename... Rest>
double expr_sum(const char *expression, const SMArray<T> &first, const Rest &...rest) {
    return expr_sum<T>(expression, std::initializer_list<T>{}, first, rest...);
}

// Sum of all elements in fp64 (BASELINE config 5's reduction; no reference counterpart).
template <typename T>
double sum(const SMArray<T> &arr) {
    return arr.sum();
}
template <typename T>
double sum(SMArray<T> &&arr) {  // sm::sum(sm::pow(a - b, 2.0f)): the expression's temporary, summed in its chain's own pass
    return std::move(arr).sum();
}

// Reductions along axes (np.sum / np.mean / np.max / np.min with `axis`): SMArray<T> resident on the device.  `axis` is one
// int (negative counts from the end) or a list {0, 2}; keepdims keeps reduced axes as extents of 1; reducing every axis
// without keepdims gives shape {1}.  Semantics as SMArray::sum(axis) (SMArray.h) and smhip_reduce_axes (smhip.h).
template <typename T>
SMArray<T> sum(const SMArray<T> &arr, int axis, bool keepdims = false) { return arr.sum(axis, keepdims); }
template <typename T>
SMArray<T> sum(const SMArray<T> &arr, std::initializer_list<int> axes, bool keepdims = false) { return arr.sum(axes, keepdims); }
template <typename T>
SMArray<T> mean(const SMArray<T> &arr, int axis, bool keepdims = false) { return arr.mean(axis, keepdims); }
template <typename T>
SMArray<T> mean(const SMArray<T> &arr, std::initializer_list<int> axes, bool keepdims = false) { return arr.mean(axes, keepdims); }
template <typename T>
SMArray<T> max(const SMArray<T> &arr, int axis, bool keepdims = false) { return arr.max(axis, keepdims); }
template <typename T>
SMArray<T> max(const SMArray<T> &arr, std::initializer_list<int> axes, bool keepdims = false) { return arr.max(axes, keepdims); }
template <typename T>
SMArray<T> min(const SMArray<T> &arr, int axis, bool keepdims = false) { return arr.min(axis, keepdims); }
template <typename T>
SMArray<T> min(const SMArray<T> &arr, std::initializer_list<int> axes, bool keepdims = false) { return arr.min(axes, keepdims); }

// Cumulative scans (np.cumsum / np.cumprod / np.maximum.accumulate / np.minimum.accumulate): the result has the shape of
// `arr`; `axis` counts from the end when negative; without an axis the elements are scanned in row-major order and the
// result has shape {size}.  Semantics as SMArray::cumsum(axis) (SMArray.h) and smhip_scan_axis (smhip.h).
template <typename T>
SMArray<T> cumsum(const SMArray<T> &arr, int axis) { return arr.cumsum(axis); }
template <typename T>
SMArray<T> cumsum(const SMArray<T> &arr) { return arr.cumsum(); }
template <typename T>
SMArray<T> cumprod(const SMArray<T> &arr, int axis) { return arr.cumprod(axis); }
template <typename T>
SMArray<T> cumprod(const SMArray<T> &arr) { return arr.cumprod(); }
template <typename T>
SMArray<T> cummax(const SMArray<T> &arr, int axis) { return arr.cummax(axis); }
template <typename T>
SMArray<T> cummax(const SMArray<T> &arr) { return arr.cummax(); }
template <typename T>
SMArray<T> cummin(const SMArray<T> &arr, int axis) { return arr.cummin(axis); }
template <typename T>
SMArray<T> cummin(const SMArray<T> &arr) { return arr.cummin(); }

// Where the maximum / minimum stands (np.argmax / np.argmin): SMArray<std::int64_t> of positions along `axis` (negative
// counts from the end; keepdims keeps it as an extent of 1), the first on a tie and the first NaN if there is one; without
// an axis the row-major index of the whole array, shape {1}.  max_with_index / min_with_index return {values, positions}
// from ONE pass over the operand.  Semantics as SMArray::argmax(axis) (SMArray.h) and smhip_argreduce_axis (smhip.h).
template <typename T>
SMArray<std::int64_t> argmax(const SMArray<T> &arr, int axis, bool keepdims = false) { return arr.argmax(axis, keepdims); }
template <typename T>
SMArray<std::int64_t> argmax(const SMArray<T> &arr) { return arr.argmax(); }
template <typename T>
SMArray<std::int64_t> argmin(const SMArray<T> &arr, int axis, bool keepdims = false) { return arr.argmin(axis, keepdims); }
template <typename T>
SMArray<std::int64_t> argmin(const SMArray<T> &arr) { return arr.argmin(); }
template <typename T>
std::pair<SMArray<T>, SMArray<std::int64_t>> max_with_index(const SMArray<T> &arr, int axis, bool keepdims = false) { return arr.max_with_index(axis, keepdims); }
template <typename T>
std::pair<SMArray<T>, SMArray<std::int64_t>> min_with_index(const SMArray<T> &arr, int axis, bool keepdims = false) { return arr.min_with_index(axis, keepdims); }

// The order along an axis (np.sort / np.argsort with kind="stable"): the elements of each line in order, or their positions as
// SMArray<std::int64_t>; both of `arr`'s shape.  `axis` counts from the end when negative and is the last one when absent;
// descending puts NaNs, then the larger values first, ties still in the order of their positions.  sort_with_index returns
// {values, positions} from ONE call; sort_flat / argsort_flat sort the row-major flattening, shape {size}.  Semantics as
// SMArray::sort(axis) (SMArray.h) and smhip_sort_axis (smhip.h).
template <typename T>
SMArray<T> sort(const SMArray<T> &arr, int axis = -1, bool descending = false) { return arr.sort(axis, descending); }
template <typename T>
SMArray<std::int64_t> argsort(const SMArray<T> &arr, int axis = -1, bool descending = false) { return arr.argsort(axis, descending); }
template <typename T>
std::pair<SMArray<T>, SMArray<std::int64_t>> sort_with_index(const SMArray<T> &arr, int axis = -1, bool descending = false) { return arr.sort_with_index(axis, descending); }
template <typename T>
SMArray<T> sort_flat(const SMArray<T> &arr, bool descending = false) { return arr.sort_flat(descending); }
template <typename T>
SMArray<std::int64_t> argsort_flat(const SMArray<T> &arr, bool descending = false) { return arr.argsort_flat(descending); }

// The k first of that order without the sort: {values, positions}, the first k along `axis` of sort_with_index(arr, axis, largest),
// bit for bit; topk_flat takes the row-major flattening, shape {k}.  Semantics as SMArray::topk (SMArray.h) and smhip_topk_axis.
template <typename T>
std::pair<SMArray<T>, SMArray<std::int64_t>> topk(const SMArray<T> &arr, std::size_t k, int axis = -1, bool largest = true) { return arr.topk(k, axis, largest); }
template <typename T>
std::pair<SMArray<T>, SMArray<std::int64_t>> topk_flat(const SMArray<T> &arr, std::size_t k, bool largest = true) { return arr.topk_flat(k, largest); }

// Order statistics along an axis without sorting the line (np.quantile / np.percentile / np.median): a single probability gives the
// kept shape, a list of Q a leading axis of Q, from one read of the operand; the forms without an axis run over the row-major
// flattening, shape {1} or {Q}.  Semantics as SMArray::quantile (SMArray.h) and smhip_quantile_axis.
template <typename T>
SMArray<T> quantile(const SMArray<T> &arr, double q, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) { return arr.quantile(q, axis, method, keepdims); }
template <typename T>
SMArray<T> quantile(const SMArray<T> &arr, std::initializer_list<double> q, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) { return arr.quantile(q, axis, method, keepdims); }
template <typename T>
SMArray<T> quantile(const SMArray<T> &arr, const std::vector<double> &q, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) { return arr.quantile(q, axis, method, keepdims); }
template <typename T>
SMArray<T> quantile(const SMArray<T> &arr, double q, quantile_method method = quantile_method::linear) { return arr.quantile(q, method); }
template <typename T>
SMArray<T> quantile(const SMArray<T> &arr, std::initializer_list<double> q, quantile_method method = quantile_method::linear) { return arr.quantile(q, method); }
template <typename T>
SMArray<T> quantile(const SMArray<T> &arr, const std::vector<double> &q, quantile_method method = quantile_method::linear) { return arr.quantile(q, method); }
template <typename T>
SMArray<T> percentile(const SMArray<T> &arr, double p, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) { return arr.percentile(p, axis, method, keepdims); }
template <typename T>
SMArray<T> percentile(const SMArray<T> &arr, std::initializer_list<double> p, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) { return arr.percentile(p, axis, method, keepdims); }
template <typename T>
SMArray<T> percentile(const SMArray<T> &arr, const std::vector<double> &p, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) { return arr.percentile(p, axis, method, keepdims); }
template <typename T>
SMArray<T> percentile(const SMArray<T> &arr, const std::vector<double> &p, quantile_method method = quantile_method::linear) { return arr.percentile(p, method); }
template <typename T>
SMArray<T> percentile(const SMArray<T> &arr, double p, quantile_method method = quantile_method::linear) { return arr.percentile(p, method); }
template <typename T>
SMArray<T> percentile(const SMArray<T> &arr, std::initializer_list<double> p, quantile_method method = quantile_method::linear) { return arr.percentile(p, method); }
template <typename T>
SMArray<T> median(const SMArray<T> &arr, int axis, bool keepdims = false) { return arr.median(axis, keepdims); }
template <typename T>
SMArray<T> median(const SMArray<T> &arr) { return arr.median(); }

// softmax, log_softmax and logsumexp along an axis, fused per line (float and double): one library call each instead of the
// max / exp / sum / divide recipe.  logsumexp without an axis runs over the row-major flattening, shape {1}.  Semantics as
// SMArray::softmax (SMArray.h) and smhip_softmax_axis.
template <typename T>
SMArray<T> softmax(const SMArray<T> &arr, int axis = -1) { return arr.softmax(axis); }
template <typename T>
SMArray<T> log_softmax(const SMArray<T> &arr, int axis = -1) { return arr.log_softmax(axis); }
template <typename T>
SMArray<T> logsumexp(const SMArray<T> &arr, int axis, bool keepdims = false) { return arr.logsumexp(axis, keepdims); }
template <typename T>
SMArray<T> logsumexp(const SMArray<T> &arr) { return arr.logsumexp(); }

// var, stddev and var_mean along axes and standardize along one (float and double): the second moment centred in fp64, one library
// call each instead of the mean / subtract / square / mean recipe.  The forms without an axis run over the row-major flattening, shape
// {1}.  Semantics as SMArray::var (SMArray.h) and smhip_moments_axes / smhip_standardize_axis.
template <typename T>
SMArray<T> var(const SMArray<T> &arr, int axis, std::int64_t ddof = 0, bool keepdims = false) { return arr.var(axis, ddof, keepdims); }
template <typename T>
SMArray<T> var(const SMArray<T> &arr, std::initializer_list<int> axes, std::int64_t ddof = 0, bool keepdims = false) { return arr.var(axes, ddof, keepdims); }
template <typename T>
SMArray<T> var(const SMArray<T> &arr) { return arr.var(); }
template <typename T>
SMArray<T> stddev(const SMArray<T> &arr, int axis, std::int64_t ddof = 0, bool keepdims = false) { return arr.stddev(axis, ddof, keepdims); }
template <typename T>
SMArray<T> stddev(const SMArray<T> &arr, std::initializer_list<int> axes, std::int64_t ddof = 0, bool keepdims = false) { return arr.stddev(axes, ddof, keepdims); }
template <typename T>
SMArray<T> stddev(const SMArray<T> &arr) { return arr.stddev(); }
template <typename T>
std::pair<SMArray<T>, SMArray<T>> var_mean(const SMArray<T> &arr, int axis, std::int64_t ddof = 0, bool keepdims = false) { return arr.var_mean(axis, ddof, keepdims); }
template <typename T>
std::pair<SMArray<T>, SMArray<T>> var_mean(const SMArray<T> &arr, std::initializer_list<int> axes, std::int64_t ddof = 0, bool keepdims = false) { return arr.var_mean(axes, ddof, keepdims); }
template <typename T>
std::pair<SMArray<T>, SMArray<T>> var_mean(const SMArray<T> &arr) { return arr.var_mean(); }
template <typename T>
SMArray<T> standardize(const SMArray<T> &arr, int axis = -1, double eps = 0.0, std::int64_t ddof = 0) { return arr.standardize(axis, eps, ddof); }

// Picking by position along an axis (np.take_along_axis / np.take): result[..., j, ...] = arr[..., idx[..., j, ...], ...].
// take_along_axis: `idx` has arr's rank, its other axes equal to arr's or broadcastable; without an axis both are flattened.
// take: `idx` is 1-D, the result is arr's shape with `axis` replaced by idx.size(); take_flat indexes the row-major flattening.
// `mode`: index_mode::checked (numpy's rule; throws std::out_of_range after a stream synchronisation), clip or wrap (asynchronous).
// Semantics as SMArray::take_along_axis (SMArray.h) and smhip_take_axis (smhip.h).
template <typename T>
SMArray<T> take_along_axis(const SMArray<T> &arr, const SMArray<std::int64_t> &idx, int axis, index_mode mode = index_mode::checked) {
    return arr.take_along_axis(idx, axis, mode);
}
template <typename T>
SMArray<T> take_along_axis(const SMArray<T> &arr, const SMArray<std::int64_t> &idx, index_mode mode = index_mode::checked) {
    return arr.take_along_axis(idx, mode);
}
template <typename T>
SMArray<T> take(const SMArray<T> &arr, const SMArray<std::int64_t> &idx, int axis, index_mode mode = index_mode::checked) { return arr.take(idx, axis, mode); }
template <typename T>
SMArray<T> take_flat(const SMArray<T> &arr, const SMArray<std::int64_t> &idx, index_mode mode = index_mode::checked) { return arr.take_flat(idx, mode); }

// Writing by position along an axis, in place on `arr` (np.put_along_axis / np.put, np.add.at): the transpose of take.  `values` is
// an SMArray<T> that broadcasts against the walk shape, or a scalar.  put_along_axis / scatter_add: `idx` has arr's rank, its other
// axes equal to arr's or 1; without an axis arr, idx and the values are flattened (values of idx's size, one element or a scalar).  put / index_add: `ids` is 1-D; put_flat indexes the
// row-major flattening.  Duplicates: PUT -- the entry with the largest position along idx wins; ADD -- contributions are added
// one by one in that order (f32 in fp64), so every run gives the same bits.  `unique` promises that no two entries of a line name
// the same position (one launch, no sort).  `mode` as for take; under checked a bad entry is dropped and std::out_of_range thrown
// after the valid ones have been applied.  All return arr.  Semantics as SMArray::put_along_axis (SMArray.h) and smhip_scatter_axis.
template <typename T, typename V>
SMArray<T> &put_along_axis(SMArray<T> &arr, const SMArray<std::int64_t> &idx, const V &values, int axis, index_mode mode = index_mode::checked, bool unique = false) {
    return arr.put_along_axis(idx, values, axis, mode, unique);
}
template <typename T, typename V>
SMArray<T> &put_along_axis(SMArray<T> &arr, const SMArray<std::int64_t> &idx, const V &values, index_mode mode = index_mode::checked, bool unique = false) {
    return arr.put_along_axis(idx, values, mode, unique);
}
template <typename T, typename V>
SMArray<T> &scatter_add(SMArray<T> &arr, const SMArray<std::int64_t> &idx, const V &values, int axis, index_mode mode = index_mode::checked, bool unique = false) {
    return arr.scatter_add(idx, values, axis, mode, unique);
}
template <typename T, typename V>
SMArray<T> &put(SMArray<T> &arr, const SMArray<std::int64_t> &ids, const V &values, int axis, index_mode mode = index_mode::checked, bool unique = false) {
    return arr.put(ids, values, axis, mode, unique);
}
template <typename T, typename V>
SMArray<T> &put_flat(SMArray<T> &arr, const SMArray<std::int64_t> &ids, const V &values, index_mode mode = index_mode::checked, bool unique = false) {
    return arr.put_flat(ids, values, mode, unique);
}
template <typename T, typename V>
SMArray<T> &index_add(SMArray<T> &arr, const SMArray<std::int64_t> &ids, const V &values, int axis, index_mode mode = index_mode::checked, bool unique = false) {
    return arr.index_add(ids, values, axis, mode, unique);
}

// astype<U>(a): np.ndarray.astype between float, double, int and std::int64_t, on the device (SMArray::astype, smhip_convert).  Float to
// integer is saturating truncation: toward zero, the target's min / max beyond its range, 0 for a NaN.
template <typename U, typename T>
SMArray<U> astype(const SMArray<T> &a) { return a.template astype<U>(); }

// Counting (np.searchsorted, np.bincount, np.histogram); the results are SMArray<std::int64_t> on the device.  searchsorted: for every
// element of x its place among the ascending 1-D `edges` (side::left: at an equal edge's first copy, side::right: after its last).
// bincount: how many of the int / std::int64_t `ids` name each of nbins positions, the same bits as index_add of 1 onto zeros in every
// mode.  histogram(x, bins, lo, hi): {counts, edges} of equal bins over [lo, hi], numpy's edges; histogram(x, edges): counts between
// explicit edges.  Semantics as the members of the same names (SMArray.h) and smhip_searchsorted / smhip_bincount / smhip_histogram.
template <typename T>
SMArray<std::int64_t> searchsorted(const SMArray<T> &edges, const SMArray<T> &x, side s = side::left) { return edges.searchsorted(x, s); }
template <typename T>
SMArray<std::int64_t> bincount(const SMArray<T> &ids, std::int64_t nbins, index_mode mode = index_mode::checked) { return ids.bincount(nbins, mode); }
template <typename T>
std::pair<SMArray<std::int64_t>, SMArray<T>> histogram(const SMArray<T> &x, std::int64_t bins, double lo, double hi) { return x.histogram(bins, lo, hi); }
template <typename T>
SMArray<std::int64_t> histogram(const SMArray<T> &x, const SMArray<T> &edges) { return x.histogram(edges); }

// Choosing by condition (np.where, np.count_nonzero, np.flatnonzero, np.nonzero, a[mask], np.compress).  A condition is a comparison of
// arrays -- `a > 0.0f`, `a <= b`, `0 == a`: a sm::Cond<T>, evaluated inside the kernel that consumes it -- or an array, which stands for
// "nonzero".  where(c, a, b): c ? a : b with a and b each an array or a scalar, all broadcasting; mask(c): where(c, 1, 0), so that
// conditions combine with the arithmetic operators (and: m1 * m2; or: m1 + m2 - m1 * m2; not: -m + 1).  count_nonzero, flatnonzero,
// nonzero, select and compress have results whose size depends on the data: each WAITS FOR THE STREAM ONCE, to learn it.  Semantics as
// SMArray::assign_where / select (SMArray.h) and smhip_where / smhip_select_count / smhip_select.
namespace detail {
// An operand of where: an array or a scalar.
template <typename T>
struct WhereArg {
    const SMArray<T> *array = nullptr;
    T value{};
    WhereArg(const SMArray<T> &a) : array(&a) {}
    WhereArg(T v) : value(v) {}
};
}  // namespace detail
template <typename T>
SMArray<T> where(const Cond<T> &c, const std::type_identity_t<detail::WhereArg<T>> &a, const std::type_identity_t<detail::WhereArg<T>> &b) {
    return SMArray<T>::where_of(c, a.array, a.value, b.array, b.value);
}
template <typename T>
SMArray<T> where(const SMArray<T> &nonzero, const std::type_identity_t<detail::WhereArg<T>> &a, const std::type_identity_t<detail::WhereArg<T>> &b) {
    return SMArray<T>::where_of(Cond<T>(nonzero), a.array, a.value, b.array, b.value);
}
template <typename T>
SMArray<T> mask(const Cond<T> &c) { return SMArray<T>::where_of(c, nullptr, T{1}, nullptr, T{0}); }
template <typename T>
SMArray<T> mask(const SMArray<T> &nonzero) { return mask(Cond<T>(nonzero)); }
template <typename T>
std::int64_t count_nonzero(const Cond<T> &c) { return c.count_nonzero(); }
template <typename T>
std::int64_t count_nonzero(const SMArray<T> &arr) { return Cond<T>(arr).count_nonzero(); }
template <typename T>
SMArray<std::int64_t> flatnonzero(const Cond<T> &c) { return c.flatnonzero(); }
template <typename T>
SMArray<std::int64_t> flatnonzero(const SMArray<T> &arr) { return Cond<T>(arr).flatnonzero(); }
template <typename T>
std::vector<SMArray<std::int64_t>> nonzero(const Cond<T> &c) { return c.nonzero(); }
template <typename T>
std::vector<SMArray<std::int64_t>> nonzero(const SMArray<T> &arr) { return Cond<T>(arr).nonzero(); }
template <typename T, typename U>
SMArray<T> select(const SMArray<T> &arr, const Cond<U> &c) { return arr.select(c); }
template <typename T, typename U>
SMArray<T> select(const SMArray<T> &arr, const SMArray<U> &nonzero) { return arr.select(nonzero); }
// np.compress(cond1d, arr, axis): the slices of arr along `axis` where the 1-D condition holds, take(arr, flatnonzero(cond1d), axis).
// std::invalid_argument when the condition is not 1-D or its length differs from the axis.
template <typename U, typename T>
SMArray<T> compress(const Cond<U> &c, const SMArray<T> &arr, int axis) {
    const int nd = static_cast<int>(arr.shape().size()), ax = axis < 0 ? axis + nd : axis;
    if (ax < 0 || ax >= nd) throw std::invalid_argument("simpleMath/MI355X: compress: axis " + std::to_string(axis) + " of an array of rank " + std::to_string(nd));
    const auto cs = c.shape();
    if (cs.size() != 1 || cs[0] != arr.shape()[ax])
        throw std::invalid_argument("simpleMath/MI355X: compress: the condition must be 1-D and as long as the axis (" + std::to_string(arr.shape()[ax]) + ")");
    return arr.take(c.flatnonzero(), ax, index_mode::clip);  // the positions are valid by construction
}
template <typename U, typename T>
SMArray<T> compress(const SMArray<U> &nonzero, const SMArray<T> &arr, int axis) { return compress(Cond<U>(nonzero), arr, axis); }

// The distinct values (np.unique on the row-major flattening, the Array API's names): values ascending with one NaN last (every NaN
// with equal_nan = false), the first occurrence of each, the value number of every element (shape {size}), how often each occurs.
// unique_consecutive / run_lengths: the same without the sort -- the first element of every run of adjacent equal elements and the
// runs' lengths.  Each waits for the stream once to learn the size.  Semantics as the members of the same names (SMArray.h) and smhip_runs.
template <typename T>
SMArray<T> unique_values(const SMArray<T> &arr, bool equal_nan = true) { return arr.unique_values(equal_nan); }
template <typename T>
SMArray<T> unique(const SMArray<T> &arr, bool equal_nan = true) { return arr.unique_values(equal_nan); }
template <typename T>
std::pair<SMArray<T>, SMArray<std::int64_t>> unique_counts(const SMArray<T> &arr, bool equal_nan = true) { return arr.unique_counts(equal_nan); }
template <typename T>
std::pair<SMArray<T>, SMArray<std::int64_t>> unique_inverse(const SMArray<T> &arr, bool equal_nan = true) { return arr.unique_inverse(equal_nan); }
template <typename T>
UniqueAll<T> unique_all(const SMArray<T> &arr, bool equal_nan = true) { return arr.unique_all(equal_nan); }
template <typename T>
SMArray<T> unique_consecutive(const SMArray<T> &arr, bool equal_nan = true) { return arr.unique_consecutive(equal_nan); }
template <typename T>
std::pair<SMArray<T>, SMArray<std::int64_t>> run_lengths(const SMArray<T> &arr, bool equal_nan = true) { return arr.run_lengths(equal_nan); }

// Block until every queued kernel has finished (operators are asynchronous;
// anything that reads values on the host synchronises by itself).
inline void synchronize() { hip::check(smhip_synchronize()); }

}  // namespace sm

template <typename T>
std::ostream &operator<<(std::ostream &os, const sm::SMArray<T> &arr) {
    return os << arr.toString();
}
