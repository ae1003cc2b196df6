// SMArray.h -- sm::SMArray<T>, the drop-in array class, MI355X-resident.
//
// Public surface of the reference's class (include/SMArray.h:30-438): public
// `data` and `totalSize`; construction from (nested) initializer lists or from
// an owned `new T[]` buffer plus a shape; move-only; operator()(ints...) for
// element access and operator()(ints | Slice ...) for views; transpose(),
// repeat(); % (dot), + - * / with an array (NumPy broadcasting) or a scalar;
// toString(), shape(), strides().
//
// What is different underneath: an array's elements live in HBM.
//   * Every array (and all views of it) shares one Storage: a pooled device
//     buffer and, only when host code asks for it, a host mirror.  Two validity
//     bits track which side is current.  `data`, operator()(i...) and toString()
//     bring the host mirror up to date; arithmetic brings the device side up to
//     date.  Writable host access (`data`, the T& form of operator()) marks the
//     device side stale, so the reference's idiom `arr.data[i] = v; r = arr * 2;`
//     keeps working.  A chain of operators never leaves the GPU.
//   * + - * / % and sm::pow run libsmhip's gfx950 kernels through the C ABI
//     (smhip.h) at the points where the reference calls element_wise_op /
//     array_scalar_op / dot_product (SMArray.h:213-305).  Results are born on the
//     device from a pooled allocator instead of `new T[n]` (SMArray.h:219).
//   * There is no CPU arithmetic path: without libsmhip + a GPU the operators
//     throw std::runtime_error.
//
// Deliberate deviations from reference quirks:
//   1-D operands walk their strides (the reference reads them as dense);
//   views know their real ndim/totalSize, so scalar ops, % and toString work on
//   views; repeat() has NumPy semantics; rank > MAX_NDIM throws.
#pragma once

#include <cassert>
#include <complex>
#include <cstring>
#include <functional>
#include <initializer_list>
#include <memory>
#include <optional>
#include <sstream>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "SMUtils.h"
#include "Slice.h"
#include "math/calculate.h"
#include "math/ops.h"
#include "math/product.h"

namespace sm {

template <typename T>
concept ArithmeticOrComplex =
    std::is_arithmetic_v<T> ||
    (requires { typename T::value_type; } && std::is_arithmetic_v<typename T::value_type> &&
     std::same_as<T, std::complex<typename T::value_type>>);

template <ArithmeticOrComplex T>
class SMArray;

// A comparison that has not been evaluated yet: what `a > 0.0f` gives (defined below the class).
template <typename T>
struct Cond;

// What sm::unique_all returns: {values, index, inverse, counts} (defined below the class).
template <typename T>
struct UniqueAll;

// What take / take_along_axis do with an index outside [-R, R) of an axis of R elements (smhip.h: smhip_index_mode).
enum class index_mode {
    checked = SMHIP_INDEX_CHECKED,  // numpy's rule: negatives count from the end, anything else out of range throws std::out_of_range
    clip = SMHIP_INDEX_CLIP,        // clamp to [0, R - 1] (np.take(mode="clip")): fully asynchronous
    wrap = SMHIP_INDEX_WRAP,        // the non-negative remainder mod R (np.take(mode="wrap")): fully asynchronous
};

// How sm::quantile reads a probability whose position h = (R - 1) q falls between two elements of the ordered line (smhip.h:
// smhip_quantile_method): numpy's method names.
enum class quantile_method {
    linear = SMHIP_QUANTILE_LINEAR,      // interpolate between s[floor(h)] and the next, in fp64, rounded once
    lower = SMHIP_QUANTILE_LOWER,        // s[floor(h)]
    higher = SMHIP_QUANTILE_HIGHER,      // s[ceil(h)]
    nearest = SMHIP_QUANTILE_NEAREST,    // s[rint(h)], ties to even
    midpoint = SMHIP_QUANTILE_MIDPOINT,  // halfway between the two where h is not an integer
};

// Which of equal edges sm::searchsorted names (smhip.h: smhip_side): np.searchsorted's side.
enum class side {
    left = SMHIP_SIDE_LEFT,    // the first i with !(edges[i] before x): a value equal to an edge stands AT the edge's first copy
    right = SMHIP_SIDE_RIGHT,  // the first i with x before edges[i]: it stands AFTER the edge's last copy
};

namespace detail {

// ---- deferred operator chains ------------------------------------------------------------------------------------------
// The reference evaluates `(A * row + B) * 0.5f` as three operator calls with a temporary each (SMArray.h:217-305); here
// a temporary that feeds the next operator OF THE SAME FULL-EXPRESSION is never written to HBM: + - * / do not launch
// at once, they record a one-stage *chain* in the result's Storage, and an operator whose operand is that unevaluated
// temporary (an rvalue) extends the chain instead of reading it.  The chain is launched -- as ONE kernel where its
// operands allow, smhip_chain -- at the latest when the full-expression ends: every operator argument binds to a small
// wrapper (Operand / ScalarArg below) whose destructor, run when the statement's temporaries die, evaluates whatever is
// still pending on the thread.  So a NAMED value is always computed by the end of the statement that names it; nothing
// stays lazy across statements.  Before that point a chain is evaluated as soon as anything looks at its result (`data`,
// operator(), toString(), device_data(), another library call), and before any array is WRITTEN (host or device), so
// an operand cannot change under a recorded chain.  At most one chain is pending per thread.
struct PendingBase {
    virtual void run() = 0;  // evaluate into the Storage that owns this object (and destroy it)
    virtual ~PendingBase() = default;
};
inline thread_local PendingBase *tls_pending = nullptr;
inline void flush_pending() {
    if (PendingBase *p = tls_pending) {
        tls_pending = nullptr;
        p->run();
    }
}
// What the fusion did on this thread (tests and benchmarks read it through sm::fusion_stats()).
struct FusionStats {
    unsigned long long chains = 0;        // smhip_chain calls: expressions of two or more operators evaluated as one call
    unsigned long long fused_stages = 0;  // operators inside them
    unsigned long long single_ops = 0;    // deferred operators that ended up alone and ran as the plain operator
    unsigned long long direct_assignments = 0;  // `x = <expression>` evaluated straight into x (no temporary, no copy)
    unsigned long long summed_chains = 0;       // `(<expression>).sum()` taken in the chain's own pass, the value never written
    unsigned long long reductions = 0;          // axis reductions (smhip_reduce_axes: sum / mean / max / min along axes)
    unsigned long long scans = 0;               // cumulative scans (smhip_scan_axis: cumsum / cumprod / cummax / cummin)
    unsigned long long arg_reductions = 0;      // smhip_argreduce_axis calls: argmax / argmin / max_with_index / min_with_index
    unsigned long long sorts = 0;               // smhip_sort_axis calls: sort / argsort / sort_with_index and their _flat forms
    unsigned long long takes = 0;               // smhip_take_axis calls: take / take_along_axis / take_flat
    unsigned long long scatters = 0;            // smhip_scatter_axis calls: put_along_axis / put / put_flat / scatter_add / index_add
    unsigned long long counts = 0;              // smhip_searchsorted / smhip_bincount / smhip_histogram calls
    unsigned long long selects = 0;             // smhip_where / smhip_select_count / smhip_select calls
    unsigned long long uniques = 0;             // smhip_runs_count / smhip_runs calls: unique_* / unique_consecutive / run_lengths (a count, then the runs)
    unsigned long long topks = 0;               // smhip_topk_axis calls: topk / topk_flat
    unsigned long long quantiles = 0;           // smhip_quantile_axis calls: quantile / percentile / median
    unsigned long long softmaxes = 0;           // smhip_softmax_axis calls: softmax / log_softmax / logsumexp
    unsigned long long moments = 0;             // smhip_moments_axes / smhip_standardize_axis calls: var / stddev / var_mean / standardize
};
inline thread_local FusionStats tls_fusion_stats;
// The end of a full-expression, seen from the destructor of one of its temporaries.
inline void end_of_expression(int exceptions_at_birth) {
    if (!tls_pending) return;
    if (std::uncaught_exceptions() > exceptions_at_birth) {  // unwinding: the result is being destroyed as well, nothing to compute
        tls_pending = nullptr;
        return;
    }
    flush_pending();
}

// numpy's broadcasting of `other` into `shape`, aligned at the last axis; std::invalid_argument when the two do not broadcast.
inline void broadcast_into(std::vector<std::size_t> &shape, const std::vector<std::size_t> &other, const char *who) {
    if (other.size() > shape.size()) shape.insert(shape.begin(), other.size() - shape.size(), 1);
    const std::size_t pad = shape.size() - other.size();
    for (std::size_t d = 0; d < other.size(); ++d) {
        std::size_t &n = shape[pad + d];
        if (n == other[d] || other[d] == 1) continue;
        if (n != 1) throw std::invalid_argument(std::string("simpleMath/MI355X: ") + who + ": the shapes do not broadcast at axis " + std::to_string(pad + d));
        n = other[d];
    }
}
// The strides (in elements) of an operand seen over `over`, 0 along the axes it is broadcast; std::invalid_argument when it does not
// broadcast TO `over`.
inline std::vector<std::int64_t> strides_over(const std::vector<std::size_t> &shape, const std::vector<std::size_t> &strides, const std::vector<std::size_t> &over,
                                              const char *who) {
    if (shape.size() > over.size()) throw std::invalid_argument(std::string("simpleMath/MI355X: ") + who + ": an operand has more axes than the result");
    std::vector<std::int64_t> st(over.size(), 0);
    const std::size_t pad = over.size() - shape.size();
    for (std::size_t d = 0; d < shape.size(); ++d) {
        if (shape[d] == over[pad + d]) st[pad + d] = shape[d] == 1 ? 0 : static_cast<std::int64_t>(strides[d]);
        else if (shape[d] != 1) throw std::invalid_argument(std::string("simpleMath/MI355X: ") + who + ": the shapes do not broadcast at axis " + std::to_string(pad + d));
    }
    return st;
}

// One allocation, shared by an owning array and every view of it.
template <typename T>
struct Storage : std::enable_shared_from_this<Storage<T>> {
    T *host = nullptr;
    void *dev = nullptr;
    std::size_t count = 0;
    bool host_valid = false;  // host mirror holds the current values
    bool dev_valid = false;   // device buffer holds the current values

    int device = 0;           // the GPU the device buffer lives on (the creating thread's current device)
    unsigned inline_uses = 0; // times the host-only elements rode in a kernel's argument block instead of being uploaded
    unsigned fetches = 0;     // single elements read back one at a time (fetch()); after a few the whole array is mirrored
    std::unique_ptr<PendingBase> pending;  // the operator chain that will produce these elements, while it has not run

    // The values are about to be looked at: run the recorded chain first.
    void ensure() {
        if (pending) {
            if (tls_pending == pending.get()) tls_pending = nullptr;
            pending->run();  // resets `pending`
        }
    }
    // An array is about to be written: a chain recorded on this thread may still want its old values.
    void before_write() {
        ensure();
        if (tls_pending) flush_pending();
    }

    explicit Storage(std::size_t n) : count(n) { smhip_get_device(&device); }
    Storage(T *adopted, std::size_t n) : host(adopted), count(n), host_valid(true) { smhip_get_device(&device); }  // takes ownership of new T[]
    Storage(const Storage &) = delete;
    Storage &operator=(const Storage &) = delete;
    ~Storage() {
        if (pending && tls_pending == pending.get()) tls_pending = nullptr;  // a result nobody looked at: never computed
        if (dev) smhip_free(dev);
        delete[] host;
    }

    // host side current, device side left valid (read-only intent)
    const T *host_ro() {
        ensure();
        if (!host) host = new T[count ? count : 1];
        if (!host_valid) {
            if (dev_valid) {
                hip::DeviceGuard on(device);
                hip::check(smhip_download(host, dev, count * sizeof(T)));
            }
            host_valid = true;  // nothing valid anywhere: uninitialised, like sm::empty
        }
        return host;
    }
    // One element for reading, without mirroring the whole array: element (i) of a device-born result costs one
    // sizeof(T) copy, not a full download.
    // A loop over every element -- the reference's test idiom, `EXPECT_EQ(r(i, j, k, c), ...)` over 224 * 224 * 3 reads --
    // would be that many blocking 4-byte copies: after kFetchesBeforeMirror of them the array is mirrored once (the device
    // copy stays valid) and further reads are host reads.
    static constexpr unsigned kFetchesBeforeMirror = 8;
    T fetch(std::size_t index) {
        ensure();
        if (host_valid || !dev_valid || ++fetches > kFetchesBeforeMirror) return host_ro()[index];
        T v;
        hip::DeviceGuard on(device);
        hip::check(smhip_download(&v, static_cast<const T *>(dev) + index, sizeof(T)));
        return v;
    }
    // host side current and possibly about to be written: device side goes stale
    T *host_rw() {
        before_write();
        host_ro();
        dev_valid = false;
        return host;
    }
    // device side current, host mirror stays valid
    T *dev_ro() {
        ensure();
        if (!dev || !dev_valid) {
            hip::DeviceGuard on(device);
            if (!dev) hip::check(smhip_alloc(&dev, (count ? count : 1) * sizeof(T)));
            if (!dev_valid) {
                if (host_valid) hip::check(smhip_upload(dev, host, count * sizeof(T)));
                dev_valid = true;
            }
        }
        return static_cast<T *>(dev);
    }
    // device side current and about to be partly overwritten: host mirror goes stale
    T *dev_rw() {
        before_write();
        T *p = dev_ro();
        host_valid = false;
        return p;
    }
    // device side about to be overwritten entirely
    T *dev_wo() {
        before_write();
        if (!dev) {
            hip::DeviceGuard on(device);
            hip::check(smhip_alloc(&dev, (count ? count : 1) * sizeof(T)));
        }
        dev_valid = true;
        host_valid = false;
        return static_cast<T *>(dev);
    }
};

// What `arr.data` is.  Converts to T* / indexes like T*; touching it through a
// non-const route syncs the host mirror and marks the device copy stale.
template <typename T>
class HostPtr {
public:
    HostPtr() = default;
    HostPtr(std::shared_ptr<Storage<T>> st, std::size_t offset) : st_(std::move(st)), offset_(offset) {}

    operator T *() const { return st_ ? st_->host_rw() + offset_ : nullptr; }
    T &operator[](std::size_t i) const { return (st_->host_rw() + offset_)[i]; }
    T &operator*() const { return *(st_->host_rw() + offset_); }
    T *operator+(std::ptrdiff_t d) const { return static_cast<T *>(*this) + d; }
    explicit operator bool() const { return static_cast<bool>(st_); }
    bool operator==(std::nullptr_t) const { return !st_; }
    bool operator!=(std::nullptr_t) const { return static_cast<bool>(st_); }
    HostPtr &operator=(std::nullptr_t) {  // `arr.data = nullptr;` gives the buffer up
        st_.reset();
        offset_ = 0;
        return *this;
    }

    const T *read() const { return st_->host_ro() + offset_; }  // no invalidation
    T fetch(std::size_t i) const { return st_->fetch(offset_ + i); }  // one element, no mirror needed
    const std::shared_ptr<Storage<T>> &storage() const { return st_; }
    std::size_t offset() const { return offset_; }

private:
    std::shared_ptr<Storage<T>> st_;
    std::size_t offset_ = 0;
};

// What the array argument of + - * / binds to (implicitly, from an SMArray lvalue or rvalue).  It remembers whether the
// argument was a temporary -- only a temporary's unevaluated chain may be continued -- and its destructor marks the end
// of the full-expression (see "deferred operator chains" above).
template <typename T>
class Operand {
public:
    Operand(const SMArray<T> &a) : arr_(&a), rvalue_(false), exceptions_(std::uncaught_exceptions()) {}  // NOLINT: implicit on purpose
    Operand(SMArray<T> &&a) : arr_(&a), rvalue_(true), exceptions_(std::uncaught_exceptions()) {}       // NOLINT
    Operand(const Operand &) = delete;
    Operand &operator=(const Operand &) = delete;
    ~Operand() noexcept(false) { end_of_expression(exceptions_); }
    const SMArray<T> &array() const { return *arr_; }
    bool temporary() const { return rvalue_; }
private:
    const SMArray<T> *arr_;
    bool rvalue_;
    int exceptions_;
};
// The scalar argument of + - * / (implicitly from a T): same end-of-expression duty.
template <typename T>
class ScalarArg {
public:
    ScalarArg(T v) : value(v), exceptions_(std::uncaught_exceptions()) {}  // NOLINT: implicit on purpose
    ScalarArg(const ScalarArg &) = delete;
    ScalarArg &operator=(const ScalarArg &) = delete;
    ~ScalarArg() noexcept(false) { end_of_expression(exceptions_); }
    T value;
private:
    int exceptions_;
};

template <typename T>
struct Chain;

inline std::vector<std::size_t> dense_strides(const std::vector<std::size_t> &shape) {
    std::vector<std::size_t> st(shape.size());
    std::size_t acc = 1;
    for (std::size_t i = shape.size(); i-- > 0;) {
        st[i] = acc;
        acc *= shape[i];
    }
    return st;
}

// float, double, int and std::int64_t: the element types the axis, index, counting, condition and unique families have kernels for.
template <typename T>
inline constexpr bool four_types_v = hip::dtype_of<T>::id >= 0 && hip::dtype_of<T>::id <= SMHIP_I64;

// `axis` of an array of rank `nd`, counted from the end when negative.  Out of range: E, its message opened by the caller's `prefix`
// (the reductions, scans, argmax / argmin and sort throw std::runtime_error, take and the scatters std::invalid_argument "take: ...").
template <typename E>
int normal_axis(int axis, std::size_t nd, const char *prefix = "") {
    const int n = static_cast<int>(nd), a = axis < 0 ? axis + n : axis;
    if (a < 0 || a >= n) throw E(std::string("simpleMath/MI355X: ") + prefix + "axis " + std::to_string(axis) + " out of range for rank " + std::to_string(n));
    return a;
}

// One word of device memory that a library call writes and the host reads afterwards: a bad-index flag, a count, a sum.  Empty
// (ptr() == nullptr, nothing taken from the pool) when nobody will read it.
template <typename W = std::int64_t>
class DeviceWord {
public:
    explicit DeviceWord(bool wanted = true) {
        if (wanted) buf_ = hip::DeviceBuffer(sizeof(W));
    }
    W *ptr() const { return buf_.template as<W>(); }
    explicit operator bool() const { return buf_.get() != nullptr; }
    W read() const {  // waits for the stream
        W v{};
        hip::check(smhip_download(&v, buf_.get(), sizeof v));
        return v;
    }
private:
    hip::DeviceBuffer buf_;
};

}  // namespace detail

template <ArithmeticOrComplex T>
class SMArray {
public:
    detail::HostPtr<T> data;
    std::size_t totalSize = 0;

    SMArray(const std::initializer_list<T> &list) {
        _shape = {list.size()};
        finish_owning(new T[list.size() ? list.size() : 1]);
        std::copy(list.begin(), list.end(), static_cast<T *>(data));
    }

    SMArray(const std::initializer_list<SMArray> &list) {
        const SMArray &first = *list.begin();
        _shape.reserve(first._shape.size() + 1);
        _shape.push_back(list.size());
        _shape.insert(_shape.end(), first._shape.begin(), first._shape.end());
        finish_owning(new T[calculateTotalSize(_shape)]);
        T *dst = static_cast<T *>(data);
        for (const SMArray &child : list) {
            assert(child._shape == first._shape && "ragged nested initializer list");
            child.copy_dense_to(dst);
            dst += child.totalSize;
        }
    }

    // Takes ownership of `buffer` (allocated with new T[]), exactly like the reference.
    SMArray(T *buffer, std::vector<std::size_t> &&shape) {
        _shape = std::move(shape);
        finish_owning(buffer);
    }

    SMArray(SMArray &&other) noexcept = default;
    SMArray(const SMArray &) = delete;
    SMArray &operator=(const SMArray &) = delete;

    // Element-wise copy into an existing array of the same shape (reference SMArray.h:89-97).
    // The reference runs it as a host loop; here it is a strided device copy (smhip_copy_strided), so
    // `a(SLICE(1, 3), SLICE_ALL) = b * c;` never leaves HBM.  A source that shares storage with the
    // destination (`a = a.transpose()`) is made dense first.
    SMArray &operator=(const SMArray &&other) {
        if (_shape != other._shape) throw std::runtime_error("Shape mismatch in assignment");
        if (hip::transport_of<T>::id >= 0 && _shape.size() + (hip::transport_of<T>::lanes > 1 ? 1 : 0) <= MAX_NDIM) {
            if (totalSize == 0) return *this;
            if constexpr (hip::dtype_of<T>::id >= 0) {
                // `x = (a + b) * c;` -- the right-hand side is this thread's unevaluated temporary: evaluate it INTO x instead of
                // into a temporary that is then copied (12 instead of 20 bytes per element for `x = a + b`).  x must be a dense
                // block, and every operand that shares x's storage must be exactly x (same elements, same order: then each
                // element is read before it is written, by the same lane); anything else takes the copy below.
                if (detail::Chain<T> *c = other.continuable(); c && is_dense() && c->may_write_into(data.storage().get(), data.offset(), _shape)) {
                    detail::Storage<T> &mine = *data.storage();
                    if (mine.device == c->device || !mine.dev) {
                        mine.device = c->device;
                        mine.pending = std::move(other.data.storage()->pending);
                        c->retarget(&mine, _shape, data.offset(), data.offset() != 0 || totalSize != mine.count);
                        ++detail::tls_fusion_stats.direct_assignments;
                        mine.ensure();  // runs the chain now: an assignment is evaluated where it stands
                        return *this;
                    }
                }
            }
            hip::DeviceGuard on(common_device(*this, other));
            std::unique_ptr<SMArray> holder;
            const SMArray *src = &other;
            if (other.data.storage() == data.storage()) {
                holder.reset(new SMArray(other.contiguous()));
                src = holder.get();
            }
            auto sh = hip::to_i64(_shape), ss = hip::to_i64(src->_strides), sd = hip::to_i64(_strides);
            if (sh.empty()) { sh = {1}; ss = {1}; sd = {1}; }  // a 0-d array is one element
            lane_axis(sh, ss, &sd);
            const T *from = src->device_data();
            hip::check(smhip_copy_strided(hip::transport_of<T>::id, from, ss.data(), data.storage()->dev_rw() + data.offset(), sd.data(),
                                          sh.data(), static_cast<int>(sh.size())));
        } else {
            std::vector<T> tmp(other.totalSize ? other.totalSize : 1);
            other.copy_dense_to(tmp.data());
            T *base = static_cast<T *>(data);
            for_each_offset([&](std::size_t linear, std::size_t off) { base[off] = tmp[linear]; });
        }
        return *this;
    }

    // arr(i, j, k) -> value;  arr(i, SLICE_ALL) -> view
    template <typename... Args>
        requires((std::is_integral_v<std::remove_cvref_t<Args>> || std::is_same_v<std::remove_cvref_t<Args>, Slice>) && ...)
    auto operator()(Args &&...args) const {
        if constexpr ((std::is_integral_v<std::remove_cvref_t<Args>> && ...)) {
            return data.fetch(offset_of({static_cast<std::size_t>(args)...}, false));
        } else {
            return make_view({processIndex(std::forward<Args>(args))...});
        }
    }

    template <typename... Args>
        requires((std::is_integral_v<std::remove_cvref_t<Args>> && ...))
    T &operator()(Args &&...args) {
        return data[offset_of({static_cast<std::size_t>(args)...}, true)];
    }

    SMArray transpose() const {
        SMArray v;
        v.data = data;
        v._shape.assign(_shape.rbegin(), _shape.rend());
        v._strides.assign(_strides.rbegin(), _strides.rend());
        v.ndim = ndim;
        v.totalSize = totalSize;
        v.isView = true;
        return v;
    }

    // NumPy semantics: every element repeated `numberOfRepeats` times, flattened.  On the
    // device: a (N, r) view with strides (s, 0) gathered densely (the reference's host loop at
    // SMArray.h:138-159 writes newData[i + j], which is not a repeat -- SURVEY 8a quirk 7).
    SMArray repeat(int numberOfRepeats) const {
        assert(numberOfRepeats >= 1);
        const std::size_t r = static_cast<std::size_t>(numberOfRepeats);
        if constexpr (hip::transport_of<T>::id >= 0) {
            if (!is_dense()) return contiguous().repeat(numberOfRepeats);
            return gather({totalSize, r}, {1, 0}, {totalSize * r});  // a dense array seen as (N, r) with strides (1, 0)
        } else {  // element types without kernels (std::complex): plain host data movement
            std::vector<T> flat(totalSize ? totalSize : 1);
            copy_dense_to(flat.data());
            T *out = new T[totalSize * r ? totalSize * r : 1];
            for (std::size_t i = 0, o = 0; i < totalSize; ++i)
                for (std::size_t k = 0; k < r; ++k) out[o++] = flat[i];
            return SMArray(out, {totalSize * r});
        }
    }

    // Repeat along one axis: shape[axis] *= numberOfRepeats (a stride-0 axis inserted after `axis`).
    SMArray repeat(int numberOfRepeats, int axis) const {
        assert(axis >= 0 && axis < static_cast<int>(ndim) && numberOfRepeats >= 1);
        if (ndim == 1) return repeat(numberOfRepeats);
        const std::size_t r = static_cast<std::size_t>(numberOfRepeats);
        std::vector<std::size_t> newShape = _shape;
        newShape[axis] *= r;
        std::size_t inner = 1, outer = 1;
        for (std::size_t i = axis + 1; i < ndim; ++i) inner *= _shape[i];
        for (int i = 0; i < axis; ++i) outer *= _shape[i];
        if constexpr (hip::transport_of<T>::id >= 0) {
            if (!is_dense()) return contiguous().repeat(numberOfRepeats, axis);
            // dense: (outer, d, inner) seen as (outer, d, r, inner) with strides (d*inner, inner, 0, 1) -- rank 4 whatever ndim is
            return gather({outer, _shape[axis], r, inner}, {_shape[axis] * inner, inner, 0, 1}, std::move(newShape));
        } else {
            std::vector<T> flat(totalSize ? totalSize : 1);
            copy_dense_to(flat.data());
            T *out = new T[calculateTotalSize(newShape) ? calculateTotalSize(newShape) : 1];
            T *dst = out;
            for (std::size_t o = 0; o < outer; ++o)
                for (std::size_t j = 0; j < _shape[axis]; ++j)
                    for (std::size_t k = 0; k < r; ++k) {
                        std::memcpy(dst, flat.data() + (o * _shape[axis] + j) * inner, inner * sizeof(T));
                        dst += inner;
                    }
            return SMArray(out, std::move(newShape));
        }
    }

    // Dot product over all elements (reference SMArray.h:213-215 -> dot_product<T>).
    T operator%(const SMArray &arr) const {
        if (totalSize != arr.totalSize) throw std::runtime_error("dot product: element counts differ");
        constexpr bool c64 = std::is_same_v<T, std::complex<double>>, c32 = std::is_same_v<T, std::complex<float>>;
        static_assert(hip::dot_dtype_of<T>::id >= 0 || c64 || c32, "operator%: this element type has no gfx950 dot-product kernel (float, double, every "
                                                                   "8- to 64-bit integer type, std::complex<float> and std::complex<double> do)");
        // complex arrays are as resident as any other (16-byte elements in the same Storage): device pointers in, no host staging
        hip::DeviceGuard on(common_device(*this, arr));
        const AbiView a = flat(), b = arr.flat();
        if constexpr (c64) return hip::dot_device_c64(a.ptr, b.ptr, totalSize);
        else if constexpr (c32) return hip::dot_device_c32(a.ptr, b.ptr, totalSize);  // the generic template's instantiation, on resident arrays
        else return hip::dot_device<T>(a.ptr, b.ptr, totalSize);  // the four kernel types and the generic template's other integer types
    }

    // + - * / with an array (NumPy broadcasting) or a scalar: reference SMArray.h:217-305.  The argument types convert
    // implicitly from SMArray / T (detail::Operand, detail::ScalarArg); the && forms are chosen when the left operand
    // is a temporary, whose not-yet-evaluated chain the operator then continues (see "deferred operator chains" above):
    // `(A * row + B) * 0.5f` is one kernel and 12 bytes per element, not three and 28.
    SMArray operator+(const detail::Operand<T> &rhs) const & { return deferred<AddOp<T>>(*this, false, &rhs, T{}); }
    SMArray operator-(const detail::Operand<T> &rhs) const & { return deferred<SubtractOp<T>>(*this, false, &rhs, T{}); }
    SMArray operator*(const detail::Operand<T> &rhs) const & { return deferred<MultiplyOp<T>>(*this, false, &rhs, T{}); }
    SMArray operator/(const detail::Operand<T> &rhs) const & { return deferred<DivideOp<T>>(*this, false, &rhs, T{}); }
    SMArray operator+(const detail::Operand<T> &rhs) && { return deferred<AddOp<T>>(*this, true, &rhs, T{}); }
    SMArray operator-(const detail::Operand<T> &rhs) && { return deferred<SubtractOp<T>>(*this, true, &rhs, T{}); }
    SMArray operator*(const detail::Operand<T> &rhs) && { return deferred<MultiplyOp<T>>(*this, true, &rhs, T{}); }
    SMArray operator/(const detail::Operand<T> &rhs) && { return deferred<DivideOp<T>>(*this, true, &rhs, T{}); }
    SMArray operator+(const detail::ScalarArg<T> &val) const & { return deferred<AddOp<T>>(*this, false, nullptr, val.value); }
    SMArray operator-(const detail::ScalarArg<T> &val) const & { return deferred<SubtractOp<T>>(*this, false, nullptr, val.value); }
    SMArray operator*(const detail::ScalarArg<T> &val) const & { return deferred<MultiplyOp<T>>(*this, false, nullptr, val.value); }
    SMArray operator/(const detail::ScalarArg<T> &val) const & { return deferred<DivideOp<T>>(*this, false, nullptr, val.value); }
    SMArray operator+(const detail::ScalarArg<T> &val) && { return deferred<AddOp<T>>(*this, true, nullptr, val.value); }
    SMArray operator-(const detail::ScalarArg<T> &val) && { return deferred<SubtractOp<T>>(*this, true, nullptr, val.value); }
    SMArray operator*(const detail::ScalarArg<T> &val) && { return deferred<MultiplyOp<T>>(*this, true, nullptr, val.value); }
    SMArray operator/(const detail::ScalarArg<T> &val) && { return deferred<DivideOp<T>>(*this, true, nullptr, val.value); }

    // Broadcasted `*this Op rhs` for any Op policy: what a user-added operator calls
    // (the README's "add the operator in SMArray.h" step, without editing the class).
    template <typename Op>
    SMArray apply(const SMArray &rhs) const {
        // equal shapes need no resolving (and none of sm::broadcast's vectors): the common case, and the one that
        // matters for tiny arrays, where the operator's host work is a visible part of its few microseconds
        auto br = _shape == rhs._shape ? BroadCastResult{_shape, {}, _strides, {}, rhs._strides, totalSize}
                                       : sm::broadcast(_shape, _strides, rhs._shape, rhs._strides);
        if (br.resultShape.size() > MAX_NDIM) throw std::runtime_error("rank exceeds MAX_NDIM");
        if constexpr (hip::on_device_v<T, Op>) {
            hip::DeviceGuard on(common_device(*this, rhs));  // the kernel runs where the operands live; the result is born there
            SMArray out = device_empty(std::move(br.resultShape));
            apply_into<Op>(rhs, br, out);
            return out;
        } else {
            T *result = new T[br.totalSize ? br.totalSize : 1];
            try {
                element_wise_op<T, Op>(data.read(), br.newStrides1, rhs.data.read(), br.newStrides2, br.totalSize, result,
                                       br.resultShape);
            } catch (...) {
                delete[] result;
                throw;
            }
            return SMArray(result, std::move(br.resultShape));
        }
    }

    // `*this Op scalar` element-wise; shape preserved (reference SMArray.h:226-237 and siblings).
    template <typename Op>
    SMArray apply_scalar(T value) const {
        if constexpr (hip::on_device_v<T, Op>) {
            hip::DeviceGuard on(device());
            SMArray out = device_empty(std::vector<std::size_t>(_shape));
            apply_scalar_into<Op>(value, out);
            return out;
        } else {
            std::vector<T> flat(totalSize ? totalSize : 1);
            copy_dense_to(flat.data());
            T *result = new T[totalSize ? totalSize : 1];
            try {
                array_scalar_op<T, Op>(flat.data(), value, totalSize, result);
            } catch (...) {
                delete[] result;
                throw;
            }
            return SMArray(result, std::vector<std::size_t>(_shape));
        }
    }

private:
    // The device-side body of apply<Op>: `*this Op rhs` into `out` (dense, of br's result shape, on the operands' GPU).
    template <typename Op>
    void apply_into(const SMArray &rhs, const BroadCastResult &br, SMArray &out) const {
        {
            if (!out._shape.empty() && out.totalSize <= SMHIP_INLINE_MAX_OUTPUTS && (host_only_small() || rhs.host_only_small()) &&
                hip::device_op<Op>::id() <= SMHIP_OP_POW) {
                // a tiny operand that exists only on the host rides in the kernel's argument block: one packet instead
                // of an upload packet plus a kernel packet (smhip_elementwise_inline)
                const std::size_t ia = host_only_small(), ib = rhs.host_only_small();
                const auto sa = hip::to_i64(br.newStrides1), sb = hip::to_i64(br.newStrides2), sh = hip::to_i64(out._shape);
                hip::check(smhip_elementwise_inline(hip::device_op<Op>::id(), hip::dtype_of<T>::id,
                                                    ia ? static_cast<const void *>(data.read()) : device_data(), ia, sa.data(),
                                                    ib ? static_cast<const void *>(rhs.data.read()) : rhs.device_data(), ib, sb.data(),
                                                    sh.data(), static_cast<int>(sh.size()), out.device_data_mut()));
                if (ia) ++data.storage()->inline_uses;
                if (ib) ++rhs.data.storage()->inline_uses;
                return;
            }
            hip::element_wise_op_device<T, Op>(device_data(), br.newStrides1, rhs.device_data(), br.newStrides2,
                                               out.device_data_mut(), out._shape);
        }
    }

    // The device-side body of apply_scalar<Op>, into `out` (dense, of this array's shape).
    template <typename Op>
    void apply_scalar_into(T value, SMArray &out) const {
        {
            // The destination first: taking it runs the chain pending on this thread, and that chain may have THIS array among its
            // operands and upload it.  Whether the array is host-only (and rides inline) is decided after that, once, and the pointer
            // and the byte count passed below come from that one answer -- in an argument list their order of evaluation is not fixed,
            // and a host pointer passed with a count of 0 is read as a device pointer.
            T *dst = out.device_data_mut();
            const std::size_t host_bytes = !_shape.empty() && totalSize <= SMHIP_INLINE_MAX_OUTPUTS && hip::device_op<Op>::id() <= SMHIP_OP_POW ? host_only_small() : 0;
            if (host_bytes) {
                // host-built tiny array op scalar: both ride in the launch packet
                const auto sa = hip::to_i64(_strides), sh = hip::to_i64(_shape);
                const std::vector<std::int64_t> zeros(sh.size(), 0);
                hip::check(smhip_elementwise_inline(hip::device_op<Op>::id(), hip::dtype_of<T>::id, data.read(), host_bytes, sa.data(),
                                                    &value, sizeof(T), zeros.data(), sh.data(), static_cast<int>(sh.size()), dst));
                ++data.storage()->inline_uses;
                return;
            }
            if (is_dense()) {
                hip::array_scalar_op_device<T, Op>(device_data(), value, totalSize, dst);
            } else {  // a view: honour its strides (the reference reads views as flat here)
                hip::DeviceBuffer s(sizeof(T));
                hip::check(smhip_upload(s.get(), &value, sizeof(T)));
                hip::element_wise_op_device<T, Op>(device_data(), _strides, s.template as<T>(),
                                                   std::vector<std::size_t>(_shape.size(), 0), dst, _shape);
            }
        }
    }

public:
    [[nodiscard]] std::string toString() const {
        std::ostringstream oss;
        const T *base = data.read();
        std::function<void(std::size_t, std::size_t)> emit = [&](std::size_t offset, std::size_t dim) {
            oss << "[";
            for (std::size_t i = 0; i < _shape[dim]; ++i) {
                if (dim + 1 == _shape.size()) {
                    if (i) oss << ", ";
                    oss << base[offset + i * _strides[dim]];
                } else {
                    if (i) oss << ",\n";
                    emit(offset + i * _strides[dim], dim + 1);
                }
            }
            oss << "]";
        };
        if (_shape.empty()) return "[]";
        emit(0, 0);
        return oss.str();
    }

    [[nodiscard]] const std::vector<std::size_t> &shape() const { return _shape; }
    [[nodiscard]] const std::vector<std::size_t> &strides() const { return _strides; }

    ~SMArray() = default;  // Storage is reference-counted: the last owner/view releases it

    // ---- MI355X extensions (not in the reference) -------------------------------
    // Device pointer to this array's first element, values current.  Valid until the
    // array (and its views) die.  Work is stream-ordered on libsmhip's stream.
    // The host mirror for READING: brought up to date if needed, and -- unlike `data`, whose every use must assume a write
    // (`arr.data[i] = v` is the reference's idiom) -- the device copy stays valid, so a later operator uploads nothing.
    const T *cdata() const { return data.read(); }
    const T *device_data() const { return data.storage()->dev_ro() + data.offset(); }
    T *device_data_mut() { return data.storage()->dev_wo() + data.offset(); }
    bool is_dense() const { return is_contiguous(_shape, _strides); }
    bool is_view() const { return isView; }
    void copy_dense_out(T *dst) const { copy_dense_to(dst); }  // this array's elements, row-major, into host memory
    int device() const { return data.storage()->device; }  // the GPU this array's elements live on
    // The GPU two operands of one operator share.  Kernels run on the operands' device (the operators take a DeviceGuard on
    // it, whatever GPU the calling thread is on); operands resident on DIFFERENT GPUs cannot meet in one kernel -- peer
    // access is not assumed -- and that is an error, not a silent wrong-device launch.
    // An operand that has no device buffer yet (host-built, or a result still pending) belongs to no GPU in particular: it
    // adopts its partner's and is uploaded / born there.
    static int common_device(const SMArray &x, const SMArray &y) {
        auto &sx = *x.data.storage(), &sy = *y.data.storage();
        if (sx.device != sy.device) {
            if (!sx.dev && !sx.pending) sx.device = sy.device;
            else if (!sy.dev && !sy.pending) sy.device = sx.device;
        }
        const int dx = sx.device, dy = sy.device;
        if (dx != dy)
            throw std::runtime_error("simpleMath/MI355X: the operands live on different GPUs (" + std::to_string(dx) + " and " + std::to_string(dy) +
                                     "); bring them to one device first (sm::Sharded<T>::gather / scatter, or build both on the same GPU)");
        return dx;
    }

    // (a Op1 b) Op2 c (c == nullptr: Op2 scalar) as one recorded chain, evaluated before returning: what sm::fused is for
    // operands that broadcast against each other.
    template <typename Op1, typename Op2>
    static SMArray chain_of(const SMArray &a, const SMArray &b, const SMArray *c, T scalar) {
        detail::flush_pending();
        SMArray t = deferred_arrays<Op1>(a, false, &b, false, T{});
        SMArray r = deferred_arrays<Op2>(t, true, c, false, scalar);
        detail::flush_pending();
        return r;
    }

    // A new dense array whose elements exist only in HBM so far.
    static SMArray device_empty(std::vector<std::size_t> &&shape) {
        SMArray a;
        a._shape = std::move(shape);
        a._strides = detail::dense_strides(a._shape);
        a.ndim = a._shape.size();
        a.totalSize = calculateTotalSize(a._shape);
        a.data = detail::HostPtr<T>(std::make_shared<detail::Storage<T>>(a.totalSize), 0);
        return a;
    }
    static SMArray device_full(std::vector<std::size_t> &&shape, T value) {
        SMArray a = device_empty(std::move(shape));
        if constexpr (hip::dtype_of<T>::id >= 0) {
            hip::check(smhip_fill(hip::dtype_of<T>::id, a.device_data_mut(), &value, a.totalSize));
        } else {
            T *h = static_cast<T *>(a.data);
            for (std::size_t i = 0; i < a.totalSize; ++i) h[i] = value;
        }
        return a;
    }
    // Dense copy of a (possibly strided) array, made on the device.
    SMArray contiguous() const {
        if (hip::transport_of<T>::id >= 0 && _shape.size() + (hip::transport_of<T>::lanes > 1 ? 1 : 0) <= MAX_NDIM) {
            return gather(_shape, _strides, std::vector<std::size_t>(_shape));
        } else {
            T *out = new T[totalSize ? totalSize : 1];
            copy_dense_to(out);
            return SMArray(out, std::vector<std::size_t>(_shape));
        }
    }
    // Sum of all elements, accumulated in fp64 on the device.
    // ... of a TEMPORARY: sm::pow(a - b, 2.0f).sum().  The unevaluated result of this expression's chain, which nobody can look
    // at afterwards, is not computed at all: its sum is taken in the chain's own pass (smhip_chain_sum).  (Only the rvalue form:
    // a named array -- a by-value parameter bound to such a temporary -- may be read again after its sum.)
    double sum() && {
        static_assert(hip::dtype_of<T>::id >= 0, "sum(): element type has no kernels");
        if (detail::Chain<T> *c = pending_temporary()) return c->run_sum();
        return static_cast<const SMArray &>(*this).sum();
    }
    double sum() const & {
        static_assert(hip::dtype_of<T>::id >= 0, "sum(): element type has no kernels");
        hip::DeviceGuard on(device());
        const AbiView in = flat();
        double s = 0;
        hip::check(smhip_sum(hip::dtype_of<T>::id, in.ptr, totalSize, &s));
        return s;
    }

    // Reductions ALONG AXES (np.sum / np.mean / np.max / np.min with `axis`), resident on the device like every result:
    //   sum   f32: fp64 accumulation, rounded once; f64: fp64; integers: wrapping in T (np.sum(x, axis, dtype=T))
    //   mean  fp64 sum / count, rounded once (floating-point T only: a static_assert)
    //   max / min  exact, NaN propagates
    // `axis` counts from the end when negative; a list names several axes.  A bad or repeated axis throws std::runtime_error.
    // keepdims = true keeps each reduced axis as an extent of 1 (the result then broadcasts straight back into an operator
    // chain: `(n - n.mean(0, true)) / s`); reducing every axis without keepdims gives shape {1} -- SMArray has no 0-d form.
    // A pending operator chain as the operand is evaluated first; the reduction is ONE smhip_reduce_axes call (counted in
    // sm::fusion_stats().reductions).  The whole-array `double sum()` above is unchanged.
    SMArray sum(int axis, bool keepdims = false) const { return reduce_along(SMHIP_REDUCE_SUM, {axis}, keepdims); }
    SMArray sum(std::initializer_list<int> axes, bool keepdims = false) const { return reduce_along(SMHIP_REDUCE_SUM, axes, keepdims); }
    SMArray mean(int axis, bool keepdims = false) const { return mean(std::initializer_list<int>{axis}, keepdims); }
    SMArray mean(std::initializer_list<int> axes, bool keepdims = false) const {
        static_assert(std::is_floating_point_v<T>, "mean(): the mean of an integer type is not offered (sum() and divide)");
        return reduce_along(SMHIP_REDUCE_MEAN, axes, keepdims);
    }
    SMArray max(int axis, bool keepdims = false) const { return reduce_along(SMHIP_REDUCE_MAX, {axis}, keepdims); }
    SMArray max(std::initializer_list<int> axes, bool keepdims = false) const { return reduce_along(SMHIP_REDUCE_MAX, axes, keepdims); }
    SMArray min(int axis, bool keepdims = false) const { return reduce_along(SMHIP_REDUCE_MIN, {axis}, keepdims); }
    SMArray min(std::initializer_list<int> axes, bool keepdims = false) const { return reduce_along(SMHIP_REDUCE_MIN, axes, keepdims); }

    // Cumulative scans ALONG AN AXIS (np.cumsum / np.cumprod / np.maximum.accumulate / np.minimum.accumulate): the result has
    // the shape of this array, element r along `axis` holding the fold of elements 0 .. r, resident on the device.
    //   cumsum / cumprod   f32: the running value held in fp64, each output rounded once; f64: fp64; integers: wrapping in T
    //   cummax / cummin    exact; from a NaN on, every later output along the axis is NaN
    // `axis` counts from the end when negative; an axis out of range throws std::runtime_error.  Without an axis the elements
    // are scanned in row-major order and the result has shape {totalSize}, as np.cumsum(a) does.  A pending operator chain as
    // the operand is evaluated first; the scan is ONE smhip_scan_axis call (counted in sm::fusion_stats().scans) and its
    // result feeds the next chain like any array: `h.cumsum(0) / h.sum(0, true)` is a CDF.
    SMArray cumsum(int axis) const { return scan_of(SMHIP_SCAN_SUM, axis); }
    SMArray cumprod(int axis) const { return scan_of(SMHIP_SCAN_PROD, axis); }
    SMArray cummax(int axis) const { return scan_of(SMHIP_SCAN_MAX, axis); }
    SMArray cummin(int axis) const { return scan_of(SMHIP_SCAN_MIN, axis); }
    SMArray cumsum() const { return scan_of(SMHIP_SCAN_SUM, std::nullopt); }
    SMArray cumprod() const { return scan_of(SMHIP_SCAN_PROD, std::nullopt); }
    SMArray cummax() const { return scan_of(SMHIP_SCAN_MAX, std::nullopt); }
    SMArray cummin() const { return scan_of(SMHIP_SCAN_MIN, std::nullopt); }

    // WHERE the maximum / minimum along an axis stands (np.argmax / np.argmin): positions along `axis` as std::int64_t, the
    // first one on a tie (-0 == +0) and the first NaN if the axis holds one; resident on the device.  `axis` counts from the
    // end when negative, an axis out of range throws std::runtime_error, keepdims keeps the axis as an extent of 1.  Without
    // an axis the result is the row-major index into this array, shape {1} (a view that is not dense is copied dense first).
    // A pending operator chain as the operand is evaluated first, a transposed view is read in place; ONE
    // smhip_argreduce_axis call (counted in sm::fusion_stats().arg_reductions).  max_with_index / min_with_index give
    // {the extreme itself, its position} from the same single pass; the value is exactly the element at that position.
    SMArray<std::int64_t> argmax(int axis, bool keepdims = false) const { return arg_of(SMHIP_ARG_MAX, axis, keepdims, false).second; }
    SMArray<std::int64_t> argmin(int axis, bool keepdims = false) const { return arg_of(SMHIP_ARG_MIN, axis, keepdims, false).second; }
    SMArray<std::int64_t> argmax() const { return arg_of(SMHIP_ARG_MAX, std::nullopt, false, false).second; }
    SMArray<std::int64_t> argmin() const { return arg_of(SMHIP_ARG_MIN, std::nullopt, false, false).second; }
    std::pair<SMArray, SMArray<std::int64_t>> max_with_index(int axis, bool keepdims = false) const { return arg_of(SMHIP_ARG_MAX, axis, keepdims, true); }
    std::pair<SMArray, SMArray<std::int64_t>> min_with_index(int axis, bool keepdims = false) const { return arg_of(SMHIP_ARG_MIN, axis, keepdims, true); }

    // The NORMALISATION those pipelines start from, fused per line: softmax(x)_r = exp(x_r - m) / S, log_softmax(x)_r = (x_r - m) - ln S and
    // logsumexp(x) = m + ln S along `axis`, with m the line's maximum and S the fp64 sum of the exp(x_r - m); float and double only (a
    // static_assert).  softmax and log_softmax have this array's shape; logsumexp has the kept shape (keepdims keeps the axis as an
    // extent of 1), and without an axis runs over the row-major flattening, shape {1}.  A NaN in a line, or a maximum that is not
    // finite, gives NaN (logsumexp: the maximum itself); the differences are formed in fp64, every result is rounded once
    // (smhip.h, "softmax", has the bounds).  `axis` counts from the end when negative and is the last one by default; an axis out of
    // range throws std::runtime_error.  The operand may be a view (a transposed one is read in place) or a pending operator chain
    // (evaluated first); each is ONE smhip_softmax_axis call (counted in sm::fusion_stats().softmaxes) whose result stays on the
    // device and feeds the next chain, argmax or take_along_axis.
    SMArray softmax(int axis = -1) const { return softmax_of(SMHIP_SOFTMAX, axis, false); }
    SMArray log_softmax(int axis = -1) const { return softmax_of(SMHIP_LOG_SOFTMAX, axis, false); }
    SMArray logsumexp(int axis, bool keepdims = false) const { return softmax_of(SMHIP_LOGSUMEXP, axis, keepdims); }
    SMArray logsumexp() const { return softmax_of(SMHIP_LOGSUMEXP, std::nullopt, false); }

    // The SECOND MOMENT along axes (np.var / np.std with `axis` and `ddof`), centred in fp64: the fp64 mean, d = x - mean in fp64,
    // M2 = sum d^2 - (sum d)^2 / N, var = M2 / (N - ddof) and stddev its fp64 square root, each rounded once; float and double only (a
    // static_assert; astype first).  Data on a large offset keep every digit (smhip.h, "var / std / standardize", has the bounds), a
    // constant line gives exactly +0, a NaN or an infinity in a line NaN.  var_mean returns {var, mean} from one call, the mean bit for
    // bit mean(axes)'s.  standardize(axis, eps, ddof) is (x - mean) / sqrt(var + eps) along ONE axis (the last by default), of this
    // array's shape, the statistics and the quotient in fp64: layer normalisation without its affine part, in one read for a line the
    // library holds in registers.  Axes count from the end when negative; keepdims keeps each reduced axis as an extent of 1; the forms
    // without an axis run over the row-major flattening and give shape {1}.  A bad or repeated axis, ddof < 0, N - ddof <= 0 (with
    // something to write) and a negative, NaN or infinite eps throw std::runtime_error.  A pending operator chain as the operand is
    // evaluated first; each is ONE library call (counted in sm::fusion_stats().moments) whose result stays on the device.
    SMArray var(int axis, std::int64_t ddof = 0, bool keepdims = false) const { return var(std::initializer_list<int>{axis}, ddof, keepdims); }
    SMArray var(std::initializer_list<int> axes, std::int64_t ddof = 0, bool keepdims = false) const { return moments_of(SMHIP_MOMENT_VAR, &axes, ddof, keepdims, false).first; }
    SMArray var() const { return moments_of(SMHIP_MOMENT_VAR, nullptr, 0, false, false).first; }
    SMArray stddev(int axis, std::int64_t ddof = 0, bool keepdims = false) const { return stddev(std::initializer_list<int>{axis}, ddof, keepdims); }
    SMArray stddev(std::initializer_list<int> axes, std::int64_t ddof = 0, bool keepdims = false) const { return moments_of(SMHIP_MOMENT_STD, &axes, ddof, keepdims, false).first; }
    SMArray stddev() const { return moments_of(SMHIP_MOMENT_STD, nullptr, 0, false, false).first; }
    std::pair<SMArray, SMArray> var_mean(int axis, std::int64_t ddof = 0, bool keepdims = false) const { return var_mean(std::initializer_list<int>{axis}, ddof, keepdims); }
    std::pair<SMArray, SMArray> var_mean(std::initializer_list<int> axes, std::int64_t ddof = 0, bool keepdims = false) const { return moments_of(SMHIP_MOMENT_VAR, &axes, ddof, keepdims, true); }
    std::pair<SMArray, SMArray> var_mean() const { return moments_of(SMHIP_MOMENT_VAR, nullptr, 0, false, true); }
    SMArray standardize(int axis = -1, double eps = 0.0, std::int64_t ddof = 0) const {
        static_assert(std::is_floating_point_v<T>, "standardize: float and double only (astype first)");
        const int a = detail::normal_axis<std::runtime_error>(axis, _shape.size());
        if (!(eps >= 0.0) || eps > std::numeric_limits<double>::max()) throw std::runtime_error("simpleMath/MI355X: standardize: eps is negative, NaN or infinite");
        if (ddof < 0) throw std::runtime_error("simpleMath/MI355X: standardize: ddof " + std::to_string(ddof) + " is negative");
        if (totalSize && static_cast<std::int64_t>(_shape[a]) - ddof <= 0)
            throw std::runtime_error("simpleMath/MI355X: standardize: N - ddof = " + std::to_string(_shape[a]) + " - " + std::to_string(ddof) + " is not positive");
        hip::DeviceGuard on(device());
        const AbiView in = along_axis(a);  // a pending chain that produces this operand runs here
        SMArray out = device_empty(std::vector<std::size_t>(_shape));
        hip::check(smhip_standardize_axis(hip::dtype_of<T>::id, in.ptr, in.shape.data(), in.strides.data(), in.ndim(), in.axis, eps, ddof, out.device_data_mut()));
        ++detail::tls_fusion_stats.moments;
        return out;
    }

    // The ORDER along an axis (np.sort / np.argsort with kind="stable"): sort gives the elements of each line in order, argsort
    // their positions along `axis` as std::int64_t; both have this array's shape and are resident on the device.  Ascending puts
    // the smaller values first and NaNs last (-0 == +0, all NaNs tie); descending = true puts NaNs, then the larger values first.
    // In both orders tied elements keep the order of their positions, so descending is not the ascending result reversed: its
    // first element is where argmax points.  The sorted values are the operand's own bits (which zero, which NaN).  `axis`
    // counts from the end when negative and is the last one by default; an axis out of range throws std::runtime_error.
    // sort_flat / argsort_flat sort the row-major flattening, shape {totalSize}.  A pending operator chain as the operand is
    // evaluated first; each is ONE smhip_sort_axis call (counted in sm::fusion_stats().sorts), sort_with_index giving {values,
    // positions} from the same call.  The result feeds the next chain or a slice like any array: `x.sort(-1)(SLICE_ALL,
    // SLICE(0, 5))` is a view of the five smallest of each row.
    SMArray sort(int axis = -1, bool descending = false) const { return sort_of(axis, descending, true, false).first; }
    SMArray<std::int64_t> argsort(int axis = -1, bool descending = false) const { return sort_of(axis, descending, false, true).second; }
    std::pair<SMArray, SMArray<std::int64_t>> sort_with_index(int axis = -1, bool descending = false) const { return sort_of(axis, descending, true, true); }
    SMArray sort_flat(bool descending = false) const { return sort_of(std::nullopt, descending, true, false).first; }
    SMArray<std::int64_t> argsort_flat(bool descending = false) const { return sort_of(std::nullopt, descending, false, true).second; }

    // The k FIRST of that order without sorting the line: {values, positions}, bit for bit the first k along `axis` of
    // sort_with_index(axis, largest), of this array's shape with k on `axis` (topk_flat: of the row-major flattening, shape {k}).
    // largest = true gives NaNs, then the k largest, entry 0 where argmax points; largest = false the k smallest, NaNs last; equal
    // elements come in rising position, and the results are always in that order.  The operand may be a view or a pending chain
    // (evaluated first); each is ONE smhip_topk_axis call (counted in sm::fusion_stats().topks) whose results stay on the device and
    // feed the next chain, take_along_axis or put_along_axis.  A negative axis counts from the end; an axis out of range or a k
    // above the axis' extent throws std::invalid_argument.
    std::pair<SMArray, SMArray<std::int64_t>> topk(std::size_t k, int axis = -1, bool largest = true) const { return topk_of(k, axis, largest); }
    std::pair<SMArray, SMArray<std::int64_t>> topk_flat(std::size_t k, bool largest = true) const { return topk_of(k, std::nullopt, largest); }

    // ORDER STATISTICS along an axis without sorting the line (np.quantile / np.percentile / np.median): the element of the ordered line
    // at position (R - 1) q, interpolated in fp64 and rounded once where that falls between two (quantile_method; smhip.h, "quantile",
    // has the rules); float and double only (a static_assert; astype first).  A line that holds a NaN gives NaN, every zero is read as
    // +0.  A single q gives the kept shape (keepdims keeps the axis as an extent of 1); a list of Q gives a leading axis of Q in front
    // of it, from ONE read of the operand; the forms without an axis run over the row-major flattening and give shape {1}, or {Q}.
    // `axis` counts from the end when negative.  The operand may be a view or a pending chain (evaluated first); each is ONE
    // smhip_quantile_axis call (counted in sm::fusion_stats().quantiles) whose result stays on the device and feeds the next chain:
    // `(x - x.median(-1, true)) / (x.quantile(0.75, -1, m, true) - x.quantile(0.25, -1, m, true))`.  An axis out of range, a q outside
    // [0, 1] or NaN, an empty list and an empty axis with a result that is not empty throw std::invalid_argument.
    SMArray quantile(double q, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) const { return quantile_of(&q, 1, false, axis, method, keepdims, 1.0, "quantile: "); }
    SMArray quantile(std::initializer_list<double> q, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) const { return quantile_of(q.begin(), q.size(), true, axis, method, keepdims, 1.0, "quantile: "); }
    SMArray quantile(const std::vector<double> &q, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) const { return quantile_of(q.data(), q.size(), true, axis, method, keepdims, 1.0, "quantile: "); }
    SMArray quantile(double q, quantile_method method = quantile_method::linear) const { return quantile_of(&q, 1, false, std::nullopt, method, false, 1.0, "quantile: "); }
    SMArray quantile(std::initializer_list<double> q, quantile_method method = quantile_method::linear) const { return quantile_of(q.begin(), q.size(), true, std::nullopt, method, false, 1.0, "quantile: "); }
    SMArray quantile(const std::vector<double> &q, quantile_method method = quantile_method::linear) const { return quantile_of(q.data(), q.size(), true, std::nullopt, method, false, 1.0, "quantile: "); }
    SMArray percentile(double p, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) const { return quantile_of(&p, 1, false, axis, method, keepdims, 100.0, "percentile: "); }
    SMArray percentile(std::initializer_list<double> p, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) const { return quantile_of(p.begin(), p.size(), true, axis, method, keepdims, 100.0, "percentile: "); }
    SMArray percentile(const std::vector<double> &p, int axis, quantile_method method = quantile_method::linear, bool keepdims = false) const { return quantile_of(p.data(), p.size(), true, axis, method, keepdims, 100.0, "percentile: "); }
    SMArray percentile(const std::vector<double> &p, quantile_method method = quantile_method::linear) const { return quantile_of(p.data(), p.size(), true, std::nullopt, method, false, 100.0, "percentile: "); }
    SMArray percentile(double p, quantile_method method = quantile_method::linear) const { return quantile_of(&p, 1, false, std::nullopt, method, false, 100.0, "percentile: "); }
    SMArray percentile(std::initializer_list<double> p, quantile_method method = quantile_method::linear) const { return quantile_of(p.begin(), p.size(), true, std::nullopt, method, false, 100.0, "percentile: "); }
    SMArray median(int axis, bool keepdims = false) const { const double q = 0.5; return quantile_of(&q, 1, false, axis, quantile_method::linear, keepdims, 1.0, "median: "); }
    SMArray median() const { const double q = 0.5; return quantile_of(&q, 1, false, std::nullopt, quantile_method::linear, false, 1.0, "median: "); }

    // PICKING BY POSITION along an axis (np.take_along_axis / np.take): the consumer of what argmax, argsort and sort_with_index
    // produce.  take_along_axis: `idx` is an SMArray<std::int64_t> of this array's rank whose other axes equal this array's
    // or broadcast against them; result[..., j, ...] = (*this)[..., idx[..., j, ...], ...], of the broadcast shape with idx's
    // extent on `axis`.  Without an axis both are flattened row-major.  take: `idx` is 1-D and the result has this array's
    // shape with `axis` replaced by idx.size(); take_flat indexes the row-major flattening and gives shape {idx.size()}.
    // `axis` counts from the end when negative; a bad axis, a rank mismatch or shapes that do not broadcast throw
    // std::invalid_argument.  Both operands may be views or pending chains (evaluated first); the result is a dense array in
    // HBM holding the operand's own bits, and feeds the next chain.  Each is ONE smhip_take_axis call (sm::fusion_stats().takes).
    // index_mode::checked (the default) behaves like numpy: after the launch the one-word flag is downloaded -- a stream
    // synchronisation -- and std::out_of_range is thrown if an index was outside [-R, R).  clip and wrap never wait; indices
    // that came from argsort / argmax are valid by construction, so clip costs nothing there.
    SMArray take_along_axis(const SMArray<std::int64_t> &idx, int axis, index_mode mode = index_mode::checked) const {
        const std::size_t nd = _shape.size();
        if (idx.shape().size() != nd)
            throw std::invalid_argument("simpleMath/MI355X: take_along_axis: the index array has rank " + std::to_string(idx.shape().size()) +
                                        ", the operand rank " + std::to_string(nd));
        const int ax = detail::normal_axis<std::invalid_argument>(axis, nd, "take: ");
        hip::DeviceGuard on(device());
        std::vector<std::int64_t> shape(nd), sa(nd), si(nd);
        std::vector<std::size_t> result(nd);
        for (std::size_t d = 0; d < nd; ++d) {
            const std::size_t na = _shape[d], ni = idx.shape()[d];
            if (static_cast<int>(d) == ax) {
                result[d] = ni, sa[d] = static_cast<std::int64_t>(_strides[d]), si[d] = static_cast<std::int64_t>(idx.strides()[d]);
            } else {
                if (na != ni && na != 1 && ni != 1)
                    throw std::invalid_argument("simpleMath/MI355X: take_along_axis: the shapes do not broadcast at axis " + std::to_string(d));
                result[d] = na == 1 ? ni : na;
                sa[d] = na == result[d] && na != 1 ? static_cast<std::int64_t>(_strides[d]) : 0;
                si[d] = ni == result[d] && ni != 1 ? static_cast<std::int64_t>(idx.strides()[d]) : 0;
            }
            shape[d] = static_cast<std::int64_t>(result[d]);
        }
        return take_run(device_data(), idx.device_data(), shape, sa, si, ax, _shape[ax], mode, std::move(result));
    }
    SMArray take_along_axis(const SMArray<std::int64_t> &idx, index_mode mode = index_mode::checked) const {
        return take_flat_of(idx, mode);
    }
    SMArray take(const SMArray<std::int64_t> &idx, int axis, index_mode mode = index_mode::checked) const {
        if (idx.shape().size() != 1) throw std::invalid_argument("simpleMath/MI355X: take: the index array must be 1-D");
        const std::size_t nd = _shape.size();
        const int ax = detail::normal_axis<std::invalid_argument>(axis, nd, "take: ");
        hip::DeviceGuard on(device());
        std::vector<std::int64_t> shape = hip::to_i64(_shape), sa = hip::to_i64(_strides), si(nd, 0);
        std::vector<std::size_t> result(_shape);
        result[ax] = idx.totalSize, shape[ax] = static_cast<std::int64_t>(idx.totalSize), si[ax] = static_cast<std::int64_t>(idx.strides()[0]);
        return take_run(device_data(), idx.device_data(), shape, sa, si, ax, _shape[ax], mode, std::move(result));
    }
    SMArray take_flat(const SMArray<std::int64_t> &idx, index_mode mode = index_mode::checked) const {
        if (idx.shape().size() != 1) throw std::invalid_argument("simpleMath/MI355X: take_flat: the index array must be 1-D");
        return take_flat_of(idx, mode);
    }

    // WRITING BY POSITION along an axis, IN PLACE on this array (np.put_along_axis / np.put, np.add.at; torch's scatter_add_ /
    // index_add_): the transpose of take.  put_along_axis / scatter_add: `idx` is an SMArray<std::int64_t> of this array's rank
    // whose other axes equal this array's or are 1; (*this)[..., pick(idx[..., j, ...]), ...] = (or +=) values[..., j, ...];
    // `values` broadcasts against the walk shape (this array's shape with idx's extent on `axis`) or is a scalar T.  Without an
    // axis the array and idx are flattened row-major, and so are the values: in the flat forms (this one and put_flat) they have
    // idx's element count, or one element, or are a scalar -- nothing else broadcasts against a line.  put / index_add: `ids` is 1-D, `values` has this array's shape with `axis`
    // replaced by ids.size(), or broadcasts to it, or is a scalar; put_flat indexes the row-major flattening.
    // The rule for duplicates is fixed by the data, so the result is the same bits on every run: PUT -- among the entries of a
    // line that name the same position the one with the largest j wins (numpy's sequential assignment); ADD -- a destination's
    // contributions are added one by one in ascending j, f32 in fp64 rounded once.  unique = true is the caller's promise that
    // no two entries of a line name the same position (a permutation from argsort, an argmax with keepdims): one launch, no sort.
    // `axis` counts from the end when negative; a bad axis, a rank mismatch or shapes that do not broadcast throw
    // std::invalid_argument.  Operands may be views or pending chains (evaluated first).  A target that is not dense row-major
    // (a strided slice, a transpose) is staged: dense copy, scatter, strided assignment back.  Each is ONE smhip_scatter_axis call
    // (sm::fusion_stats().scatters).  index_mode::checked (the default): negatives count from the end, an entry outside [-R, R) is
    // DROPPED, and after the launches the one-word flag is downloaded -- a stream synchronisation -- and std::out_of_range thrown;
    // THE VALID ENTRIES HAVE BEEN APPLIED BY THEN.  clip and wrap never wait.  All forms return *this.
    SMArray &put_along_axis(const SMArray<std::int64_t> &idx, const SMArray &values, int axis, index_mode mode = index_mode::checked, bool unique = false) {
        return scatter_along(SMHIP_SCATTER_PUT, idx, &values, T{}, axis, mode, unique);
    }
    SMArray &put_along_axis(const SMArray<std::int64_t> &idx, T value, int axis, index_mode mode = index_mode::checked, bool unique = false) {
        return scatter_along(SMHIP_SCATTER_PUT, idx, nullptr, value, axis, mode, unique);
    }
    SMArray &put_along_axis(const SMArray<std::int64_t> &idx, const SMArray &values, index_mode mode = index_mode::checked, bool unique = false) {
        return scatter_flat(SMHIP_SCATTER_PUT, idx, &values, T{}, mode, unique);
    }
    SMArray &put_along_axis(const SMArray<std::int64_t> &idx, T value, index_mode mode = index_mode::checked, bool unique = false) {
        return scatter_flat(SMHIP_SCATTER_PUT, idx, nullptr, value, mode, unique);
    }
    SMArray &scatter_add(const SMArray<std::int64_t> &idx, const SMArray &values, int axis, index_mode mode = index_mode::checked, bool unique = false) {
        return scatter_along(SMHIP_SCATTER_ADD, idx, &values, T{}, axis, mode, unique);
    }
    SMArray &scatter_add(const SMArray<std::int64_t> &idx, T value, int axis, index_mode mode = index_mode::checked, bool unique = false) {
        return scatter_along(SMHIP_SCATTER_ADD, idx, nullptr, value, axis, mode, unique);
    }
    SMArray &put(const SMArray<std::int64_t> &ids, const SMArray &values, int axis, index_mode mode = index_mode::checked, bool unique = false) {
        return scatter_ids(SMHIP_SCATTER_PUT, ids, &values, T{}, axis, mode, unique);
    }
    SMArray &put(const SMArray<std::int64_t> &ids, T value, int axis, index_mode mode = index_mode::checked, bool unique = false) {
        return scatter_ids(SMHIP_SCATTER_PUT, ids, nullptr, value, axis, mode, unique);
    }
    SMArray &put_flat(const SMArray<std::int64_t> &ids, const SMArray &values, index_mode mode = index_mode::checked, bool unique = false) {
        if (ids.shape().size() != 1) throw std::invalid_argument("simpleMath/MI355X: put_flat: the index array must be 1-D");
        return scatter_flat(SMHIP_SCATTER_PUT, ids, &values, T{}, mode, unique);
    }
    SMArray &put_flat(const SMArray<std::int64_t> &ids, T value, index_mode mode = index_mode::checked, bool unique = false) {
        if (ids.shape().size() != 1) throw std::invalid_argument("simpleMath/MI355X: put_flat: the index array must be 1-D");
        return scatter_flat(SMHIP_SCATTER_PUT, ids, nullptr, value, mode, unique);
    }
    SMArray &index_add(const SMArray<std::int64_t> &ids, const SMArray &values, int axis, index_mode mode = index_mode::checked, bool unique = false) {
        return scatter_ids(SMHIP_SCATTER_ADD, ids, &values, T{}, axis, mode, unique);
    }
    SMArray &index_add(const SMArray<std::int64_t> &ids, T value, int axis, index_mode mode = index_mode::checked, bool unique = false) {
        return scatter_ids(SMHIP_SCATTER_ADD, ids, nullptr, value, axis, mode, unique);
    }

    // COUNTING (np.searchsorted, np.bincount, np.histogram).  The results are SMArray<std::int64_t>, resident on the device, and
    // feed the next chain like any array.  Values are ordered as sort() orders them ascending: -0 == +0, every NaN after every
    // number, NaNs equal among themselves.
    //   edges.searchsorted(x, side)   *this is the 1-D table of edges, sorted ascending; the result has x's shape and holds, for
    //                                 every element of x, the first i with !(edges[i] before x) (side::left) or the first i with
    //                                 x before edges[i] (side::right), in [0, edges.size()].
    //   ids.bincount(nbins, mode)     *this holds int or std::int64_t ids, read row-major; result[p] = how many of them name position
    //                                 p of nbins.  The same bits as index_add of 1 onto nbins zeros, in every mode.  checked (the
    //                                 default): negatives count from the end, an id outside [-nbins, nbins) is DROPPED and, after the
    //                                 flag word is downloaded -- a stream synchronisation --, std::out_of_range is thrown; clip and wrap
    //                                 never wait.  The length is never inferred from the data: write sm::max of the ids if you want it.
    //   x.histogram(bins, lo, hi)     {counts, edges} of `bins` equal bins over [lo, hi] (float and double): np.histogram(x, bins,
    //                                 range=(lo, hi)), with numpy's own edges, np.linspace(lo, hi, bins + 1) rounded to T, computed on
    //                                 the host and uploaded.  lo == hi stands for (lo - 0.5, hi + 0.5).
    //   x.histogram(edges)            counts between explicit edges (1-D, non-decreasing, at least two; any of the four types).
    //                                 The bin of a value is searchsorted(edges, v, side::right) - 1; a value equal to the last edge
    //                                 goes to the last bin; values outside the edges and NaNs are not counted.
    // Integer counts are summed with atomic adds: integer addition commutes, so every run gives the same bits.  Operands may be
    // views (copied dense first) or pending chains (evaluated first).  std::invalid_argument: 0 bins with entries to count, a
    // negative count, a table that is not 1-D, and where numpy raises for a range -- bins < 1, lo or hi not finite, lo > hi, edges
    // that do not increase once rounded to T.  Each is ONE library call (sm::fusion_stats().counts).
    SMArray<std::int64_t> searchsorted(const SMArray &x, side s = side::left) const {
        static_assert(detail::four_types_v<T>, "searchsorted: f32, f64, i32 and i64");
        if (_shape.size() != 1) throw std::invalid_argument("simpleMath/MI355X: searchsorted: the edges must be 1-D");
        hip::DeviceGuard on(common_device(*this, x));
        const AbiView edges = flat();
        const AbiView in = x.along_axis(0);  // a pending chain that produces the operand runs here
        Index out = Index::device_empty(std::vector<std::size_t>(x._shape));
        if (out.totalSize == 0) return out;
        hip::check(smhip_searchsorted(static_cast<int>(s), hip::dtype_of<T>::id, edges.ptr, static_cast<std::int64_t>(totalSize), in.ptr, in.shape.data(),
                                      in.strides.data(), in.ndim(), out.device_data_mut()));
        ++detail::tls_fusion_stats.counts;
        return out;
    }
    SMArray<std::int64_t> bincount(std::int64_t nbins, index_mode mode = index_mode::checked) const {
        static_assert(std::is_same_v<T, int> || std::is_same_v<T, std::int64_t>, "bincount: the ids are int or std::int64_t");
        if (nbins < 0 || (nbins == 0 && totalSize != 0))
            throw std::invalid_argument("simpleMath/MI355X: bincount: cannot count " + std::to_string(totalSize) + " ids into " + std::to_string(nbins) + " bins");
        hip::DeviceGuard on(device());
        const AbiView ids = along_axis(0);  // a pending chain that produces the ids runs here
        Index out = Index::device_empty(std::vector<std::size_t>{static_cast<std::size_t>(nbins)});
        if (nbins == 0) return out;
        const detail::DeviceWord<> flag(mode == index_mode::checked && totalSize != 0);  // only when someone will read it
        hip::check(smhip_bincount(static_cast<int>(mode), hip::dtype_of<T>::id, ids.ptr, ids.shape.data(), ids.strides.data(), ids.ndim(), nbins,
                                  out.device_data_mut(), flag.ptr()));
        ++detail::tls_fusion_stats.counts;
        if (flag && flag.read()) throw std::out_of_range("simpleMath/MI355X: bincount: an id is out of bounds for " + std::to_string(nbins) + " bins");
        return out;
    }
    std::pair<SMArray<std::int64_t>, SMArray> histogram(std::int64_t bins, double lo, double hi) const {
        static_assert(std::is_floating_point_v<T>, "histogram over a range: float and double");
        std::unique_ptr<T[]> table(bins >= 1 ? new T[static_cast<std::size_t>(bins) + 1] : nullptr);
        const int rc = smhip_histogram_edges(hip::dtype_of<T>::id, bins, lo, hi, table.get());
        if (rc == SMHIP_ERR_INVALID) throw std::invalid_argument(std::string("simpleMath/MI355X: ") + smhip_last_error());
        hip::check(rc);
        SMArray edges(table.release(), std::vector<std::size_t>{static_cast<std::size_t>(bins) + 1});
        Index counts = count_between(edges, SMHIP_HISTOGRAM_UNIFORM, lo, hi);
        return {std::move(counts), std::move(edges)};
    }
    SMArray<std::int64_t> histogram(const SMArray &edges) const {
        if (edges._shape.size() != 1 || edges.totalSize < 2)
            throw std::invalid_argument("simpleMath/MI355X: histogram: the edges must be 1-D and at least two");
        return count_between(edges, 0, 0.0, 0.0);
    }

    // CHOOSING BY CONDITION (np.where, np.putmask, np.count_nonzero, np.flatnonzero, np.nonzero, a[mask]).  A condition is what the
    // comparison operators below the class give -- `a > 0.0f`, `a <= b`, `0 == a` -- a sm::Cond<T>, evaluated inside the kernel that
    // consumes it (the mask is never written to HBM); an SMArray<T> where a condition is expected stands for "nonzero".  Semantics are
    // numpy's: a comparison with a NaN is false except !=, -0.0 == +0.0, a NaN is nonzero.  Operands may be views (copied dense
    // first) or pending chains (evaluated first).
    //   sm::where(c, a, b)        c ? a : b, a and b each an array or a T, everything broadcasting by numpy's rule; a dense array
    //                             holding the chosen operand's own bits.  Asynchronous.
    //   x.assign_where(c, v)      np.putmask / x[mask] = v, in place; c and v broadcast to x's shape.  A target that is not dense is
    //                             staged like put.  Returns x.  Asynchronous.
    //   sm::mask(c)               where(c, T{1}, T{0}): conditions then combine with the arithmetic operators.
    //   sm::count_nonzero(c), sm::flatnonzero(c), sm::nonzero(c), x.select(c) / sm::select(x, c), sm::compress(c1d, x, axis)
    //                             the size of the result depends on the data: each counts first and WAITS FOR THE STREAM ONCE to learn
    //                             it, then allocates exactly and selects.  x.select(c) is x[mask] in row-major order; x may have another
    //                             element type than the condition's operands, the shapes must be equal.
    // std::invalid_argument: shapes that do not broadcast (where, assign_where) or are not equal (select).  Each library call is
    // counted in sm::fusion_stats().selects.
    // THE DISTINCT VALUES (np.unique on the row-major flattening, under the Array API's names).  values: ascending, -0 == +0, one NaN
    // last (every NaN with equal_nan = false), each holding the bits of its FIRST occurrence; index: where that is in the flattening;
    // inverse: shape {size}, the value number of every element, so values.take_flat(inverse) rebuilds the flattening (up to which zero
    // and which NaN payload); counts: how often each value occurs.  The operand may be a view (copied dense) or a pending chain
    // (evaluated first).  Each is ONE smhip_sort_axis call (positions only when index or inverse is wanted), a count of the runs, ONE
    // WAIT FOR THE STREAM to learn how many there are, and one smhip_runs call into arrays of exactly that size; the two run calls are
    // counted in sm::fusion_stats().uniques.  An empty operand gives arrays of shape {0}; 2^31 elements or more throw what sort_flat
    // throws.  unique_consecutive / run_lengths do the same WITHOUT the sort and without that limit: the first element of every run of
    // adjacent equal elements, and the runs' lengths (run-length encoding).  With inverse and index_add they make a group-by:
    //   auto [keys, inverse] = sm::unique_inverse(k);  auto sums = sm::zeros<float>(keys.totalSize);  sums.index_add(inverse, v, 0);
    SMArray unique_values(bool equal_nan = true) const { return runs_of(true, equal_nan, false, false, false).values; }
    SMArray unique(bool equal_nan = true) const { return unique_values(equal_nan); }
    std::pair<SMArray, SMArray<std::int64_t>> unique_counts(bool equal_nan = true) const {
        UniqueAll<T> r = runs_of(true, equal_nan, false, false, true);
        return {std::move(r.values), std::move(r.counts)};
    }
    std::pair<SMArray, SMArray<std::int64_t>> unique_inverse(bool equal_nan = true) const {
        UniqueAll<T> r = runs_of(true, equal_nan, false, true, false);
        return {std::move(r.values), std::move(r.inverse)};
    }
    UniqueAll<T> unique_all(bool equal_nan = true) const { return runs_of(true, equal_nan, true, true, true); }
    SMArray unique_consecutive(bool equal_nan = true) const { return runs_of(false, equal_nan, false, false, false).values; }
    std::pair<SMArray, SMArray<std::int64_t>> run_lengths(bool equal_nan = true) const {
        UniqueAll<T> r = runs_of(false, equal_nan, false, false, true);
        return {std::move(r.values), std::move(r.counts)};
    }

    SMArray &assign_where(const Cond<T> &c, const SMArray &v) { return assign_where_of(c, &v, T{}); }
    SMArray &assign_where(const Cond<T> &c, T v) { return assign_where_of(c, nullptr, v); }
    template <typename U>
    SMArray select(const Cond<U> &c) const {
        static_assert(hip::transport_of<T>::id >= 0 && (sizeof(T) == 4 || sizeof(T) == 8), "select: elements of 4 or 8 bytes");
        if (c.shape() != _shape) throw std::invalid_argument("simpleMath/MI355X: select: the array and the condition have different shapes");
        hip::DeviceGuard on(device());
        const typename Cond<U>::Call call(c, _shape, "select");
        const T *src = device_data();  // a pending chain that produces the array runs here
        const std::int64_t total = call.count();
        SMArray out = device_empty(std::vector<std::size_t>{static_cast<std::size_t>(total)});
        if (total == 0) return out;
        auto ss = hip::to_i64(_strides);
        if (ss.empty()) ss = {1};
        hip::check(smhip_select(SMHIP_SELECT_VALUES, call.cmp, hip::dtype_of<U>::id, call.x, call.sx.data(), call.y, call.sy.data(), &call.scalar, call.shape.data(),
                                call.ndim(), src, ss.data(), static_cast<int>(sizeof(T)), out.device_data_mut(), total, nullptr));
        ++detail::tls_fusion_stats.selects;
        return out;
    }
    template <typename U>
    SMArray select(const SMArray<U> &nonzero) const { return select(Cond<U>(nonzero)); }
    // c ? a : b (a / b == nullptr: the scalar) over the broadcast shape: what sm::where calls.
    static SMArray where_of(const Cond<T> &c, const SMArray *a, T sa, const SMArray *b, T sb) {
        std::vector<std::size_t> shape = c.shape();
        if (a) detail::broadcast_into(shape, a->_shape, "where");
        if (b) detail::broadcast_into(shape, b->_shape, "where");
        SMArray out = device_empty(std::vector<std::size_t>(shape));
        if (out.totalSize != 0) run_where(c, a, sa, b, sb, shape, nullptr, out.device_data_mut());
        return out;
    }

private:
    std::vector<std::size_t> _shape;
    std::vector<std::size_t> _strides;
    std::size_t ndim = 0;
    bool isView = false;

    SMArray() = default;  // internal: views and device-born results

    friend struct detail::Chain<T>;
    template <typename U>
    friend struct Cond;
    template <ArithmeticOrComplex U>
    friend class SMArray;  // an operand of another element type (the index arrays) is seen through its own flat()

    using Index = SMArray<std::int64_t>;  // positions, counts

    // Another handle on the same elements (same storage, offset, shape, strides): what a recorded chain keeps of an operand.
    SMArray alias() const {
        SMArray v;
        v.data = data;
        v._shape = _shape;
        v._strides = _strides;
        v.ndim = ndim;
        v.totalSize = totalSize;
        v.isView = true;
        return v;
    }

    // Is this array the unevaluated result of the chain pending on this thread, with nobody else holding its storage?  Only
    // then may an operator that consumes it (as a temporary) continue the chain instead of reading the result.
    detail::Chain<T> *continuable() const {
        detail::Chain<T> *c = pending_temporary();
        return (c && !c->full()) ? c : nullptr;
    }
    // ... the chain itself, room for another stage or not (a reduction of its value takes no stage)
    detail::Chain<T> *pending_temporary() const {
        const auto &st = data.storage();
        if (!st || !st->pending || detail::tls_pending != st->pending.get() || isView || data.offset() != 0 || st.use_count() != 1) return nullptr;
        return static_cast<detail::Chain<T> *>(st->pending.get());
    }

public:
    // sm::pow(<temporary>, s) (UserFunctions.h): when the temporary is the unevaluated result of this full-expression's chain --
    // sm::pow(a - b, 2.0f) -- the power is one more stage of that chain (s = 2 is fused into its kernel, any other exponent cuts
    // the chain and runs pow's own evaluation on the value so far: the same bits as the operator by itself).  The chain is
    // launched by the operators' argument temporaries at the end of the full-expression, like every chain.
    static SMArray pow_of(const SMArray &x, bool x_temporary, T value) {
        if constexpr (hip::on_device_v<T, PowOp<T>> && hip::is_builtin_op<PowOp<T>>::value) {
            if (x_temporary) {
                if (detail::Chain<T> *cx = x.continuable()) {
                    hip::DeviceGuard on(x.device());
                    SMArray out = device_empty(std::vector<std::size_t>(x._shape));
                    detail::Storage<T> &ost = *out.data.storage();
                    ost.pending = std::move(x.data.storage()->pending);
                    cx->retarget(&ost, out._shape);
                    cx->push(SMHIP_OP_POW, false, value);
                    return out;
                }
            }
        }
        return x.template apply_scalar<PowOp<T>>(value);
    }

    // sm::exp / log / sqrt / abs and unary minus (UserFunctions.h; fn = smhip_unary_fn).  Of the unevaluated temporary of this
    // full-expression's chain -- sm::exp(x - m), sm::sqrt(a * a + b * b), -(a * row) -- the function is one more stage of that
    // chain (smhip.h: SMHIP_OP_UNARY_BASE; counted in sm::fusion_stats() like any stage), exactly as pow_of continues it.  Of
    // anything else -- a named array, a view -- it launches smhip_unary, which reads views in place; the result lives in HBM.
    static SMArray unary_of(const SMArray &x, bool x_temporary, int fn) {
        static_assert(detail::four_types_v<T>, "sm::exp / log / sqrt / abs / unary minus: f32, f64, i32 and i64 arrays");
        if (x_temporary) {
            if (detail::Chain<T> *cx = x.continuable()) {
                hip::DeviceGuard on(x.device());
                SMArray out = device_empty(std::vector<std::size_t>(x._shape));
                detail::Storage<T> &ost = *out.data.storage();
                ost.pending = std::move(x.data.storage()->pending);
                cx->retarget(&ost, out._shape);
                cx->push(SMHIP_OP_UNARY_BASE + fn, false, T{});  // a stage without an operand: the scalar slot, ignored
                return out;
            }
        }
        hip::DeviceGuard on(x.device());
        const T *in = x.device_data();  // a pending chain that produces this operand runs here
        SMArray out = device_empty(std::vector<std::size_t>(x._shape));
        if (x._shape.empty() || x.totalSize == 0) return out;
        const auto sh = hip::to_i64(x._shape), st = hip::to_i64(x._strides);
        hip::check(smhip_unary(fn, hip::dtype_of<T>::id, in, st.data(), sh.data(), static_cast<int>(sh.size()), out.device_data_mut()));
        return out;
    }
    // -a: sign flipped (floats, NaN included) / wrapping negation (integers: -INT_MIN == INT_MIN, as numpy)
    SMArray operator-() const & { return unary_of(*this, false, SMHIP_UNARY_NEG); }
    SMArray operator-() && { return unary_of(*this, true, SMHIP_UNARY_NEG); }

    // CHANGING THE ELEMENT TYPE (np.ndarray.astype): a.astype<U>() / sm::astype<U>(a), T and U each float, double, int or
    // std::int64_t.  A new dense array of a's shape in HBM, converted on the device by ONE library call (smhip_convert; smhip.h has the
    // table): integers round to nearest even once, i64 -> i32 wraps, and float -> integer is SATURATING TRUNCATION -- toward zero, the
    // target's min / max beyond its range, 0 for a NaN (numpy leaves that case undefined).  A view is passed with its strides; a
    // pending chain, as in (a * b).astype<double>(), is evaluated first; U == T gives a dense copy, as numpy's astype does.  The
    // result feeds the next chain like any device-born array; no host mirror is touched.  Asynchronous.
    template <typename U>
    SMArray<U> astype() const {
        static_assert(detail::four_types_v<T>, "astype: the array's element type must be float, double, int or std::int64_t");
        static_assert(detail::four_types_v<U>, "astype<U>: U must be float, double, int or std::int64_t");
        hip::DeviceGuard on(device());
        const T *in = device_data();  // a pending chain that produces this operand runs here
        SMArray<U> out = SMArray<U>::device_empty(std::vector<std::size_t>(_shape));
        if (_shape.empty() || totalSize == 0) return out;
        const auto sh = hip::to_i64(_shape), st = hip::to_i64(_strides);
        hip::check(smhip_convert(hip::dtype_of<T>::id, hip::dtype_of<U>::id, in, st.data(), sh.data(), static_cast<int>(sh.size()), out.device_data_mut()));
        return out;
    }

private:
    // x Op y (y == nullptr: x Op scalar), recorded rather than launched when it can be part of a one-pass chain: built-in
    // + - * / on an element type with kernels.  See "deferred operator chains" at the top of this file.
    template <typename Op>
    static SMArray deferred(const SMArray &x, bool x_temporary, const detail::Operand<T> *rhs, T scalar) {
        return deferred_arrays<Op>(x, x_temporary, rhs ? &rhs->array() : nullptr, rhs && rhs->temporary(), scalar);
    }
    template <typename Op>
    static SMArray deferred_arrays(const SMArray &x, bool x_temporary, const SMArray *y, bool y_temporary, T scalar) {
        constexpr bool chainable = hip::on_device_v<T, Op> && hip::is_builtin_op<Op>::value && !std::is_same_v<Op, PowOp<T>>;
        if constexpr (!chainable) {
            return y ? x.template apply<Op>(*y) : x.template apply_scalar<Op>(scalar);
        } else {
            std::vector<std::size_t> shape = (!y || x._shape == y->_shape) ? x._shape : sm::broadcast(x._shape, x._strides, y->_shape, y->_strides).resultShape;
            if (shape.size() > MAX_NDIM) throw std::runtime_error("rank exceeds MAX_NDIM");
            const std::size_t n = calculateTotalSize(shape);
            // nothing to gain from waiting: empty and 0-d results, and tiny host-built operands (they ride in the launch
            // packet of the plain operator, apply_into)
            detail::Chain<T> *cx = x_temporary ? x.continuable() : nullptr;
            detail::Chain<T> *cy = (!cx && y && y_temporary) ? y->continuable() : nullptr;
            if (shape.empty() || n == 0 || (!cx && !cy && n <= SMHIP_INLINE_MAX_OUTPUTS && (x.host_only_small() || (y && y->host_only_small()))))
                return y ? x.template apply<Op>(*y) : x.template apply_scalar<Op>(scalar);
            const int device = y ? common_device(x, *y) : x.device();
            const int op = hip::device_op<Op>::id();
            hip::DeviceGuard on(device);
            SMArray out = device_empty(std::move(shape));  // no device buffer yet: Storage allocates on first use
            detail::Storage<T> &ost = *out.data.storage();
            if (cx) {  // (pending temporary) Op y: the chain goes on
                ost.pending = std::move(x.data.storage()->pending);
                cx->retarget(&ost, out._shape);
                if (y) cx->push(op, false, *y); else cx->push(op, false, scalar);
            } else if (cy) {  // x Op (pending temporary): the same, with the stage's operands exchanged
                ost.pending = std::move(y->data.storage()->pending);
                cy->retarget(&ost, out._shape);
                cy->push(op, true, x);
            } else {
                detail::flush_pending();  // one chain per thread
                auto c = std::make_unique<detail::Chain<T>>(&ost, out._shape, device, x);
                if (y) c->push(op, false, *y); else c->push(op, false, scalar);
                detail::tls_pending = c.get();
                ost.pending = std::move(c);
            }
            return out;
        }
    }

    void finish_owning(T *buffer) {
        ndim = _shape.size();
        totalSize = calculateTotalSize(_shape);
        _strides = detail::dense_strides(_shape);
        data = detail::HostPtr<T>(std::make_shared<detail::Storage<T>>(buffer, totalSize), 0);
    }

    std::size_t offset_of(std::initializer_list<std::size_t> indices, [[maybe_unused]] bool exact) const {
        assert((exact ? indices.size() == _shape.size() : indices.size() <= _shape.size()) && "wrong number of indices");
        std::size_t off = 0, k = 0;
        for (std::size_t idx : indices) {
            assert(idx < _shape[k] && "Index out of bounds");
            off += idx * _strides[k++];
        }
        return off;
    }

    // f(linear, element offset) over all elements in row-major order
    template <typename F>
    void for_each_offset(F &&f) const {
        std::vector<std::size_t> idx(_shape.size(), 0);
        for (std::size_t linear = 0; linear < totalSize; ++linear) {
            std::size_t off = 0;
            for (std::size_t k = 0; k < idx.size(); ++k) off += idx[k] * _strides[k];
            f(linear, off);
            for (std::size_t k = idx.size(); k-- > 0;) {
                if (++idx[k] < _shape[k]) break;
                idx[k] = 0;
            }
        }
    }

    void copy_dense_to(T *dst) const {
        const T *base = data.read();
        if (is_dense()) std::copy(base, base + totalSize, dst);
        else for_each_offset([&](std::size_t linear, std::size_t off) { dst[linear] = base[off]; });
    }

    // Dense device copy of this array's storage seen through (vshape, vstrides), labelled `outShape`
    // (same element count): SMHIP_OP_LEFT through the broadcast kernels.
    SMArray gather(const std::vector<std::size_t> &vshape, const std::vector<std::size_t> &vstrides,
                   std::vector<std::size_t> &&outShape) const {
        hip::DeviceGuard on(device());
        SMArray out = device_empty(std::move(outShape));
        auto sh = hip::to_i64(vshape), st = hip::to_i64(vstrides);
        lane_axis(sh, st, nullptr);
        const std::vector<std::int64_t> zeros(sh.size(), 0);
        const T *src = device_data();
        hip::check(smhip_elementwise(SMHIP_OP_LEFT, hip::transport_of<T>::id, src, st.data(), src, zeros.data(), sh.data(),
                                     static_cast<int>(sh.size()), out.device_data_mut()));
        return out;
    }

    // An element type that moves as `lanes` elements of a kernel type (std::complex: {re, im}) gets an innermost axis of
    // extent `lanes`, stride 1, and its element strides counted in lanes (math/ops.h: transport_of).
    static void lane_axis(std::vector<std::int64_t> &shape, std::vector<std::int64_t> &strides, std::vector<std::int64_t> *strides2) {
        constexpr int lanes = hip::transport_of<T>::lanes;
        if constexpr (lanes > 1) {
            for (auto &x : strides) x *= lanes;
            if (strides2) for (auto &x : *strides2) x *= lanes;
            shape.push_back(lanes);
            strides.push_back(1);
            if (strides2) strides2->push_back(1);
        } else {
            (void)shape; (void)strides; (void)strides2;
        }
    }

    // Bytes from this array's first element to the end of its storage when the elements exist ONLY in host memory and
    // that is at most SMHIP_INLINE_MAX_BYTES (such an operand can ride in a kernel's argument block); 0 otherwise.
    std::size_t host_only_small() const {
        const auto &st = data.storage();
        if (!st || st->dev_valid || !st->host_valid || st->count <= data.offset()) return 0;
        // Once only: an array that is used AGAIN is worth its upload -- reading the argument block costs the kernel a
        // trip over the fabric (a launch with an inline operand takes ~4.0 us against ~2.8 us with resident ones), so
        // the second use uploads it and every later one runs resident.  simple_check builds its array anew each time
        // and never gets that far; BM_SMArrayPow_1D / _2D reuse theirs and do.
        if (st->inline_uses != 0) return 0;
        const std::size_t bytes = (st->count - data.offset()) * sizeof(T);
        return bytes <= SMHIP_INLINE_MAX_BYTES ? bytes : 0;
    }

    // ---- the front's rules for the axis, index and counting families, each written once
    // This array's shape without the axes that `mask` names (keepdims: with an extent of 1 in their place); {1} when nothing is left.
    std::vector<std::size_t> kept_shape(std::uint32_t mask, bool keepdims) const {
        std::vector<std::size_t> shape;
        for (std::size_t d = 0; d < _shape.size(); ++d) {
            if (!(mask >> d & 1u)) shape.push_back(_shape[d]);
            else if (keepdims) shape.push_back(1);
        }
        if (shape.empty()) shape.push_back(1);
        return shape;
    }
    // An operand as the C ABI takes it: the device pointer (building one is where a pending chain that produces the operand runs),
    // shape and strides in elements, the axis the call runs along, and the dense copy the pointer belongs to if one had to be made.
    struct AbiView {
        const T *ptr = nullptr;
        std::vector<std::int64_t> shape, strides;
        int axis = 0;
        std::unique_ptr<SMArray> dense;
        int ndim() const { return static_cast<int>(shape.size()); }
    };
    // ... along `axis` (already normalised; 0 for a call that names none) of this view, read in place.
    AbiView along_axis(int axis) const { return AbiView{device_data(), hip::to_i64(_shape), hip::to_i64(_strides), axis, nullptr}; }
    // ... as its row-major flattening, one line of totalSize elements: a view that is not dense is copied dense first.
    AbiView flat() const {
        AbiView v;
        if (!is_dense()) v.dense.reset(new SMArray(contiguous()));
        v.ptr = v.dense ? v.dense->device_data() : device_data();
        v.shape = {static_cast<std::int64_t>(totalSize)}, v.strides = {1};
        return v;
    }
    // ... along an axis (counted from the end when negative; std::runtime_error out of range), or flattened when there is none.
    // The axis is checked before anything touches the device.
    std::optional<int> line_axis(std::optional<int> axis) const {
        if (axis) axis = detail::normal_axis<std::runtime_error>(*axis, _shape.size());
        return axis;
    }
    AbiView line(std::optional<int> axis) const { return axis ? along_axis(*axis) : flat(); }

    SMArray reduce_along(int kind, std::initializer_list<int> axes, bool keepdims) const {
        static_assert(detail::four_types_v<T>, "axis reductions: f32, f64, i32 and i64");
        std::uint32_t mask = 0;
        for (int ax : axes) {
            const int a = detail::normal_axis<std::runtime_error>(ax, _shape.size());
            if (mask >> a & 1u) throw std::runtime_error("simpleMath/MI355X: axis " + std::to_string(ax) + " repeated");
            mask |= 1u << a;
        }
        if (!mask) throw std::runtime_error("simpleMath/MI355X: no axis to reduce");
        std::vector<std::size_t> shape = kept_shape(mask, keepdims);
        hip::DeviceGuard on(device());
        const AbiView in = along_axis(0);  // a pending chain that produces this operand runs here
        SMArray out = device_empty(std::move(shape));
        hip::check(smhip_reduce_axes(kind, hip::dtype_of<T>::id, in.ptr, in.shape.data(), in.strides.data(), in.ndim(), mask, out.device_data_mut()));
        ++detail::tls_fusion_stats.reductions;
        return out;
    }

    // Without an axis: the elements in row-major order as one line, shape {totalSize}.
    SMArray scan_of(int kind, std::optional<int> axis) const {
        static_assert(detail::four_types_v<T>, "cumulative scans: f32, f64, i32 and i64");
        axis = line_axis(axis);
        hip::DeviceGuard on(device());
        const AbiView in = line(axis);  // a pending chain that produces this operand runs here
        SMArray out = device_empty(axis ? std::vector<std::size_t>(_shape) : std::vector<std::size_t>{totalSize});
        hip::check(smhip_scan_axis(kind, hip::dtype_of<T>::id, in.ptr, in.shape.data(), in.strides.data(), in.ndim(), in.axis, out.device_data_mut()));
        ++detail::tls_fusion_stats.scans;
        return out;
    }

    // {the extremes themselves, their positions}, of the kept shape (without an axis: the row-major index into this array, shape {1});
    // the values have shape {0} when they are not wanted.
    std::pair<SMArray, Index> arg_of(int kind, std::optional<int> axis, bool keepdims, bool want_values) const {
        static_assert(detail::four_types_v<T>, "argmax / argmin: f32, f64, i32 and i64");
        axis = line_axis(axis);
        hip::DeviceGuard on(device());
        const AbiView in = line(axis);  // a pending chain that produces this operand runs here
        const std::vector<std::size_t> shape = axis ? kept_shape(1u << *axis, keepdims) : std::vector<std::size_t>{1};
        std::pair<SMArray, Index> r{device_empty(want_values ? std::vector<std::size_t>(shape) : std::vector<std::size_t>{0}), Index::device_empty(std::vector<std::size_t>(shape))};
        hip::check(smhip_argreduce_axis(kind, hip::dtype_of<T>::id, in.ptr, in.shape.data(), in.strides.data(), in.ndim(), in.axis, r.second.device_data_mut(),
                                        want_values ? r.first.device_data_mut() : nullptr));
        ++detail::tls_fusion_stats.arg_reductions;
        return r;
    }

    // {the sorted elements, their positions}, of this array's shape (without an axis: of {totalSize}); one that is not wanted has shape {0}.
    std::pair<SMArray, Index> sort_of(std::optional<int> axis, bool descending, bool want_values, bool want_where) const {
        static_assert(detail::four_types_v<T>, "sort / argsort: f32, f64, i32 and i64");
        axis = line_axis(axis);
        hip::DeviceGuard on(device());
        const AbiView in = line(axis);  // a pending chain that produces this operand runs here
        const auto shape = [&](bool wanted) { return !wanted ? std::vector<std::size_t>{0} : axis ? _shape : std::vector<std::size_t>{totalSize}; };
        std::pair<SMArray, Index> r{device_empty(shape(want_values)), Index::device_empty(shape(want_where))};
        hip::check(smhip_sort_axis(descending ? SMHIP_SORT_DESCENDING : SMHIP_SORT_ASCENDING, hip::dtype_of<T>::id, in.ptr, in.shape.data(), in.strides.data(),
                                   in.ndim(), in.axis, want_values ? r.first.device_data_mut() : nullptr, want_where ? r.second.device_data_mut() : nullptr));
        ++detail::tls_fusion_stats.sorts;
        return r;
    }

    // {var or stddev, the mean}, of the kept shape (axes == nullptr: over the row-major flattening, shape {1}); the mean has shape {0}
    // when it is not wanted.
    std::pair<SMArray, SMArray> moments_of(int kind, const std::initializer_list<int> *axes, std::int64_t ddof, bool keepdims, bool want_mean) const {
        static_assert(std::is_floating_point_v<T>, "var / stddev / var_mean: float and double only (astype first)");
        std::uint32_t mask = axes ? 0u : 1u;
        if (axes) {
            for (int ax : *axes) {
                const int a = detail::normal_axis<std::runtime_error>(ax, _shape.size());
                if (mask >> a & 1u) throw std::runtime_error("simpleMath/MI355X: axis " + std::to_string(ax) + " repeated");
                mask |= 1u << a;
            }
            if (!mask) throw std::runtime_error("simpleMath/MI355X: no axis to reduce");
        }
        if (ddof < 0) throw std::runtime_error("simpleMath/MI355X: ddof " + std::to_string(ddof) + " is negative");
        std::vector<std::size_t> shape = axes ? kept_shape(mask, keepdims) : std::vector<std::size_t>{1};
        std::int64_t n = 1, results = 1;
        for (std::size_t d = 0; d < _shape.size(); ++d)
            if (!axes || (mask >> d & 1u)) n *= static_cast<std::int64_t>(_shape[d]);
        for (std::size_t e : shape) results *= static_cast<std::int64_t>(e);
        if (results && n - ddof <= 0) throw std::runtime_error("simpleMath/MI355X: N - ddof = " + std::to_string(n) + " - " + std::to_string(ddof) + " is not positive");
        hip::DeviceGuard on(device());
        const AbiView in = axes ? along_axis(0) : flat();  // a pending chain that produces this operand runs here
        std::pair<SMArray, SMArray> r{device_empty(std::vector<std::size_t>(shape)), device_empty(want_mean ? std::vector<std::size_t>(shape) : std::vector<std::size_t>{0})};
        hip::check(smhip_moments_axes(kind, hip::dtype_of<T>::id, in.ptr, in.shape.data(), in.strides.data(), in.ndim(), mask, ddof, r.first.device_data_mut(),
                                      want_mean ? r.second.device_data_mut() : nullptr));
        ++detail::tls_fusion_stats.moments;
        return r;
    }

    // softmax / log_softmax: of this array's shape; logsumexp: of the kept shape (without an axis: the flattening's, shape {1}).
    SMArray softmax_of(int kind, std::optional<int> axis, bool keepdims) const {
        static_assert(std::is_floating_point_v<T>, "softmax / log_softmax / logsumexp: float and double only");
        axis = line_axis(axis);
        hip::DeviceGuard on(device());
        const AbiView in = line(axis);  // a pending chain that produces this operand runs here
        SMArray out = device_empty(kind != SMHIP_LOGSUMEXP ? std::vector<std::size_t>(_shape) : axis ? kept_shape(1u << *axis, keepdims) : std::vector<std::size_t>{1});
        hip::check(smhip_softmax_axis(kind, hip::dtype_of<T>::id, in.ptr, in.shape.data(), in.strides.data(), in.ndim(), in.axis, out.device_data_mut()));
        ++detail::tls_fusion_stats.softmaxes;
        return out;
    }

    // {the first k of the order, their positions}, of this array's shape with k on the axis (without an axis: of {k}).
    std::pair<SMArray, Index> topk_of(std::size_t k, std::optional<int> axis, bool largest) const {
        static_assert(detail::four_types_v<T>, "topk: f32, f64, i32 and i64");
        if (axis) axis = detail::normal_axis<std::invalid_argument>(*axis, _shape.size(), "topk: ");
        const std::size_t extent = axis ? _shape[*axis] : totalSize;
        if (k > extent) throw std::invalid_argument("simpleMath/MI355X: topk: k " + std::to_string(k) + " above the axis' extent " + std::to_string(extent));
        hip::DeviceGuard on(device());
        const AbiView in = line(axis);  // a pending chain that produces this operand runs here
        std::vector<std::size_t> shape = axis ? _shape : std::vector<std::size_t>{totalSize};
        shape[in.axis] = k;
        std::pair<SMArray, Index> r{device_empty(std::vector<std::size_t>(shape)), Index::device_empty(std::vector<std::size_t>(shape))};
        hip::check(smhip_topk_axis(largest ? SMHIP_SORT_DESCENDING : SMHIP_SORT_ASCENDING, hip::dtype_of<T>::id, in.ptr, in.shape.data(), in.strides.data(),
                                   in.ndim(), in.axis, static_cast<std::int64_t>(k), r.first.device_data_mut(), r.second.device_data_mut()));
        ++detail::tls_fusion_stats.topks;
        return r;
    }

    // The quantiles of `n` probabilities (each divided by `scale`: 100 for percentiles), of the kept shape (without an axis: {1}) with a
    // leading axis of n when they came as a list.
    SMArray quantile_of(const double *q, std::size_t n, bool list, std::optional<int> axis, quantile_method method, bool keepdims, double scale, const char *who) const {
        static_assert(std::is_floating_point_v<T>, "quantile / percentile / median: float and double only (astype first)");
        if (axis) axis = detail::normal_axis<std::invalid_argument>(*axis, _shape.size(), who);
        if (n == 0) throw std::invalid_argument(std::string("simpleMath/MI355X: ") + who + "no probability given");
        std::vector<double> qs(q, q + n);
        for (double &v : qs) {
            if (scale != 1.0) v /= scale;
            if (!(v >= 0.0 && v <= 1.0)) throw std::invalid_argument(std::string("simpleMath/MI355X: ") + who + "a probability outside [0, " + (scale == 1.0 ? "1" : "100") + "] or NaN");
        }
        std::vector<std::size_t> shape;
        if (list) shape.push_back(n);
        for (std::size_t d = 0; axis && d < _shape.size(); ++d) {
            if (static_cast<int>(d) != *axis) shape.push_back(_shape[d]);
            else if (keepdims) shape.push_back(1);
        }
        if (shape.empty()) shape.push_back(1);
        std::size_t results = 1;
        for (std::size_t e : shape) results *= e;
        if (results && (axis ? _shape[*axis] : totalSize) == 0) throw std::invalid_argument(std::string("simpleMath/MI355X: ") + who + "an empty axis with a result that is not empty");
        hip::DeviceGuard on(device());
        const AbiView in = line(axis);  // a pending chain that produces this operand runs here
        SMArray out = device_empty(std::move(shape));
        hip::check(smhip_quantile_axis(static_cast<int>(method), hip::dtype_of<T>::id, in.ptr, in.shape.data(), in.strides.data(), in.ndim(), in.axis, qs.data(),
                                       static_cast<std::int64_t>(qs.size()), out.device_data_mut()));
        ++detail::tls_fusion_stats.quantiles;
        return out;
    }

    // Both operands in row-major order as one line each (views are made dense first), shape {idx.size()}.
    SMArray take_flat_of(const Index &idx, index_mode mode) const {
        hip::DeviceGuard on(device());
        const AbiView in = flat();
        const typename Index::AbiView ix = idx.flat();
        return take_run(in.ptr, ix.ptr, ix.shape, in.strides, ix.strides, 0, totalSize, mode, std::vector<std::size_t>{idx.totalSize});
    }
    // `in` / `ix`: device pointers to the operands' first elements, pending chains already evaluated.
    SMArray take_run(const T *in, const std::int64_t *ix, const std::vector<std::int64_t> &shape, const std::vector<std::int64_t> &sa,
                     const std::vector<std::int64_t> &si, int axis, std::size_t extent, index_mode mode, std::vector<std::size_t> &&result) const {
        static_assert(detail::four_types_v<T>, "take / take_along_axis: f32, f64, i32 and i64");
        hip::DeviceGuard on(device());
        SMArray out = device_empty(std::move(result));
        if (out.totalSize == 0) return out;
        if (extent == 0) throw std::out_of_range("simpleMath/MI355X: take: cannot take from an axis of 0 elements");
        const detail::DeviceWord<> flag(mode == index_mode::checked);  // only when someone will read it
        hip::check(smhip_take_axis(static_cast<int>(mode), hip::dtype_of<T>::id, in, sa.data(), static_cast<std::int64_t>(extent), ix, si.data(), shape.data(),
                                   static_cast<int>(shape.size()), axis, out.device_data_mut(), flag.ptr()));
        ++detail::tls_fusion_stats.takes;
        if (flag && flag.read()) throw std::out_of_range("simpleMath/MI355X: take: an index is out of bounds for an axis of " + std::to_string(extent) + " elements");
        return out;
    }

    // ---- scatter: the walk shape is this array's shape with `axis` replaced by the entries per line
    SMArray &scatter_along(int kind, const Index &idx, const SMArray *values, T scalar, int axis, index_mode mode, bool unique) {
        const std::size_t nd = _shape.size();
        if (idx.shape().size() != nd)
            throw std::invalid_argument("simpleMath/MI355X: put_along_axis / scatter_add: the index array has rank " + std::to_string(idx.shape().size()) +
                                        ", the target rank " + std::to_string(nd));
        const int ax = detail::normal_axis<std::invalid_argument>(axis, nd, "take: ");
        std::vector<std::int64_t> walk(nd), si(nd);
        for (std::size_t d = 0; d < nd; ++d) {
            const std::size_t na = _shape[d], ni = idx.shape()[d];
            const bool along = static_cast<int>(d) == ax;
            if (!along && ni != na && ni != 1)
                throw std::invalid_argument("simpleMath/MI355X: put_along_axis / scatter_add: the index array does not match the target at axis " + std::to_string(d));
            walk[d] = static_cast<std::int64_t>(along ? ni : na);
            si[d] = along || (ni == na && na != 1) ? static_cast<std::int64_t>(idx.strides()[d]) : 0;
        }
        return scatter_run(kind, walk, ax, idx, si, values, scalar, mode, unique);
    }
    SMArray &scatter_ids(int kind, const Index &ids, const SMArray *values, T scalar, int axis, index_mode mode, bool unique) {
        if (ids.shape().size() != 1) throw std::invalid_argument("simpleMath/MI355X: put / index_add: the index array must be 1-D");
        const std::size_t nd = _shape.size();
        const int ax = detail::normal_axis<std::invalid_argument>(axis, nd, "take: ");
        std::vector<std::int64_t> walk = hip::to_i64(_shape), si(nd, 0);
        walk[ax] = static_cast<std::int64_t>(ids.totalSize), si[ax] = static_cast<std::int64_t>(ids.strides()[0]);
        return scatter_run(kind, walk, ax, ids, si, values, scalar, mode, unique);
    }
    // This array and idx in row-major order as one line each.
    SMArray &scatter_flat(int kind, const Index &idx, const SMArray *values, T scalar, index_mode mode, bool unique) {
        if (!is_dense()) return staged([&](SMArray &dense) { dense.scatter_flat(kind, idx, values, scalar, mode, unique); });
        std::unique_ptr<Index> idx_holder;
        if (!idx.is_dense()) idx_holder.reset(new Index(idx.contiguous()));
        std::unique_ptr<SMArray> val_line;
        if (values) {
            val_line.reset(new SMArray(values->is_dense() ? values->alias() : values->contiguous()));
            val_line->as_line();
        }
        SMArray line = alias();
        line.as_line();
        line.scatter_run(kind, {static_cast<std::int64_t>(idx.totalSize)}, 0, idx_holder ? *idx_holder : idx, {1}, val_line.get(), scalar, mode, unique);
        return *this;
    }
    // A dense array seen as one line of totalSize elements.
    void as_line() { _shape = {totalSize}, _strides = {1}, ndim = 1; }
    // fn on a dense copy of this array, assigned back element by element -- also when fn throws for a bad index under
    // index_mode::checked: the valid entries have been applied.
    template <typename Fn> SMArray &staged(Fn &&fn) {
        SMArray dense = contiguous();
        try {
            fn(dense);
        } catch (const std::out_of_range &) {
            *this = std::move(dense);
            throw;
        }
        *this = std::move(dense);
        return *this;
    }
    SMArray &scatter_run(int kind, const std::vector<std::int64_t> &walk, int axis, const Index &idx, const std::vector<std::int64_t> &si,
                         const SMArray *values, T scalar, index_mode mode, bool unique) {
        static_assert(detail::four_types_v<T>, "put / put_along_axis / scatter_add / index_add: f32, f64, i32 and i64");
        const std::size_t nd = walk.size();
        // values against the walk shape, aligned at the last axis
        std::vector<std::int64_t> sv(nd, 0);
        if (values) {
            const std::size_t nv = values->_shape.size();
            if (nv > nd) throw std::invalid_argument("simpleMath/MI355X: scatter: the values have a higher rank than the target");
            for (std::size_t d = 0; d < nv; ++d) {
                const std::size_t w = static_cast<std::size_t>(walk[nd - nv + d]), n = values->_shape[d];
                if (n != w && n != 1) throw std::invalid_argument("simpleMath/MI355X: scatter: the values do not broadcast at axis " + std::to_string(nd - nv + d));
                sv[nd - nv + d] = n == w && w != 1 ? static_cast<std::int64_t>(values->_strides[d]) : 0;
            }
        }
        std::int64_t entries = 1;
        for (std::int64_t w : walk) entries *= w;
        if (entries == 0) return *this;
        if (_shape[axis] == 0) throw std::out_of_range("simpleMath/MI355X: scatter: cannot place entries on an axis of 0 elements");
        if (!is_dense())
            return staged([&](SMArray &dense) { dense.scatter_run(kind, walk, axis, idx, si, values, scalar, mode, unique); });
        hip::DeviceGuard on(device());
        // an operand that shares the target's storage is copied first: the C ABI refuses the overlap
        std::unique_ptr<SMArray> val_holder;
        std::unique_ptr<Index> idx_holder;
        std::vector<std::int64_t> si_used(si);
        if (values && values->data.storage() == data.storage()) {
            val_holder.reset(new SMArray(values->contiguous()));
            for (std::size_t d = 0, nv = values->_shape.size(); d < nv; ++d)
                if (sv[nd - nv + d]) sv[nd - nv + d] = static_cast<std::int64_t>(val_holder->_strides[d]);
            values = val_holder.get();
        } else if (!values) {
            val_holder.reset(new SMArray(device_full(std::vector<std::size_t>{1}, scalar)));
            values = val_holder.get();
        }
        if constexpr (std::is_same_v<T, std::int64_t>) {
            if (idx.data.storage() == data.storage()) {
                idx_holder.reset(new Index(idx.contiguous()));
                for (std::size_t d = 0; d < nd; ++d)  // the copy is dense: a line (1-D ids, a flattened idx) has stride 1
                    if (si_used[d]) si_used[d] = idx.shape().size() == nd ? static_cast<std::int64_t>(idx_holder->strides()[d]) : 1;
            }
        }
        const T *vp = values->device_data();  // pending chains that produce the operands run here
        const std::int64_t *ip = idx_holder ? idx_holder->device_data() : idx.device_data();
        const auto out_shape = hip::to_i64(_shape);
        const detail::DeviceWord<> flag(mode == index_mode::checked);  // only when someone will read it
        hip::check(smhip_scatter_axis(kind, static_cast<int>(mode), unique ? SMHIP_SCATTER_UNIQUE : 0, hip::dtype_of<T>::id,
                                      data.storage()->dev_rw() + data.offset(), out_shape.data(), static_cast<int>(nd), axis, ip, si_used.data(), vp, sv.data(),
                                      walk[axis], flag.ptr()));
        ++detail::tls_fusion_stats.scatters;
        if (flag && flag.read())
            throw std::out_of_range("simpleMath/MI355X: scatter: an index is out of bounds for an axis of " + std::to_string(_shape[axis]) +
                                    " elements (the valid entries have been applied)");
        return *this;
    }

    // counts of this array's values between `edges` (1-D, bins + 1 of them); flags / lo / hi as smhip_histogram takes them.
    Index count_between(const SMArray &edges, int flags, double lo, double hi) const {
        static_assert(detail::four_types_v<T>, "histogram: f32, f64, i32 and i64");
        hip::DeviceGuard on(common_device(*this, edges));
        const AbiView table = edges.flat();
        const AbiView in = along_axis(0);  // a pending chain that produces the operand runs here
        const std::size_t bins = edges.totalSize - 1;
        Index out = Index::device_empty(std::vector<std::size_t>{bins});
        hip::check(smhip_histogram(flags, hip::dtype_of<T>::id, in.ptr, in.shape.data(), in.strides.data(), in.ndim(), table.ptr, static_cast<std::int64_t>(bins), lo, hi,
                                   out.device_data_mut()));
        ++detail::tls_fusion_stats.counts;
        return out;
    }

    // ---- where: `target` (dense) is both b and the result when given (assign_where), else the result goes to `out`
    static void run_where(const Cond<T> &c, const SMArray *a, T sa, const SMArray *b, T sb, const std::vector<std::size_t> &shape, SMArray *target, T *out) {
        static_assert(detail::four_types_v<T>, "where / assign_where: f32, f64, i32 and i64");
        int device = c.right() ? common_device(c.left(), *c.right()) : c.left().device();
        if (a) device = common_device(c.left(), *a);
        if (b) device = common_device(c.left(), *b);
        hip::DeviceGuard on(device);
        if (target) out = target->data.storage()->dev_rw() + target->data.offset();  // before the operands' pointers: this may allocate
        const typename Cond<T>::Call call(c, shape, "where");
        std::vector<std::int64_t> sta, stb;
        if (a) sta = detail::strides_over(a->_shape, a->_strides, shape, "where");
        if (b) stb = detail::strides_over(b->_shape, b->_strides, shape, "where");
        if (shape.empty()) sta = stb = {1};
        const T *pa = a ? a->device_data() : nullptr, *pb = b ? b->device_data() : nullptr;  // pending chains run here
        hip::check(smhip_where(call.cmp, hip::dtype_of<T>::id, call.x, call.sx.data(), call.y, call.sy.data(), &call.scalar, pa, sta.data(), &sa, pb, stb.data(), &sb,
                               call.shape.data(), call.ndim(), out));
        ++detail::tls_fusion_stats.selects;
    }
    SMArray &assign_where_of(const Cond<T> &c, const SMArray *v, T s) {
        if (!is_dense()) return staged([&](SMArray &dense) { dense.assign_where_of(c, v, s); });
        // the shapes are checked also when there is nothing to write
        detail::strides_over(c.shape(), std::vector<std::size_t>(c.shape().size(), 0), _shape, "assign_where");
        if (v) detail::strides_over(v->_shape, v->_strides, _shape, "assign_where");
        if (totalSize != 0) run_where(c, v, s, this, T{}, _shape, this, nullptr);
        return *this;
    }

    // The runs of the flattening (sort_first: of its stable ascending sort): count, wait, allocate exactly, emit.  A result that is not
    // wanted comes back with shape {0}.
    UniqueAll<T> runs_of(bool sort_first, bool equal_nan, bool want_index, bool want_inverse, bool want_counts) const {
        static_assert(detail::four_types_v<T>, "unique / unique_consecutive: f32, f64, i32 and i64");
        const auto none = [] { return std::vector<std::size_t>{0}; };
        if (totalSize == 0) return UniqueAll<T>{device_empty(none()), Index::device_empty(none()), Index::device_empty(none()), Index::device_empty(none())};
        hip::DeviceGuard on(device());
        const AbiView flattened = flat();  // a pending chain that produces this operand runs here
        const T *in = flattened.ptr;
        const std::int64_t n = static_cast<std::int64_t>(totalSize);
        const int flags = equal_nan ? 0 : SMHIP_RUNS_NAN_DISTINCT;
        const bool positions = sort_first && (want_index || want_inverse);
        SMArray sorted = device_empty(std::vector<std::size_t>{sort_first ? totalSize : 0});
        Index order = Index::device_empty(std::vector<std::size_t>{positions ? totalSize : 0});
        const std::int64_t *ord = nullptr;
        if (sort_first) {
            hip::check(smhip_sort_axis(SMHIP_SORT_ASCENDING, hip::dtype_of<T>::id, in, flattened.shape.data(), flattened.strides.data(), 1, 0, sorted.device_data_mut(),
                                       positions ? order.device_data_mut() : nullptr));
            ++detail::tls_fusion_stats.sorts;
            in = sorted.device_data();
            if (positions) ord = order.device_data();
        }
        std::int64_t total = 0;
        {
            const detail::DeviceWord<> word;
            hip::check(smhip_runs_count(flags, hip::dtype_of<T>::id, in, n, word.ptr()));
            ++detail::tls_fusion_stats.uniques;
            total = word.read();  // waits for the stream
        }
        const std::size_t runs = static_cast<std::size_t>(total);
        UniqueAll<T> r{device_empty(std::vector<std::size_t>{runs}), Index::device_empty(std::vector<std::size_t>{want_index ? runs : 0}),
                       Index::device_empty(std::vector<std::size_t>{want_inverse ? totalSize : 0}), Index::device_empty(std::vector<std::size_t>{want_counts ? runs : 0})};
        hip::check(smhip_runs(flags, hip::dtype_of<T>::id, in, n, ord, r.values.device_data_mut(), want_index ? r.index.device_data_mut() : nullptr,
                              want_counts ? r.counts.device_data_mut() : nullptr, want_inverse ? r.inverse.device_data_mut() : nullptr, total, nullptr));
        ++detail::tls_fusion_stats.uniques;
        return r;
    }

    // arr(i, SLICE(a, b), ...): INDEX entries drop their axis, Slice entries keep a sub-range;
    // missing trailing entries mean SLICE_ALL.  Shares storage (reference SMArray.h:397-437).
    SMArray make_view(std::initializer_list<Slice> slices) const {
        SMArray v;
        std::size_t off = data.offset();
        std::size_t axis = 0;
        auto it = slices.begin();
        for (; axis < _shape.size(); ++axis) {
            const Slice s = it != slices.end() ? *it++ : Slice(0);
            assert(s.start <= _shape[axis] && "slice start out of bounds");
            off += s.start * _strides[axis];
            if (s.sliceType == Slice::INDEX) continue;
            const std::size_t stop = s.open_ended() ? _shape[axis] : s.end;
            assert(stop <= _shape[axis] && stop >= s.start && "slice end out of bounds");
            // SliceStep only names SINGLE_STEP, but the reference's view code honours any positive value stored in
            // `step` (SMArray.h:416-424: extent = ceil(range / step), stride * step); so does this one
            const std::size_t step = static_cast<int>(s.step) > 1 ? static_cast<std::size_t>(s.step) : 1;
            v._shape.push_back((stop - s.start + step - 1) / step);
            v._strides.push_back(_strides[axis] * step);
        }
        v.data = detail::HostPtr<T>(data.storage(), off);
        v.ndim = v._shape.size();
        v.totalSize = calculateTotalSize(v._shape);
        v.isView = true;
        return v;
    }
};

namespace detail {

// A recorded operator chain: r = leaf[0]; r = r op[k] leaf[k + 1] (swapped[k]: leaf[k + 1] op[k] r).  Owned by the Storage
// of its (not yet computed) result; run() evaluates it there -- through smhip_chain (csrc/chain.hip: one pass where the
// operands allow), or, for a chain that stayed one operator long, through the plain operator's entry point.  A leaf keeps
// the operand's storage alive and a copy of its offset / shape / strides in place (no allocation per operand: recording an
// operator costs one allocation, the chain itself).
template <typename T>
struct Chain final : PendingBase {
    static constexpr int kMaxLeaves = 8;
    struct Leaf {
        std::shared_ptr<Storage<T>> st;
        std::size_t offset = 0, total = 0;
        int ndim = 0;
        std::size_t shape[MAX_NDIM] = {}, strides[MAX_NDIM] = {};
        bool is_scalar = false;
        T value{};
        bool dense() const {
            std::size_t expect = 1;
            for (int i = ndim; i-- > 0;) {
                if (strides[i] != expect) return false;
                expect *= shape[i];
            }
            return true;
        }
    };
    Storage<T> *out;
    std::size_t out_offset = 0;  // the result's first element in `out` (assignment into a dense block of an existing array)
    bool out_partial = false;    // ... which is then only part of that storage: its other elements stay what they are
    int out_ndim = 0;
    std::size_t out_shape[MAX_NDIM] = {};
    int device;
    int n_leaves = 0;
    Leaf leaves[kMaxLeaves];
    int ops[kMaxLeaves] = {}, swapped[kMaxLeaves] = {};

    Chain(Storage<T> *o, const std::vector<std::size_t> &sh, int dev, const SMArray<T> &head) : out(o), device(dev) {
        retarget(o, sh);
        set(leaves[n_leaves++], head);
    }
    bool full() const { return n_leaves == kMaxLeaves; }
    void retarget(Storage<T> *o, const std::vector<std::size_t> &sh, std::size_t offset = 0, bool partial = false) {
        out = o;
        out_offset = offset;
        out_partial = partial;
        out_ndim = static_cast<int>(sh.size());
        for (int i = 0; i < out_ndim; ++i) out_shape[i] = sh[i];
    }
    // May the chain's result be written straight into the dense block (st, offset, shape)?  Yes if no operand lives in that
    // storage, or every operand that does IS that block (same offset, same shape, dense): an in-place elementwise update.
    bool may_write_into(const Storage<T> *st, std::size_t offset, const std::vector<std::size_t> &sh) const {
        if (static_cast<int>(sh.size()) != out_ndim) return false;
        for (int i = 0; i < out_ndim; ++i)
            if (sh[i] != out_shape[i]) return false;
        for (int k = 0; k < n_leaves; ++k) {
            const Leaf &lf = leaves[k];
            if (lf.is_scalar || lf.st.get() != st) continue;
            if (lf.offset != offset || lf.ndim != out_ndim || !lf.dense()) return false;
            for (int i = 0; i < out_ndim; ++i)
                if (lf.shape[i] != out_shape[i]) return false;
        }
        return true;
    }
    void push(int op, bool swap, const SMArray<T> &operand) {
        ops[n_leaves - 1] = op;
        swapped[n_leaves - 1] = swap;
        set(leaves[n_leaves++], operand);
    }
    void push(int op, bool swap, T scalar) {
        ops[n_leaves - 1] = op;
        swapped[n_leaves - 1] = swap;
        Leaf &lf = leaves[n_leaves++];
        lf.is_scalar = true;
        lf.value = scalar;
    }

    void run() override {
        std::unique_ptr<PendingBase> self = std::move(out->pending);  // the result is no longer pending; *this lives to the end of run()
        if (tls_pending == this) tls_pending = nullptr;
        hip::DeviceGuard on(device);
        const int n = n_leaves, nd = out_ndim;
        std::int64_t strides[kMaxLeaves * MAX_NDIM] = {}, sh[MAX_NDIM];
        for (int i = 0; i < nd; ++i) sh[i] = static_cast<std::int64_t>(out_shape[i]);
        const void *ptrs[kMaxLeaves] = {};
        T scalars[kMaxLeaves] = {};
        for (int k = 0; k < n; ++k) {
            const Leaf &lf = leaves[k];
            if (lf.is_scalar) { scalars[k] = lf.value; continue; }
            const int shift = nd - lf.ndim;  // right-aligned, as sm::broadcast aligns them (SMUtils.h:51-72)
            for (int i = 0; i < lf.ndim; ++i)
                strides[k * nd + shift + i] = (lf.shape[i] == 1 && out_shape[shift + i] != 1) ? 0 : static_cast<std::int64_t>(lf.strides[i]);
            ptrs[k] = lf.st->dev_ro() + lf.offset;
        }
        T *dst = (out_partial ? out->dev_rw() : out->dev_wo()) + out_offset;
        if (n == 2) {  // one operator after all: the plain operator's entry points, exactly as before chains existed
            ++tls_fusion_stats.single_ops;
            const Leaf &x = leaves[0], &y = leaves[1];
            if (!y.is_scalar) {
                hip::check(smhip_elementwise(ops[0], hip::dtype_of<T>::id, ptrs[0], strides, ptrs[1], strides + nd, sh, nd, dst));
            } else if (x.dense()) {
                hip::check(smhip_array_scalar(ops[0], hip::dtype_of<T>::id, ptrs[0], &y.value, x.total, dst));
            } else {  // a view against a scalar: honour its strides (the reference reads views as flat here)
                hip::DeviceBuffer s(sizeof(T));
                hip::check(smhip_upload(s.get(), &y.value, sizeof(T)));
                hip::check(smhip_elementwise(ops[0], hip::dtype_of<T>::id, ptrs[0], strides, s.get(), strides + nd, sh, nd, dst));  // strides + nd: the scalar's row, all zero
            }
            return;
        }
        ++tls_fusion_stats.chains;
        tls_fusion_stats.fused_stages += static_cast<unsigned long long>(n - 1);
        hip::check(smhip_chain(hip::dtype_of<T>::id, n, ptrs, strides, scalars, ops, swapped, sh, nd, dst));
    }

    // The SUM of the chain's value instead of the value (SMArray::sum() of the expression's unevaluated temporary): the same
    // operands and stages through smhip_chain_sum; the result's storage is left without elements -- it is a temporary nobody
    // else refers to (pending_temporary()), and goes away with the expression.
    double run_sum() {
        std::unique_ptr<PendingBase> self = std::move(out->pending);
        if (tls_pending == this) tls_pending = nullptr;
        hip::DeviceGuard on(device);
        const int n = n_leaves, nd = out_ndim;
        std::int64_t strides[kMaxLeaves * MAX_NDIM] = {}, sh[MAX_NDIM];
        for (int i = 0; i < nd; ++i) sh[i] = static_cast<std::int64_t>(out_shape[i]);
        const void *ptrs[kMaxLeaves] = {};
        T scalars[kMaxLeaves] = {};
        for (int k = 0; k < n; ++k) {
            const Leaf &lf = leaves[k];
            if (lf.is_scalar) { scalars[k] = lf.value; continue; }
            const int shift = nd - lf.ndim;
            for (int i = 0; i < lf.ndim; ++i)
                strides[k * nd + shift + i] = (lf.shape[i] == 1 && out_shape[shift + i] != 1) ? 0 : static_cast<std::int64_t>(lf.strides[i]);
            ptrs[k] = lf.st->dev_ro() + lf.offset;
        }
        ++tls_fusion_stats.chains;
        ++tls_fusion_stats.summed_chains;
        tls_fusion_stats.fused_stages += static_cast<unsigned long long>(n - 1);
        double total = 0;
        hip::check(smhip_chain_sum(hip::dtype_of<T>::id, n, ptrs, strides, scalars, ops, swapped, sh, nd, &total));
        return total;
    }

private:
    static void set(Leaf &lf, const SMArray<T> &a) {
        lf.st = a.data.storage();
        lf.offset = a.data.offset();
        lf.total = a.totalSize;
        lf.ndim = static_cast<int>(a._shape.size());
        for (int i = 0; i < lf.ndim; ++i) { lf.shape[i] = a._shape[i]; lf.strides[i] = a._strides[i]; }
    }
};

}  // namespace detail

// What sm::unique_all returns (the Array API's names): the distinct values, where each first occurs in the flattening, the value
// number of every element, and how often each value occurs.
template <typename T>
struct UniqueAll {
    SMArray<T> values;
    SMArray<std::int64_t> index, inverse, counts;
};

// A CONDITION: cmp(x, rhs) with rhs an array or a scalar, or "x is nonzero".  A small value: handles on its operands (which keep
// their storage alive, so `auto c = a * b > 1.0f;` is safe) and the comparison.  Nothing is computed until sm::where, assign_where,
// count_nonzero, flatnonzero, nonzero or select asks, and then inside their kernels.  It is not an array, and it does not convert to
// bool: `if (a > b)` does not compile.
template <typename T>
struct Cond {
    static_assert(detail::four_types_v<T>, "a condition compares float, double, int or std::int64_t arrays");
    Cond(const SMArray<T> &nonzero) : x_(nonzero.alias()) {}  // implicit: an array where a condition is expected stands for "nonzero"
    Cond(const SMArray<T> &x, smhip_cmp cmp, const SMArray<T> &y) : x_(x.alias()), y_(new SMArray<T>(y.alias())), cmp_(cmp) {}
    Cond(const SMArray<T> &x, smhip_cmp cmp, T scalar) : x_(x.alias()), cmp_(cmp), scalar_(scalar) {}

    const SMArray<T> &left() const { return x_; }
    const SMArray<T> *right() const { return y_.get(); }  // nullptr: the right-hand side is scalar() (or there is none: nonzero)
    smhip_cmp cmp() const { return cmp_; }
    T scalar() const { return scalar_; }
    // x against y by numpy's rule; std::invalid_argument when they do not broadcast.
    std::vector<std::size_t> shape() const {
        std::vector<std::size_t> s = x_.shape();
        if (y_) detail::broadcast_into(s, y_->shape(), "condition");
        return s;
    }

    // The condition as the C ABI takes it, seen over `over`: device pointers (pending chains are evaluated here), strides in elements.
    struct Call {
        std::vector<std::int64_t> shape, sx, sy;
        const T *x = nullptr, *y = nullptr;
        T scalar;
        int cmp;
        Call(const Cond &c, const std::vector<std::size_t> &over, const char *who) : shape(hip::to_i64(over)), scalar(c.scalar_), cmp(c.cmp_) {
            sx = detail::strides_over(c.x_.shape(), c.x_.strides(), over, who);
            if (c.y_) sy = detail::strides_over(c.y_->shape(), c.y_->strides(), over, who);
            if (shape.empty()) shape = {1}, sx = {1}, sy = std::vector<std::int64_t>(c.y_ ? 1 : 0, 1);  // a 0-d array is one element
            for (std::int64_t n : shape) empty |= n == 0;
            if (empty) return;
            x = c.x_.device_data();
            if (c.y_) y = c.y_->device_data();
        }
        int ndim() const { return static_cast<int>(shape.size()); }
        // np.count_nonzero: one word from the pool, downloaded -- WAITS FOR THE STREAM.
        std::int64_t count() const {
            if (empty) return 0;
            const detail::DeviceWord<> word;
            hip::check(smhip_select_count(cmp, hip::dtype_of<T>::id, x, sx.data(), y, sy.data(), &scalar, shape.data(), ndim(), word.ptr()));
            ++detail::tls_fusion_stats.selects;
            return word.read();
        }
        bool empty = false;
    };

    std::int64_t count_nonzero() const {
        const auto over = shape();
        hip::DeviceGuard on(device());
        return Call(*this, over, "count_nonzero").count();
    }
    // The row-major positions where the condition holds, shape {count}.
    SMArray<std::int64_t> flatnonzero() const {
        const auto over = shape();
        hip::DeviceGuard on(device());
        const Call call(*this, over, "flatnonzero");
        const std::int64_t total = call.count();
        SMArray<std::int64_t> out = SMArray<std::int64_t>::device_empty(std::vector<std::size_t>{static_cast<std::size_t>(total)});
        if (total == 0) return out;
        hip::check(smhip_select(SMHIP_SELECT_INDEX, call.cmp, hip::dtype_of<T>::id, call.x, call.sx.data(), call.y, call.sy.data(), &call.scalar, call.shape.data(),
                                call.ndim(), nullptr, nullptr, 0, out.device_data_mut(), total, nullptr));
        ++detail::tls_fusion_stats.selects;
        return out;
    }
    // One array of shape {count} per axis: the coordinates where the condition holds, in row-major order.
    std::vector<SMArray<std::int64_t>> nonzero() const {
        const auto over = shape();
        hip::DeviceGuard on(device());
        const Call call(*this, over, "nonzero");
        const std::int64_t total = call.count();
        const std::size_t nd = static_cast<std::size_t>(call.ndim());
        std::vector<SMArray<std::int64_t>> out;
        if (total == 0) {
            for (std::size_t d = 0; d < nd; ++d) out.push_back(SMArray<std::int64_t>::device_empty(std::vector<std::size_t>{0}));
            return out;
        }
        SMArray<std::int64_t> planes = SMArray<std::int64_t>::device_empty(std::vector<std::size_t>{nd, static_cast<std::size_t>(total)});
        hip::check(smhip_select(SMHIP_SELECT_COORDS, call.cmp, hip::dtype_of<T>::id, call.x, call.sx.data(), call.y, call.sy.data(), &call.scalar, call.shape.data(),
                                call.ndim(), nullptr, nullptr, 0, planes.device_data_mut(), total, nullptr));
        ++detail::tls_fusion_stats.selects;
        for (std::size_t d = 0; d < nd; ++d) out.push_back(planes(d, SLICE_ALL));  // views of the one buffer
        return out;
    }

private:
    int device() const { return y_ ? SMArray<T>::common_device(x_, *y_) : x_.device(); }
    SMArray<T> x_;
    std::unique_ptr<SMArray<T>> y_;
    smhip_cmp cmp_ = SMHIP_CMP_NONZERO;
    T scalar_{};
};

// == != < <= > >= between two arrays, an array and a scalar, or a scalar and an array (the comparison turned round): a Cond<T>.
#define SM_COMPARISON(OP, CMP, TURNED)                                                                                       \
    template <typename T>                                                                                                    \
    Cond<T> operator OP(const SMArray<T> &x, const SMArray<T> &y) { return Cond<T>(x, CMP, y); }                             \
    template <typename T>                                                                                                    \
    Cond<T> operator OP(const SMArray<T> &x, std::type_identity_t<T> s) { return Cond<T>(x, CMP, s); }                       \
    template <typename T>                                                                                                    \
    Cond<T> operator OP(std::type_identity_t<T> s, const SMArray<T> &x) { return Cond<T>(x, TURNED, s); }
SM_COMPARISON(==, SMHIP_CMP_EQ, SMHIP_CMP_EQ)
SM_COMPARISON(!=, SMHIP_CMP_NE, SMHIP_CMP_NE)
SM_COMPARISON(<, SMHIP_CMP_LT, SMHIP_CMP_GT)
SM_COMPARISON(<=, SMHIP_CMP_LE, SMHIP_CMP_GE)
SM_COMPARISON(>, SMHIP_CMP_GT, SMHIP_CMP_LT)
SM_COMPARISON(>=, SMHIP_CMP_GE, SMHIP_CMP_LE)
#undef SM_COMPARISON

// What the operator fusion did on the calling thread so far (chains evaluated as one call, operators inside them, deferred
// operators that stayed alone).
inline detail::FusionStats fusion_stats() { return detail::tls_fusion_stats; }

}  // namespace sm
