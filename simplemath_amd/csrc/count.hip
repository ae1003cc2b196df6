// count.hip -- the counting family: np.searchsorted (smhip_searchsorted), np.bincount (smhip_bincount) and np.histogram
// (smhip_histogram).  numpy is the contract (smhip.h has it in full).
//
// INTEGER COUNTS MAY USE ATOMICS.  Every other family of this library avoids them because a float sum depends on the order of its
// terms; integer addition commutes and associates, so whatever order the increments arrive in, the counts are the same bits on every
// run, stream and grid.  The atomics here are plain C++ atomicAdd on 32-bit words in LDS and on the 64-bit words of the result.
//
// NO ADDRESS OUTSIDE THE RESULT IS EVER FORMED.  An id goes through pick() (index_mode.hip.h, shared with take_axis.hip and
// scatter_axis.hip) and is a position in [0, nbins - 1] BEFORE it is used as an address; under CHECKED an id outside [-nbins, nbins) is
// dropped and any lane that meets one stores the constant 1 to *bad_out.  A value's bin comes from a search that cannot leave
// [0, E], and everything outside [0, bins - 1] is not counted.
//
// The order of values is sort_axis.hip's ascending order: -0 == +0, every NaN after every number, NaNs equal among themselves.
//   searchsorted   edges of at most kEdgeLdsBytes are staged in LDS once per workgroup (route LDS), longer tables are searched in
//                  global memory (route GLOBAL).  x is read with 16-byte loads, the int64 result written with 16-byte stores; the
//                  elements before the first aligned vector and after the last whole one go one per lane.
//   counting       one kernel, written against a Binner: IdBinner (bincount: pick), EdgeBinner (histogram with explicit edges: the
//                  binary search of searchsorted, side right, minus 1; a value equal to the last edge in the last bin) and
//                  UniformBinner (histogram over a range: a guess from one multiply, corrected against the uploaded table by two
//                  one-directional loops, each bounded by the bin count).  The bin numbers never reach HBM.
//     route LDS    (bins <= kLdsBins) the entries are cut into fixed contiguous SLICES; a workgroup clears a private table of
//                  32-bit counters in LDS ([bin][replica]: `replicas` copies of each counter, a lane adds to copy lane % replicas, so
//                  that entries which all name one bin do not serialise on one word), walks its slice with 16-byte loads, counts with
//                  LDS atomic adds, folds the replicas and writes row `slice` of a pooled [slices][bins] buffer with plain stores.  A
//                  finishing launch sums the rows per bin into the int64 result (no global atomics; the result needs no clearing).
//                  With one slice the workgroup widens straight into the result.  A slice is at most kMaxSlice < 2^32 entries, so
//                  a 32-bit counter cannot wrap between two write-outs, whatever the grid cap: the loop is over slices.
//     route GLOBAL (bins > kLdsBins) the result is cleared in stream order and the same walk adds with atomicAdd on its 64-bit words.
//                  Entries that all name one bin serialise on one word of HBM: slow by construction, recorded in DESIGN.md.
// An operand that is not dense row-major is copied dense first through Pooled (SMHIP_COUNT_COPY).  Every kernel loops grid-stride
// under one capped grid (SMHIP_COUNT_GRID_CAP).
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "index_mode.hip.h"
#include "internal.h"

namespace smhip {
namespace {

using namespace axis_plan;  // kBlock, GridCap, Pooled, row_major, ceil_div

constexpr int kLdsBins = 8192;                      // K: the most bins route LDS takes (32 KiB of 32-bit counters, one replica)
constexpr int kEdgeLdsBytes = 32768;                // the most bytes of an edge table staged in LDS
constexpr int kMaxReplicas = 16;                    // copies of a counter, at most
constexpr int kLoadsInFlight = 4;                   // 16-byte loads a lane has outstanding
constexpr int64_t kMinSlice = (int64_t)1 << 14;     // entries of a slice, at least (a multiple of kSliceUnit)
constexpr int64_t kMaxSlice = (int64_t)1 << 31;     // ... and at most: below 2^32, what a 32-bit counter holds
constexpr int64_t kSliceUnit = 1024;                // slices are whole multiples of it: every slice starts at the same offset mod 16 bytes
constexpr int kFinishBins = 16, kFinishRows = 16;   // the finishing launch: a workgroup sums 16 bins over 16 interleaved row sets

template <typename T> struct alignas(16) Vec16 { T v[16 / sizeof(T)]; };
struct alignas(16) I64x2 { int64_t v[2]; };

// sort_axis.hip's ascending order: a number before a larger number and before every NaN.
template <typename T> __device__ __forceinline__ bool before(T a, T b) {
    if constexpr (std::is_floating_point<T>::value) return a < b || (b != b && a == a);
    else return a < b;
}

// Right: the first i with x before tab[i]; else the first i with !(tab[i] before x).  In [0, n]; at most ceil(log2(n + 1)) steps
// whatever the table holds.
template <typename T, bool Right, typename Index> __device__ __forceinline__ Index search(const T *tab, Index n, T x) {
    Index lo = 0, hi = n;
    while (lo < hi) {
        const Index mid = lo + ((hi - lo) >> 1);
        const bool right_of_mid = Right ? !before(x, tab[mid]) : before(tab[mid], x);
        if (right_of_mid) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// ------------------------------------------------------------------------------------------------------ searchsorted
// out[i] = search(edges, x[i]).  `head` elements stand before the first 16-byte boundary of x; out_vec: out + head is 16-byte aligned.
template <typename T, bool Right, bool Staged>
__global__ __launch_bounds__(kBlock) void searchsorted_kernel(const T *__restrict__ edges, int64_t E, const T *__restrict__ x, int64_t n, int64_t head,
                                                              int64_t *__restrict__ out, int out_vec) {
    extern __shared__ __attribute__((aligned(16))) unsigned char count_smem[];
    constexpr int W = 16 / (int)sizeof(T);
    using Index = typename std::conditional<Staged, int, int64_t>::type;
    const T *tab = edges;
    if constexpr (Staged) {
        T *staged = reinterpret_cast<T *>(count_smem);
        for (int i = threadIdx.x; i < (int)E; i += kBlock) staged[i] = edges[i];
        __syncthreads();
        tab = staged;
    }
    const Index ne = (Index)E;
    const int64_t nv = (n - head) / W, tail = n - head - nv * W;
    if (blockIdx.x == 0) {  // the elements that are not part of a whole aligned vector
        if ((int64_t)threadIdx.x < head) out[threadIdx.x] = (int64_t)search<T, Right, Index>(tab, ne, x[threadIdx.x]);
        if ((int64_t)threadIdx.x < tail) {
            const int64_t i = head + nv * W + threadIdx.x;
            out[i] = (int64_t)search<T, Right, Index>(tab, ne, x[i]);
        }
    }
    const Vec16<T> *xv = reinterpret_cast<const Vec16<T> *>(x + head);
    int64_t *ov = out + head;
    const int64_t step = (int64_t)gridDim.x * kBlock;
    for (int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x; v < nv; v += step) {
        const Vec16<T> in = xv[v];
        int64_t r[W];
#pragma unroll
        for (int w = 0; w < W; ++w) r[w] = (int64_t)search<T, Right, Index>(tab, ne, in.v[w]);
        int64_t *o = ov + v * W;
        if (out_vec) {
#pragma unroll
            for (int w = 0; w < W; w += 2) *reinterpret_cast<I64x2 *>(o + w) = I64x2{{r[w], r[w + 1]}};
        } else {
#pragma unroll
            for (int w = 0; w < W; ++w) o[w] = r[w];
        }
    }
}

// ------------------------------------------------------------------------------------------------------ the binners
// bin(tab, v, bad): the bin of entry v in [0, bins - 1], or -1 when it is not counted.  `tab` is the edge table, in LDS when kStaged.
template <typename I, int Mode> struct IdBinner {
    using Elem = I;
    static constexpr bool kStaged = false;
    int64_t R;
    __device__ __forceinline__ const I *table() const { return nullptr; }
    __device__ __forceinline__ int64_t edges() const { return 0; }
    __device__ __forceinline__ int64_t bin(const I *, I v, bool &bad) const {
        bool b = false;
        const int64_t p = pick<Mode>((int64_t)v, R, b);
        bad |= b;
        return b ? -1 : p;
    }
};

template <typename T, bool Staged> struct EdgeBinner {
    using Elem = T;
    static constexpr bool kStaged = Staged;
    using Index = typename std::conditional<Staged, int, int64_t>::type;
    const T *tab_global;
    int64_t bins;
    __device__ __forceinline__ const T *table() const { return tab_global; }
    __device__ __forceinline__ int64_t edges() const { return bins + 1; }
    __device__ __forceinline__ int64_t bin(const T *tab, T v, bool &) const {
        const Index at = search<T, true, Index>(tab, (Index)(bins + 1), v);
        if (at <= (Index)bins) return (int64_t)at - 1;  // -1: before the first edge
        return v == tab[bins] ? bins - 1 : -1;          // past every edge: the last edge itself belongs to the last bin; above it, and NaN, nowhere
    }
};

template <typename T, bool Staged> struct UniformBinner {
    using Elem = T;
    static constexpr bool kStaged = Staged;
    const T *tab_global;
    int64_t bins;
    double lo, scale;  // scale = bins / (hi - lo)
    __device__ __forceinline__ const T *table() const { return tab_global; }
    __device__ __forceinline__ int64_t edges() const { return bins + 1; }
    __device__ __forceinline__ int64_t bin(const T *tab, T v, bool &) const {
        if (!(v >= tab[0] && v <= tab[bins])) return -1;  // below, above, NaN
        const double gd = ((double)v - lo) * scale;
        int64_t g = !(gd >= 0.0) ? 0 : !(gd < (double)bins) ? bins - 1 : (int64_t)gd;
        // the guess against the table: down while v is below its bin's left edge, then up while it is at or past the right one;
        // each loop bounded by the bin count, neither entered again
        for (int64_t k = 0; k < bins && g > 0 && v < tab[g]; ++k) --g;
        for (int64_t k = 0; k < bins && g + 1 < bins && v >= tab[g + 1]; ++k) ++g;
        return g;
    }
};

// ------------------------------------------------------------------------------------------------------ the counting kernel
struct CountArgs {
    int64_t n, per, slices, bins;  // slice s = entries [s * per, min(n, (s + 1) * per))
    int replicas, direct;          // direct: one slice, widened straight into the result
};

template <typename B, bool Lds>
__global__ __launch_bounds__(kBlock) void count_kernel(B b, const typename B::Elem *__restrict__ x, CountArgs g, uint32_t *__restrict__ rows,
                                                       unsigned long long *__restrict__ out, int64_t *bad_out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char count_smem[];
    using T = typename B::Elem;
    constexpr int W = 16 / (int)sizeof(T), U = kLoadsInFlight;
    const int tid = threadIdx.x;
    const int cells = Lds ? (int)g.bins * g.replicas : 0;
    uint32_t *cnt = reinterpret_cast<uint32_t *>(count_smem);  // [bins][replicas]
    const T *tab = b.table();
    if constexpr (B::kStaged) {
        T *staged = reinterpret_cast<T *>(count_smem + (((size_t)cells * sizeof(uint32_t) + 15) & ~(size_t)15));
        const int ne = (int)b.edges();
        for (int i = tid; i < ne; i += kBlock) staged[i] = b.table()[i];
        tab = staged;  // the first barrier of the slice loop stands between these stores and the first search
    }
    const int mine = tid & (g.replicas - 1);
    bool bad = false;
    auto count_one = [&](T v) {
        const int64_t k = b.bin(tab, v, bad);
        if (k < 0) return;
        if constexpr (Lds) atomicAdd(&cnt[(int)k * g.replicas + mine], 1u);
        else atomicAdd(&out[k], 1ull);
    };
    for (int64_t s = blockIdx.x; s < g.slices; s += gridDim.x) {  // workgroup-uniform
        if constexpr (Lds)
            for (int c = tid; c < cells; c += kBlock) cnt[c] = 0;
        __syncthreads();
        const int64_t first = s * g.per, len = (first + g.per < g.n ? first + g.per : g.n) - first;
        const T *p = x + first;
        int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15) / sizeof(T));
        if (head > len) head = len;
        const int64_t nv = (len - head) / W, tail = len - head - nv * W;
        if (tid < head) count_one(p[tid]);
        const Vec16<T> *pv = reinterpret_cast<const Vec16<T> *>(p + head);
        for (int64_t v0 = tid; v0 < nv; v0 += (int64_t)kBlock * U) {
            Vec16<T> in[U];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (v0 + (int64_t)u * kBlock < nv) in[u] = pv[v0 + (int64_t)u * kBlock];
#pragma unroll
            for (int u = 0; u < U; ++u)
                if (v0 + (int64_t)u * kBlock < nv) {
#pragma unroll
                    for (int w = 0; w < W; ++w) count_one(in[u].v[w]);
                }
        }
        if (tid < tail) count_one(p[head + nv * W + tid]);
        if constexpr (Lds) {
            __syncthreads();
            for (int k = tid; k < (int)g.bins; k += kBlock) {
                uint32_t sum = 0;  // a slice holds fewer than 2^32 entries
                for (int r = 0; r < g.replicas; ++r) sum += cnt[k * g.replicas + r];
                if (g.direct) out[k] = sum;
                else rows[s * g.bins + k] = sum;
            }
            __syncthreads();
        }
    }
    if (bad && bad_out) *bad_out = 1;
}

// out[bin] = the sum of rows[s][bin] over the slices: a lane per (bin, row set), the row sets folded through LDS.
__global__ __launch_bounds__(kBlock) void count_finish_kernel(const uint32_t *__restrict__ rows, int64_t slices, int64_t bins, unsigned long long *__restrict__ out) {
    static_assert(kFinishBins * kFinishRows == kBlock, "a lane per (bin, row set)");
    __shared__ unsigned long long part[kFinishRows][kFinishBins];
    const int bl = threadIdx.x % kFinishBins, sl = threadIdx.x / kFinishBins;
    for (int64_t base = (int64_t)blockIdx.x * kFinishBins; base < bins; base += (int64_t)gridDim.x * kFinishBins) {  // workgroup-uniform
        const int64_t bin = base + bl;
        unsigned long long acc = 0;
        if (bin < bins)
            for (int64_t s = sl; s < slices; s += kFinishRows) acc += rows[s * bins + bin];
        part[sl][bl] = acc;
        __syncthreads();
        if (sl == 0 && bin < bins) {
            unsigned long long sum = 0;
#pragma unroll
            for (int r = 0; r < kFinishRows; ++r) sum += part[r][bl];
            out[bin] = sum;
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------------ the planner
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_COUNT_GRID_CAP")); return g; }  // the cap of every launch here, read once

struct Plan {
    int route = SMHIP_COUNT_ROUTE_NONE;
    bool copy = false, staged = false;
    int64_t n = 0, bins = 0, slices = 0, per = 0, groups = 0, edge_budget = 0;
    int replicas = 1;
    int launches() const {
        if (route == SMHIP_COUNT_ROUTE_NONE) return 0;
        return (copy ? 1 : 0) + 1 + (finish() ? 1 : 0);
    }
    bool finish() const { return counting && route == SMHIP_COUNT_ROUTE_LDS && slices > 1; }
    int code() const { return route | (copy && route != SMHIP_COUNT_ROUTE_NONE ? SMHIP_COUNT_COPY : 0); }
    bool counting = false;
};

int replicas_for(int64_t bins) {
    int r = 1;
    while (r < kMaxReplicas && bins * r * 2 <= kLdsBins) r *= 2;
    return r;
}

// `bins`: the edges of searchsorted, the bins of bincount and histogram.  `edge_size`: the bytes of an edge, 0 when there is no table.
void make_plan(int what, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int64_t bins, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    p.counting = what != SMHIP_COUNT_SEARCHSORTED;
    p.bins = bins;
    p.edge_budget = what == SMHIP_COUNT_BINCOUNT ? 0 : kEdgeLdsBytes / (int64_t)dtype_size(dtype);
    int64_t n = 1;
    for (int d = 0; d < ndim; ++d) n *= shape[d];  // the checks have bounded it
    p.n = n;
    if (n == 0 || bins == 0) return;
    p.copy = !row_major(shape, strides, ndim);
    const int W = 16 / (int)dtype_size(dtype);
    if (!p.counting) {
        p.staged = bins <= p.edge_budget;
        p.route = p.staged ? SMHIP_COUNT_ROUTE_LDS : SMHIP_COUNT_ROUTE_GLOBAL;
        p.groups = grid_cap().capped(ceil_div(ceil_div(n, W), kBlock));
        p.per = ceil_div(n, p.groups);
        p.slices = p.groups;
        return;
    }
    p.route = bins <= kLdsBins ? SMHIP_COUNT_ROUTE_LDS : SMHIP_COUNT_ROUTE_GLOBAL;
    p.staged = what == SMHIP_COUNT_HISTOGRAM && bins + 1 <= p.edge_budget;
    p.replicas = p.route == SMHIP_COUNT_ROUTE_LDS ? replicas_for(bins) : 1;
    // as many slices as keep the device busy, none shorter than kMinSlice, none of 2^32 entries or more
    const int64_t target = p.route == SMHIP_COUNT_ROUTE_GLOBAL ? 4096 : bins <= 2048 ? 1024 : 512;
    int64_t per = std::max(ceil_div(n, target), kMinSlice);
    per = std::min(ceil_div(per, kSliceUnit) * kSliceUnit, kMaxSlice);
    p.per = per;
    p.slices = ceil_div(n, per);
    p.groups = grid_cap().capped(p.slices);
}

// ------------------------------------------------------------------------------------------------------ launching
template <typename B, bool Lds>
int run_count_route(const B &b, const typename B::Elem *x, const Plan &p, int64_t *counts, int64_t *bad, hipStream_t s) {
    unsigned long long *out = reinterpret_cast<unsigned long long *>(counts);
    CountArgs g{p.n, p.per, p.slices, p.bins, p.replicas, Lds && p.slices == 1 ? 1 : 0};
    size_t lds = Lds ? (size_t)p.bins * p.replicas * sizeof(uint32_t) : 0;
    if (B::kStaged) lds = ((lds + 15) & ~(size_t)15) + (size_t)(p.bins + 1) * sizeof(typename B::Elem);
    Pooled pool;
    uint32_t *rows = nullptr;
    if (Lds && p.slices > 1) {
        void *raw;
        if (int rc = pool.take((size_t)p.slices * p.bins * sizeof(uint32_t), &raw)) return rc;
        rows = static_cast<uint32_t *>(raw);
    }
    if (!Lds) SMHIP_TRY(hipMemsetAsync(counts, 0, (size_t)p.bins * sizeof(int64_t), s));
    hipLaunchKernelGGL((count_kernel<B, Lds>), dim3((unsigned)p.groups), dim3(kBlock), lds, s, b, x, g, rows, out, bad);
    SMHIP_LAUNCH_CHECK("count");
    if (rows) {
        const unsigned blocks = grid_cap().capped(ceil_div(p.bins, kFinishBins));
        hipLaunchKernelGGL(count_finish_kernel, dim3(blocks), dim3(kBlock), 0, s, rows, p.slices, p.bins, out);
        SMHIP_LAUNCH_CHECK("count finish");
    }
    return SMHIP_OK;
}

template <typename B> int run_count(const B &b, const void *x, const Plan &p, int64_t *counts, int64_t *bad, hipStream_t s) {
    const typename B::Elem *px = static_cast<const typename B::Elem *>(x);
    return p.route == SMHIP_COUNT_ROUTE_LDS ? run_count_route<B, true>(b, px, p, counts, bad, s) : run_count_route<B, false>(b, px, p, counts, bad, s);
}

template <typename I> int run_bincount(int mode, const void *ids, const Plan &p, int64_t *counts, int64_t *bad, hipStream_t s) {
    return with_index_mode("bincount", mode, [&](auto m) { return run_count(IdBinner<I, decltype(m)::value>{p.bins}, ids, p, counts, bad, s); });
}

template <typename T> int run_histogram(bool uniform, const void *x, const void *edges, double lo, double hi, const Plan &p, int64_t *counts, hipStream_t s) {
    const T *tab = static_cast<const T *>(edges);
    if constexpr (std::is_floating_point<T>::value) {
        if (uniform) {
            const double scale = (double)p.bins / (hi - lo);
            if (p.staged) return run_count(UniformBinner<T, true>{tab, p.bins, lo, scale}, x, p, counts, nullptr, s);
            return run_count(UniformBinner<T, false>{tab, p.bins, lo, scale}, x, p, counts, nullptr, s);
        }
    }
    if (p.staged) return run_count(EdgeBinner<T, true>{tab, p.bins}, x, p, counts, nullptr, s);
    return run_count(EdgeBinner<T, false>{tab, p.bins}, x, p, counts, nullptr, s);
}

template <typename T> int run_searchsorted(int side, const void *edges, const void *x, const Plan &p, int64_t *out, hipStream_t s) {
    constexpr int W = 16 / (int)sizeof(T);
    const T *pe = static_cast<const T *>(edges), *px = static_cast<const T *>(x);
    const int64_t head = std::min<int64_t>(p.n, (int64_t)(((16 - (reinterpret_cast<uintptr_t>(px) & 15)) & 15) / sizeof(T)));
    const int out_vec = (reinterpret_cast<uintptr_t>(out + head) & 15) == 0;
    (void)W;
    const dim3 grid((unsigned)p.groups), block(kBlock);
    const size_t lds = p.staged ? (size_t)p.bins * sizeof(T) : 0;
    const bool right = side == SMHIP_SIDE_RIGHT;
    if (p.staged) {
        if (right) hipLaunchKernelGGL((searchsorted_kernel<T, true, true>), grid, block, lds, s, pe, p.bins, px, p.n, head, out, out_vec);
        else hipLaunchKernelGGL((searchsorted_kernel<T, false, true>), grid, block, lds, s, pe, p.bins, px, p.n, head, out, out_vec);
    } else {
        if (right) hipLaunchKernelGGL((searchsorted_kernel<T, true, false>), grid, block, lds, s, pe, p.bins, px, p.n, head, out, out_vec);
        else hipLaunchKernelGGL((searchsorted_kernel<T, false, false>), grid, block, lds, s, pe, p.bins, px, p.n, head, out, out_vec);
    }
    SMHIP_LAUNCH_CHECK("searchsorted");
    return SMHIP_OK;
}

// numpy's (lo - 0.5, hi + 0.5) for a range of one point.
void widen_point_range(double *lo, double *hi) {
    if (*lo == *hi) *lo -= 0.5, *hi += 0.5;
}

template <typename T> int fill_edges(int64_t bins, double lo, double hi, T *edges) {
    // np.linspace(lo, hi, bins + 1): i * step + lo in fp64 -- the product rounded before the sum, so it is kept in a volatile and no
    // fused multiply-add can be formed --, the last edge hi itself, each rounded to T
    const double delta = hi - lo, step = delta / (double)bins;
    for (int64_t i = 0; i <= bins; ++i) {
        volatile double prod = step != 0.0 ? (double)i * step : (double)i / (double)bins * delta;
        const double e = i == bins ? hi : prod + lo;
        edges[i] = (T)e;
        if (!isfinite((double)edges[i]) || (i > 0 && !(edges[i - 1] < edges[i])))
            return fail(SMHIP_ERR_INVALID, "histogram: too many bins for the range: %lld bins over [%g, %g] leave edges that do not increase", (long long)bins, lo, hi);
    }
    return SMHIP_OK;
}

// Validation: everything that can be said without a device or a pointer.  *n_out: the element count of x.
int count_check(const char *who, int what, int flags, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int64_t bins) {
    if (what != SMHIP_COUNT_SEARCHSORTED && what != SMHIP_COUNT_BINCOUNT && what != SMHIP_COUNT_HISTOGRAM) return fail(SMHIP_ERR_INVALID, "%s: bad operation %d", who, what);
    if (flags & ~SMHIP_HISTOGRAM_UNIFORM) return fail(SMHIP_ERR_INVALID, "%s: unknown flag bits 0x%x", who, flags);
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (what == SMHIP_COUNT_BINCOUNT && dtype != SMHIP_I32 && dtype != SMHIP_I64) return fail(SMHIP_ERR_INVALID, "%s: bad dtype %d: the ids are i32 or i64", who, dtype);
    if (flags && (what != SMHIP_COUNT_HISTOGRAM || (dtype != SMHIP_F32 && dtype != SMHIP_F64)))
        return fail(SMHIP_ERR_INVALID, "%s: bad dtype %d: the uniform table is for a histogram of f32 or f64", who, dtype);
    if (int rc = check_extents(who, shape, strides, ndim)) return rc;
    if (bins < 0) return fail(SMHIP_ERR_INVALID, "%s: %lld %s: negative", who, (long long)bins, what == SMHIP_COUNT_SEARCHSORTED ? "edges" : "bins");
    const int64_t limit = (int64_t)1 << 59;
    if (bins >= limit) return fail(SMHIP_ERR_INVALID, "%s: %lld bins or edges exceed 2^59", who, (long long)bins);
    int64_t n = 1, span = 0;
    bool empty = false;
    for (int d = 0; d < ndim; ++d) empty |= shape[d] == 0;
    for (int d = 0; d < ndim && !empty; ++d) {
        int64_t t;
        if (__builtin_mul_overflow(n, shape[d], &n) || n >= limit || __builtin_mul_overflow(shape[d] - 1, strides[d], &t) || __builtin_add_overflow(span, t, &span) ||
            span >= limit)
            return fail(SMHIP_ERR_INVALID, "%s: the operand's span exceeds 2^59 elements", who);
    }
    if (what != SMHIP_COUNT_SEARCHSORTED && !empty && bins == 0) return fail(SMHIP_ERR_INVALID, "%s: cannot count entries into 0 bins", who);
    return SMHIP_OK;
}

void count_plan(int what, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int64_t bins, int *route, int *launches, int64_t *info6) {
    Plan pl;
    make_plan(what, dtype, shape, strides, ndim, bins, &pl);
    if (route) *route = pl.code();
    if (launches) *launches = pl.launches();
    if (info6) {
        info6[0] = pl.groups, info6[1] = pl.per, info6[2] = pl.replicas, info6[3] = kLdsBins, info6[4] = pl.edge_budget, info6[5] = pl.staged ? 1 : 0;
    }
}

int histogram_range_check(const char *who, int64_t bins, double *lo, double *hi) {
    if (bins < 1) return fail(SMHIP_ERR_INVALID, "%s: %lld bins: at least 1", who, (long long)bins);
    if (!isfinite(*lo) || !isfinite(*hi)) return fail(SMHIP_ERR_INVALID, "%s: the range [%g, %g] is not finite", who, *lo, *hi);
    if (*lo > *hi) return fail(SMHIP_ERR_INVALID, "%s: the range's upper end %g is below its lower end %g", who, *hi, *lo);
    widen_point_range(lo, hi);
    return SMHIP_OK;
}

int histogram_edges(int dtype, int64_t bins, double lo, double hi, void *edges_host) {
    if (dtype != SMHIP_F32 && dtype != SMHIP_F64) return fail(SMHIP_ERR_INVALID, "histogram_edges: bad dtype %d: f32 or f64", dtype);
    if (int rc = histogram_range_check("histogram_edges", bins, &lo, &hi)) return rc;
    if (!edges_host) return fail(SMHIP_ERR_INVALID, "histogram_edges: null table");
    return dtype == SMHIP_F32 ? fill_edges(bins, lo, hi, static_cast<float *>(edges_host)) : fill_edges(bins, lo, hi, static_cast<double *>(edges_host));
}

// x dense over `shape`, or copied dense here.
int dense_operand(const Plan &p, axis_plan::Pooled *pool, int dtype, const void **x, const int64_t *shape, const int64_t *strides, int ndim, hipStream_t s) {
    if (!p.copy) return SMHIP_OK;
    return pool->dense_copy(dtype, *x, shape, strides, ndim, s, x);
}

int launch_searchsorted(int side, int dtype, const void *edges, int64_t n_edges, const void *x, const int64_t *shape, const int64_t *strides, int ndim, int64_t *out,
                        hipStream_t s) {
    Plan pl;
    make_plan(SMHIP_COUNT_SEARCHSORTED, dtype, shape, strides, ndim, n_edges, &pl);
    if (pl.n == 0) return SMHIP_OK;
    if (n_edges == 0) {  // every value stands at position 0
        SMHIP_TRY(hipMemsetAsync(out, 0, (size_t)pl.n * sizeof(int64_t), s));
        return SMHIP_OK;
    }
    axis_plan::Pooled pool;
    if (int rc = dense_operand(pl, &pool, dtype, &x, shape, strides, ndim, s)) return rc;
    switch (dtype) {
        case SMHIP_F32: return run_searchsorted<float>(side, edges, x, pl, out, s);
        case SMHIP_F64: return run_searchsorted<double>(side, edges, x, pl, out, s);
        case SMHIP_I32: return run_searchsorted<int32_t>(side, edges, x, pl, out, s);
        case SMHIP_I64: return run_searchsorted<int64_t>(side, edges, x, pl, out, s);
    }
    return fail(SMHIP_ERR_INVALID, "searchsorted: bad dtype %d", dtype);
}

int launch_bincount(int mode, int dtype, const void *ids, const int64_t *shape, const int64_t *strides, int ndim, int64_t nbins, int64_t *counts, int64_t *bad_out,
                    hipStream_t s) {
    Plan pl;
    make_plan(SMHIP_COUNT_BINCOUNT, dtype, shape, strides, ndim, nbins, &pl);
    if (bad_out) SMHIP_TRY(hipMemsetAsync(bad_out, 0, sizeof(int64_t), s));
    if (pl.route == SMHIP_COUNT_ROUTE_NONE) {
        if (nbins) SMHIP_TRY(hipMemsetAsync(counts, 0, (size_t)nbins * sizeof(int64_t), s));
        return SMHIP_OK;
    }
    axis_plan::Pooled pool;
    if (int rc = dense_operand(pl, &pool, dtype, &ids, shape, strides, ndim, s)) return rc;
    return dtype == SMHIP_I32 ? run_bincount<int32_t>(mode, ids, pl, counts, bad_out, s) : run_bincount<int64_t>(mode, ids, pl, counts, bad_out, s);
}

int launch_histogram(int flags, int dtype, const void *x, const int64_t *shape, const int64_t *strides, int ndim, const void *edges, int64_t bins, double lo, double hi,
                     int64_t *counts, hipStream_t s) {
    Plan pl;
    make_plan(SMHIP_COUNT_HISTOGRAM, dtype, shape, strides, ndim, bins, &pl);
    if (pl.route == SMHIP_COUNT_ROUTE_NONE) {
        if (bins) SMHIP_TRY(hipMemsetAsync(counts, 0, (size_t)bins * sizeof(int64_t), s));
        return SMHIP_OK;
    }
    axis_plan::Pooled pool;
    if (int rc = dense_operand(pl, &pool, dtype, &x, shape, strides, ndim, s)) return rc;
    const bool uniform = (flags & SMHIP_HISTOGRAM_UNIFORM) != 0;
    switch (dtype) {
        case SMHIP_F32: return run_histogram<float>(uniform, x, edges, lo, hi, pl, counts, s);
        case SMHIP_F64: return run_histogram<double>(uniform, x, edges, lo, hi, pl, counts, s);
        case SMHIP_I32: return run_histogram<int32_t>(false, x, edges, lo, hi, pl, counts, s);
        case SMHIP_I64: return run_histogram<int64_t>(false, x, edges, lo, hi, pl, counts, s);
    }
    return fail(SMHIP_ERR_INVALID, "histogram: bad dtype %d", dtype);
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_searchsorted(int side, int dtype, const void *edges, int64_t n_edges, const void *x, const int64_t *shape, const int64_t *strides, int ndim,
                       int64_t *out) {
    if (side != SMHIP_SIDE_LEFT && side != SMHIP_SIDE_RIGHT) return fail(SMHIP_ERR_INVALID, "searchsorted: bad side %d", side);
    if (int rc = count_check("searchsorted", SMHIP_COUNT_SEARCHSORTED, 0, dtype, shape, strides, ndim, n_edges)) return rc;
    const int64_t n = element_count(shape, ndim);
    if (n == 0) return SMHIP_OK;
    if (!x || !out || (n_edges && !edges)) return fail(SMHIP_ERR_INVALID, "searchsorted: null operand, table or result");
    const size_t esz = dtype_size(dtype);
    if (misaligned(x, esz) || misaligned(edges, esz) || misaligned(out, sizeof(int64_t))) return fail(SMHIP_ERR_INVALID, "searchsorted: a pointer is not aligned to its element");
    const Span sx{x, span_bytes(shape, strides, ndim, esz)}, se{edges, (size_t)n_edges * esz}, so{out, (size_t)n * sizeof(int64_t)};
    if (spans_overlap(so, sx) || spans_overlap(so, se)) return fail(SMHIP_ERR_INVALID, "searchsorted: the result overlaps the operand or the table");
    SMHIP_ACQUIRE(s);  // undeclared spans (a pooled dense copy): ordered behind everything, recorded tiny operators flushed first
    return launch_searchsorted(side, dtype, edges, n_edges, x, shape, strides, ndim, out, s);
}

int smhip_bincount(int mode, int ids_dtype, const void *ids, const int64_t *shape, const int64_t *strides, int ndim, int64_t nbins, int64_t *counts,
                   int64_t *bad_out) {
    if (int rc = check_index_mode("bincount", mode)) return rc;
    if (int rc = count_check("bincount", SMHIP_COUNT_BINCOUNT, 0, ids_dtype, shape, strides, ndim, nbins)) return rc;
    const int64_t n = element_count(shape, ndim);
    if (n == 0 && nbins == 0) return SMHIP_OK;
    if ((n && !ids) || !counts) return fail(SMHIP_ERR_INVALID, "bincount: null ids or result");
    const size_t esz = dtype_size(ids_dtype);
    if (misaligned(ids, esz) || misaligned(counts, sizeof(int64_t)) || misaligned(bad_out, sizeof(int64_t)))
        return fail(SMHIP_ERR_INVALID, "bincount: a pointer is not aligned to its element");
    const Span si{ids, n ? span_bytes(shape, strides, ndim, esz) : 0}, so{counts, (size_t)nbins * sizeof(int64_t)}, sb{bad_out, bad_out ? sizeof(int64_t) : 0};
    if (spans_overlap(so, si) || spans_overlap(so, sb) || spans_overlap(sb, si)) return fail(SMHIP_ERR_INVALID, "bincount: the result, the ids and bad_out overlap");
    SMHIP_ACQUIRE(s);  // undeclared spans (the pooled rows, a dense copy)
    return launch_bincount(mode, ids_dtype, ids, shape, strides, ndim, nbins, counts, bad_out, s);
}

int smhip_histogram(int flags, int dtype, const void *x, const int64_t *shape, const int64_t *strides, int ndim, const void *edges_dev, int64_t bins, double lo,
                    double hi, int64_t *counts) {
    if (int rc = count_check("histogram", SMHIP_COUNT_HISTOGRAM, flags, dtype, shape, strides, ndim, bins)) return rc;
    if (flags & SMHIP_HISTOGRAM_UNIFORM)
        if (int rc = histogram_range_check("histogram", bins, &lo, &hi)) return rc;
    const int64_t n = element_count(shape, ndim);
    if (n == 0 && bins == 0) return SMHIP_OK;
    if ((n && (!x || !edges_dev)) || !counts) return fail(SMHIP_ERR_INVALID, "histogram: null operand, table or result");
    const size_t esz = dtype_size(dtype);
    if (misaligned(x, esz) || misaligned(edges_dev, esz) || misaligned(counts, sizeof(int64_t))) return fail(SMHIP_ERR_INVALID, "histogram: a pointer is not aligned to its element");
    const Span sx{x, n ? span_bytes(shape, strides, ndim, esz) : 0}, se{edges_dev, (size_t)(bins + 1) * esz}, so{counts, (size_t)bins * sizeof(int64_t)};
    // without elements the table may be null while its length is not: its span is then still taken from address 0
    const bool in_null_table = !edges_dev && so.bytes && reinterpret_cast<uintptr_t>(counts) < se.bytes;
    if (spans_overlap(so, sx) || spans_overlap(so, se) || in_null_table) return fail(SMHIP_ERR_INVALID, "histogram: the result overlaps the operand or the table");
    SMHIP_ACQUIRE(s);  // undeclared spans (the pooled rows, a dense copy)
    return launch_histogram(flags, dtype, x, shape, strides, ndim, edges_dev, bins, lo, hi, counts, s);
}

int smhip_histogram_edges(int dtype, int64_t bins, double lo, double hi, void *edges_host) { return histogram_edges(dtype, bins, lo, hi, edges_host); }

int smhip_count_plan(int what, int flags, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int64_t bins, int *route, int *launches,
                     int64_t *info6) {
    if (int rc = count_check("count_plan", what, flags, dtype, shape, strides, ndim, bins)) return rc;
    count_plan(what, dtype, shape, strides, ndim, bins, route, launches, info6);
    return SMHIP_OK;
}
