// unique.hip -- the runs of a dense 1-D array: np.unique's four results on sorted input (smhip_runs behind smhip_sort_axis) and
// run-length encoding on any input (unique_consecutive).  smhip.h has the contract in full.
//
// A RUN is a maximal stretch of adjacent elements that are the same in smhip_sort_axis's order: a == b, or both NaN (never, with
// SMHIP_RUNS_NAN_DISTINCT).  Element i STARTS a run when i == 0 || !same(s[i - 1], s[i]); that flag is never written to memory.  The
// rank of an element among the flags is its run number, and from one ranked pass come all four results:
//   values[k] = s[start_k]      index[k] = order[start_k]      starts[k] = start_k      inverse[order[i]] = the run of element i
// (order NULL: the identity).  The structure is select.hip's compaction, with the flag taken from an element AND its left neighbour:
//   TILES of kBlock lanes x kTileVecs vectors, lane l's u-th vector being vector u * kBlock + l of the tile (VecTraits' element-aligned
//   vectors: an operand off the 16-byte grid takes the same kernel).  The left neighbour of a vector's first element is ONE EXTRA
//   element load, s[e0 - 1]: the line it lies in is the one the lane before has just loaded.  Taking it from that lane through a DPP
//   move instead was measured and is 1 -- 20 % slower (profiles/unique_neighbour_ab.txt).
//     launch 1  runs_kernel<T, kCount>, kModeCount: the flags of a lane's 8 vectors in one 32-bit word, __ballot and __popcll per flag,
//               one int32 per tile
//     launch 2  select.hip's tile_scan_kernel: the exclusive prefix per tile in int64, the total to *count_dev
//     launch 3  runs_kernel<T, kFirsts or kAll>, kModeEmit: the flags again, per u the lane counts through wave_scan, the kTileVecs x 4
//               wave totals through LDS; the vectors are still in registers, so values are written from them.  kFirsts touches only
//               lanes that hold a flag; kAll (an inverse is wanted) visits every element.
//     launch 4  run_lengths_kernel, only when counts are wanted: counts[k] = starts[k + 1] - starts[k] over the pooled starts, the
//               last run ending at n.  The starts go through a pooled buffer of min(capacity + 1, n) words because a run's length
//               needs the NEXT run's start, which another workgroup may hold: a launch boundary orders them, nothing waits.
//   Up to kOneGroupTiles tiles ONE workgroup does all of it in one launch (kModeOne), the lengths behind a workgroup barrier.
// No atomics, no workgroup waits for another: the same bytes on every run, stream and grid.  The tile kernels loop grid-stride under
// select's capped grid.  All index arithmetic is int64; a tile's count fits int32.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "internal.h"
#include "ops.hip.h"
#include "wave.hip.h"

namespace smhip {
namespace {

using namespace axis_plan;  // kBlock, GridCap, Pooled, ceil_div
using namespace dev;

constexpr int kTileVecs = 8;           // as select.hip: a tile is 32 KiB of s
constexpr int kWaves = kBlock / 64;
constexpr int64_t kOneGroupTiles = 4;  // the one-workgroup route takes at most this many tiles
constexpr int kCount = 0, kFirsts = 1, kAll = 2;  // runs_kernel's What: count only / the runs' first elements / every element (inverse)
constexpr int kModeCount = 0, kModeEmit = 1, kModeOne = 2;
constexpr int kOutputs = SMHIP_RUNS_VALUES | SMHIP_RUNS_INDEX | SMHIP_RUNS_COUNTS | SMHIP_RUNS_INVERSE;

inline int64_t tile_elems(int dtype) { return (int64_t)kBlock * kTileVecs * vec_width(dtype); }

struct RunArgs {
    const void *s;
    const int64_t *order;
    void *values;
    int64_t *index, *counts, *inverse;
    int64_t *starts;              // pooled: the first element of run k, k < starts_cap (null: no counts)
    int32_t *tile_counts;         // kModeCount writes, tile_scan_kernel reads
    const int64_t *tile_offsets;  // kModeEmit reads
    int64_t *count_dev;           // kModeOne writes the total (may be null)
    int64_t n, n_vec, tiles, capacity, starts_cap;
    int tail, mode, nt, nan_distinct;
};

template <typename S, int N> struct Packed { typedef S type __attribute__((ext_vector_type(N), aligned(sizeof(S)))); };

template <typename T> __device__ __forceinline__ bool same(T a, T b, int nan_distinct) {
    if constexpr (std::is_floating_point<T>::value) return a == b || (!nan_distinct && a != a && b != b);
    else return a == b;
}

// The elements of vector v that exist: all of a whole vector, the n % W behind the last whole one, none past the data.
template <int W> __device__ __forceinline__ int present(const RunArgs &g, int64_t v) { return v < g.n_vec ? W : v == g.n_vec ? g.tail : 0; }

// Loads this lane's kTileVecs vectors of tile t into vx (the tail elements one by one) and returns their flags: bit u * W + w = element
// (first vector of the tile + u * kBlock + lane) * W + w starts a run.
template <typename T, bool NT>
__device__ __forceinline__ uint32_t run_flags(const RunArgs &g, int64_t t, typename VecTraits<T>::full_t (&vx)[kTileVecs]) {
    typedef typename VecTraits<T>::vec_t V;
    constexpr int W = VecTraits<T>::width;
    const T *x = static_cast<const T *>(g.s);
    const V *xv = static_cast<const V *>(g.s);
    const int64_t v0 = t * ((int64_t)kBlock * kTileVecs) + threadIdx.x;
    T left[kTileVecs];  // s[e0 - 1]: the element before the vector's first
#pragma unroll
    for (int u = 0; u < kTileVecs; ++u) {
        const int64_t v = v0 + (int64_t)u * kBlock;
        if (v < g.n_vec) {
            vx[u] = load_stream_as(T, xv + v, NT);
        } else if (v == g.n_vec) {
#pragma unroll
            for (int w = 0; w < W; ++w) vx[u][w] = w < g.tail ? x[v * W + w] : T(0);
        }
        left[u] = v > 0 && v <= g.n_vec ? x[v * W - 1] : T(0);  // v == n_vec: element n_vec * W - 1 < n exists
    }
    uint32_t bits = 0;
#pragma unroll
    for (int u = 0; u < kTileVecs; ++u) {
        const int64_t v = v0 + (int64_t)u * kBlock;
        const int cnt = present<W>(g, v);
#pragma unroll
        for (int w = 0; w < W; ++w) {
            if (w < cnt) {
                const bool starts = w == 0 ? v == 0 || !same<T>(left[u], vx[u][0], g.nan_distinct) : !same<T>(vx[u][w ? w - 1 : 0], vx[u][w], g.nan_distinct);
                bits |= (uint32_t)starts << (u * W + w);
            }
        }
    }
    return bits;
}

template <typename T, int What, bool NT> __device__ __forceinline__ void runs_body(const RunArgs &g) {
    typedef typename VecTraits<T>::full_t F;
    typedef typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type S;
    constexpr int W = VecTraits<T>::width;
    constexpr uint32_t kVecMask = (1u << W) - 1;
    __shared__ int totals[kTileVecs][kWaves];  // emit: the flags of (u, wave); count: [0][wave] alone
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool one = g.mode == kModeOne;
    int64_t carry = 0;  // kModeOne: the runs that start in the tiles before
    for (int64_t t = one ? 0 : blockIdx.x; t < g.tiles; t += one ? 1 : gridDim.x) {  // workgroup-uniform
        F vx[kTileVecs];
        const uint32_t bits = run_flags<T, NT>(g, t, vx);
        if constexpr (What == kCount) {
            int wave_total = 0;
#pragma unroll
            for (int k = 0; k < kTileVecs * W; ++k) wave_total += (int)__popcll(__ballot((bits >> k) & 1));
            if (lane == 0) totals[0][wave] = wave_total;
            __syncthreads();
            int total = 0;
#pragma unroll
            for (int k = 0; k < kWaves; ++k) total += totals[0][k];
            if (one) carry += total;
            else if (tid == 0) g.tile_counts[t] = total;
            __syncthreads();
        } else {
            int before[kTileVecs];  // the flags of the lanes before this one in its wave, per vector
#pragma unroll
            for (int u = 0; u < kTileVecs; ++u) {
                const int c = __popc((bits >> (u * W)) & kVecMask);
                const int inc = wave_scan<int>(c, lane, 0, [](int p, int q) { return p + q; });
                before[u] = inc - c;
                if (lane == 63) totals[u][wave] = inc;
            }
            __syncthreads();
            const int64_t base = one ? carry : g.tile_offsets[t];
            S *values = static_cast<S *>(g.values);
            int running = 0;
#pragma unroll
            for (int u = 0; u < kTileVecs; ++u) {
                int mine = 0;
#pragma unroll
                for (int k = 0; k < kWaves; ++k) {
                    if (k == wave) mine = running;
                    running += totals[u][k];
                }
                const uint32_t m = (bits >> (u * W)) & kVecMask;
                const int64_t v = t * ((int64_t)kBlock * kTileVecs) + (int64_t)u * kBlock + tid, e0 = v * W;
                const int cnt = present<W>(g, v);
                if (What == kAll ? cnt > 0 : m != 0) {
                    int64_t rank = base + mine + before[u];  // the runs that start before element e0
                    int64_t at[W];                           // kAll: where the element stood before the sort (order[e], or e itself)
                    if constexpr (What == kAll) {
                        if (!g.order) {
#pragma unroll
                            for (int w = 0; w < W; ++w) at[w] = e0 + w;
                        } else if (cnt == W) {  // the whole vector of order lies inside it
                            const typename Packed<int64_t, W>::type ov = *reinterpret_cast<const typename Packed<int64_t, W>::type *>(g.order + e0);
#pragma unroll
                            for (int w = 0; w < W; ++w) at[w] = ov[w];
                        } else {
#pragma unroll
                            for (int w = 0; w < W; ++w) at[w] = w < cnt ? g.order[e0 + w] : 0;
                        }
                    }
                    typename Packed<int64_t, W>::type inv;
#pragma unroll
                    for (int w = 0; w < W; ++w) {
                        if (m >> w & 1) {  // (a flag is only ever set on an element that exists)
                            if (rank < g.capacity) {
                                if (values) values[rank] = __builtin_bit_cast(S, (T)vx[u][w]);
                                if (g.index) {
                                    if constexpr (What == kAll) g.index[rank] = at[w];
                                    else g.index[rank] = g.order ? g.order[e0 + w] : e0 + w;
                                }
                            }
                            if (g.starts && rank < g.starts_cap) g.starts[rank] = e0 + w;
                            ++rank;
                        }
                        inv[w] = rank - 1;  // element 0 always starts a run: never negative on an element that exists
                    }
                    if constexpr (What == kAll) {
                        if (g.order) {
#pragma unroll
                            for (int w = 0; w < W; ++w)
                                if (w < cnt && (uint64_t)at[w] < (uint64_t)g.n) g.inverse[at[w]] = inv[w];  // a position outside [0, n) writes nothing
                        } else if (cnt == W) {
                            *reinterpret_cast<typename Packed<int64_t, W>::type *>(g.inverse + e0) = inv;
                        } else {
#pragma unroll
                            for (int w = 0; w < W; ++w)
                                if (w < cnt) g.inverse[e0 + w] = inv[w];
                        }
                    }
                }
            }
            carry += running;  // the tile's total
            __syncthreads();
        }
    }
    if (one) {
        if (tid == 0 && g.count_dev) *g.count_dev = carry;
        if constexpr (What != kCount) {
            if (g.counts) {  // the barrier that ended the last tile has made this workgroup's starts visible to all of it
                const int64_t written = carry < g.capacity ? carry : g.capacity;
                for (int64_t k = tid; k < written; k += kBlock) g.counts[k] = (k + 1 < carry ? g.starts[k + 1] : g.n) - g.starts[k];
            }
        }
    }
}

template <typename T, int What> __global__ __launch_bounds__(kBlock) void runs_kernel(RunArgs g) {
    if (g.nt) runs_body<T, What, true>(g);
    else runs_body<T, What, false>(g);
}

// counts[k] = the length of run k for k < min(U, capacity), U = the total that the prefix of the tile counts ends in.
__global__ __launch_bounds__(kBlock) void run_lengths_kernel(const int64_t *__restrict__ starts, const int64_t *__restrict__ tile_offsets,
                                                             const int32_t *__restrict__ tile_counts, int64_t tiles, int64_t n, int64_t capacity,
                                                             int64_t *__restrict__ counts) {
    const int64_t total = tile_offsets[tiles - 1] + tile_counts[tiles - 1];
    const int64_t written = total < capacity ? total : capacity;
    for (int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x; k < written; k += (int64_t)gridDim.x * kBlock)
        counts[k] = (k + 1 < total ? starts[k + 1] : n) - starts[k];
}

// ------------------------------------------------------------------------------------------------------ the planner
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_SELECT_GRID_CAP")); return g; }  // select's cap: the same tile launches

struct Plan {
    int route = SMHIP_RUNS_ROUTE_NONE, launches = 0;
    int64_t tiles = 0;
};

// outputs: the SMHIP_RUNS_* results wanted; 0: the count alone.
Plan make_plan(int dtype, int64_t n, int outputs) {
    Plan p;
    if (n == 0) return p;
    p.tiles = ceil_div(ceil_div(n, (int64_t)vec_width(dtype)), (int64_t)kBlock * kTileVecs);
    if (p.tiles <= kOneGroupTiles) p.route = SMHIP_RUNS_ROUTE_ONE, p.launches = 1;
    else p.route = SMHIP_RUNS_ROUTE_TILES, p.launches = !outputs ? 2 : outputs & SMHIP_RUNS_COUNTS ? 4 : 3;
    return p;
}

// ------------------------------------------------------------------------------------------------------ launching
template <typename T> int run_runs(int what, const Plan &p, RunArgs g, hipStream_t s) {
    auto launch = [&](int w, int mode, unsigned blocks) -> int {
        g.mode = mode;
        const dim3 grid(blocks), block(kBlock);
        if (w == kCount) hipLaunchKernelGGL((runs_kernel<T, kCount>), grid, block, 0, s, g);
        else if (w == kFirsts) hipLaunchKernelGGL((runs_kernel<T, kFirsts>), grid, block, 0, s, g);
        else hipLaunchKernelGGL((runs_kernel<T, kAll>), grid, block, 0, s, g);
        SMHIP_LAUNCH_CHECK("runs");
        return SMHIP_OK;
    };
    const bool lengths = what != kCount && g.counts;
    g.starts_cap = !lengths ? 0 : g.capacity < g.n ? g.capacity + 1 : g.n;  // run `capacity` itself ends the last length written
    const bool tiles = p.route == SMHIP_RUNS_ROUTE_TILES;
    const size_t count_bytes = tiles ? ((size_t)p.tiles * sizeof(int32_t) + 15) & ~(size_t)15 : 0;
    const size_t offset_bytes = tiles && what != kCount ? (size_t)p.tiles * sizeof(int64_t) : 0;
    const size_t pooled = count_bytes + offset_bytes + (size_t)g.starts_cap * sizeof(int64_t);
    Pooled pool;
    char *raw = nullptr;
    if (pooled) {
        void *got;
        if (int rc = pool.take(pooled, &got)) return rc;
        raw = static_cast<char *>(got);
    }
    g.starts = lengths ? reinterpret_cast<int64_t *>(raw + count_bytes + offset_bytes) : nullptr;
    if (!tiles) return launch(what, kModeOne, 1);
    g.tile_counts = reinterpret_cast<int32_t *>(raw);
    int64_t *offsets = what == kCount ? nullptr : reinterpret_cast<int64_t *>(raw + count_bytes);
    g.tile_offsets = offsets;
    const unsigned blocks = grid_cap().capped(p.tiles);
    if (int rc = launch(kCount, kModeCount, blocks)) return rc;
    if (int rc = launch_tile_scan(g.tile_counts, p.tiles, offsets, g.count_dev, s)) return rc;
    if (what == kCount) return SMHIP_OK;
    if (int rc = launch(what, kModeEmit, blocks)) return rc;
    if (lengths) {
        const int64_t most = std::min(g.capacity, g.n);  // the lengths written at most; the kernel knows how many there are
        hipLaunchKernelGGL(run_lengths_kernel, dim3(grid_cap().capped(ceil_div(most, (int64_t)kBlock))), dim3(kBlock), 0, s, g.starts, g.tile_offsets, g.tile_counts,
                           p.tiles, g.n, g.capacity, g.counts);
        SMHIP_LAUNCH_CHECK("run lengths");
    }
    return SMHIP_OK;
}

int launch_runs(int what, int flags, int dtype, RunArgs g, hipStream_t s) {
    const int outputs = what == kCount ? 0 : (g.values ? SMHIP_RUNS_VALUES : 0) | (g.index ? SMHIP_RUNS_INDEX : 0) | (g.counts ? SMHIP_RUNS_COUNTS : 0) |
                                                 (g.inverse ? SMHIP_RUNS_INVERSE : 0);
    const Plan p = make_plan(dtype, g.n, outputs);
    const int W = vec_width(dtype);
    g.n_vec = g.n / W, g.tail = (int)(g.n % W), g.tiles = p.tiles;
    g.nt = stream_reads((size_t)g.n * dtype_size(dtype));
    g.nan_distinct = (flags & SMHIP_RUNS_NAN_DISTINCT) != 0;
    switch (dtype) {
        case SMHIP_F32: return run_runs<float>(what, p, g, s);
        case SMHIP_F64: return run_runs<double>(what, p, g, s);
        case SMHIP_I32: return run_runs<int32_t>(what, p, g, s);
        case SMHIP_I64: return run_runs<int64_t>(what, p, g, s);
    }
    return fail(SMHIP_ERR_INVALID, "runs: bad dtype %d", dtype);
}

// What can be said without a pointer: flags, dtype, n.
int runs_check(const char *who, int flags, int dtype, int64_t n) {
    if (flags & ~SMHIP_RUNS_NAN_DISTINCT) return fail(SMHIP_ERR_INVALID, "%s: unknown flag bits 0x%x", who, flags);
    if (!valid_dtype(dtype)) return fail(SMHIP_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    if (n < 0) return fail(SMHIP_ERR_INVALID, "%s: n %lld: negative", who, (long long)n);
    if (n >= (int64_t)1 << 59) return fail(SMHIP_ERR_INVALID, "%s: %lld elements exceed 2^59", who, (long long)n);
    return SMHIP_OK;
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_runs_count(int flags, int dtype, const void *s, int64_t n, int64_t *count_dev) {
    if (int rc = runs_check("runs_count", flags, dtype, n)) return rc;
    if (!count_dev) return fail(SMHIP_ERR_INVALID, "runs_count: null result");
    if (n && !s) return fail(SMHIP_ERR_INVALID, "runs_count: null operand");
    const size_t esz = dtype_size(dtype);
    if (misaligned(s, esz) || misaligned(count_dev, sizeof(int64_t))) return fail(SMHIP_ERR_INVALID, "runs_count: a pointer is not aligned to its element");
    if (spans_overlap(Span{count_dev, sizeof(int64_t)}, Span{s, (size_t)n * esz})) return fail(SMHIP_ERR_INVALID, "runs_count: the result overlaps the operand");
    hipStream_t st;
    OpScope op_scope;  // undeclared spans (the pooled counts): ordered behind everything, recorded tiny operators flushed first
    if (int rc = op_scope.begin_barrier(&st)) return rc;
    if (n == 0) {
        SMHIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(int64_t), st));
        return SMHIP_OK;
    }
    RunArgs g{};
    g.s = s, g.n = n, g.count_dev = count_dev;
    return launch_runs(kCount, flags, dtype, g, st);
}

int smhip_runs(int flags, int dtype, const void *s, int64_t n, const int64_t *order_or_null, void *values_out, int64_t *index_out, int64_t *counts_out,
               int64_t *inverse_out, int64_t capacity, int64_t *count_dev_or_null) {
    if (int rc = runs_check("runs", flags, dtype, n)) return rc;
    if (capacity < 0) return fail(SMHIP_ERR_INVALID, "runs: capacity %lld: negative", (long long)capacity);
    if (!values_out && !index_out && !counts_out && !inverse_out) return fail(SMHIP_ERR_INVALID, "runs: all four results are null");
    if (n && !s) return fail(SMHIP_ERR_INVALID, "runs: null operand");
    const size_t esz = dtype_size(dtype), word = sizeof(int64_t);
    if (misaligned(s, esz) || misaligned(values_out, esz) || misaligned(order_or_null, word) || misaligned(index_out, word) || misaligned(counts_out, word) ||
        misaligned(inverse_out, word) || misaligned(count_dev_or_null, word))
        return fail(SMHIP_ERR_INVALID, "runs: a pointer is not aligned to its element");
    const size_t items = (size_t)std::min(capacity, n);  // there are at most n runs
    const Span spans[7] = {{values_out, items * esz}, {index_out, items * word}, {counts_out, items * word}, {inverse_out, (size_t)n * word},
                           {count_dev_or_null, word},  {s, (size_t)n * esz},     {order_or_null, (size_t)n * word}};
    const char *names[7] = {"values_out", "index_out", "counts_out", "inverse_out", "count_dev", "s", "order"};
    for (int a = 0; a < 5; ++a)      // every span that is written ...
        for (int b = a + 1; b < 7; ++b)  // ... against every other one
            if (spans_overlap(spans[a], spans[b])) return fail(SMHIP_ERR_INVALID, "runs: %s overlaps %s", names[a], names[b]);
    const bool firsts = items && (values_out || index_out || counts_out);
    if (n == 0 || (!firsts && !inverse_out)) {  // nothing to write but, perhaps, the count
        if (!count_dev_or_null) return SMHIP_OK;
        return smhip_runs_count(flags, dtype, s, n, count_dev_or_null);
    }
    hipStream_t st;
    OpScope op_scope;  // undeclared spans (the pooled counts and starts): ordered behind everything, recorded tiny operators flushed first
    if (int rc = op_scope.begin_barrier(&st)) return rc;
    RunArgs g{};
    g.s = s, g.n = n, g.order = order_or_null, g.inverse = inverse_out, g.capacity = capacity, g.count_dev = count_dev_or_null;
    if (firsts) g.values = values_out, g.index = index_out, g.counts = counts_out;
    return launch_runs(inverse_out ? kAll : kFirsts, flags, dtype, g, st);
}

int smhip_runs_plan(int flags, int dtype, int64_t n, int outputs, int *route, int *launches, int64_t *info3) {
    if (int rc = runs_check("runs_plan", flags, dtype, n)) return rc;
    if (outputs & ~kOutputs) return fail(SMHIP_ERR_INVALID, "runs_plan: unknown result bits 0x%x", outputs);
    const Plan p = make_plan(dtype, n, outputs);
    if (route) *route = p.route;
    if (launches) *launches = p.launches;
    if (info3) info3[0] = p.tiles, info3[1] = tile_elems(dtype), info3[2] = kOneGroupTiles * tile_elems(dtype);
    return SMHIP_OK;
}
