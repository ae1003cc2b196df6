// select.hip -- selection by condition: np.where (smhip_where), np.count_nonzero (smhip_select_count) and the compaction behind
// np.flatnonzero / np.nonzero / a[mask] (smhip_select).  numpy is the contract (smhip.h has it in full).
//
// A CONDITION is cmp(x, rhs) and is never written to memory: every kernel here evaluates it on the elements it has loaded.  The three
// ordered relations of a pair (less, equal, greater) are computed once and the comparison is a 4-bit set over {less, equal, greater,
// unordered} (Rel): EQ = {equal}, NE = {less, greater, unordered}, ... -- IEEE's and numpy's answers for NaN and the two zeros, exact
// for the integers, and no branch on `cmp` in any loop.  NONZERO is NE against the scalar 0.
//
//   where        one pass, one 16-byte vector per lane (VecTraits' element-aligned vectors, so operands that start off a 16-byte
//                boundary take the same kernel), the launch's streaming policy: unary.hip's dense kernel with
//                up to four read streams, in the pieces internal.h's piece_for names for the mix.  An operand given by the same pointer as an earlier one is not loaded again (wave-uniform
//                branches).  out may be an operand: a lane stores only the vector it has loaded itself.
//   compaction   TILES of kBlock lanes x kTileVecs vectors; lane l's u-th vector is vector u * kBlock + l of the tile, so a wave's load
//                is 1 KiB of consecutive bytes.  Row-major order inside a tile is therefore (u, wave, lane, element).
//                  launch 1  select_kernel<.., kNone>, kModeCount: the flags of a lane's 8 vectors in one 32-bit word, __ballot and
//                            __popcll per flag, the four wave totals through LDS, one int32 per tile
//                  launch 2  tile_scan_kernel: ONE workgroup, 16 counts per lane and pass, wave_scan in int64 and a carry: the exclusive
//                            prefix per tile, the total to *count_dev (smhip_select_count: the total alone)
//                  launch 3  select_kernel<.., What>, kModeEmit: the flags again, per u the lane counts through wave_scan, the
//                            kTileVecs x 4 wave totals through LDS; a lane's rank is the tile's offset + the totals before its (u, wave)
//                            + the lanes before it + the flags before it in its own vector.  It writes when rank < capacity.
//                No workgroup waits for another one.  Up to kOneGroupTiles tiles ONE workgroup does everything in one launch
//                (kModeOne): the same tile code in a loop with the carry in a register.
// An operand that is not dense row-major is copied dense first through Pooled (SMHIP_SELECT_COPY).  The tile kernels loop grid-stride
// under one capped grid (SMHIP_SELECT_GRID_CAP).  All index arithmetic is int64; a tile's count fits int32.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "internal.h"
#include "ops.hip.h"
#include "wave.hip.h"

namespace smhip {
namespace {

using namespace axis_plan;  // kBlock, GridCap, Pooled, row_major, ceil_div
using namespace dev;

constexpr int kTileVecs = 8;                        // 16-byte vectors a lane holds of a tile: a tile is 32 KiB of x
constexpr int kWaves = kBlock / 64;
constexpr int64_t kOneGroupTiles = 4;               // the one-workgroup route takes at most this many tiles
constexpr int kScanPerLane = 16;                    // tile counts a lane of the prefix kernel takes per pass
constexpr size_t kPieceVec = (size_t)1 << 27;       // where: vectors of a launch at most (a grid is counted in 32 bits of work-items)
constexpr int kNone = -1;                           // select_kernel's What for "count only"
constexpr int kValues4 = SMHIP_SELECT_VALUES, kValues8 = SMHIP_SELECT_VALUES + 8;
constexpr int kModeCount = 0, kModeEmit = 1, kModeOne = 2;

inline int64_t tile_elems(int dtype) { return (int64_t)kBlock * kTileVecs * vec_width(dtype); }

// ------------------------------------------------------------------------------------------------------ the condition
struct Rel { int lt, eq, gt, un; };  // does the comparison hold when x is less than / equal to / greater than rhs / unordered?
Rel rel_of(int cmp) {
    switch (cmp) {
        case SMHIP_CMP_EQ: return Rel{0, 1, 0, 0};
        case SMHIP_CMP_LT: return Rel{1, 0, 0, 0};
        case SMHIP_CMP_LE: return Rel{1, 1, 0, 0};
        case SMHIP_CMP_GT: return Rel{0, 0, 1, 0};
        case SMHIP_CMP_GE: return Rel{0, 1, 1, 0};
    }
    return Rel{1, 0, 1, 1};  // NE, and NONZERO against 0
}
template <typename T> __device__ __forceinline__ bool holds(Rel r, T x, T y) {
    const bool lt = x < y, eq = x == y, gt = x > y;
    return (lt && r.lt) || (eq && r.eq) || (gt && r.gt) || (!(lt || eq || gt) && r.un);
}
template <typename T> __device__ __forceinline__ T from_bits(uint64_t bits) {
    if constexpr (sizeof(T) == 4) return __builtin_bit_cast(T, (uint32_t)bits);
    else return __builtin_bit_cast(T, bits);
}
uint64_t scalar_bits(int dtype, const void *host) {
    uint64_t bits = 0;
    if (host) memcpy(&bits, host, dtype_size(dtype));  // little endian: a 4-byte scalar lands in the low word
    return bits;
}

// ------------------------------------------------------------------------------------------------------ where
struct WhereArgs {
    const void *x, *y, *a, *b;
    void *out;
    uint64_t rhs, sa, sb;  // the scalars' bits
    size_t n_vec;
    int tail, pol;
    int a_from, b_from;    // 0: its own load; 1: x's vector; 2: y's; 3 (b only): a's
    Rel rel;
};

template <typename T, bool HasY, bool HasA, bool HasB, bool NT>
__device__ __forceinline__ void where_vector(const WhereArgs &g, size_t i) {
    typedef typename VecTraits<T>::vec_t V;
    typedef typename VecTraits<T>::full_t F;
    constexpr int W = VecTraits<T>::width;
    const F vx = load_stream_as(T, reinterpret_cast<const V *>(g.x) + i, NT);
    F vy = vx, va = vx, vb = vx;
    if constexpr (HasY) vy = load_stream_as(T, reinterpret_cast<const V *>(g.y) + i, NT);
    if constexpr (HasA) {
        if (g.a_from == 0) va = load_stream_as(T, reinterpret_cast<const V *>(g.a) + i, NT);
        else if (g.a_from == 2) va = vy;
    }
    if constexpr (HasB) {
        if (g.b_from == 0) vb = load_stream_as(T, reinterpret_cast<const V *>(g.b) + i, NT);
        else if (g.b_from == 2) vb = vy;
        else if (g.b_from == 3) vb = va;
    }
    const T rhs = from_bits<T>(g.rhs), sa = from_bits<T>(g.sa), sb = from_bits<T>(g.sb);
    F r;
#pragma unroll
    for (int w = 0; w < W; ++w) r[w] = holds<T>(g.rel, vx[w], HasY ? vy[w] : rhs) ? (HasA ? va[w] : sa) : (HasB ? vb[w] : sb);
    store_stream_if(T, reinterpret_cast<V *>(g.out) + i, r, g.pol);
}

// (no __restrict__: out may BE an operand, each element read before it is written by the same lane)
template <typename T, bool HasY, bool HasA, bool HasB>
__global__ __launch_bounds__(kBlock) void where_kernel(WhereArgs g) {
    constexpr int W = VecTraits<T>::width;
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < g.n_vec) {
        if (g.pol & kLoadNt) where_vector<T, HasY, HasA, HasB, true>(g, i);
        else where_vector<T, HasY, HasA, HasB, false>(g, i);
    } else if (i == g.n_vec) {  // the n % W elements past the last whole vector: the first lane past the body
        const T *x = static_cast<const T *>(g.x), *y = static_cast<const T *>(g.y), *a = static_cast<const T *>(g.a), *b = static_cast<const T *>(g.b);
        T *out = static_cast<T *>(g.out);
        for (int k = 0; k < g.tail; ++k) {
            const size_t e = g.n_vec * W + k;
            const T ex = x[e], ey = HasY ? y[e] : from_bits<T>(g.rhs), ea = HasA ? a[e] : from_bits<T>(g.sa), eb = HasB ? b[e] : from_bits<T>(g.sb);
            out[e] = holds<T>(g.rel, ex, ey) ? ea : eb;
        }
    }
}

template <typename T, bool HasY, bool HasA, bool HasB> int run_where_kernel(WhereArgs g, size_t n, hipStream_t s) {
    constexpr int W = VecTraits<T>::width;
    const size_t n_vec = n / W;
    const int tail = (int)(n % W);
    // the plan knows no pointers, so an array operand counts as a stream whether or not it is x again; honours SMHIP_PIECE_LOG2VEC
    size_t piece = piece_for(n_vec, HasY || HasA || HasB ? 3 : 2);
    if (piece == 0 || piece > kPieceVec) piece = kPieceVec;
    const char *x = static_cast<const char *>(g.x), *y = static_cast<const char *>(g.y), *a = static_cast<const char *>(g.a), *b = static_cast<const char *>(g.b);
    char *out = static_cast<char *>(g.out);
    for (size_t v0 = 0;; v0 += piece) {
        const bool last = v0 + piece >= n_vec;
        const size_t nv = last ? n_vec - v0 : piece, off = v0 * 16;
        g.x = x + off, g.y = HasY ? y + off : nullptr, g.a = HasA ? a + off : nullptr, g.b = HasB ? b + off : nullptr, g.out = out + off;
        g.n_vec = nv, g.tail = last ? tail : 0;
        const size_t threads = nv + (last && tail ? 1 : 0);
        const size_t grid = (threads + kBlock - 1) / kBlock;  // <= 2^27 / 256 + 1
        if (grid) hipLaunchKernelGGL((where_kernel<T, HasY, HasA, HasB>), dim3((unsigned)grid), dim3(kBlock), 0, s, g);
        if (last) break;
    }
    SMHIP_LAUNCH_CHECK("where");
    return SMHIP_OK;
}

template <typename T> int run_where(const WhereArgs &g, size_t n, hipStream_t s) {
    const int form = (g.y ? 4 : 0) | (g.a ? 2 : 0) | (g.b ? 1 : 0);
    switch (form) {
        case 0: return run_where_kernel<T, false, false, false>(g, n, s);
        case 1: return run_where_kernel<T, false, false, true>(g, n, s);
        case 2: return run_where_kernel<T, false, true, false>(g, n, s);
        case 3: return run_where_kernel<T, false, true, true>(g, n, s);
        case 4: return run_where_kernel<T, true, false, false>(g, n, s);
        case 5: return run_where_kernel<T, true, false, true>(g, n, s);
        case 6: return run_where_kernel<T, true, true, false>(g, n, s);
    }
    return run_where_kernel<T, true, true, true>(g, n, s);
}

// ------------------------------------------------------------------------------------------------------ the compaction
struct SelectArgs {
    const void *x, *y, *src;
    void *out;
    int32_t *tile_counts;         // kModeCount writes, tile_scan_kernel reads
    const int64_t *tile_offsets;  // kModeEmit reads
    int64_t *count_dev;           // kModeOne writes the total (may be null)
    uint64_t rhs;
    int64_t n, n_vec, tiles, capacity;
    int tail, mode, nt, ndim;
    Rel rel;
    int64_t shape[SMHIP_MAX_NDIM];
};

template <typename S, int N> struct Packed { typedef S type __attribute__((ext_vector_type(N), aligned(sizeof(S)))); };

// The flags of this lane's kTileVecs vectors of tile t: bit u * W + w = the condition on element (first vector of the tile + u * kBlock
// + lane) * W + w.  A vector past the data has no flags; the n % W elements behind the last whole vector belong to the lane that
// would hold it and are read one by one.
template <typename T, bool HasY, bool NT> __device__ __forceinline__ uint32_t tile_flags(const SelectArgs &g, int64_t t) {
    typedef typename VecTraits<T>::vec_t V;
    typedef typename VecTraits<T>::full_t F;
    constexpr int W = VecTraits<T>::width;
    const V *xv = static_cast<const V *>(g.x), *yv = static_cast<const V *>(g.y);
    const T rhs = from_bits<T>(g.rhs);
    const int64_t v0 = t * ((int64_t)kBlock * kTileVecs) + threadIdx.x;
    F vx[kTileVecs], vy[kTileVecs];
#pragma unroll
    for (int u = 0; u < kTileVecs; ++u) {
        const int64_t v = v0 + (int64_t)u * kBlock;
        if (v < g.n_vec) {
            vx[u] = load_stream_as(T, xv + v, NT);
            if constexpr (HasY) vy[u] = load_stream_as(T, yv + v, NT);
        }
    }
    uint32_t bits = 0;
#pragma unroll
    for (int u = 0; u < kTileVecs; ++u) {
        const int64_t v = v0 + (int64_t)u * kBlock;
        if (v < g.n_vec) {
#pragma unroll
            for (int w = 0; w < W; ++w) bits |= (uint32_t)holds<T>(g.rel, vx[u][w], HasY ? vy[u][w] : rhs) << (u * W + w);
        } else if (v == g.n_vec) {
            const T *x = static_cast<const T *>(g.x), *y = static_cast<const T *>(g.y);
            for (int w = 0; w < g.tail; ++w) bits |= (uint32_t)holds<T>(g.rel, x[v * W + w], HasY ? y[v * W + w] : rhs) << (u * W + w);
        }
    }
    return bits;
}

// Item `rank` of the result for element e.
template <int What> __device__ __forceinline__ void emit_index(const SelectArgs &g, int64_t rank, int64_t e) {
    int64_t *out = static_cast<int64_t *>(g.out);
    if constexpr (What == SMHIP_SELECT_INDEX) out[rank] = e;
    else {
        for (int d = g.ndim - 1; d > 0; --d) {  // unravel, last axis first; an extent is never 0 here (there are elements)
            const int64_t q = e / g.shape[d];
            out[(int64_t)d * g.capacity + rank] = e - q * g.shape[d];
            e = q;
        }
        out[rank] = e;
    }
}

// What: kNone (count only), SMHIP_SELECT_INDEX, SMHIP_SELECT_COORDS, kValues4, kValues8.
template <typename T, bool HasY, int What, bool NT> __device__ __forceinline__ void select_body(const SelectArgs &g) {
    constexpr int W = VecTraits<T>::width;
    constexpr uint32_t kVecMask = (1u << W) - 1;
    __shared__ int totals[kTileVecs][kWaves];  // emit: the selected elements of (u, wave); count: [0][wave] alone
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool one = g.mode == kModeOne;
    int64_t carry = 0;  // kModeOne: the selected elements of the tiles before
    for (int64_t t = one ? 0 : blockIdx.x; t < g.tiles; t += one ? 1 : gridDim.x) {  // workgroup-uniform
        const uint32_t bits = tile_flags<T, HasY, NT>(g, t);
        if constexpr (What == kNone) {
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
            int before[kTileVecs];  // the selected elements of the lanes before this one in its wave, per vector
#pragma unroll
            for (int u = 0; u < kTileVecs; ++u) {
                const int c = __popc((bits >> (u * W)) & kVecMask);
                const int inc = wave_scan<int>(c, lane, 0, [](int p, int q) { return p + q; });
                before[u] = inc - c;
                if (lane == 63) totals[u][wave] = inc;
            }
            __syncthreads();
            int64_t base = one ? carry : g.tile_offsets[t];
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
                if (m) {
                    int64_t rank = base + mine + before[u];
                    const int64_t v = t * ((int64_t)kBlock * kTileVecs) + (int64_t)u * kBlock + tid, e0 = v * W;
                    if constexpr (What == kValues4 || What == kValues8) {
                        typedef typename std::conditional<What == kValues4, uint32_t, uint64_t>::type S;
                        const S *src = static_cast<const S *>(g.src);
                        S *out = static_cast<S *>(g.out);
                        if (v < g.n_vec) {  // the whole vector of src lies inside it
                            const typename Packed<S, W>::type sv = *reinterpret_cast<const typename Packed<S, W>::type *>(src + e0);
#pragma unroll
                            for (int w = 0; w < W; ++w)
                                if (m >> w & 1) {
                                    if (rank < g.capacity) out[rank] = sv[w];
                                    ++rank;
                                }
                        } else {
                            for (int w = 0; w < g.tail; ++w)
                                if (m >> w & 1) {
                                    if (rank < g.capacity) out[rank] = src[e0 + w];
                                    ++rank;
                                }
                        }
                    } else {
#pragma unroll
                        for (int w = 0; w < W; ++w)
                            if (m >> w & 1) {
                                if (rank < g.capacity) emit_index<What>(g, rank, e0 + w);
                                ++rank;
                            }
                    }
                }
            }
            carry += running;  // the tile's total
            __syncthreads();
        }
    }
    if (one && tid == 0 && g.count_dev) *g.count_dev = carry;
}

template <typename T, bool HasY, int What> __global__ __launch_bounds__(kBlock) void select_kernel(SelectArgs g) {
    if (g.nt) select_body<T, HasY, What, true>(g);
    else select_body<T, HasY, What, false>(g);
}

// offsets[i] = counts[0] + ... + counts[i - 1] (when offsets is given) and *total = their sum (when total is given): one workgroup,
// kScanPerLane counts per lane and pass, the carry in a register.  Exact in int64.
__global__ __launch_bounds__(kBlock) void tile_scan_kernel(const int32_t *__restrict__ counts, int64_t tiles, int64_t *__restrict__ offsets, int64_t *__restrict__ total) {
    __shared__ uint64_t wave_sum[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t carry = 0;
    for (int64_t base = 0; base < tiles; base += (int64_t)kBlock * kScanPerLane) {  // workgroup-uniform
        const int64_t i0 = base + (int64_t)tid * kScanPerLane;
        int32_t c[kScanPerLane];
        uint64_t mine = 0;
#pragma unroll
        for (int k = 0; k < kScanPerLane; ++k) {
            c[k] = i0 + k < tiles ? counts[i0 + k] : 0;
            mine += (uint64_t)c[k];
        }
        const uint64_t inc = wave_scan<uint64_t>(mine, lane, 0, [](uint64_t p, uint64_t q) { return p + q; });
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        uint64_t before = 0, all = 0;
#pragma unroll
        for (int k = 0; k < kWaves; ++k) {
            if (k == wave) before = all;
            all += wave_sum[k];
        }
        if (offsets) {
            uint64_t run = carry + before + inc - mine;
#pragma unroll
            for (int k = 0; k < kScanPerLane; ++k) {
                if (i0 + k < tiles) offsets[i0 + k] = (int64_t)run;
                run += (uint64_t)c[k];
            }
        }
        carry += all;
        __syncthreads();
    }
    if (tid == 0 && total) *total = (int64_t)carry;
}

// ------------------------------------------------------------------------------------------------------ the planner
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_SELECT_GRID_CAP")); return g; }  // the cap of the tile launches, read once

struct Plan {
    int route = SMHIP_SELECT_ROUTE_NONE, copies = 0;
    bool copy_x = false, copy_y = false, copy_a = false, copy_b = false;
    int64_t n = 0, tiles = 0, pieces = 0;
    int kernel_launches = 0;
    int launches() const { return route == SMHIP_SELECT_ROUTE_NONE ? 0 : copies + kernel_launches; }
    int code() const { return route | (copies && route != SMHIP_SELECT_ROUTE_NONE ? SMHIP_SELECT_COPY : 0); }
};

// a_strides: src for VALUES, a for WHERE; null strides: no such array (a scalar, or unused).
void make_plan(int what, int dtype, const int64_t *shape, int ndim, const int64_t *sx, const int64_t *sy, const int64_t *sa, const int64_t *sb, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    int64_t n = 1;
    for (int d = 0; d < ndim; ++d) n *= shape[d];  // the checks have bounded it
    p.n = n;
    if (n == 0) return;
    const bool where = what == SMHIP_SELECT_WHERE;
    p.copy_x = !row_major(shape, sx, ndim);
    p.copy_y = sy && !row_major(shape, sy, ndim);
    p.copy_a = sa && (where || what == SMHIP_SELECT_VALUES) && !row_major(shape, sa, ndim);
    p.copy_b = sb && where && !row_major(shape, sb, ndim);
    p.copies = (int)p.copy_x + (int)p.copy_y + (int)p.copy_a + (int)p.copy_b;
    const int W = vec_width(dtype);
    if (where) {
        p.route = SMHIP_SELECT_ROUTE_DENSE;
        const int64_t n_vec = n / W;
        size_t piece = piece_for((size_t)n_vec, sy || sa || sb ? 3 : 2);
        if (piece == 0 || piece > kPieceVec) piece = kPieceVec;
        p.pieces = std::max<int64_t>(1, ceil_div(n_vec, (int64_t)piece));
        p.kernel_launches = (int)std::min<int64_t>(p.pieces, 1 << 30);
        return;
    }
    p.tiles = ceil_div(ceil_div(n, W), (int64_t)kBlock * kTileVecs);
    if (p.tiles <= kOneGroupTiles) p.route = SMHIP_SELECT_ROUTE_ONE, p.kernel_launches = 1;
    else p.route = SMHIP_SELECT_ROUTE_TILES, p.kernel_launches = what == SMHIP_SELECT_COUNT ? 2 : 3;
}

// ------------------------------------------------------------------------------------------------------ launching
template <typename T, bool HasY> int launch_select_kernel(int what, int src_bytes, const SelectArgs &g, unsigned blocks, hipStream_t s) {
    const dim3 grid(blocks), block(kBlock);
    if (what == kNone) hipLaunchKernelGGL((select_kernel<T, HasY, kNone>), grid, block, 0, s, g);
    else if (what == SMHIP_SELECT_INDEX) hipLaunchKernelGGL((select_kernel<T, HasY, SMHIP_SELECT_INDEX>), grid, block, 0, s, g);
    else if (what == SMHIP_SELECT_COORDS) hipLaunchKernelGGL((select_kernel<T, HasY, SMHIP_SELECT_COORDS>), grid, block, 0, s, g);
    else if (src_bytes == 4) hipLaunchKernelGGL((select_kernel<T, HasY, kValues4>), grid, block, 0, s, g);
    else hipLaunchKernelGGL((select_kernel<T, HasY, kValues8>), grid, block, 0, s, g);
    SMHIP_LAUNCH_CHECK("select");
    return SMHIP_OK;
}

template <typename T> int run_select(int what, int src_bytes, const Plan &p, SelectArgs g, hipStream_t s) {
    auto launch = [&](int w, int mode, unsigned blocks) {
        g.mode = mode;
        return g.y ? launch_select_kernel<T, true>(w, src_bytes, g, blocks, s) : launch_select_kernel<T, false>(w, src_bytes, g, blocks, s);
    };
    if (p.route == SMHIP_SELECT_ROUTE_ONE) return launch(what, kModeOne, 1);
    Pooled pool;
    void *raw;
    const size_t count_bytes = ((size_t)p.tiles * sizeof(int32_t) + 15) & ~(size_t)15;
    if (int rc = pool.take(count_bytes + (what == kNone ? 0 : (size_t)p.tiles * sizeof(int64_t)), &raw)) return rc;
    g.tile_counts = static_cast<int32_t *>(raw);
    int64_t *offsets = what == kNone ? nullptr : reinterpret_cast<int64_t *>(static_cast<char *>(raw) + count_bytes);
    g.tile_offsets = offsets;
    const unsigned blocks = grid_cap().capped(p.tiles);
    if (int rc = launch(kNone, kModeCount, blocks)) return rc;
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(kBlock), 0, s, g.tile_counts, p.tiles, offsets, g.count_dev);
    SMHIP_LAUNCH_CHECK("select prefix");
    if (what == kNone) return SMHIP_OK;
    return launch(what, kModeEmit, blocks);
}

// Everything that can be said about a condition's shape without a device or a pointer; *n_out = the element count.
int check_view(const char *who, const char *name, const int64_t *shape, const int64_t *strides, int ndim, bool empty) {
    if (!strides) return fail(SMHIP_ERR_INVALID, "%s: null strides of %s", who, name);
    const int64_t limit = (int64_t)1 << 59;
    int64_t span = 0;
    for (int d = 0; d < ndim; ++d) {
        if (strides[d] < 0) return fail(SMHIP_ERR_INVALID, "%s: negative stride of %s at dim %d", who, name, d);
        int64_t t;
        if (!empty && (__builtin_mul_overflow(shape[d] - 1, strides[d], &t) || __builtin_add_overflow(span, t, &span) || span >= limit))
            return fail(SMHIP_ERR_INVALID, "%s: the span of %s exceeds 2^59 elements", who, name);
    }
    return SMHIP_OK;
}

int select_check(const char *who, int cmp, int dtype, const int64_t *shape, int ndim, const int64_t *sx, const int64_t *sy, int64_t *n_out) {
    if (cmp < SMHIP_CMP_NONZERO || cmp > SMHIP_CMP_GE) return fail(SMHIP_ERR_INVALID, "%s: bad comparison %d", who, cmp);
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (!shape) return fail(SMHIP_ERR_INVALID, "%s: null shape", who);
    const int64_t limit = (int64_t)1 << 59;
    int64_t n = 1;
    bool empty = false;
    for (int d = 0; d < ndim; ++d) {
        if (shape[d] < 0) return fail(SMHIP_ERR_INVALID, "%s: negative extent at dim %d", who, d);
        empty |= shape[d] == 0;
    }
    for (int d = 0; d < ndim && !empty; ++d)
        if (__builtin_mul_overflow(n, shape[d], &n) || n >= limit) return fail(SMHIP_ERR_INVALID, "%s: the shape exceeds 2^59 elements", who);
    if (int rc = check_view(who, "x", shape, sx, ndim, empty)) return rc;
    if (sy)
        if (int rc = check_view(who, "y", shape, sy, ndim, empty)) return rc;
    *n_out = empty ? 0 : n;
    return SMHIP_OK;
}

// The condition's operands dense: x (and y) copied through the pools where the plan says so.
int dense_condition(const Plan &p, Pooled *px, Pooled *py, int dtype, const void **x, const int64_t *sx, const void **y, const int64_t *sy, const int64_t *shape, int ndim,
                    hipStream_t s) {
    if (p.copy_x)
        if (int rc = px->dense_copy(dtype, *x, shape, sx, ndim, s, x)) return rc;
    if (p.copy_y)
        if (int rc = py->dense_copy(dtype, *y, shape, sy, ndim, s, y)) return rc;
    return SMHIP_OK;
}

int launch_select(int what, int cmp, int dtype, const void *x, const int64_t *sx, const void *y, const int64_t *sy, const void *rhs_host, const int64_t *shape, int ndim,
                  const void *src, const int64_t *ssrc, int src_bytes, void *out, int64_t capacity, int64_t *count_dev, hipStream_t s) {
    Plan p;
    make_plan(what == kNone ? SMHIP_SELECT_COUNT : what, dtype, shape, ndim, sx, y ? sy : nullptr, ssrc, nullptr, &p);
    Pooled px, py, ps;
    if (int rc = dense_condition(p, &px, &py, dtype, &x, sx, &y, sy, shape, ndim, s)) return rc;
    if (p.copy_a)
        if (int rc = ps.dense_copy(src_bytes == 4 ? SMHIP_I32 : SMHIP_I64, src, shape, ssrc, ndim, s, &src)) return rc;
    SelectArgs g{};
    g.x = x, g.y = y, g.src = src, g.out = out, g.count_dev = count_dev;
    g.rhs = cmp == SMHIP_CMP_NONZERO ? 0 : scalar_bits(dtype, y ? nullptr : rhs_host);
    g.rel = rel_of(cmp);
    const int W = vec_width(dtype);
    g.n = p.n, g.n_vec = p.n / W, g.tail = (int)(p.n % W), g.tiles = p.tiles, g.capacity = capacity;
    g.nt = stream_reads((size_t)p.n * dtype_size(dtype) * (y ? 2 : 1));
    g.ndim = ndim;
    for (int d = 0; d < ndim; ++d) g.shape[d] = shape[d];
    switch (dtype) {
        case SMHIP_F32: return run_select<float>(what, src_bytes, p, g, s);
        case SMHIP_F64: return run_select<double>(what, src_bytes, p, g, s);
        case SMHIP_I32: return run_select<int32_t>(what, src_bytes, p, g, s);
        case SMHIP_I64: return run_select<int64_t>(what, src_bytes, p, g, s);
    }
    return fail(SMHIP_ERR_INVALID, "select: bad dtype %d", dtype);
}

}  // namespace

// The prefix kernel for the other compaction built on tile counts (unique.hip).
int launch_tile_scan(const int32_t *counts, int64_t tiles, int64_t *offsets, int64_t *total, hipStream_t s) {
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(axis_plan::kBlock), 0, s, counts, tiles, offsets, total);
    SMHIP_LAUNCH_CHECK("tile prefix");
    return SMHIP_OK;
}

}  // namespace smhip

using namespace smhip;

int smhip_where(int cmp, int dtype, const void *x, const int64_t *x_strides, const void *y, const int64_t *y_strides, const void *rhs_scalar_host, const void *a,
                const int64_t *a_strides, const void *a_scalar_host, const void *b, const int64_t *b_strides, const void *b_scalar_host, const int64_t *shape, int ndim,
                void *out) {
    if (cmp == SMHIP_CMP_NONZERO) y = nullptr;  // NONZERO ignores rhs
    int64_t n;
    if (int rc = select_check("where", cmp, dtype, shape, ndim, x_strides, y ? y_strides : nullptr, &n)) return rc;
    if (y && !y_strides) return fail(SMHIP_ERR_INVALID, "where: null strides of y");
    if (a)
        if (int rc = check_view("where", "a", shape, a_strides, ndim, n == 0)) return rc;
    if (b)
        if (int rc = check_view("where", "b", shape, b_strides, ndim, n == 0)) return rc;
    if (n == 0) return SMHIP_OK;
    if (!x || !out) return fail(SMHIP_ERR_INVALID, "where: null operand or result");
    if ((!y && cmp != SMHIP_CMP_NONZERO && !rhs_scalar_host) || (!a && !a_scalar_host) || (!b && !b_scalar_host))
        return fail(SMHIP_ERR_INVALID, "where: an operand is a scalar but its host pointer is null");
    const size_t esz = dtype_size(dtype);
    if (misaligned(x, esz) || misaligned(y, esz) || misaligned(a, esz) || misaligned(b, esz) || misaligned(out, esz))
        return fail(SMHIP_ERR_INVALID, "where: a pointer is not aligned to its element");
    // In place is the one overlap a where can take: `out` IS an operand, and that operand is dense row-major over `shape` (a lane
    // reads element i of every operand before it writes element i).
    const void *ptr[4] = {x, y, a, b};
    const int64_t *st[4] = {x_strides, y_strides, a_strides, b_strides};
    const char *name[4] = {"x", "y", "a", "b"};
    const Span so{out, (size_t)n * esz};
    Span reads[4];
    for (int k = 0; k < 4; ++k) {
        reads[k] = ptr[k] ? Span{ptr[k], span_bytes(shape, st[k], ndim, esz)} : Span{nullptr, 0};
        if (!ptr[k] || !spans_overlap(reads[k], so)) continue;
        if (!(ptr[k] == out && row_major(shape, st[k], ndim)))
            return fail(SMHIP_ERR_INVALID, "where: the result overlaps operand %s (only out == an operand that is dense over the result's shape is allowed)", name[k]);
    }
    Plan p;
    make_plan(SMHIP_SELECT_WHERE, dtype, shape, ndim, x_strides, y ? y_strides : nullptr, a ? a_strides : nullptr, b ? b_strides : nullptr, &p);
    hipStream_t s;
    OpScope op_scope;  // recorded tiny operators are flushed first; with a pooled copy the call orders itself behind everything
    if (int rc = op_scope.begin(reads, 4, so, &s, p.copies > 0)) return rc;
    Pooled px, py, pa, pb;
    if (int rc = dense_condition(p, &px, &py, dtype, &x, x_strides, &y, y_strides, shape, ndim, s)) return rc;
    if (p.copy_a)
        if (int rc = pa.dense_copy(dtype, a, shape, a_strides, ndim, s, &a)) return rc;
    if (p.copy_b)
        if (int rc = pb.dense_copy(dtype, b, shape, b_strides, ndim, s, &b)) return rc;
    WhereArgs g{};
    g.x = x, g.y = y, g.a = a, g.b = b, g.out = out;
    g.rhs = cmp == SMHIP_CMP_NONZERO ? 0 : scalar_bits(dtype, y ? nullptr : rhs_scalar_host);
    g.sa = scalar_bits(dtype, a ? nullptr : a_scalar_host), g.sb = scalar_bits(dtype, b ? nullptr : b_scalar_host);
    g.rel = rel_of(cmp);
    // an operand that IS an earlier one (the same pointer, both dense) is not loaded twice
    if (a && a == x) g.a_from = 1;
    else if (a && a == y) g.a_from = 2;
    if (b && b == x) g.b_from = 1;
    else if (b && b == y) g.b_from = 2;
    else if (b && b == a) g.b_from = 3;
    Span streams[4];
    size_t n_streams = 0, bytes_read = 0;
    streams[n_streams++] = Span{x, (size_t)n * esz};
    if (y) streams[n_streams++] = Span{y, (size_t)n * esz};
    if (a && g.a_from == 0) streams[n_streams++] = Span{a, (size_t)n * esz};
    if (b && g.b_from == 0) streams[n_streams++] = Span{b, (size_t)n * esz};
    bytes_read = n_streams * (size_t)n * esz;
    g.pol = refine_policy(stream_policy(bytes_read, (size_t)n * esz), streams, n_streams, so);
    switch (dtype) {
        case SMHIP_F32: return run_where<float>(g, (size_t)n, s);
        case SMHIP_F64: return run_where<double>(g, (size_t)n, s);
        case SMHIP_I32: return run_where<int32_t>(g, (size_t)n, s);
        case SMHIP_I64: return run_where<int64_t>(g, (size_t)n, s);
    }
    return fail(SMHIP_ERR_INVALID, "where: bad dtype %d", dtype);
}

int smhip_select_count(int cmp, int dtype, const void *x, const int64_t *x_strides, const void *y, const int64_t *y_strides, const void *rhs_scalar_host,
                       const int64_t *shape, int ndim, int64_t *count_dev) {
    if (cmp == SMHIP_CMP_NONZERO) y = nullptr;  // NONZERO ignores rhs
    int64_t n;
    if (int rc = select_check("select_count", cmp, dtype, shape, ndim, x_strides, y ? y_strides : nullptr, &n)) return rc;
    if (y && !y_strides) return fail(SMHIP_ERR_INVALID, "select_count: null strides of y");
    if (!count_dev) return fail(SMHIP_ERR_INVALID, "select_count: null result");
    if (n && !x) return fail(SMHIP_ERR_INVALID, "select_count: null operand");
    if (n && !y && cmp != SMHIP_CMP_NONZERO && !rhs_scalar_host) return fail(SMHIP_ERR_INVALID, "select_count: the right-hand side is a scalar but its host pointer is null");
    const size_t esz = dtype_size(dtype);
    if (misaligned(x, esz) || misaligned(y, esz) || misaligned(count_dev, sizeof(int64_t))) return fail(SMHIP_ERR_INVALID, "select_count: a pointer is not aligned to its element");
    const Span sx{x, n ? span_bytes(shape, x_strides, ndim, esz) : 0}, sy{y, n && y ? span_bytes(shape, y_strides, ndim, esz) : 0}, sc{count_dev, sizeof(int64_t)};
    if (spans_overlap(sc, sx) || spans_overlap(sc, sy)) return fail(SMHIP_ERR_INVALID, "select_count: the result overlaps an operand");
    hipStream_t s;
    OpScope op_scope;  // undeclared spans (the pooled counts, a dense copy): ordered behind everything, recorded tiny operators flushed first
    if (int rc = op_scope.begin_barrier(&s)) return rc;
    if (n == 0) {
        SMHIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(int64_t), s));
        return SMHIP_OK;
    }
    return launch_select(kNone, cmp, dtype, x, x_strides, y, y_strides, rhs_scalar_host, shape, ndim, nullptr, nullptr, 0, nullptr, 0, count_dev, s);
}

int smhip_select(int what, int cmp, int dtype, const void *x, const int64_t *x_strides, const void *y, const int64_t *y_strides, const void *rhs_scalar_host,
                 const int64_t *shape, int ndim, const void *src, const int64_t *src_strides, int src_elem_bytes, void *out, int64_t capacity, int64_t *count_dev) {
    if (what != SMHIP_SELECT_INDEX && what != SMHIP_SELECT_COORDS && what != SMHIP_SELECT_VALUES) return fail(SMHIP_ERR_INVALID, "select: bad operation %d", what);
    if (cmp == SMHIP_CMP_NONZERO) y = nullptr;  // NONZERO ignores rhs
    int64_t n;
    if (int rc = select_check("select", cmp, dtype, shape, ndim, x_strides, y ? y_strides : nullptr, &n)) return rc;
    if (y && !y_strides) return fail(SMHIP_ERR_INVALID, "select: null strides of y");
    const bool values = what == SMHIP_SELECT_VALUES;
    if (values) {
        if (src_elem_bytes != 4 && src_elem_bytes != 8) return fail(SMHIP_ERR_INVALID, "select: src elements of %d bytes (4 or 8)", src_elem_bytes);
        if (int rc = check_view("select", "src", shape, src_strides, ndim, n == 0)) return rc;
    }
    const int64_t limit = (int64_t)1 << 59;
    if (capacity < 0) return fail(SMHIP_ERR_INVALID, "select: capacity %lld: negative", (long long)capacity);
    if (capacity >= limit) return fail(SMHIP_ERR_INVALID, "select: a capacity of %lld items exceeds 2^59", (long long)capacity);
    const size_t esz = dtype_size(dtype), item = values ? (size_t)src_elem_bytes : sizeof(int64_t);
    if (misaligned(count_dev, sizeof(int64_t))) return fail(SMHIP_ERR_INVALID, "select: a pointer is not aligned to its element");
    if (n && capacity) {
        if (!x || !out || (values && !src)) return fail(SMHIP_ERR_INVALID, "select: null operand, source or result");
    } else if (n && !x && count_dev) return fail(SMHIP_ERR_INVALID, "select: null operand");
    if (n && !y && cmp != SMHIP_CMP_NONZERO && !rhs_scalar_host) return fail(SMHIP_ERR_INVALID, "select: the right-hand side is a scalar but its host pointer is null");
    if (misaligned(x, esz) || misaligned(y, esz) || (values && misaligned(src, item)) || misaligned(out, item))
        return fail(SMHIP_ERR_INVALID, "select: a pointer is not aligned to its element");
    const Span sx{x, n ? span_bytes(shape, x_strides, ndim, esz) : 0}, sy{y, n && y ? span_bytes(shape, y_strides, ndim, esz) : 0},
        ss{src, n && values && src ? span_bytes(shape, src_strides, ndim, item) : 0},
        so{out, (size_t)capacity * item * (what == SMHIP_SELECT_COORDS ? (size_t)ndim : 1)}, sc{count_dev, count_dev ? sizeof(int64_t) : 0};
    if (spans_overlap(so, sx) || spans_overlap(so, sy) || spans_overlap(so, ss)) return fail(SMHIP_ERR_INVALID, "select: the result overlaps an operand");
    // with nothing to select from the result may be null while its capacity is not: its span is then still taken from address 0
    const bool in_null_result = !out && sc.bytes && reinterpret_cast<uintptr_t>(count_dev) < so.bytes;
    if (spans_overlap(sc, sx) || spans_overlap(sc, sy) || spans_overlap(sc, ss) || spans_overlap(sc, so) || in_null_result)
        return fail(SMHIP_ERR_INVALID, "select: count_dev overlaps an operand or the result");
    if ((n == 0 || capacity == 0) && !count_dev) return SMHIP_OK;
    hipStream_t s;
    OpScope op_scope;  // undeclared spans (the pooled counts, dense copies): ordered behind everything, recorded tiny operators flushed first
    if (int rc = op_scope.begin_barrier(&s)) return rc;
    if (n == 0) {
        SMHIP_TRY(hipMemsetAsync(count_dev, 0, sizeof(int64_t), s));
        return SMHIP_OK;
    }
    if (capacity == 0) return launch_select(kNone, cmp, dtype, x, x_strides, y, y_strides, rhs_scalar_host, shape, ndim, nullptr, nullptr, 0, nullptr, 0, count_dev, s);
    return launch_select(what, cmp, dtype, x, x_strides, y, y_strides, rhs_scalar_host, shape, ndim, values ? src : nullptr, values ? src_strides : nullptr,
                         values ? src_elem_bytes : 0, out, capacity, count_dev, s);
}

int smhip_select_plan(int what, int cmp, int dtype, const int64_t *shape, int ndim, const int64_t *x_strides, const int64_t *y_strides, const int64_t *a_strides,
                      const int64_t *b_strides, int *route, int *launches, int64_t *info4) {
    if (what < SMHIP_SELECT_INDEX || what > SMHIP_SELECT_WHERE) return fail(SMHIP_ERR_INVALID, "select_plan: bad operation %d", what);
    if (cmp == SMHIP_CMP_NONZERO) y_strides = nullptr;  // NONZERO ignores rhs
    int64_t n;
    if (int rc = select_check("select_plan", cmp, dtype, shape, ndim, x_strides, y_strides, &n)) return rc;
    if (a_strides)
        if (int rc = check_view("select_plan", "a", shape, a_strides, ndim, n == 0)) return rc;
    if (b_strides)
        if (int rc = check_view("select_plan", "b", shape, b_strides, ndim, n == 0)) return rc;
    Plan p;
    make_plan(what, dtype, shape, ndim, x_strides, y_strides, a_strides, b_strides, &p);
    if (route) *route = p.code();
    if (launches) *launches = p.launches();
    if (info4) info4[0] = p.tiles, info4[1] = tile_elems(dtype), info4[2] = kOneGroupTiles * tile_elems(dtype), info4[3] = p.copies;
    return SMHIP_OK;
}
