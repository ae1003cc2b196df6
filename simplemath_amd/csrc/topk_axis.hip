// topk_axis.hip -- the first k of the order along one axis without sorting the line: the k largest (or smallest) elements and /
// or their positions (smhip_topk_axis).
//
// The contract is sort's (smhip.h, "sort / argsort"): the result is, bit for bit, the first k entries along the axis of
// smhip_sort_axis in the same order -- (element, position) pairs under `before()` of sort_axis.hip, repeated below.  The pairs of
// a line are totally ordered, so the k first ones are ONE set and have ONE order: whatever selects them, the bytes are the same.
//
// Selection (select_line), on a line of at most L elements held in LDS:
//   key      a monotone unsigned key computed on the fly from the element's bits (key_of): -0 maps to +0, every NaN to the one key
//            above +inf, the whole key is complemented for DESCENDING.  It is never converted back (and only the ranking kernel
//            below keeps it, in LDS, for the length of a line): what is written are the operand's own bits.  Equal keys are exactly the ties of `before()`, and those are broken by the SLOT
//            of the element in the LDS line.  At the first level the slot is the position in the tile.  At later levels of TILED
//            it is the candidate's slot: a tile's candidates are written in sorted order and tiles are visited in rising order, so
//            equal elements stand in rising original position, and the slot orders them as the carried position would.
//   radix    the composite (key, slot) is unique in the line, so its k-th smallest -- the pivot -- is found by a radix select with
//            8-bit digits from the top: 4 or 8 passes over the key, 2 over the slot (L <= 2^16).  A pass counts the elements that
//            match the digits fixed so far into a 256-bin histogram in LDS and one wave narrows it by a lane-parallel scan of the
//            bins.  The passes stop as soon as the bin that holds the pivot is taken whole (with distinct values after 2 or 3).
//   gather   every element whose composite is <= the pivot -- exactly k -- takes a slot of the selection buffer from a counter.
//   order    a bitonic network with `before()` over the k selected pairs (for k = 5: 8 slots), with their ORIGINAL positions.
// The ONLY atomics are integer counts in LDS: the histogram's bins and the gather's counter.  Both the counts and the SET gathered
// are independent of the order in which the lanes arrive; the order of the gathered pairs is not, and the network that follows
// removes it.  So the bytes are the same on every run, stream and grid.
//
// Planner (host only; smhip_topk_plan reports it), with axis_plan.h's merging.  The kernels take ROWS: O lines of R contiguous
// elements, results as dense rows [O][k].  Staging in and out is decided exactly as sort's planner decides it.
//   ROW      R <= L, k <= kmax: ONE launch, one read of the operand.  Lines of at most 128 elements are not selected from but
//            RANKED, a wave per line (topk_rank_kernel: each pair counts the pairs before it; the time does not depend on k).
//            Longer lines of at most L / 4 elements with at most kmax / 4 to select take a WAVE each for the selection above (four
//            lines per workgroup, no workgroup barrier), the others a workgroup.
//   TILED    R > L, k <= kmax: level 1 selects the first min(k, tile) pairs of every tile of L elements into pooled candidates
//            (element bits, 32-bit position); the same selection runs on each line's candidates until one tile is left, and that
//            level writes the results.  k <= L / 4, so every level shrinks a line at least fourfold.
//   SORT     k > kmax, or 2k > R on a line of 129 .. L elements (a selection that keeps most of the line costs what sorting it
//            costs): the existing sort into pooled arrays, then a strided copy of the first k along the axis per output.
// Every kernel loops over its tasks under a capped grid (SMHIP_TOPK_GRID_CAP).
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "internal.h"
#include "wave.hip.h"

namespace smhip {
namespace {

using namespace axis_plan;  // kBlock, Canon, GridCap, Pooled and the planner's rules

constexpr int kLine = 4096;          // L: elements of a line in LDS (DESIGN.md "topk" has the residency this gives)
constexpr int kMaxK = kLine / 4;     // kmax: the most pairs a selection takes
constexpr int kWaves = kBlock / 64;  // a wave per line: the workgroup's line and selection buffers are cut in four
constexpr int kWaveLine = kLine / kWaves, kWaveK = kMaxK / kWaves;
constexpr int kRankLine = SMHIP_TOPK_RANKED;  // the longest line that is ranked by all pairs: two pairs a lane
constexpr int64_t kMaxAxis = (int64_t)1 << 31;  // positions travel as 32 bits
static_assert(kLine <= 1 << 16, "the slot takes two 8-bit digits");
static_assert(kRankLine == 128 && kRankLine <= kMaxK, "topk_rank_kernel<T, 1 or 2>: 64 or 128 keys a wave, any k up to the line");

// sort_axis.hip's pair order: does pair (av, ar) come before pair (bv, br)?
template <typename T> __device__ __forceinline__ bool before(bool desc, T av, uint32_t ar, T bv, uint32_t br) {
    const bool first = ar < br, lt = desc ? bv < av : av < bv;
    if constexpr (std::is_floating_point<T>::value) {
        const bool an = av != av, bn = bv != bv;
        return (desc ? an && !bn : bn && !an) || lt || ((av == bv || (an && bn)) && first);
    } else {
        return lt || (av == bv && first);
    }
}

template <typename T> using KeyOf = typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type;

// The monotone key: a is before b in the order (positions aside) exactly when key_of(a) < key_of(b); ties have equal keys.
template <typename T> __device__ __forceinline__ KeyOf<T> key_of(bool desc, T x) {
    using K = KeyOf<T>;
    constexpr K top = (K)1 << (sizeof(K) * 8 - 1);
    K u = __builtin_bit_cast(K, x);
    if constexpr (std::is_floating_point<T>::value) {
        if (x != x) u = ~(K)0;  // one key for every NaN, above +inf's (no number has it)
        else {
            if (u == top) u = 0;  // -0 == +0
            u = (u & top) ? ~u : (u | top);
        }
    } else {
        u ^= top;
    }
    return desc ? (K)~u : u;
}

// What a radix select has fixed so far (in LDS, one per group of lanes that share a line).
template <typename K> struct Pivot {
    K key;          // the digits of the pivot's key found so far, zeros below
    uint32_t slot;  // ... and of its slot
    uint32_t need;  // the pivot's rank (from 1) among the elements that match those digits
    uint32_t done;  // the bin that holds the pivot is taken whole: key / slot are filled up with ones below
};

// A group's rendezvous: the workgroup's barrier, or, for a wave on a line of its own, the order of its own LDS operations.
template <bool WAVE> __device__ __forceinline__ void group_sync() {
    if constexpr (WAVE) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else {
        __syncthreads();
    }
}

// Selects the first k (1 <= k <= len, k <= the capacity of sv / sr) pairs of the line v[0 .. len) into sv / sr, in order.  r holds the
// carried positions (CARRY) or the line starts at position p0.  `lane` is the lane's number in its group of G = 64 (WAVE) or kBlock
// lanes; every lane of the group makes the call, and leaves it with the results visible.
template <typename T, bool CARRY, bool WAVE>
__device__ void select_line(const T *v, const uint32_t *r, uint32_t p0, int len, int k, bool desc, T *sv, uint32_t *sr, uint32_t *hist,
                            Pivot<KeyOf<T>> *pv, int lane) {
    using K = KeyOf<T>;
    constexpr int G = WAVE ? 64 : kBlock, kKeyPasses = (int)sizeof(K);
    for (int b = lane; b < 256; b += G) hist[b] = 0;
    if (lane == 0) pv->key = 0, pv->slot = 0, pv->need = (uint32_t)k, pv->done = 0;
    group_sync<WAVE>();
    for (int pass = 0; pass < kKeyPasses + 2; ++pass) {
        const K pkey = pv->key;
        const uint32_t pslot = pv->slot;
        if (pv->done) break;  // group-uniform: read behind a rendezvous
        const bool on_key = pass < kKeyPasses;
        const int shift = on_key ? (kKeyPasses - 1 - pass) * 8 : (kKeyPasses + 1 - pass) * 8;
        for (int s = lane; s < len; s += G) {
            const K key = key_of(desc, v[s]);
            bool match;
            uint32_t digit;
            if (on_key) match = pass == 0 || ((key ^ pkey) >> shift >> 8) == 0, digit = (uint32_t)(key >> shift) & 255u;
            else match = key == pkey && (((uint32_t)s ^ pslot) >> shift >> 8) == 0, digit = ((uint32_t)s >> shift) & 255u;
            if (match) atomicAdd(&hist[digit], 1u);  // an integer count: the same whatever the order of arrival
        }
        group_sync<WAVE>();
        if (lane < 64) {  // one whole wave: lane l owns bins 4l .. 4l + 3, and clears them for the next pass
            uint32_t c[4], sum = 0;
            for (int j = 0; j < 4; ++j) c[j] = hist[4 * lane + j], hist[4 * lane + j] = 0, sum += c[j];
            uint32_t running = dev::wave_scan(sum, lane, 0u, [](uint32_t x, uint32_t y) { return x + y; }) - sum;
            const uint32_t need = pv->need;
            for (int j = 0; j < 4; ++j) {
                if (running < need && need <= running + c[j]) {  // true for exactly one bin of the 256: 1 <= need <= the matches
                    const uint32_t d = (uint32_t)(4 * lane + j), left = need - running;
                    const bool whole = left == c[j];
                    K key = pkey;
                    uint32_t slot = pslot;
                    if (on_key) {
                        key |= (K)d << shift;
                        if (whole) key |= ((K)1 << shift) - 1, slot = ~0u;
                    } else {
                        slot |= d << shift;
                        if (whole) slot |= (1u << shift) - 1;
                    }
                    pv->key = key, pv->slot = slot, pv->need = left, pv->done = whole;
                }
                running += c[j];
            }
        }
        group_sync<WAVE>();
    }
    {
        const K pkey = pv->key;
        const uint32_t pslot = pv->slot;
        for (int s = lane; s < len; s += G) {
            const T x = v[s];
            const K key = key_of(desc, x);
            if (key < pkey || (key == pkey && (uint32_t)s <= pslot)) {
                const uint32_t at = atomicAdd(&hist[0], 1u);  // an integer count; WHICH slot a pair takes is settled by the network below
                if (at < (uint32_t)k) {                          // (always: exactly k composites are <= the pivot)
                    sv[at] = x;
                    if constexpr (CARRY) sr[at] = r[s];
                    else sr[at] = p0 + (uint32_t)s;
                }
            }
        }
    }
    group_sync<WAVE>();
    // sort_axis.hip's network on N = 2^ceil(log2 k) slots: every merge stage opens with the mirrored step and the earlier pair goes
    // to the lower slot, so slots >= k are never touched
    int N = 1;
    while (N < k) N <<= 1;
    for (int kk = 2; kk <= N; kk <<= 1)
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int c = lane; c < N >> 1; c += G) {
                const int low = c & (j - 1), i = ((c - low) << 1) | low;
                const int p = j == kk >> 1 ? i ^ (kk - 1) : i | j;
                if (p < k) {
                    const T vi = sv[i], vp = sv[p];
                    const uint32_t ri = sr[i], rp = sr[p];
                    if (before(desc, vp, rp, vi, ri)) sv[i] = vp, sr[i] = rp, sv[p] = vi, sr[p] = ri;
                }
            }
            group_sync<WAVE>();
        }
}

// ---- one level of the selection.  Line `line` of the input is n elements at in_v + line*so (CARRY: with their positions at
// in_r + line*so), cut into `tiles` tiles of kLine.  A task is a tile (a whole line when tiles == 1; WAVE: a line per wave).  The first
// min(k, tile length) pairs of a tile go to the candidates (out_v, out_r), line `line` of them out_n long and tile t's at t*k, or, when
// out_r is null (tiles == 1), to the results val / idx (either may be null) as rows of k.
template <typename T, bool CARRY, bool WAVE>
__global__ __launch_bounds__(kBlock) void topk_level_kernel(const T *__restrict__ in_v, const uint32_t *__restrict__ in_r, int64_t lines, int64_t so, int64_t n,
                                                            int64_t tiles, int k, int desc_i, T *__restrict__ out_v, uint32_t *__restrict__ out_r, int64_t out_n,
                                                            T *__restrict__ val, int64_t *__restrict__ idx) {
    static_assert(!(CARRY && WAVE), "a wave per line: first-level lines only");
    __shared__ T v_all[kLine];
    __shared__ uint32_t r_all[CARRY ? kLine : 1];
    __shared__ T sv_all[kMaxK];
    __shared__ uint32_t sr_all[kMaxK];
    __shared__ uint32_t hist_all[WAVE ? kWaves : 1][256];
    __shared__ Pivot<KeyOf<T>> pv_all[WAVE ? kWaves : 1];
    constexpr int G = WAVE ? 64 : kBlock;
    const bool desc = desc_i != 0;
    const int g = WAVE ? (int)(threadIdx.x >> 6) : 0, lane = WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    T *v = v_all + g * kWaveLine, *sv = sv_all + g * kWaveK;  // (g = 0 for a workgroup's line: the whole buffers)
    uint32_t *r = r_all, *sr = sr_all + g * kWaveK;
    const int64_t tasks = lines * tiles;
    const int64_t first = WAVE ? (int64_t)blockIdx.x * kWaves + g : (int64_t)blockIdx.x, step = WAVE ? (int64_t)gridDim.x * kWaves : (int64_t)gridDim.x;
    for (int64_t task = first; task < tasks; task += step) {  // group-uniform
        const int64_t line = task / tiles, tile = task - line * tiles, p0 = tile * kLine;
        const int len = (int)std::min<int64_t>(kLine, n - p0), kk = std::min(k, len);
        const int64_t from = line * so + p0;
        for (int s = lane; s < len; s += G) {
            v[s] = in_v[from + s];
            if constexpr (CARRY) r[s] = in_r[from + s];
        }
        // (select_line opens with a rendezvous behind the loads; no lane reads sv / sr of the task before once it is past that one)
        select_line<T, CARRY, WAVE>(v, r, (uint32_t)p0, len, kk, desc, sv, sr, hist_all[g], &pv_all[g], lane);
        if (out_r) {
            const int64_t to = line * out_n + tile * k;
            for (int s = lane; s < kk; s += G) out_v[to + s] = sv[s], out_r[to + s] = sr[s];
        } else {
            const int64_t to = line * k;
            for (int s = lane; s < kk; s += G) {
                if (val) val[to + s] = sv[s];
                if (idx) idx[to + s] = (int64_t)sr[s];
            }
        }
    }
}

// ---- lines of at most kRankLine elements: a wave per line and no selection at all.  The keys go to LDS once; every lane counts the
// pairs that come before its own (at most E = 2 of them) by reading every key of the line -- one LDS address for the whole wave, a
// broadcast -- and that count IS the pair's place in the order, so the lanes whose count is below k write their pair straight to the
// results.  R * E comparisons per lane whatever k is; no atomics, no network.
template <typename T, int E>
__global__ __launch_bounds__(kBlock) void topk_rank_kernel(const T *__restrict__ in, int64_t lines, int64_t so, int R, int k, int desc_i, T *__restrict__ val,
                                                           int64_t *__restrict__ idx) {
    using K = KeyOf<T>;
    __shared__ K keys_all[kWaves][64 * E];
    const bool desc = desc_i != 0;
    const int g = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    K *keys = keys_all[g];
    for (int64_t line = (int64_t)blockIdx.x * kWaves + g; line < lines; line += (int64_t)gridDim.x * kWaves) {  // wave-uniform
        T x[E];
        K key[E];
        uint32_t rank[E];
        for (int e = 0; e < E; ++e) {
            const int s = lane + 64 * e;
            x[e] = T(), key[e] = 0, rank[e] = 0;
            if (s < R) x[e] = in[line * so + s], key[e] = key_of(desc, x[e]), keys[s] = key[e];
        }
        group_sync<true>();
        for (int j = 0; j < R; ++j) {
            const K kj = keys[j];
            for (int e = 0; e < E; ++e) rank[e] += (kj < key[e] || (kj == key[e] && j < lane + 64 * e)) ? 1u : 0u;  // equal keys: the lower position first
        }
        for (int e = 0; e < E; ++e) {
            const int s = lane + 64 * e;
            if (s < R && rank[e] < (uint32_t)k) {
                if (val) val[line * k + rank[e]] = x[e];
                if (idx) idx[line * k + rank[e]] = (int64_t)s;
            }
        }
        group_sync<true>();  // the next line overwrites the keys
    }
}

// ------------------------------------------------------------------------------------------------------ the planner
struct Plan {
    int route = SMHIP_TOPK_ROUTE_NONE;
    bool stage_in = false, stage_out = false, wave = false, rank = false;
    int64_t O = 1, R = 1, I = 1;  // ori3
    int64_t lines = 0, so = 0;    // the rows the kernels take: line o at in + o*so
    int64_t total = 0, k = 0;
    int levels = 0;                       // selection launches (ROW: 1)
    int sort_launches = 0;                // SORT: what the sort itself launches
    int64_t stage_a[SMHIP_MAX_NDIM];      // where element [idx] of the operand stands in the staged rows [lines][R], as strides over `shape`
    int64_t stage_res[SMHIP_MAX_NDIM];    // where element [idx] of a result stands in the rows [lines][k], as strides over the result's shape
    int launches() const {  // of a call that asks for both outputs
        if (route == SMHIP_TOPK_ROUTE_NONE) return 0;
        if (route == SMHIP_TOPK_ROUTE_COPYONLY) return 2;
        if (route == SMHIP_TOPK_ROUTE_SORT) return sort_launches + 2;
        return (stage_in ? 1 : 0) + levels + (stage_out ? 2 : 0);
    }
    int code() const {
        return route | (route == SMHIP_TOPK_ROUTE_ROW && R > kLine ? SMHIP_TOPK_TILED : 0) | (stage_in || stage_out ? SMHIP_TOPK_COPY : 0);
    }
};

// The length of a line's candidates after a level over n elements: every tile but the last gives k, the last min(k, its length).
int64_t candidates(int64_t n, int64_t k) {
    const int64_t tiles = ceil_div(n, kLine);
    return (tiles - 1) * k + std::min(k, n - (tiles - 1) * kLine);
}

void make_plan(int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, int64_t k, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    int64_t before_n = 1, after_n = 1;
    bool zero_stride = false;
    for (int d = 0; d < ndim; ++d) {
        if (d < axis) before_n *= shape[d];
        if (d > axis) after_n *= shape[d];
        if (shape[d] > 1 && strides[d] == 0) zero_stride = true;
    }
    p.R = shape[axis], p.O = before_n, p.I = after_n, p.total = before_n * after_n * p.R, p.k = k;
    if (p.total == 0 || k == 0) return;
    if (p.R == 1) {
        p.route = SMHIP_TOPK_ROUTE_COPYONLY;
        return;
    }
    // SORT: k beyond a selection's reach, or a selection that would keep more than half of a line it holds whole (it then costs what
    // the sort costs: profiles/topk_handover_sweep.txt); ranked lines cost the same whatever k is.  The sort stages for itself.
    if (k > kMaxK || (p.R > kRankLine && p.R <= kLine && 2 * k > p.R)) {
        int route = 0;
        p.route = SMHIP_TOPK_ROUTE_SORT;
        sort_axis_plan(dtype, shape, strides, ndim, axis, &route, &p.sort_launches, nullptr, nullptr);
        p.stage_in = p.stage_out = (route & SMHIP_SORT_COPY) != 0;
        return;
    }
    p.route = SMHIP_TOPK_ROUTE_ROW;
    int64_t in_lines[SMHIP_MAX_NDIM];  // the line of element [idx], as strides over `shape` (0 along the axis)
    Ax ax[SMHIP_MAX_NDIM];
    const int n = merge_axes(shape, strides, ndim, 1u << axis, false, ax);
    Canon c;
    if (!zero_stride && canonical(ax, n, &c) == kWalkRow) {  // read in place: every kept stride is a multiple of so
        p.O = c.O, p.I = 1, p.lines = c.O, p.so = c.so;
        for (int d = 0; d < ndim; ++d) in_lines[d] = shape[d] == 1 || d == axis ? 0 : strides[d] / c.so;
    } else {  // staged: the kept axes in index order, then the axis
        p.stage_in = true, p.lines = before_n * after_n, p.so = p.R;
        int64_t acc = 1;
        for (int d = ndim - 1; d >= 0; --d) {
            if (d == axis) in_lines[d] = 0;
            else in_lines[d] = shape[d] == 1 ? 0 : acc, acc *= shape[d];
        }
    }
    int64_t res_shape[SMHIP_MAX_NDIM];
    for (int d = 0; d < ndim; ++d) {
        res_shape[d] = d == axis ? k : shape[d];
        p.stage_a[d] = d == axis ? 1 : in_lines[d] * p.R;
        p.stage_res[d] = d == axis ? 1 : in_lines[d] * k;
    }
    p.stage_out = !row_major(res_shape, p.stage_res, ndim);
    int N = 1;
    while (N < k) N <<= 1;
    p.rank = p.R <= kRankLine, p.wave = p.R <= kWaveLine && N <= kWaveK;
    p.levels = 1;
    for (int64_t len = p.R; len > kLine; len = candidates(len, k)) ++p.levels;
}

// ------------------------------------------------------------------------------------------------------ launching
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_TOPK_GRID_CAP")); return g; }  // the cap of every launch here, read once

template <typename T>
int run_rows(const Plan &p, int desc, const T *in, T *val, int64_t *idx, hipStream_t s) {
    const int k = (int)p.k;
    if (p.levels == 1) {
        if (p.rank) {
            const dim3 grid(grid_cap().blocks_for(p.lines));
            if (p.R <= 64) hipLaunchKernelGGL((topk_rank_kernel<T, 1>), grid, dim3(kBlock), 0, s, in, p.lines, p.so, (int)p.R, k, desc, val, idx);
            else hipLaunchKernelGGL((topk_rank_kernel<T, 2>), grid, dim3(kBlock), 0, s, in, p.lines, p.so, (int)p.R, k, desc, val, idx);
        } else if (p.wave) {
            hipLaunchKernelGGL((topk_level_kernel<T, false, true>), dim3(grid_cap().blocks_for(p.lines)), dim3(kBlock), 0, s, in, (const uint32_t *)nullptr, p.lines,
                               p.so, p.R, (int64_t)1, k, desc, (T *)nullptr, (uint32_t *)nullptr, (int64_t)0, val, idx);
        } else {
            hipLaunchKernelGGL((topk_level_kernel<T, false, false>), dim3(grid_cap().capped(p.lines)), dim3(kBlock), 0, s, in, (const uint32_t *)nullptr, p.lines, p.so,
                               p.R, (int64_t)1, k, desc, (T *)nullptr, (uint32_t *)nullptr, (int64_t)0, val, idx);
        }
        SMHIP_LAUNCH_CHECK("topk_axis");
        return SMHIP_OK;
    }
    // two buffers of candidates, each the values then the positions; the first level's output is the longest
    Pooled pool;
    void *raw;
    const int64_t n1 = candidates(p.R, p.k);
    const size_t cap = (size_t)p.lines * (size_t)n1, half = cap * (sizeof(T) + sizeof(uint32_t));
    if (int rc = pool.take(2 * half, &raw)) return rc;
    T *bv[2] = {static_cast<T *>(raw), reinterpret_cast<T *>(static_cast<char *>(raw) + half)};
    uint32_t *br[2] = {reinterpret_cast<uint32_t *>(bv[0] + cap), reinterpret_cast<uint32_t *>(bv[1] + cap)};
    int64_t n = p.R;
    for (int level = 0; level < p.levels; ++level) {
        const int to = level & 1, from = to ^ 1;
        const bool last = level + 1 == p.levels;
        const int64_t tiles = ceil_div(n, kLine), out_n = candidates(n, p.k);
        const dim3 grid(grid_cap().capped(p.lines * tiles));
        if (level == 0) {
            hipLaunchKernelGGL((topk_level_kernel<T, false, false>), grid, dim3(kBlock), 0, s, in, (const uint32_t *)nullptr, p.lines, p.so, n, tiles, k, desc, bv[to],
                               br[to], out_n, (T *)nullptr, (int64_t *)nullptr);
        } else {
            hipLaunchKernelGGL((topk_level_kernel<T, true, false>), grid, dim3(kBlock), 0, s, (const T *)bv[from], (const uint32_t *)br[from], p.lines, n, n, tiles, k,
                               desc, last ? (T *)nullptr : bv[to], last ? (uint32_t *)nullptr : br[to], out_n, last ? val : (T *)nullptr,
                               last ? idx : (int64_t *)nullptr);
        }
        SMHIP_LAUNCH_CHECK("topk_axis level");
        n = out_n;
    }
    return SMHIP_OK;
}

template <typename T>
int run_plan(const Plan &p, int desc, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, void *values_out,
             int64_t *index_out, hipStream_t s) {
    int64_t res_shape[SMHIP_MAX_NDIM], dense[SMHIP_MAX_NDIM];
    for (int d = 0; d < ndim; ++d) res_shape[d] = d == axis ? p.k : shape[d];
    dense_strides(res_shape, ndim, dense);
    const size_t results = (size_t)p.lines * (size_t)p.k;
    Pooled in_pool, val_pool, idx_pool;
    const T *in = static_cast<const T *>(a);
    if (p.stage_in) {
        void *buf;
        if (int rc = in_pool.take((size_t)p.total * sizeof(T), &buf)) return rc;
        if (int rc = launch_copy_strided(dtype, a, strides, buf, p.stage_a, shape, ndim, s)) return rc;
        in = static_cast<const T *>(buf);
    }
    T *val = static_cast<T *>(values_out);
    int64_t *idx = index_out;
    if (p.stage_out) {
        void *buf;
        if (values_out) {
            if (int rc = val_pool.take(results * sizeof(T), &buf)) return rc;
            val = static_cast<T *>(buf);
        }
        if (index_out) {
            if (int rc = idx_pool.take(results * sizeof(int64_t), &buf)) return rc;
            idx = static_cast<int64_t *>(buf);
        }
    }
    if (int rc = run_rows<T>(p, desc, in, val, idx, s)) return rc;
    if (p.stage_out) {
        if (values_out)
            if (int rc = launch_copy_strided(dtype, val, p.stage_res, values_out, dense, res_shape, ndim, s)) return rc;
        if (index_out)
            if (int rc = launch_copy_strided(SMHIP_I64, idx, p.stage_res, index_out, dense, res_shape, ndim, s)) return rc;
    }
    return SMHIP_OK;
}

// SORT: the whole order into pooled arrays of the operand's shape, then the first k along the axis of each.
int run_sort(const Plan &p, int order, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, void *values_out,
             int64_t *index_out, hipStream_t s) {
    int64_t res_shape[SMHIP_MAX_NDIM], dense[SMHIP_MAX_NDIM], sorted[SMHIP_MAX_NDIM];
    for (int d = 0; d < ndim; ++d) res_shape[d] = d == axis ? p.k : shape[d];
    dense_strides(res_shape, ndim, dense);
    dense_strides(shape, ndim, sorted);
    Pooled val_pool, idx_pool;
    void *val = nullptr, *idx = nullptr;
    if (values_out)
        if (int rc = val_pool.take((size_t)p.total * dtype_size(dtype), &val)) return rc;
    if (index_out)
        if (int rc = idx_pool.take((size_t)p.total * sizeof(int64_t), &idx)) return rc;
    if (int rc = launch_sort_axis(order, dtype, a, shape, strides, ndim, axis, val, static_cast<int64_t *>(idx), s)) return rc;
    if (values_out)
        if (int rc = launch_copy_strided(dtype, val, sorted, values_out, dense, res_shape, ndim, s)) return rc;
    if (index_out)
        if (int rc = launch_copy_strided(SMHIP_I64, idx, sorted, index_out, dense, res_shape, ndim, s)) return rc;
    return SMHIP_OK;
}

int launch_topk_axis(int order, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, int64_t k, void *values_out,
                     int64_t *index_out, hipStream_t s) {
    Plan pl;
    make_plan(dtype, shape, strides, ndim, axis, k, &pl);
    if (pl.route == SMHIP_TOPK_ROUTE_NONE) return SMHIP_OK;
    if (pl.route == SMHIP_TOPK_ROUTE_COPYONLY) {
        int64_t dense[SMHIP_MAX_NDIM];
        dense_strides(shape, ndim, dense);
        if (values_out)
            if (int rc = launch_copy_strided(dtype, a, strides, values_out, dense, shape, ndim, s)) return rc;
        const int64_t zero = 0;
        return index_out ? launch_fill(SMHIP_I64, index_out, &zero, (size_t)pl.total, s) : SMHIP_OK;
    }
    if (pl.route == SMHIP_TOPK_ROUTE_SORT) return run_sort(pl, order, dtype, a, shape, strides, ndim, axis, values_out, index_out, s);
    const int desc = order == SMHIP_SORT_DESCENDING;
    switch (dtype) {
        case SMHIP_F32: return run_plan<float>(pl, desc, dtype, a, shape, strides, ndim, axis, values_out, index_out, s);
        case SMHIP_F64: return run_plan<double>(pl, desc, dtype, a, shape, strides, ndim, axis, values_out, index_out, s);
        case SMHIP_I32: return run_plan<int32_t>(pl, desc, dtype, a, shape, strides, ndim, axis, values_out, index_out, s);
        case SMHIP_I64: return run_plan<int64_t>(pl, desc, dtype, a, shape, strides, ndim, axis, values_out, index_out, s);
    }
    return fail(SMHIP_ERR_INVALID, "topk_axis: bad dtype %d", dtype);
}

// Validation: everything that can be said without a device or a pointer (sort's checks, then k).
int topk_axis_check(const char *who, int order, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, int64_t k) {
    if (order != SMHIP_SORT_ASCENDING && order != SMHIP_SORT_DESCENDING) return fail(SMHIP_ERR_INVALID, "%s: bad order %d", who, order);
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (int rc = check_axis(who, axis, ndim)) return rc;
    if (int rc = check_extents(who, shape, strides, ndim)) return rc;
    if (shape[axis] >= kMaxAxis) return fail(SMHIP_ERR_UNSUPPORTED, "%s: an axis of %lld elements (positions are 32 bits wide: below 2^31)", who, (long long)shape[axis]);
    if (k < 0 || k > shape[axis]) return fail(SMHIP_ERR_INVALID, "%s: k %lld outside 0..%lld", who, (long long)k, (long long)shape[axis]);
    return SMHIP_OK;
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_topk_axis(int order, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, int64_t k, void *values_out,
                    int64_t *index_out) {
    if (int rc = topk_axis_check("topk_axis", order, dtype, shape, strides, ndim, axis, k)) return rc;
    if (element_count(shape, ndim) == 0 || k == 0) return SMHIP_OK;
    if (!a) return fail(SMHIP_ERR_INVALID, "topk_axis: null operand");
    if (!values_out && !index_out) return fail(SMHIP_ERR_INVALID, "topk_axis: neither values_out nor index_out is given");
    const size_t esz = dtype_size(dtype), n = (size_t)(element_count(shape, ndim) / shape[axis] * k);
    const Span sa{a, span_bytes(shape, strides, ndim, esz)}, sv{values_out, values_out ? n * esz : 0}, si{index_out, index_out ? n * sizeof(int64_t) : 0};
    // no in-place form: the results are shorter than the lines they come from
    if (spans_overlap(sv, sa)) return fail(SMHIP_ERR_INVALID, "topk_axis: values_out overlaps the operand");
    if (spans_overlap(si, sa) || spans_overlap(si, sv)) return fail(SMHIP_ERR_INVALID, "topk_axis: index_out overlaps the operand or values_out");
    SMHIP_ACQUIRE(s);  // undeclared spans (pooled staging, the candidates): ordered behind everything, recorded tiny operators flushed first
    return launch_topk_axis(order, dtype, a, shape, strides, ndim, axis, k, values_out, index_out, s);
}

int smhip_topk_plan(int order, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, int64_t k, int *route, int *launches,
                    int64_t *ori3, int64_t *info3) {
    if (int rc = topk_axis_check("topk_plan", order, dtype, shape, strides, ndim, axis, k)) return rc;
    Plan pl;
    make_plan(dtype, shape, strides, ndim, axis, k, &pl);
    if (route) *route = pl.code();
    if (launches) *launches = pl.launches();
    if (ori3) ori3[0] = pl.O, ori3[1] = pl.R, ori3[2] = pl.I;
    if (info3) info3[0] = kLine, info3[1] = kMaxK, info3[2] = pl.levels;
    return SMHIP_OK;
}
