// quantile_axis.hip -- np.quantile / np.percentile / np.median along one axis without sorting the line (smhip_quantile_axis), f32
// and f64.
//
// The contract is smhip.h's ("quantile"); the arithmetic -- the key, (j, g) from (R, q, method), the interpolation -- is sm_quantile.h.
// A probability needs the element of rank j of the line, and for an interpolated one the element of rank j + 1: no positions, no
// gather, no network.  A rank is found by a radix select over the monotone key alone (select_rank): 8-bit digits from the top, a
// pass counting the elements that agree with the digits fixed so far into a 256-bin histogram, one wave narrowing it by a
// lane-parallel scan of the bins.  The passes stop when the bin that holds the rank holds ONE element.  The value is then taken from
// an element whose key agrees with the fixed digits, read as canonical() -- all such elements are that one element, or (after the
// last pass) elements of equal key, which canonical() makes equal bits: whichever lane stores, the bytes are the same.
//
// Planner (host only; smhip_quantile_plan reports it).  The kernels take ROWS: O lines of R contiguous elements, results dense
// [Q][O]; staging in and out is decided as sort's planner decides it (topk_axis.hip does the same).
//   ROW       R <= L, Q <= 16: ONE launch, one read of the operand.  The line goes to LDS once; a NaN met during the load settles the
//             line; each probability's lo is one selection, and its hi a second one unless the last pass showed that rank j + 1 has
//             the same key (then hi = lo).  A wave per line up to L / 4 elements (four lines a workgroup, no workgroup barrier), a
//             workgroup otherwise.  The ranks and g of every q travel in the kernel arguments.
//   STREAM    R > L, Q <= 16: the digit passes run over the line in HBM.  Every rank wanted (at most 32: lo and hi of 16) is a SLOT
//             with a state in a pooled table: the key digits fixed so far, the rank among the elements that agree with them, and how
//             many those are.  A pass has two launches: stream_count_kernel -- a workgroup counts the next digit of its tile's
//             agreeing elements into one LDS histogram per slot and adds the non-empty bins to the line's table (integer atomics) --
//             and stream_narrow_kernel, a wave per slot, which fixes the digit and clears the table.  A slot whose agreeing elements
//             are at most L is finished with streaming: later passes skip it, and a workgroup all of whose line's slots are finished
//             reads nothing.  stream_compact_kernel then gathers each such slot's agreeing elements into a pooled buffer (a counter
//             per slot; the order of arrival does not matter, only the set, and the data fix that), and stream_finish_kernel selects
//             from them in LDS.  A slot that never shrank to L -- a line of equal elements -- has every key digit fixed after the
//             last pass: the compaction sweep stores one agreeing element's canonical value instead.  No workgroup waits on another.
//             The host queues the same launches whatever the data are: nothing is read back.
//   SORT      Q > 16; more than 2 distinct ranks wanted of a wave's line (R <= L / 4) or more than 8 of a workgroup's (measured:
//             profiles/quantile_handover_sweep.txt); or a STREAM whose compaction buffers would exceed kStreamPoolBytes: the existing sort into a pooled array, then
//             pick_kernel reads s[j], s[j + 1] and interpolates, 16 probabilities a launch.  The sort puts NaNs last, so s[R - 1]
//             tells whether the line holds one.
//   COPYONLY  R = 1: the kept elements copied dense, then pick_kernel.
// Every kernel loops over its tasks under a capped grid (SMHIP_QUANTILE_GRID_CAP).  The only atomics are integer counts.
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "abi_args.h"
#include "axis_plan.h"
#include "internal.h"
#include "sm_quantile.h"
#include "wave.hip.h"

namespace smhip {
namespace {

using namespace axis_plan;  // kBlock, Canon, GridCap, Pooled and the planner's rules
using smquantile::KeyOf;

constexpr int kLine = 4096;          // L: elements of a line in LDS
constexpr int kMaxQ = 16;            // probabilities a selection serves
constexpr int kMaxSlots = 2 * kMaxQ; // STREAM: ranks followed through the passes
constexpr int kWaves = kBlock / 64;  // a wave per line: the workgroup's line buffer is cut in four
constexpr int kWaveLine = kLine / kWaves;
constexpr int kTile = 4 * kLine;     // STREAM: elements of a line a workgroup counts per task
constexpr int64_t kMaxAxis = (int64_t)1 << 31;  // ranks travel as 32 bits
constexpr size_t kStreamPoolBytes = (size_t)256 << 20;  // STREAM: the most its compaction buffers may take
// The most ranks (lo and hi of every probability, equal ones counted once) a line held in LDS is selected for before the sort is the
// cheaper way (profiles/quantile_handover_sweep.txt): a wave's line, a workgroup's line.  STREAM serves all 32.
constexpr int kWaveRanks = 2, kLineRanks = 8;

// The probabilities of one launch (a kernel argument): lo = s[lo[i]]; hi = s[hi[i]], consulted only when g[i] != 0.
struct QArgs {
    int n;
    uint32_t lo[kMaxQ], hi[kMaxQ];
    double g[kMaxQ];
};
// STREAM: the distinct ranks as slots, and each probability's two slots.
struct SArgs {
    int n, slots;
    uint32_t rank[kMaxSlots];
    uint8_t lo[kMaxQ], hi[kMaxQ];
    double g[kMaxQ];
};

// What a radix select has fixed so far (ROW: in LDS, one per group of lanes that share a line; STREAM: pooled, one per line and slot).
template <typename K> struct Sel {
    K key;            // the digits found so far, zeros below
    uint32_t need;    // the rank (from 1) among the elements that agree with those digits
    uint32_t count;   // how many those are
    uint32_t passes;  // digits fixed
    uint32_t done;    // ROW: count == 1, the element is known
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

// One wave (lane = 0 .. 63) narrows a 256-bin histogram: the bin that holds rank `need` (from 1; 1 <= need <= the sum of the bins), the
// rank inside it and its count go to *bin / *left / *count in the ONE lane that owns the bin, which returns true.  Clears the bins.
__device__ __forceinline__ bool narrow_bins(uint32_t *hist, uint32_t need, int lane, uint32_t *bin, uint32_t *left, uint32_t *count) {
    uint32_t c[4], sum = 0;
    for (int j = 0; j < 4; ++j) c[j] = hist[4 * lane + j], hist[4 * lane + j] = 0, sum += c[j];
    uint32_t running = dev::wave_scan(sum, lane, 0u, [](uint32_t x, uint32_t y) { return x + y; }) - sum;
    bool mine = false;
    for (int j = 0; j < 4; ++j) {
        if (running < need && need <= running + c[j]) mine = true, *bin = (uint32_t)(4 * lane + j), *left = need - running, *count = c[j];
        running += c[j];
    }
    return mine;
}

// The element of rank `rank` (from 0, < len) of the line v[0 .. len) in LDS, read as canonical(): left in *res, visible to every lane of
// the group on return, with *pv as the last pass left it (done, or every digit fixed: `count` elements of that key, the rank the
// `need`-th of them).  `lane` is the lane's number in its group of G = 64 (WAVE) or kBlock lanes; every lane of the group makes the
// call.  hist: 256 zeroed bins, left zeroed.
template <typename T, bool WAVE>
__device__ void select_rank(const T *v, int len, uint32_t rank, uint32_t *hist, Sel<KeyOf<T>> *pv, T *res, int lane) {
    using K = KeyOf<T>;
    constexpr int G = WAVE ? 64 : kBlock, kPasses = (int)sizeof(K);
    if (lane == 0) pv->key = 0, pv->need = rank + 1, pv->count = (uint32_t)len, pv->passes = 0, pv->done = 0;
    group_sync<WAVE>();
    for (int pass = 0; pass < kPasses; ++pass) {
        const K pkey = pv->key;
        if (pv->done) break;  // group-uniform: read behind a rendezvous
        for (int s = lane; s < len; s += G) {
            const K key = smquantile::key_of(v[s]);
            if (smquantile::agrees(key, pkey, pass)) atomicAdd(&hist[smquantile::digit(key, pass)], 1u);  // an integer count
        }
        group_sync<WAVE>();
        if (lane < 64) {
            uint32_t bin = 0, left = 0, count = 0;
            if (narrow_bins(hist, pv->need, lane, &bin, &left, &count))
                pv->key = pkey | ((K)bin << smquantile::shift_of<K>(pass)), pv->need = left, pv->count = count, pv->passes = (uint32_t)pass + 1, pv->done = count == 1;
        }
        group_sync<WAVE>();
    }
    const K pkey = pv->key;
    const int passes = (int)pv->passes;
    for (int s = lane; s < len; s += G) {
        const T x = v[s];
        if (smquantile::agrees(smquantile::key_of(x), pkey, passes)) *res = smquantile::canonical(x);  // every writer stores the same bits
    }
    group_sync<WAVE>();
}

// ---- ROW: line `line` is R <= kLine elements at in + line*so; out[i*lines + line] = the quantile of probability i.
template <typename T, bool WAVE>
__global__ __launch_bounds__(kBlock) void quantile_row_kernel(const T *__restrict__ in, int64_t lines, int64_t so, int R, QArgs qa, T *__restrict__ out) {
    using K = KeyOf<T>;
    __shared__ T v_all[kLine];
    __shared__ uint32_t hist_all[WAVE ? kWaves : 1][256];
    __shared__ Sel<K> pv_all[WAVE ? kWaves : 1];
    __shared__ T res_all[WAVE ? kWaves : 1];
    __shared__ uint32_t nan_all[WAVE ? kWaves : 1];
    constexpr int G = WAVE ? 64 : kBlock;
    const int g = WAVE ? (int)(threadIdx.x >> 6) : 0, lane = WAVE ? (int)(threadIdx.x & 63) : (int)threadIdx.x;
    T *v = v_all + g * kWaveLine;  // (g = 0 for a workgroup's line: the whole buffer)
    uint32_t *hist = hist_all[g];
    for (int b = lane; b < 256; b += G) hist[b] = 0;
    const int64_t first = WAVE ? (int64_t)blockIdx.x * kWaves + g : (int64_t)blockIdx.x, step = WAVE ? (int64_t)gridDim.x * kWaves : (int64_t)gridDim.x;
    for (int64_t line = first; line < lines; line += step) {  // group-uniform
        if (lane == 0) nan_all[g] = 0;
        group_sync<WAVE>();
        for (int s = lane; s < R; s += G) {
            const T x = in[line * so + s];
            v[s] = x;
            if (x != x) nan_all[g] = 1;  // every writer stores the same value
        }
        group_sync<WAVE>();
        const bool nan = nan_all[g] != 0;  // group-uniform
        for (int i = 0; i < qa.n; ++i) {
            T lo = smquantile::quiet_nan<T>(), hi = lo;
            if (!nan) {
                select_rank<T, WAVE>(v, R, qa.lo[i], hist, &pv_all[g], &res_all[g], lane);
                lo = hi = res_all[g];
                // after the last pass the bin holds the elements of lo's key: rank j + 1 is one of them when lo is not the last of them
                const bool same = !pv_all[g].done && pv_all[g].need < pv_all[g].count;
                group_sync<WAVE>();  // res and pv are read before the next selection writes them
                if (qa.g[i] != 0.0 && !same) {
                    select_rank<T, WAVE>(v, R, qa.hi[i], hist, &pv_all[g], &res_all[g], lane);
                    hi = res_all[g];
                    group_sync<WAVE>();
                }
            }
            if (lane == 0) out[(int64_t)i * lines + line] = nan ? lo : smquantile::finish<T>(lo, hi, qa.g[i]);
        }
        group_sync<WAVE>();  // the next line overwrites v and the flag
    }
}

// ---- STREAM.  Pooled per call: Sel st[lines][slots], uint32 table[lines][slots][256], uint32 fill[lines][slots] (the compaction
// counters), uint32 nan[lines], T vals[lines][slots], T comp[lines][slots][kLine].
template <typename T>
__global__ __launch_bounds__(kBlock) void stream_init_kernel(int64_t lines, int64_t R, SArgs sa, Sel<KeyOf<T>> *st, uint32_t *table, uint32_t *fill, uint32_t *nan) {
    const int64_t slots = lines * sa.slots, bins = slots * 256;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < bins; t += (int64_t)gridDim.x * kBlock) {
        table[t] = 0;
        if (t < slots) {
            Sel<KeyOf<T>> z;
            z.key = 0, z.need = sa.rank[t % sa.slots] + 1, z.count = (uint32_t)std::min<int64_t>(R, 0xffffffffll), z.passes = 0, z.done = 0;
            st[t] = z, fill[t] = 0;
        }
        if (t < lines) nan[t] = 0;
    }
}

// Pass `pass`: a task is a tile of kTile elements of a line.  A slot takes part while more than kLine elements agree with its digits.
template <typename T>
__global__ __launch_bounds__(kBlock) void stream_count_kernel(const T *__restrict__ in, int64_t lines, int64_t so, int64_t R, int64_t tiles, int slots, int pass,
                                                              const Sel<KeyOf<T>> *__restrict__ st, uint32_t *__restrict__ table, uint32_t *__restrict__ nan) {
    using K = KeyOf<T>;
    __shared__ uint32_t hist[kMaxSlots][256];
    __shared__ K prefix[kMaxSlots];
    __shared__ uint32_t active[kMaxSlots];
    __shared__ uint32_t any;
    const int lane = (int)threadIdx.x;
    for (int64_t task = blockIdx.x; task < lines * tiles; task += gridDim.x) {
        const int64_t line = task / tiles, tile = task - line * tiles, p0 = tile * kTile;
        const int len = (int)std::min<int64_t>(kTile, R - p0);
        if (lane == 0) any = 0;
        __syncthreads();
        if (lane < slots) {
            const Sel<K> s = st[line * slots + lane];
            const bool on = s.count > (uint32_t)kLine && (int)s.passes == pass;
            prefix[lane] = s.key, active[lane] = on;
            if (on) any = 1;  // every writer stores the same value
        }
        __syncthreads();
        if (any) {  // workgroup-uniform
            for (int b = lane; b < slots * 256; b += kBlock) (&hist[0][0])[b] = 0;
            __syncthreads();
            bool saw_nan = false;
            for (int s = lane; s < len; s += kBlock) {
                const T x = in[line * so + p0 + s];
                const K key = smquantile::key_of(x);
                saw_nan |= x != x;
                const uint32_t d = smquantile::digit(key, pass);
                for (int k = 0; k < slots; ++k)
                    if (active[k] && smquantile::agrees(key, prefix[k], pass)) atomicAdd(&hist[k][d], 1u);  // an integer count
            }
            if (pass == 0 && saw_nan) nan[line] = 1;  // every writer stores the same value
            __syncthreads();
            for (int b = lane; b < slots * 256; b += kBlock) {
                const uint32_t c = (&hist[0][0])[b];
                if (c) atomicAdd(&table[line * slots * 256 + b], c);  // integer addition commutes: the table is the same whatever the order
            }
        }
        __syncthreads();  // the next task overwrites the flags
    }
}

// A wave per (line, slot): fixes the digit of pass `pass` from the line's table and clears it.
template <typename T>
__global__ __launch_bounds__(kBlock) void stream_narrow_kernel(int64_t slots_total, int pass, Sel<KeyOf<T>> *__restrict__ st, uint32_t *__restrict__ table) {
    using K = KeyOf<T>;
    const int lane = (int)(threadIdx.x & 63);
    for (int64_t t = (int64_t)blockIdx.x * kWaves + (threadIdx.x >> 6); t < slots_total; t += (int64_t)gridDim.x * kWaves) {  // wave-uniform
        const Sel<K> s = st[t];
        if (!(s.count > (uint32_t)kLine && (int)s.passes == pass)) continue;
        uint32_t bin = 0, left = 0, count = 0;
        if (narrow_bins(table + t * 256, s.need, lane, &bin, &left, &count)) {
            Sel<K> n = s;
            n.key = s.key | ((K)bin << smquantile::shift_of<K>(pass)), n.need = left, n.count = count, n.passes = (uint32_t)pass + 1;
            st[t] = n;
        }
    }
}

// One more sweep of the line: a slot's agreeing elements go to its compaction buffer (count <= kLine), or, with every digit fixed and
// still more than kLine of them (equal keys), one of them leaves its canonical value.
template <typename T>
__global__ __launch_bounds__(kBlock) void stream_compact_kernel(const T *__restrict__ in, int64_t lines, int64_t so, int64_t R, int64_t tiles, int slots,
                                                                const Sel<KeyOf<T>> *__restrict__ st, uint32_t *__restrict__ fill, T *__restrict__ vals, T *__restrict__ comp) {
    using K = KeyOf<T>;
    __shared__ Sel<K> sel[kMaxSlots];
    const int lane = (int)threadIdx.x;
    for (int64_t task = blockIdx.x; task < lines * tiles; task += gridDim.x) {
        const int64_t line = task / tiles, tile = task - line * tiles, p0 = tile * kTile;
        const int len = (int)std::min<int64_t>(kTile, R - p0);
        if (lane < slots) sel[lane] = st[line * slots + lane];
        __syncthreads();
        for (int s = lane; s < len; s += kBlock) {
            const T x = in[line * so + p0 + s];
            const K key = smquantile::key_of(x);
            for (int k = 0; k < slots; ++k) {
                if (!smquantile::agrees(key, sel[k].key, (int)sel[k].passes)) continue;
                const int64_t slot = line * slots + k;
                if (sel[k].count <= (uint32_t)kLine) {
                    const uint32_t at = atomicAdd(&fill[slot], 1u);  // an integer count; which place an element takes does not matter
                    if (at < (uint32_t)kLine) comp[slot * kLine + at] = x;  // (always: exactly count elements agree)
                } else {
                    vals[slot] = smquantile::canonical(x);  // equal keys: every writer stores the same bits
                }
            }
        }
        __syncthreads();  // the next task overwrites sel
    }
}

// A workgroup per line: each slot's selection from its compacted elements, then the interpolation of every probability.
template <typename T>
__global__ __launch_bounds__(kBlock) void stream_finish_kernel(int64_t lines, SArgs sa, const Sel<KeyOf<T>> *__restrict__ st, const uint32_t *__restrict__ nan,
                                                               const T *__restrict__ vals, const T *__restrict__ comp, T *__restrict__ out) {
    using K = KeyOf<T>;
    __shared__ T v[kLine];
    __shared__ uint32_t hist[256];
    __shared__ Sel<K> pv;
    __shared__ T res;
    __shared__ T value[kMaxSlots];
    const int lane = (int)threadIdx.x;
    for (int b = lane; b < 256; b += kBlock) hist[b] = 0;
    for (int64_t line = blockIdx.x; line < lines; line += gridDim.x) {
        const bool has_nan = nan[line] != 0;
        for (int k = 0; k < sa.slots && !has_nan; ++k) {
            const int64_t slot = line * sa.slots + k;
            const Sel<K> s = st[slot];  // workgroup-uniform
            if (s.count <= (uint32_t)kLine) {
                const int len = (int)s.count;
                __syncthreads();  // v is free: the selection before has been read
                for (int e = lane; e < len; e += kBlock) v[e] = comp[slot * kLine + e];
                select_rank<T, false>(v, len, s.need - 1, hist, &pv, &res, lane);  // (opens with a rendezvous behind the loads)
                if (lane == 0) value[k] = res;
            } else if (lane == 0) {
                value[k] = vals[slot];
            }
        }
        __syncthreads();
        if (lane < sa.n) {
            const T lo = has_nan ? smquantile::quiet_nan<T>() : value[sa.lo[lane]], hi = has_nan ? lo : value[sa.hi[lane]];
            out[(int64_t)lane * lines + line] = has_nan ? lo : smquantile::finish<T>(lo, hi, sa.g[lane]);
        }
        __syncthreads();  // the next line overwrites value
    }
}

// ---- SORT / COPYONLY: `sorted` is dense [O][R][I], ascending along R with NaNs last; out[(q0 + i)*O*I + o*I + c] for the launch's
// probabilities i.
template <typename T>
__global__ __launch_bounds__(kBlock) void pick_kernel(const T *__restrict__ sorted, int64_t O, int64_t R, int64_t I, QArgs qa, int64_t q0, T *__restrict__ out) {
    const int64_t kept = O * I, total = kept * qa.n;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < total; t += (int64_t)gridDim.x * kBlock) {
        const int64_t i = t / kept, rem = t - i * kept, o = rem / I, c = rem - o * I;
        const T *line = sorted + o * R * I + c;
        const T last = line[(R - 1) * I];
        T r = smquantile::quiet_nan<T>();
        if (last == last) {
            const T lo = smquantile::canonical(line[(int64_t)qa.lo[i] * I]);
            const T hi = qa.g[i] != 0.0 ? smquantile::canonical(line[(int64_t)qa.hi[i] * I]) : lo;
            r = smquantile::finish<T>(lo, hi, qa.g[i]);
        }
        out[(q0 + i) * kept + rem] = r;
    }
}

// ------------------------------------------------------------------------------------------------------ the planner
struct Plan {
    int route = SMHIP_QUANTILE_ROUTE_NONE;
    bool stream = false, stage_in = false, stage_out = false, wave = false;
    int64_t O = 1, R = 1, I = 1;  // ori3
    int64_t lines = 0, so = 0;    // the rows the kernels take: line o at in + o*so
    int64_t total = 0, kept = 0, nq = 0;
    int passes = 0;               // STREAM: digit passes queued (the key's bytes)
    int slots = 0;                // the distinct ranks wanted (STREAM: followed through the passes)
    int sort_launches = 0;        // SORT: what the sort itself launches, as smhip_sort_plan counts them
    int64_t stage_a[SMHIP_MAX_NDIM];    // where element [idx] of the operand stands in the staged rows [lines][R], as strides over `shape`
    int64_t stage_res[SMHIP_MAX_NDIM];  // where result [q][kept idx] stands in the rows [Q][lines], as strides over {Q, kept extents}
    int res_ndim = 1;
    int64_t res_shape[SMHIP_MAX_NDIM];  // {Q, kept extents}
    int launches() const {
        if (route == SMHIP_QUANTILE_ROUTE_NONE) return 0;
        if (route == SMHIP_QUANTILE_ROUTE_COPYONLY) return 1 + (int)ceil_div(nq, kMaxQ);
        if (route == SMHIP_QUANTILE_ROUTE_SORT) return sort_launches + (int)ceil_div(nq, kMaxQ);
        return (stage_in ? 1 : 0) + (stream ? 2 * passes + 3 : 1) + (stage_out ? 1 : 0);
    }
    int code() const { return route | (stream ? SMHIP_QUANTILE_STREAM : 0) | (stage_in || stage_out ? SMHIP_QUANTILE_COPY : 0); }
    int reads() const {  // of the operand, at most
        if (route == SMHIP_QUANTILE_ROUTE_NONE) return 0;
        return stream ? passes + 1 : 1;
    }
};

// The slots of a call's probabilities: the distinct ranks in order of first use.
void make_slots(const smquantile::Rank *rk, int nq, SArgs *sa) {
    sa->n = nq, sa->slots = 0;
    auto slot_of = [&](int64_t rank) {
        for (int k = 0; k < sa->slots; ++k)
            if (sa->rank[k] == (uint32_t)rank) return k;
        sa->rank[sa->slots] = (uint32_t)rank;
        return sa->slots++;
    };
    for (int i = 0; i < nq; ++i) sa->lo[i] = (uint8_t)slot_of(rk[i].j), sa->hi[i] = (uint8_t)slot_of(rk[i].j1), sa->g[i] = rk[i].g;
}

void make_plan(int method, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, const double *q, int64_t nq, Plan *pl) {
    *pl = Plan();
    Plan &p = *pl;
    int64_t before_n = 1, after_n = 1;
    bool zero_stride = false;
    for (int d = 0; d < ndim; ++d) {
        if (d < axis) before_n *= shape[d];
        if (d > axis) after_n *= shape[d];
        if (shape[d] > 1 && strides[d] == 0) zero_stride = true;
    }
    p.R = shape[axis], p.O = before_n, p.I = after_n, p.kept = before_n * after_n, p.total = p.kept * p.R, p.nq = nq;
    p.res_ndim = 0, p.res_shape[p.res_ndim++] = nq;
    for (int d = 0; d < ndim; ++d)
        if (d != axis) p.res_shape[p.res_ndim++] = shape[d];
    if (p.kept == 0) return;
    if (p.R == 1) {
        p.route = SMHIP_QUANTILE_ROUTE_COPYONLY;
        return;
    }
    const auto to_sort = [&]() {
        int route = 0;
        int64_t ori[3];
        p.route = SMHIP_QUANTILE_ROUTE_SORT, p.stream = false;
        sort_axis_plan(dtype, shape, strides, ndim, axis, &route, &p.sort_launches, ori, nullptr);
        p.O = ori[0], p.I = ori[2];
        p.stage_in = p.stage_out = (route & SMHIP_SORT_COPY) != 0;
    };
    if (nq > kMaxQ) return to_sort();
    p.route = SMHIP_QUANTILE_ROUTE_ROW;
    int64_t in_lines[SMHIP_MAX_NDIM];  // the line of element [idx], as strides over `shape` (0 along the axis)
    Ax ax[SMHIP_MAX_NDIM];
    const int n = merge_axes(shape, strides, ndim, 1u << axis, false, ax);
    Canon c;
    if (!zero_stride && canonical(ax, n, &c) == kWalkRow) {  // read in place: every kept stride is a multiple of so
        p.O = c.O, p.I = 1, p.lines = c.O, p.so = c.so;
        for (int d = 0; d < ndim; ++d) in_lines[d] = shape[d] == 1 || d == axis ? 0 : strides[d] / c.so;
    } else {  // staged: the kept axes in index order, then the axis
        p.stage_in = true, p.lines = p.kept, p.so = p.R;
        int64_t acc = 1;
        for (int d = ndim - 1; d >= 0; --d) {
            if (d == axis) in_lines[d] = 0;
            else in_lines[d] = shape[d] == 1 ? 0 : acc, acc *= shape[d];
        }
    }
    int at = 0;
    p.stage_res[at++] = p.lines;
    for (int d = 0; d < ndim; ++d) {
        p.stage_a[d] = d == axis ? 1 : in_lines[d] * p.R;
        if (d != axis) p.stage_res[at++] = in_lines[d];
    }
    // (read in place, canonical() has merged the kept axes into ONE outer group, which only happens where they run on in the result as
    // well: the rows are then in the result's order and nothing is scattered; the check is the guard of that)
    p.stage_out = !row_major(p.res_shape, p.stage_res, p.res_ndim);
    p.wave = p.R <= kWaveLine;
    smquantile::Rank rk[kMaxQ];
    SArgs sa;
    for (int i = 0; i < (int)nq; ++i) rk[i] = smquantile::rank_of(p.R, q[i], method);
    make_slots(rk, (int)nq, &sa);
    p.slots = sa.slots;
    if (p.R > kLine) {
        p.stream = true, p.passes = (int)dtype_size(dtype);
        if ((size_t)p.lines * (size_t)p.slots > kStreamPoolBytes / ((size_t)kLine * dtype_size(dtype))) return to_sort();
    } else if (p.slots > (p.wave ? kWaveRanks : kLineRanks)) {
        return to_sort();  // every selection sweeps the line two or three times: beyond these counts one sort of the line is cheaper
    }
}

// ------------------------------------------------------------------------------------------------------ launching
const GridCap &grid_cap() { static const GridCap g(getenv("SMHIP_QUANTILE_GRID_CAP")); return g; }  // the cap of every launch here, read once

void fill_qargs(const smquantile::Rank *rk, int n, QArgs *qa) {
    qa->n = n;
    for (int i = 0; i < kMaxQ; ++i) qa->lo[i] = qa->hi[i] = 0, qa->g[i] = 0.0;
    for (int i = 0; i < n; ++i) qa->lo[i] = (uint32_t)rk[i].j, qa->hi[i] = (uint32_t)rk[i].j1, qa->g[i] = rk[i].g;
}

template <typename T>
int run_stream(const Plan &p, const smquantile::Rank *rk, const T *in, T *out, hipStream_t s) {
    using K = KeyOf<T>;
    SArgs sa = SArgs();
    make_slots(rk, (int)p.nq, &sa);
    const size_t slots = (size_t)p.lines * (size_t)sa.slots;
    // one pooled block, its parts on 16-byte boundaries: the states, the tables, the counters, the flags, the values, the compacted elements
    const size_t bytes[6] = {slots * sizeof(Sel<K>), slots * 256 * sizeof(uint32_t), slots * sizeof(uint32_t), (size_t)p.lines * sizeof(uint32_t), slots * sizeof(T),
                             slots * kLine * sizeof(T)};
    size_t offset[6], all = 0;
    for (int i = 0; i < 6; ++i) offset[i] = all, all += (bytes[i] + 15) / 16 * 16;
    Pooled pool;
    void *raw;
    if (int rc = pool.take(all, &raw)) return rc;
    char *base = static_cast<char *>(raw);
    Sel<K> *st = reinterpret_cast<Sel<K> *>(base + offset[0]);
    uint32_t *table = reinterpret_cast<uint32_t *>(base + offset[1]), *fill = reinterpret_cast<uint32_t *>(base + offset[2]), *nan = reinterpret_cast<uint32_t *>(base + offset[3]);
    T *vals = reinterpret_cast<T *>(base + offset[4]), *comp = reinterpret_cast<T *>(base + offset[5]);
    const int64_t tiles = ceil_div(p.R, kTile);
    const dim3 block(kBlock), sweep(grid_cap().capped(p.lines * tiles));
    hipLaunchKernelGGL((stream_init_kernel<T>), dim3(grid_cap().capped(ceil_div((int64_t)slots * 256, kBlock))), block, 0, s, p.lines, p.R, sa, st, table, fill, nan);
    SMHIP_LAUNCH_CHECK("quantile_axis stream init");
    for (int pass = 0; pass < p.passes; ++pass) {
        hipLaunchKernelGGL((stream_count_kernel<T>), sweep, block, 0, s, in, p.lines, p.so, p.R, tiles, sa.slots, pass, (const Sel<K> *)st, table, nan);
        SMHIP_LAUNCH_CHECK("quantile_axis stream count");
        hipLaunchKernelGGL((stream_narrow_kernel<T>), dim3(grid_cap().blocks_for((int64_t)slots)), block, 0, s, (int64_t)slots, pass, st, table);
        SMHIP_LAUNCH_CHECK("quantile_axis stream narrow");
    }
    hipLaunchKernelGGL((stream_compact_kernel<T>), sweep, block, 0, s, in, p.lines, p.so, p.R, tiles, sa.slots, (const Sel<K> *)st, fill, vals, comp);
    SMHIP_LAUNCH_CHECK("quantile_axis stream compact");
    hipLaunchKernelGGL((stream_finish_kernel<T>), dim3(grid_cap().capped(p.lines)), block, 0, s, p.lines, sa, (const Sel<K> *)st, (const uint32_t *)nan, (const T *)vals,
                       (const T *)comp, out);
    SMHIP_LAUNCH_CHECK("quantile_axis stream finish");
    return SMHIP_OK;
}

template <typename T>
int run_rows(const Plan &p, const smquantile::Rank *rk, const T *in, T *out, hipStream_t s) {
    if (p.stream) return run_stream<T>(p, rk, in, out, s);
    QArgs qa;
    fill_qargs(rk, (int)p.nq, &qa);
    if (p.wave) hipLaunchKernelGGL((quantile_row_kernel<T, true>), dim3(grid_cap().blocks_for(p.lines)), dim3(kBlock), 0, s, in, p.lines, p.so, (int)p.R, qa, out);
    else hipLaunchKernelGGL((quantile_row_kernel<T, false>), dim3(grid_cap().capped(p.lines)), dim3(kBlock), 0, s, in, p.lines, p.so, (int)p.R, qa, out);
    SMHIP_LAUNCH_CHECK("quantile_axis");
    return SMHIP_OK;
}

// ROW / STREAM: staged in, selected, staged out.
template <typename T>
int run_plan(const Plan &p, const smquantile::Rank *rk, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, void *out_v, hipStream_t s) {
    Pooled in_pool, out_pool;
    const T *in = static_cast<const T *>(a);
    if (p.stage_in) {
        void *buf;
        if (int rc = in_pool.take((size_t)p.total * sizeof(T), &buf)) return rc;
        if (int rc = launch_copy_strided(dtype, a, strides, buf, p.stage_a, shape, ndim, s)) return rc;
        in = static_cast<const T *>(buf);
    }
    T *out = static_cast<T *>(out_v);
    if (p.stage_out) {
        void *buf;
        if (int rc = out_pool.take((size_t)p.lines * (size_t)p.nq * sizeof(T), &buf)) return rc;
        out = static_cast<T *>(buf);
    }
    if (int rc = run_rows<T>(p, rk, in, out, s)) return rc;
    if (p.stage_out) {
        int64_t dense[SMHIP_MAX_NDIM];
        dense_strides(p.res_shape, p.res_ndim, dense);
        if (int rc = launch_copy_strided(dtype, out, p.stage_res, out_v, dense, p.res_shape, p.res_ndim, s)) return rc;
    }
    return SMHIP_OK;
}

// SORT and COPYONLY: the lines in order (or the lines of one element) dense in a pooled array of the operand's shape, then the picks.
template <typename T>
int run_sorted(const Plan &p, int method, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, const double *q, void *out,
               hipStream_t s) {
    Pooled pool;
    void *buf;
    if (int rc = pool.take((size_t)p.total * sizeof(T), &buf)) return rc;
    if (p.route == SMHIP_QUANTILE_ROUTE_SORT) {
        if (int rc = launch_sort_axis(SMHIP_SORT_ASCENDING, dtype, a, shape, strides, ndim, axis, buf, nullptr, s)) return rc;
    } else {
        int64_t dense[SMHIP_MAX_NDIM];
        dense_strides(shape, ndim, dense);
        if (int rc = launch_copy_strided(dtype, a, strides, buf, dense, shape, ndim, s)) return rc;
    }
    int64_t before_n = 1, after_n = 1;
    for (int d = 0; d < ndim; ++d) {
        if (d < axis) before_n *= shape[d];
        if (d > axis) after_n *= shape[d];
    }
    for (int64_t q0 = 0; q0 < p.nq; q0 += kMaxQ) {
        const int n = (int)std::min<int64_t>(kMaxQ, p.nq - q0);
        smquantile::Rank rk[kMaxQ];
        for (int i = 0; i < n; ++i) rk[i] = smquantile::rank_of(p.R, q[q0 + i], method);
        QArgs qa;
        fill_qargs(rk, n, &qa);
        hipLaunchKernelGGL((pick_kernel<T>), dim3(grid_cap().capped(ceil_div(p.kept * n, kBlock))), dim3(kBlock), 0, s, (const T *)buf, before_n, p.R, after_n, qa, q0,
                           static_cast<T *>(out));
        SMHIP_LAUNCH_CHECK("quantile_axis pick");
    }
    return SMHIP_OK;
}

template <typename T>
int run(const Plan &p, int method, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, const double *q, void *out,
        hipStream_t s) {
    if (p.route == SMHIP_QUANTILE_ROUTE_SORT || p.route == SMHIP_QUANTILE_ROUTE_COPYONLY) return run_sorted<T>(p, method, dtype, a, shape, strides, ndim, axis, q, out, s);
    smquantile::Rank rk[kMaxQ];
    for (int i = 0; i < (int)p.nq; ++i) rk[i] = smquantile::rank_of(p.R, q[i], method);
    return run_plan<T>(p, rk, dtype, a, shape, strides, ndim, out, s);
}

// Validation: everything that can be said without a device or a pointer.
int quantile_check(const char *who, int method, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, const double *q, int64_t nq) {
    if (method < SMHIP_QUANTILE_LINEAR || method > SMHIP_QUANTILE_MIDPOINT) return fail(SMHIP_ERR_INVALID, "%s: bad method %d", who, method);
    if (int rc = check_dtype_ndim(who, dtype, ndim)) return rc;
    if (dtype != SMHIP_F32 && dtype != SMHIP_F64) return fail(SMHIP_ERR_UNSUPPORTED, "%s: an integer dtype (f32 and f64 only: astype first)", who);
    if (int rc = check_axis(who, axis, ndim)) return rc;
    if (int rc = check_extents(who, shape, strides, ndim)) return rc;
    if (!q) return fail(SMHIP_ERR_INVALID, "%s: null q", who);
    if (nq < 1) return fail(SMHIP_ERR_INVALID, "%s: %lld probabilities (at least one)", who, (long long)nq);
    for (int64_t i = 0; i < nq; ++i)
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(SMHIP_ERR_INVALID, "%s: q[%lld] = %g outside [0, 1]", who, (long long)i, q[i]);
    if (shape[axis] >= kMaxAxis) return fail(SMHIP_ERR_UNSUPPORTED, "%s: an axis of %lld elements (ranks are 32 bits wide: below 2^31)", who, (long long)shape[axis]);
    if (shape[axis] == 0) {
        int64_t kept = 1;
        for (int d = 0; d < ndim; ++d)
            if (d != axis) kept *= shape[d];
        if (kept) return fail(SMHIP_ERR_INVALID, "%s: an empty axis with a result that is not empty", who);
    }
    return SMHIP_OK;
}

}  // namespace
}  // namespace smhip

using namespace smhip;

int smhip_quantile_axis(int method, int dtype, const void *a, const int64_t *shape, const int64_t *strides, int ndim, int axis, const double *q, int64_t nq,
                        void *out) {
    if (int rc = quantile_check("quantile_axis", method, dtype, shape, strides, ndim, axis, q, nq)) return rc;
    if (element_count(shape, ndim) == 0) return SMHIP_OK;
    if (!a) return fail(SMHIP_ERR_INVALID, "quantile_axis: null operand");
    if (!out) return fail(SMHIP_ERR_INVALID, "quantile_axis: null out");
    const size_t esz = dtype_size(dtype), n = (size_t)(element_count(shape, ndim) / shape[axis] * nq);
    const Span sa{a, span_bytes(shape, strides, ndim, esz)}, so{out, n * esz};
    if (spans_overlap(so, sa)) return fail(SMHIP_ERR_INVALID, "quantile_axis: out overlaps the operand");
    Plan pl;
    make_plan(method, dtype, shape, strides, ndim, axis, q, nq, &pl);
    SMHIP_ACQUIRE(s);  // undeclared spans (pooled staging, the tables): ordered behind everything, recorded tiny operators flushed first
    return dtype == SMHIP_F32 ? run<float>(pl, method, dtype, a, shape, strides, ndim, axis, q, out, s)
                              : run<double>(pl, method, dtype, a, shape, strides, ndim, axis, q, out, s);
}

int smhip_quantile_plan(int method, int dtype, const int64_t *shape, const int64_t *strides, int ndim, int axis, const double *q, int64_t nq, int *route,
                        int *launches, int64_t *ori3, int64_t *info3) {
    if (int rc = quantile_check("quantile_plan", method, dtype, shape, strides, ndim, axis, q, nq)) return rc;
    Plan pl;
    make_plan(method, dtype, shape, strides, ndim, axis, q, nq, &pl);
    if (route) *route = pl.code();
    if (launches) *launches = pl.launches();
    if (ori3) ori3[0] = pl.O, ori3[1] = pl.R, ori3[2] = pl.I;
    if (info3) info3[0] = kLine, info3[1] = kMaxQ, info3[2] = pl.reads();
    return SMHIP_OK;
}
