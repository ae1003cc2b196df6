// wave.hip.h -- in-wave folds and scans through DPP moves, shared by reduce.hip (whole-array reductions), reduce_axis.hip (axis
// reductions) and scan_axis.hip (cumulative scans).
#pragma once

#include <stdint.h>

#include <type_traits>

namespace smhip {
namespace dev {

// Wave total through DPP moves (v_mov_b32 row_shr / row_bcast: VALU-speed lane exchange inside the SIMD) instead of
// __shfl_down, which the compiler lowers to ds_bpermute_b32 -- an LDS-crossbar round trip per 32-bit half and stage, with a
// full lgkmcnt wait behind each: 6 stages x 2 halves for the wave, and round 2 ran the same 6 stages AGAIN in wave 0 to add
// four numbers.  Every wave of the fused op+sum kernel carried ~1000 cycles of that behind its last store, holding its slot
// (the kernel ran 2 % behind the plain add: 496-498 us against 486 on one box, tools/sweep_fused2.hip).
// The scan: row_shr 1, 2, 4, 8 leave each row of 16 lanes' running sum in its lane 15; row_bcast:15 adds it to the next
// row (rows 1 and 3), row_bcast:31 adds lane 31 to rows 2 and 3: lane 63 holds the wave's total.  Lanes without a source
// receive `old` = 0, the sum's identity.  The order of the additions is fixed, so the bits are the same on every run
// (they differ from round 2's tree order in the last place, as any reassociation does).
constexpr int kWaveTotalLane = 63;
template <int CTRL, int ROW_MASK> __device__ __forceinline__ double dpp_move(double v) {
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROW_MASK, 0xf, false);
    return __hiloint2double(hi, lo);
}
template <int CTRL, int ROW_MASK> __device__ __forceinline__ uint64_t dpp_move(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, ROW_MASK, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, ROW_MASK, 0xf, false);
    return ((uint64_t)hi << 32) | lo;
}
// the wave's total, valid in lane kWaveTotalLane
template <typename A> __device__ __forceinline__ A wave_reduce(A v) {
    v += dpp_move<0x111, 0xf>(v);  // row_shr:1
    v += dpp_move<0x112, 0xf>(v);  // row_shr:2
    v += dpp_move<0x114, 0xf>(v);  // row_shr:4
    v += dpp_move<0x118, 0xf>(v);  // row_shr:8
    v += dpp_move<0x142, 0xa>(v);  // row_bcast:15 into rows 1 and 3
    v += dpp_move<0x143, 0xc>(v);  // row_bcast:31 into rows 2 and 3
    return v;
}

// The same moves for any 4- or 8-byte value, lanes without a source receiving `old` (the fold's identity).
template <int CTRL, int ROW_MASK, typename A> __device__ __forceinline__ A dpp_move_or(A v, A old) {
    static_assert(sizeof(A) == 4 || sizeof(A) == 8, "dpp_move_or: 4- or 8-byte values");
    if constexpr (sizeof(A) == 4) {
        const int r = __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false);
        return __builtin_bit_cast(A, r);
    } else {
        const uint64_t vb = __builtin_bit_cast(uint64_t, v), ob = __builtin_bit_cast(uint64_t, old);
        const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)ob, (int)(uint32_t)vb, CTRL, ROW_MASK, 0xf, false);
        const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(ob >> 32), (int)(uint32_t)(vb >> 32), CTRL, ROW_MASK, 0xf, false);
        return __builtin_bit_cast(A, ((uint64_t)hi << 32) | lo);
    }
}
// wave_reduce's scan, cut short for SEGMENTS of g lanes (g = 1, 2, 4, ..., 64, wave-uniform) and with any associative fold
// F and its identity: after the row_shr steps up to g / 2, lane i holds the fold of lanes i - g + 1 .. i of its 16-lane row,
// so the fold of segment s (lanes s*g .. s*g + g - 1) is valid in its LAST lane, s*g + g - 1 (for g = 64: kWaveTotalLane).
// The order of the operations is fixed: the same bits on every run.
template <typename A, typename F> __device__ __forceinline__ A segment_fold(A v, int g, A id, F f) {
    if (g >= 2) v = f(v, dpp_move_or<0x111, 0xf>(v, id));
    if (g >= 4) v = f(v, dpp_move_or<0x112, 0xf>(v, id));
    if (g >= 8) v = f(v, dpp_move_or<0x114, 0xf>(v, id));
    if (g >= 16) v = f(v, dpp_move_or<0x118, 0xf>(v, id));
    if (g >= 32) v = f(v, dpp_move_or<0x142, 0xa>(v, id));
    if (g >= 64) v = f(v, dpp_move_or<0x143, 0xc>(v, id));
    return v;
}

// segment_fold for PAIRS (argreduce_axis.hip: a value and where it stands): both halves go through the SAME DPP controls, so a
// lane always meets the pair of one source lane, and `take(v, r, mv, mr)` then replaces (v, r) by (mv, mr) where the pair
// combine prefers it.  Lanes without a source meet (idv, idr), which `take` never prefers.  The combine is associative, so as
// in segment_fold the segment's pair is valid in its LAST lane; it is commutative and idempotent too, so the windows that
// reach over a segment's start in between do no harm.
template <typename V, typename R, typename F> __device__ __forceinline__ void segment_fold_pair(V &v, R &r, int g, V idv, R idr, F take) {
    if (g >= 2) take(v, r, dpp_move_or<0x111, 0xf>(v, idv), dpp_move_or<0x111, 0xf>(r, idr));
    if (g >= 4) take(v, r, dpp_move_or<0x112, 0xf>(v, idv), dpp_move_or<0x112, 0xf>(r, idr));
    if (g >= 8) take(v, r, dpp_move_or<0x114, 0xf>(v, idv), dpp_move_or<0x114, 0xf>(r, idr));
    if (g >= 16) take(v, r, dpp_move_or<0x118, 0xf>(v, idv), dpp_move_or<0x118, 0xf>(r, idr));
    if (g >= 32) take(v, r, dpp_move_or<0x142, 0xa>(v, idv), dpp_move_or<0x142, 0xa>(r, idr));
    if (g >= 64) take(v, r, dpp_move_or<0x143, 0xc>(v, idv), dpp_move_or<0x143, 0xc>(r, idr));
}

// The same moves as an inclusive SCAN (scan_axis.hip): after it lane i holds f over lanes s*g .. i of its segment of g lanes
// (g = 1, 2, 4, ..., 64, wave-uniform; `lane` = the lane's number in the wave), earlier lanes on the left of f.  A step whose
// source lies in the segment before is skipped, so every lane's value is valid, not only the segment's last.  Every value
// that meets another in f covers the lanes just before it: a fold of runs of CONSECUTIVE lanes, in a fixed order.  All 64
// lanes must be active.
template <typename A, typename F> __device__ __forceinline__ A segment_scan(A v, int g, int lane, A id, F f) {
    const int sl = lane & ((g < 16 ? g : 16) - 1);  // the lane's place in its segment, or in its row of 16
    A m;
    if (g >= 2) { m = dpp_move_or<0x111, 0xf>(v, id); v = sl >= 1 ? f(m, v) : v; }    // row_shr:1
    if (g >= 4) { m = dpp_move_or<0x112, 0xf>(v, id); v = sl >= 2 ? f(m, v) : v; }    // row_shr:2
    if (g >= 8) { m = dpp_move_or<0x114, 0xf>(v, id); v = sl >= 4 ? f(m, v) : v; }    // row_shr:4
    if (g >= 16) { m = dpp_move_or<0x118, 0xf>(v, id); v = sl >= 8 ? f(m, v) : v; }   // row_shr:8
    if (g >= 32) { m = dpp_move_or<0x142, 0xa>(v, id); v = (lane & 16) ? f(m, v) : v; }  // row_bcast:15 into rows 1 and 3
    if (g >= 64) { m = dpp_move_or<0x143, 0xc>(v, id); v = (lane & 32) ? f(m, v) : v; }  // row_bcast:31 into rows 2 and 3
    return v;
}
// The value of the lane before (wave_shr:1), `id` in the first lane of each segment of g lanes: the scan of it is the
// EXCLUSIVE scan of v.  All 64 lanes must be active.
template <typename A> __device__ __forceinline__ A segment_prev(A v, int g, int lane, A id) {
    const A p = dpp_move_or<0x138, 0xf>(v, id);
    return (lane & (g - 1)) == 0 ? id : p;
}
template <typename A, typename F> __device__ __forceinline__ A wave_scan(A v, int lane, A id, F f) { return segment_scan(v, 64, lane, id, f); }

}  // namespace dev
}  // namespace smhip
