// index_mode.hip.h -- what an index mode (smhip.h: smhip_index_mode) means, once, for the three families whose memory safety rests
// on it: take_axis.hip, scatter_axis.hip and count.hip (bincount).  pick() is the one place where an index read from memory becomes a
// position; the host side is the check of the mode, its dispatch onto pick's template argument, and the report of a bad index.
#pragma once

#include <stdint.h>

#include <type_traits>
#include <utility>

#include "internal.h"
#include "smhip.h"

namespace smhip {

// The position along the gathered axis that index `i` names, in [0, R - 1] whatever `i` is.  R >= 1.
template <int Mode> __device__ __forceinline__ int64_t pick(int64_t i, int64_t R, bool &bad) {
    if constexpr (Mode == SMHIP_INDEX_WRAP) {
        if ((uint64_t)i < (uint64_t)R) return i;  // the common case, without the 64-bit division
        const int64_t m = i % R;                    // |m| < R; INT64_MIN % R is defined (R != -1)
        return m < 0 ? m + R : m;
    } else {
        if constexpr (Mode == SMHIP_INDEX_CHECKED)
            if (i < 0) i += R;  // cannot overflow: i < 0 < R
        const int64_t c = i < 0 ? 0 : i >= R ? R - 1 : i;
        if constexpr (Mode == SMHIP_INDEX_CHECKED) bad |= c != i;
        return c;
    }
}

// A bad index under CHECKED is reported, not followed: every lane that met one stores the same constant with a plain store.
template <int Mode> __device__ __forceinline__ void report_bad(bool bad, int64_t *bad_out) {
    if (Mode == SMHIP_INDEX_CHECKED && bad && bad_out) *bad_out = 1;
}

inline bool valid_index_mode(int mode) { return mode == SMHIP_INDEX_CHECKED || mode == SMHIP_INDEX_CLIP || mode == SMHIP_INDEX_WRAP; }
inline int check_index_mode(const char *who, int mode) { return valid_index_mode(mode) ? SMHIP_OK : fail(SMHIP_ERR_INVALID, "%s: bad mode %d", who, mode); }

// fn(std::integral_constant<int, Mode>) for the run-time `mode`: the one switch onto pick's template argument.
template <typename Fn> int with_index_mode(const char *who, int mode, Fn &&fn) {
    switch (mode) {
        case SMHIP_INDEX_CHECKED: return fn(std::integral_constant<int, SMHIP_INDEX_CHECKED>{});
        case SMHIP_INDEX_CLIP: return fn(std::integral_constant<int, SMHIP_INDEX_CLIP>{});
        case SMHIP_INDEX_WRAP: return fn(std::integral_constant<int, SMHIP_INDEX_WRAP>{});
    }
    return check_index_mode(who, mode);
}

}  // namespace smhip
