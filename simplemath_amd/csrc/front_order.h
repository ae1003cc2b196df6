// front_order.h -- the order in which a long streaming launch's workgroups walk their arrays.
//
// The hardware deals workgroups to the eight XCDs in turn: blocks b and b + 8 share an XCD.  In natural order each XCD
// therefore touches every eighth 16 KiB tile.  front_tile() lets class b % 8 take C = 2^lc CONSECUTIVE tiles out of every
// group of 8 C instead, so that one XCD streams C tiles of each operand back to back while all eight stay inside the same
// window of 8 C tiles.  C = 32 (512 KiB of each stream per visit) is the size that pays inside the pieces of a large
// operand: the f32 add at 2^28 elements 82.3 -> 83.5 % of HBM peak, the fused add+sum 80.8 -> 82.3 %
// (profiles/front_order_ab.txt); C <= 4 and C >= 128 lose 3-10 % (tools/sweep_fronts.hip -> profiles/sweep_fronts.txt).
// It does not keep the XCDs' fronts together -- they drift apart by 5 % of the distance covered either way
// (profiles/front_drift.txt); launching in pieces still does that.
//
// The mapping is a bijection on [0, nb) for every nb >= full_tiles: the identity where lc == 0, on the ragged end (blocks
// from the last whole group of 8 C full tiles on -- the partial tile and the tail thread's block among them), and so for
// every launch of fewer than 8 C full tiles.  Plain integer code: the kernels and tests/cpp/front_order_host.cpp share it.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMHIP_FRONT_HD __host__ __device__
#else
#define SMHIP_FRONT_HD
#endif

namespace smhip {

constexpr unsigned kFrontLog2C = 5;     // the library's choice where the order applies (internal.h: front_order_for)
constexpr unsigned kFrontMaxLog2C = 8;  // the largest the test override may ask for

// b: blockIdx.x;  lc: log2 C, 0 = natural order;  full_tiles: the launch's whole tiles (n_vec / BLOCK)
SMHIP_FRONT_HD inline unsigned front_tile(unsigned b, unsigned lc, unsigned full_tiles) {
    const unsigned group = 8u << lc;
    if (lc == 0 || b >= (full_tiles & ~(group - 1u))) return b;
    const unsigned r = b & (group - 1u);
    return (b - r) + ((r & 7u) << lc) + (r >> 3);
}

}  // namespace smhip
