// front_order_host.cpp -- csrc/front_order.h's block-to-tile mapping, checked on the host (no GPU, no library).
// For every launch shape the kernels can see -- nb workgroups of which `full` are whole tiles (full = nb, or nb - 1 where the
// last workgroup holds the partial tile / the tail thread) -- and every C = 2^lc the library can choose:
//   * a bijection on [0, nb);
//   * the identity for lc = 0, where full < 8 C, and on the ragged end (blocks from the last whole group of 8 C on);
//   * inside a whole group, class b % 8 takes C consecutive tiles of that group, in order.
#include <cstdio>
#include <vector>

#include "front_order.h"

static long checked = 0;

static bool check(unsigned nb, unsigned full, unsigned lc) {
    const unsigned C = 1u << lc, G = 8u * C, whole = lc ? full / G * G : 0;
    std::vector<unsigned char> seen(nb, 0);
    for (unsigned b = 0; b < nb; ++b) {
        const unsigned t = smhip::front_tile(b, lc, full);
        if (t >= nb || seen[t]) { printf("nb %u full %u lc %u: block %u -> tile %u (%s)\n", nb, full, lc, b, t, t >= nb ? "out of range" : "taken twice"); return false; }
        seen[t] = 1;
        if (b >= whole) {
            if (t != b) { printf("nb %u full %u lc %u: block %u on the ragged end -> tile %u\n", nb, full, lc, b, t); return false; }
        } else {
            const unsigned g = b / G, r = b % G, want = g * G + (r % 8) * C + r / 8;
            if (t != want) { printf("nb %u full %u lc %u: block %u -> tile %u, not %u\n", nb, full, lc, b, t, want); return false; }
        }
    }
    ++checked;
    return true;
}

int main() {
    bool ok = true;
    for (unsigned lc = 0; lc <= smhip::kFrontMaxLog2C && ok; ++lc) {
        const unsigned G = 8u << lc;
        for (unsigned nb = 1; nb <= 5000 && ok; ++nb) ok = check(nb, nb, lc) && check(nb, nb - 1, lc);
        std::vector<unsigned> big = {1u << 17, (1u << 17) + 1, (1u << 19) - 3};
        for (unsigned k : {1u, 2u, 3u, 63u, 64u, 1000u}) for (int d = -1; d <= 1; ++d) big.push_back(G * k + d);
        for (unsigned nb : big) if (ok) ok = check(nb, nb, lc) && check(nb, nb - 1, lc);
    }
    if (smhip::kFrontLog2C < 1 || smhip::kFrontLog2C > smhip::kFrontMaxLog2C) { printf("kFrontLog2C out of range\n"); ok = false; }
    printf("front_order %s shapes %ld\n", ok ? "ok" : "FAILED", checked);
    return ok ? 0 : 1;
}
