// Stand-alone host program (no GPU, no library): csrc/philox_core.hpp against the known answers of Random123's Philox4x32-10
// (kat_vectors), then the integer helpers at their extremes: range() stays in [0, n), the geometry stays inside the city for a jitter
// far larger than the city, and a sample's words depend on (seed, key, stream, slot) alone.  Meant for an -fsanitize=address,undefined
// build as well:   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I fabric_amd/csrc tools/philox_host_check.cpp -o philox_host_check
// Prints the three answers as hex words, one line each, and "ok"; exits non-zero on the first failure.
#include <cstdio>
#include <cstdlib>

#include "philox_core.hpp"

static int fail(const char* what) { std::printf("FAIL: %s\n", what); return 1; }

int main() {
    struct { uint32_t c[4], k[2], want[4]; } kat[] = {
        {{0, 0, 0, 0}, {0, 0}, {0x6627e8d5u, 0xe169c58du, 0xbc57ac4cu, 0x9b00dbd8u}},
        {{0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu}, {0xffffffffu, 0xffffffffu}, {0x408f276du, 0x41c83b0eu, 0xa20bc7c6u, 0x6d5451fdu}},
        {{0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u}, {0xa4093822u, 0x299f31d0u}, {0xd16cfe09u, 0x94fdccebu, 0x5001e420u, 0x24126ea1u}},
    };
    for (const auto& v : kat) {
        const Philox4 r = philox4x32_10(v.c[0], v.c[1], v.c[2], v.c[3], v.k[0], v.k[1]);
        std::printf("%08x %08x %08x %08x\n", r.w[0], r.w[1], r.w[2], r.w[3]);
        for (int i = 0; i < 4; i++)
            if (r.w[i] != v.want[i]) return fail("known answer");
    }
    // philox_draw places (key_lo, key_hi, slot, stream) in the counter and the seed in the key
    const Philox4 a = philox_draw(0x299f31d0a4093822ull, 0x85a308d3243f6a88ull, 0x03707344u, 0x13198a2eu);
    for (int i = 0; i < 4; i++)
        if (a.w[i] != kat[2].want[i]) return fail("counter layout of philox_draw");
    const uint32_t words[] = {0u, 1u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu}, ns[] = {1u, 2u, 3u, 17u, 0x80000000u, 0xffffffffu};
    for (uint32_t w : words)
        for (uint32_t n : ns)
            if (philox_range(w, n) >= n) return fail("range left [0, n)");
    if (philox_range(0xffffffffu, 7u) != 6u || philox_range(0u, 7u) != 0u) return fail("range ends");
    // a jitter of 2^24 on a city barely larger than the patch: every window stays inside, for every key tried
    for (uint64_t key = 0; key < 2000; key++) {
        const int H = 20, W = 13, S = 12;
        const PhiloxGeom g = philox_geometry(7, key << 20 | key, 3, 1, 5, H, W, S, 1 << 24, true, true, 1, S);
        if (g.row < 0 || g.row > H - S || g.col < 0 || g.col > W - S) return fail("clamp");
        if (g.sym < 0 || g.sym > 7) return fail("sym");
        if (g.eh < 1 || g.eh > S || g.ew < 1 || g.ew > S || g.top < 0 || g.top + g.eh > S || g.left < 0 || g.left + g.ew > S) return fail("rectangle");
        const PhiloxGeom off = philox_geometry(7, key, 3, 1, 5, H, W, S, 0, false, false, 0, 0);
        if (off.row != 3 || off.col != 1 || off.sym != 5 || off.eh || off.ew || off.top || off.left) return fail("stages off");
    }
    std::printf("ok\n");
    return 0;
}
