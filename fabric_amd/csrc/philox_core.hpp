// The counter-based generator of bdn_sample_patches_aug (scene.hip) and the integer part of its draws: Philox4x32-10 (Salmon, Moraes,
// Dror, Shaw, "Parallel random numbers: as easy as 1, 2, 3", SC 2011).  Integers only, plain functions, so tools/philox_host_check.cpp
// runs them on the host against Random123's known answers (cc_core.hpp's arrangement).
//
// One call maps a 128-bit counter and a 64-bit key to four 32-bit words; it keeps no state.  The sampler's use of it:
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (sample_key & 0xffffffff, sample_key >> 32, slot, stream),   sample_key = epoch << 32 | dataset index
// so a draw depends on (seed, epoch, dataset index, stream, slot) and on nothing else: not on the batch, the rank or the thread.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PHILOX_HD __host__ __device__ __forceinline__
#else
#define PHILOX_HD inline
#endif

struct Philox4 { uint32_t w[4]; };

constexpr uint32_t PHILOX_M0 = 0xD2511F53u, PHILOX_M1 = 0xCD9E8D57u;      // round multipliers
constexpr uint32_t PHILOX_W0 = 0x9E3779B9u, PHILOX_W1 = 0xBB67AE85u;      // key increments (golden ratio, sqrt(3) - 1)

constexpr uint32_t PHILOX_GEOMETRY = 0, PHILOX_RADIOMETRY = 1, PHILOX_NOISE = 2;      // streams; noise plane p uses PHILOX_NOISE + p
constexpr uint32_t PHILOX_WARP = 0x57415250u;      // bdn_sample_patches_warp's stream ('WARP'): far above any noise stream 2 .. 2 + 2C - 1
constexpr uint32_t PHILOX_MIX = 0x4D495820u;       // bdn_mix_plan's stream ('MIX '): distinct from PHILOX_WARP, above every noise stream too

PHILOX_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)PHILOX_M0 * c0, p1 = (uint64_t)PHILOX_M1 * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += PHILOX_W0; k1 += PHILOX_W1;
    }
    return Philox4{{c0, c1, c2, c3}};
}

// the sampler's call: words of (seed, sample key, stream, slot)
PHILOX_HD Philox4 philox_draw(uint64_t seed, uint64_t sample_key, uint32_t stream, uint32_t slot) {
    return philox4x32_10((uint32_t)sample_key, (uint32_t)(sample_key >> 32), slot, stream, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// an integer in [0, n) from a word: (w * n) >> 32.  n >= 1; the product of two 32-bit values fits 64 bits
PHILOX_HD uint32_t philox_range(uint32_t w, uint32_t n) { return (uint32_t)(((uint64_t)w * n) >> 32); }

// the 24 bits behind u(w) = float(w >> 8) * 2^-24 in [0, 1): every such value is a float32, so the conversion and the scaling are exact
PHILOX_HD uint32_t philox_u24(uint32_t w) { return w >> 8; }

PHILOX_HD int philox_clamp(long long v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

// ---- stream 0: the geometry of one sample, integers only except the erase decision (erased: u(w3) < erase_p, taken by the caller)
struct PhiloxGeom { int row, col, sym, top, left, eh, ew; uint32_t erase_u24; };

// (row, col, sym): the validated descriptor, H x W its city, S the patch, J >= 0 the jitter.  The clamp keeps every window inside the
// city for any draw.  The rectangle (slot 1) is drawn only when the erase stage is on (erase_on: erase_p > 0; then 1 <= lo <= hi <= S)
// and is (0, 0, 0, 0) otherwise.
PHILOX_HD PhiloxGeom philox_geometry(uint64_t seed, uint64_t sample_key, int row, int col, int sym, int H, int W, int S, int J,
                                     bool draw_sym, bool erase_on, int lo, int hi) {
    PhiloxGeom g;
    if (J == 0 && !draw_sym && !erase_on) {                  // every geometric stage off: the descriptor as it is, no draw
        g.row = row; g.col = col; g.sym = sym; g.erase_u24 = 0; g.eh = g.ew = g.top = g.left = 0;
        return g;
    }
    const Philox4 a = philox_draw(seed, sample_key, PHILOX_GEOMETRY, 0);
    const uint32_t span = 2u * (uint32_t)J + 1u;
    g.row = philox_clamp((long long)row + (long long)philox_range(a.w[0], span) - J, 0, H - S);
    g.col = philox_clamp((long long)col + (long long)philox_range(a.w[1], span) - J, 0, W - S);
    g.sym = draw_sym ? (int)(a.w[2] >> 29) : sym;
    g.erase_u24 = philox_u24(a.w[3]);
    g.eh = g.ew = g.top = g.left = 0;
    if (!erase_on) return g;
    const Philox4 b = philox_draw(seed, sample_key, PHILOX_GEOMETRY, 1);
    g.eh = lo + (int)philox_range(b.w[0], (uint32_t)(hi - lo + 1));
    g.ew = lo + (int)philox_range(b.w[1], (uint32_t)(hi - lo + 1));
    g.top = (int)philox_range(b.w[2], (uint32_t)(S - g.eh + 1));
    g.left = (int)philox_range(b.w[3], (uint32_t)(S - g.ew + 1));
    return g;
}

// ---- stream PHILOX_MIX: whether a sample is mixed, its donor and its rectangle (bdn_mix_plan), integers only except the one comparison
struct PhiloxMix { int on, pick, top, left, h, w; };

// key: the RECIPIENT's sample key.  p in [0, 1]; 1 <= lo <= hi <= S; n_pool >= 1.  pick in [0, n_pool) indexes the donor pool.  box: slot 1
// places the h x w rectangle; otherwise (object mode) the rectangle is the patch and slot 1 is not drawn.  An unmixed sample is all zero.
PHILOX_HD PhiloxMix philox_mix(uint64_t seed, uint64_t sample_key, int S, float p, bool box, int lo, int hi, uint32_t n_pool) {
    PhiloxMix m{0, 0, 0, 0, 0, 0};
    const Philox4 a = philox_draw(seed, sample_key, PHILOX_MIX, 0);
    if (!((float)philox_u24(a.w[0]) * 0x1p-24f < p)) return m;
    m.on = 1;
    m.pick = (int)philox_range(a.w[1], n_pool);
    m.h = lo + (int)philox_range(a.w[2], (uint32_t)(hi - lo + 1));
    m.w = lo + (int)philox_range(a.w[3], (uint32_t)(hi - lo + 1));
    if (!box) { m.h = m.w = S; return m; }
    const Philox4 b = philox_draw(seed, sample_key, PHILOX_MIX, 1);
    m.top = (int)philox_range(b.w[0], (uint32_t)(S - m.h + 1));
    m.left = (int)philox_range(b.w[1], (uint32_t)(S - m.w + 1));
    return m;
}
