// The arithmetic of edt.hip that has no GPU-specific part: the site test, the column sweeps (pass 1) and the lower-envelope row pass
// (pass 2: Meijster, Roerdink, Hesselink, "A general algorithm for computing distance transforms in linear time", 2000) of the exact
// squared Euclidean distance transform.  Integers only.  Plain functions, so tools/edt_host_check.cpp runs them serially on the host
// against a brute-force minimum (cc_core.hpp's arrangement).
//
// Pass 1 leaves g(x) = the distance to the nearest site of column x (EDT_INF: the column holds none) as 16 bits: H <= 32767.
// Pass 2, one row: out(x) = min(limit, min over x' with g(x') finite of (x - x')^2 + g(x')^2).  Every term is below 2 * 32766^2 < 2^31.
// The row's lower envelope is a stack of (position s, first column t it wins from, g); the stack has at most one entry per column read
// so far, so its g values are written over the front of the row's own g array (entry q <= the column being read: what is overwritten
// has been consumed) and the (s, t) pairs go to a second array of W words.  The forward scan pushes and pops, the backward scan walks
// the stack down once: O(W) per row whatever the row holds -- empty rows, one site and dense rows alike.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define EDT_HD __host__ __device__ __forceinline__
#else
#define EDT_HD inline
#endif

constexpr unsigned EDT_INF = 0xFFFFu;                      // g of a column without a site
constexpr int EDT_MAX_DIM = 32767;                         // H, W: g < EDT_INF, positions fit 16 bits, every squared distance an int32

// a pixel is a site if it is valid and its byte compares to site_value as site_equal says
EDT_HD bool edt_is_site(int src, int site_value, int site_equal, bool has_valid, int valid_byte, int invalid_value) {
    if (has_valid && valid_byte == invalid_value) return false;
    return (src == site_value) == (site_equal != 0);
}

// one step of a column sweep: the distance to the last site passed, EDT_INF before the first
EDT_HD unsigned edt_col_step(unsigned d, bool site) { return site ? 0u : (d == EDT_INF ? EDT_INF : d + 1u); }
EDT_HD unsigned edt_col_min(unsigned down, unsigned up) { return down < up ? down : up; }

// an element every `stride` entries: the row of one lane in an array laid out [column][row]
template <typename T> struct EdtStrided {
    T* p; size_t stride;
    EDT_HD T& operator()(int k) const { return p[(size_t)k * stride]; }
};

// the same for a block's on-chip arrays, laid out [column][lane] for the EDT_LANES rows of a block (one wave): p points at the lane's element 0
constexpr int EDT_LANES = 64;
constexpr int EDT_LDS_W = 128;                             // rows up to this width run the row pass on chip (48 KiB per block), wider ones in the workspace
template <typename T> struct EdtLaned {
    T* p;
    EDT_HD T& operator()(int k) const { return p[k * EDT_LANES]; }
};

// the row pass.  gs(k), k < W: g of column k on entry, the stack's g values afterwards; st(k): W words of scratch, never read before
// they are written; out(k): the W results.
template <typename GS, typename ST, typename OUT>
EDT_HD void edt_row_pass(GS gs, ST st, OUT out, int W, int limit) {
    int q = -1, ts = 0, tt = 0, tg = 0;                    // the top of the stack lives in registers
    for (int u0 = 0; u0 < W; u0 += 8) {                    // eight independent loads ahead of the dependent stack work (a stack write goes
      int gb[8];                                           // to an entry <= u: never to a column that is loaded here and not yet consumed)
#pragma unroll
      for (int i = 0; i < 8; i++) gb[i] = u0 + i < W ? (int)gs(u0 + i) : (int)EDT_INF;
#pragma unroll
      for (int i = 0; i < 8; i++) {
        const int u = u0 + i, g = gb[i];
        if (g == (int)EDT_INF) continue;
        const int g2 = g * g;
        while (q >= 0) {                                   // pop what column u beats where it starts to win
            const int a = tt - ts, b = u - tt;
            if (a * a + tg * tg <= b * b + g2) break;
            if (--q >= 0) { const uint32_t e = st(q); ts = (int)(e & 0xFFFFu); tt = (int)(e >> 16); tg = (int)gs(q); }
        }
        if (q < 0) {
            q = 0; ts = u; tt = 0; tg = g;
            st(0) = (uint32_t)u; gs(0) = (uint16_t)g;
        } else {                                           // the top wins at tt, so the numerator is >= 0 and w > tt
            const int num = (u * u + g2) - (ts * ts + tg * tg);
            const int w = 1 + num / (2 * (u - ts));        // the first column where u wins
            if (w < W) {
                q++; ts = u; tt = w; tg = g;
                st(q) = (uint32_t)u | ((uint32_t)w << 16); gs(q) = (uint16_t)g;
            }
        }
      }
    }
    for (int u = W - 1; u >= 0; u--) {
        if (q < 0) { out(u) = limit; continue; }           // a row without a finite g (t of entry 0 is 0: q stays >= 0 down to u = 0)
        const int d = u - ts, v = d * d + tg * tg;
        out(u) = v < limit ? v : limit;
        if (u == tt && --q >= 0) { const uint32_t e = st(q); ts = (int)(e & 0xFFFFu); tt = (int)(e >> 16); tg = (int)gs(q); }
    }
}

// ---- the boundary of a mask (boundary F1 / Hausdorff): a foreground pixel is on it when it is valid and a 4-neighbour inside the image
// is valid and not foreground.  nb: the four neighbours' (valid && !fg), false outside the image.
EDT_HD bool edt_on_boundary(bool valid, bool fg, bool up, bool down, bool left, bool right) { return valid && fg && (up || down || left || right); }
