// Stand-alone host check of fabric_amd/csrc/edt_core.hpp: the column sweeps and the lower-envelope row pass of edt.hip run serially over a
// pattern set -- with the transposed intermediate, the in-place g stack and the (s, t) scratch exactly as the kernels lay them out: [column][lane]
// arrays per block of 64 rows up to 128 columns (the on-chip form), [column][row] in the workspace above --
// against a brute-force minimum over all sites, and the boundary test against its definition.  No GPU, no library.  Meant for a
// sanitizer build:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/edt_host_check.cpp -o /tmp/edt_host_check && /tmp/edt_host_check
#include <limits.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../fabric_amd/csrc/edt_core.hpp"

static unsigned long long g_rng = 88172645463325252ull;
static double rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (g_rng >> 11) * (1.0 / 9007199254740992.0); }

static std::vector<uint8_t> pattern(int kind, int H, int W) {
    std::vector<uint8_t> f((size_t)H * W, 0);
    auto at = [&](int y, int x) -> uint8_t& { return f[(size_t)y * W + x]; };
    const double dens[] = {0.02, 0.5, 0.98};
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            switch (kind) {
                case 0: break;                                                  // empty
                case 1: at(y, x) = 1; break;                                    // full
                case 2: at(y, x) = y == 0 && x == 0; break;                     // one pixel in each corner
                case 3: at(y, x) = y == 0 && x == W - 1; break;
                case 4: at(y, x) = y == H - 1 && x == 0; break;
                case 5: at(y, x) = y == H - 1 && x == W - 1; break;
                case 6: at(y, x) = y == H / 2; break;                           // one row
                case 7: at(y, x) = x == W / 2; break;                           // one column
                case 8: at(y, x) = (y + x) & 1; break;                          // checkerboard
                case 9: case 10: case 11: at(y, x) = rnd() < dens[kind - 9]; break;
                case 12: at(y, x) = y == 0; break;                              // the top row: every g finite and large
                case 13: at(y, x) = (x * 7 + y * 3) % 11 == 0 && y < H / 2 + 1; break;
            }
    return f;
}

struct Vec32 { int32_t* p; int32_t& operator()(int k) const { return p[k]; } };

// N = 1: the kernels' data flow on the host
static std::vector<int32_t> separable(const std::vector<uint8_t>& src, const std::vector<uint8_t>& val, int sv, int eq, int inv, int limit, int H,
                                      int W) {
    const size_t R = (size_t)H;
    std::vector<uint16_t> gT((size_t)W * R, 0xABCD);       // poisoned: every element read must have been written
    std::vector<uint32_t> st((size_t)W * R, 0xDEADBEEF);
    for (int x = 0; x < W; x++) {
        unsigned d = EDT_INF;
        for (int y = 0; y < H; y++) {
            const size_t o = (size_t)y * W + x;
            d = edt_col_step(d, edt_is_site(src[o], sv, eq, !val.empty(), val.empty() ? 0 : val[o], inv));
            gT.at((size_t)x * R + y) = (uint16_t)d;
        }
        d = EDT_INF;
        for (int y = H - 1; y >= 0; y--) {
            const unsigned down = gT.at((size_t)x * R + y);
            d = edt_col_step(d, down == 0);
            gT.at((size_t)x * R + y) = (uint16_t)edt_col_min(down, d);
        }
    }
    std::vector<int32_t> out((size_t)H * W, -7);
    if (W <= EDT_LDS_W) {                                  // the on-chip form: blocks of EDT_LANES rows, g copied in, both arrays [column][lane]
        for (int y0 = 0; y0 < H; y0 += EDT_LANES) {
            std::vector<uint16_t> lgs((size_t)W * EDT_LANES, 0xABCD);      // exactly the kernel's extent for this W: an index past it is caught
            std::vector<uint32_t> lst((size_t)W * EDT_LANES, 0xDEADBEEF);
            for (int lane = 0; lane < EDT_LANES && y0 + lane < H; lane++) {
                const int y = y0 + lane;
                for (int k = 0; k < W; k++) lgs.at((size_t)k * EDT_LANES + lane) = gT.at((size_t)k * R + y);
                edt_row_pass(EdtLaned<uint16_t>{lgs.data() + lane}, EdtLaned<uint32_t>{lst.data() + lane}, Vec32{out.data() + (size_t)y * W}, W, limit);
            }
        }
        return out;
    }
    for (int y = 0; y < H; y++)
        edt_row_pass(EdtStrided<uint16_t>{gT.data() + y, R}, EdtStrided<uint32_t>{st.data() + y, R}, Vec32{out.data() + (size_t)y * W}, W, limit);
    return out;
}

static std::vector<int32_t> brute(const std::vector<uint8_t>& src, const std::vector<uint8_t>& val, int sv, int eq, int inv, int limit, int H,
                                  int W) {
    std::vector<int> sy, sx;
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            const size_t o = (size_t)y * W + x;
            const bool valid = val.empty() || val[o] != inv;
            if (valid && ((src[o] == sv) == (eq != 0))) { sy.push_back(y); sx.push_back(x); }
        }
    std::vector<int32_t> out((size_t)H * W);
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++) {
            long long best = limit;
            for (size_t k = 0; k < sy.size(); k++) {
                const long long dy = y - sy[k], dx = x - sx[k], v = dy * dy + dx * dx;
                if (v < best) best = v;
            }
            out[(size_t)y * W + x] = (int32_t)best;
        }
    return out;
}

int main() {
    const int shapes[][2] = {{1, 1}, {1, 5}, {5, 1}, {7, 13}, {33, 65}, {8, 9}, {64, 128}, {65, 129}, {67, 93}, {130, 257}};
    const int limits[] = {1, 5, 26, INT_MAX};
    int bad = 0, n = 0;
    for (auto& s : shapes)
        for (int kind = 0; kind <= 13; kind++)
            for (int eq = 0; eq <= 1; eq++)
                for (int wv = 0; wv <= 1; wv++) {
                    const int H = s[0], W = s[1], limit = limits[(kind + eq + wv) % 4];
                    const auto f = pattern(kind, H, W);
                    std::vector<uint8_t> val;
                    if (wv) { val.resize(f.size()); for (auto& v : val) v = rnd() < 0.1 ? 255 : 0; }
                    const auto want = brute(f, val, 1, eq, 255, limit, H, W), got = separable(f, val, 1, eq, 255, limit, H, W);
                    n++;
                    if (memcmp(want.data(), got.data(), want.size() * sizeof(int32_t))) {
                        printf("MISMATCH %d x %d pattern %d site_equal %d valid %d limit %d\n", H, W, kind, eq, wv, limit);
                        bad++;
                    }
                }
    {   // the extremes of the integer range: one site in a corner of the largest row and column the transform takes
        const int L = EDT_MAX_DIM;
        for (int t = 0; t < 2; t++) {
            const int H = t ? L : 1, W = t ? 1 : L;
            std::vector<uint8_t> f((size_t)H * W, 0), val; f[0] = 1;
            const auto got = separable(f, val, 1, 1, 0, INT_MAX, H, W);
            n++;
            for (int i = 0; i < L; i++) if (got[i] != (long long)i * i) { printf("MISMATCH extreme %d at %d\n", t, i); bad++; break; }
        }
        // two far columns with g near the top of its range: the envelope's numerator and products stay inside int32
        const int W = 4000;
        std::vector<uint16_t> g(W, (uint16_t)EDT_INF); std::vector<uint32_t> st(W); std::vector<int32_t> out(W);
        g[0] = 32766; g[W - 1] = 32765; g[W / 2] = 32760;
        std::vector<uint16_t> g0 = g;
        edt_row_pass(EdtStrided<uint16_t>{g.data(), 1}, EdtStrided<uint32_t>{st.data(), 1}, Vec32{out.data()}, W, INT_MAX);
        n++;
        for (int x = 0; x < W; x++) {
            long long best = INT_MAX;
            for (int k = 0; k < W; k++) if (g0[k] != EDT_INF) { const long long v = (long long)(x - k) * (x - k) + (long long)g0[k] * g0[k]; if (v < best) best = v; }
            if (out[x] != best) { printf("MISMATCH tall columns at %d\n", x); bad++; break; }
        }
    }
    {   // the boundary test against its definition: valid & fg & ~erosion(fg | ~valid, cross, border = 1)
        for (int kind = 0; kind <= 13; kind++) {
            const int H = 9, W = 11;
            const auto f = pattern(kind, H, W);
            std::vector<uint8_t> inv((size_t)H * W);
            for (auto& v : inv) v = rnd() < 0.2;
            n++;
            for (int y = 0; y < H; y++)
                for (int x = 0; x < W; x++) {
                    auto a = [&](int yy, int xx) { return yy < 0 || yy >= H || xx < 0 || xx >= W ? true : (f[(size_t)yy * W + xx] == 1 || inv[(size_t)yy * W + xx] != 0); };
                    auto open = [&](int yy, int xx) { return !(yy < 0 || yy >= H || xx < 0 || xx >= W) && !inv[(size_t)yy * W + xx] && f[(size_t)yy * W + xx] != 1; };
                    const bool eroded = a(y, x) && a(y - 1, x) && a(y + 1, x) && a(y, x - 1) && a(y, x + 1);
                    const bool want = !inv[(size_t)y * W + x] && f[(size_t)y * W + x] == 1 && !eroded;
                    const bool got = edt_on_boundary(!inv[(size_t)y * W + x], f[(size_t)y * W + x] == 1, open(y - 1, x), open(y + 1, x), open(y, x - 1), open(y, x + 1));
                    if (want != got) { printf("MISMATCH boundary pattern %d at %d,%d\n", kind, y, x); bad++; }
                }
        }
    }
    printf("%d cases, %d bad\n", n, bad);
    return bad != 0;
}
