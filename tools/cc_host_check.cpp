// Stand-alone host check of fabric_amd/csrc/cc_core.hpp: the tile / seam / flatten decomposition of cc.hip run serially (a plain minimum in
// place of the atomicMin) over a pattern set, against a flood fill.  No GPU, no library.  Meant for a sanitizer build:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/cc_host_check.cpp -o /tmp/cc_host_check && /tmp/cc_host_check
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../fabric_amd/csrc/cc_core.hpp"

struct SerialPar {
    std::vector<int>& p;
    int load(int i) const { return p.at(i); }
    int fetch_min(int i, int v) { const int old = p.at(i); if (v < old) p.at(i) = v; return old; }
};

static std::vector<int> flood(const std::vector<uint8_t>& fg, int H, int W, int conn) {
    std::vector<int> lab((size_t)H * W, 0), stack;
    for (int s = 0; s < H * W; s++) {
        if (!fg[s] || lab[s]) continue;
        lab[s] = s + 1; stack.push_back(s);
        while (!stack.empty()) {
            const int i = stack.back(); stack.pop_back();
            const int y = i / W, x = i % W;
            for (int dy = -1; dy <= 1; dy++)
                for (int dx = -1; dx <= 1; dx++) {
                    if ((!dy && !dx) || (conn == 4 && dy && dx)) continue;
                    const int yy = y + dy, xx = x + dx;
                    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
                    const int j = yy * W + xx;
                    if (fg[j] && !lab[j]) { lab[j] = s + 1; stack.push_back(j); }
                }
        }
    }
    return lab;
}

static int g_status;

static std::vector<int> tiled(const std::vector<uint8_t>& fg, int H, int W, int conn) {
    const int T = CC_TILE, ty_n = (H + T - 1) / T, tx_n = (W + T - 1) / T;
    std::vector<int> parent((size_t)H * W, -2);
    for (int ty = 0; ty < ty_n; ty++)
        for (int tx = 0; tx < tx_n; tx++) {
            const int y0 = ty * T, x0 = tx * T;
            uint64_t rows[CC_TILE];
            std::vector<int> lp(T * T);
            for (int r = 0; r < T; r++) {
                rows[r] = 0;
                for (int c = 0; c < T; c++)
                    if (y0 + r < H && x0 + c < W && fg[(size_t)(y0 + r) * W + x0 + c]) rows[r] |= 1ull << c;
                for (int c = 0; c < T; c++) lp[r * T + c] = r * T + ((rows[r] >> c & 1) ? cc_run_start(rows[r], c) : c);
            }
            SerialPar par{lp};
            for (int r = T - 1; r >= 1; r--)               // any order must do: bottom-up and right-to-left here
                for (int c = T - 1; c >= 0; c--) {
                    const int links = cc_links(rows[r], rows[r - 1], c, T, conn);
                    for (int d = 0; d < 3; d++)
                        if (links >> d & 1)
                            cc_union(par, r * T + cc_run_start(rows[r], c), (r - 1) * T + cc_run_start(rows[r - 1], c + d - 1), T * T, &g_status);
                }
            for (int r = 0; r < T && y0 + r < H; r++)
                for (int c = 0; c < T && x0 + c < W; c++) {
                    int g = -1;
                    if (rows[r] >> c & 1) { const int root = cc_find(par, r * T + c, T * T, &g_status); g = (y0 + (root >> 6)) * W + x0 + (root & 63); }
                    parent[(size_t)(y0 + r) * W + x0 + c] = g;
                }
        }
    SerialPar par{parent};
    const long long n_h = (long long)(ty_n - 1) * W, total = n_h + (long long)(tx_n - 1) * H;
    for (long long i = total - 1; i >= 0; i--) {
        int y, x, dy, dx, lim, pos;
        if (i < n_h) { const int s = (int)(i / W); x = (int)(i - (long long)s * W); y = (s + 1) * T; dy = 0; dx = 1; lim = W; pos = x; }
        else { const long long j = i - n_h; const int s = (int)(j / H); y = (int)(j - (long long)s * H); x = (s + 1) * T; dy = 1; dx = 0; lim = H; pos = y; }
        const int cur = y * W + x;
        if (par.load(cur) < 0) continue;
        const int oy = y - dx, ox = x - dy;
        unsigned m = 2, mu = 0;
        for (int d = -1; d <= 1; d++) {
            if (pos + d < 0 || pos + d >= lim) continue;
            if (d && (pos + d) / CC_TILE == pos / CC_TILE && par.load((y + d * dy) * W + x + d * dx) >= 0) m |= 1u << (d + 1);
            if (par.load((oy + d * dy) * W + ox + d * dx) >= 0) mu |= 1u << (d + 1);
        }
        const int links = cc_links(m, mu, 1, 3, conn);
        for (int d = 0; d < 3; d++)
            if (links >> d & 1) cc_union(par, cur, (oy + (d - 1) * dy) * W + ox + (d - 1) * dx, H * W, &g_status);
    }
    std::vector<int> lab((size_t)H * W);
    for (int i = 0; i < H * W; i++) lab[i] = parent[i] < 0 ? 0 : 1 + cc_find(par, parent[i], H * W, &g_status);
    return lab;
}

static unsigned long long g_rng = 88172645463325252ull;
static double rnd() { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (g_rng >> 11) * (1.0 / 9007199254740992.0); }

static std::vector<uint8_t> pattern(int kind, int H, int W) {
    std::vector<uint8_t> f((size_t)H * W, 0);
    auto at = [&](int y, int x) -> uint8_t& { return f[(size_t)y * W + x]; };
    const double dens[] = {0.1, 0.5, 0.593, 0.9};
    for (int y = 0; y < H; y++)
        for (int x = 0; x < W; x++)
            switch (kind) {
                case 0: break;
                case 1: at(y, x) = 1; break;
                case 2: case 3: case 4: case 5: at(y, x) = rnd() < dens[kind - 2]; break;
                case 6: at(y, x) = (y + x) & 1; break;
                case 7: at(y, x) = y % W == x || (y + 3) % W == W - 1 - x; break;
                case 8: at(y, x) = (y % 2 == 0) || (((y / 2) % 2 == 0) ? x == W - 1 : x == 0); break;          // serpentine
                case 9: at(y, x) = y % 2 == 0; break;
                case 10: at(y, x) = x % 2 == 0; break;
            }
    if (kind == 11) {                                      // rectangular spiral, one pixel wide, one pixel apart
        int t = 0, b = H - 1, l = 0, r = W - 1, y = 0, x = 0;
        while (t <= b && l <= r) {
            for (x = l; x <= r; x++) at(t, x) = 1;
            for (y = t; y <= b; y++) at(y, r) = 1;
            if (b - t >= 2) for (x = r; x >= l + 2; x--) at(b, x) = 1;
            if (r - l >= 2 && b - t >= 2) for (y = b; y >= t + 2; y--) at(y, l + 2 <= r ? l + 2 : r) = 1;
            t += 2; b -= 2; l += 2; r -= 2;
            if (t <= b && l <= r) at(t, l) = 1;
        }
    }
    if (kind == 12 && H >= 3 && W >= 3) {                  // minimum in the last column, reaching back to column 0 on a lower row
        at(0, W - 1) = 1; at(1, W - 1) = 1;
        for (int x = 0; x < W; x++) at(2, x) = 1;
    }
    if (kind == 13 && H > CC_TILE && W > CC_TILE) { at(CC_TILE - 1, CC_TILE) = 1; at(CC_TILE, CC_TILE - 1) = 1; }      // the four-tile corner
    return f;
}

int main() {
    const int T = CC_TILE;
    const int shapes[][2] = {{1, 1}, {1, 5}, {5, 1}, {7, 13}, {T, T}, {T + 1, T - 1}, {2 * T + 3, 3 * T + 1}, {96, 200}, {517, 1030}};
    int bad = 0, n = 0;
    for (auto& s : shapes)
        for (int kind = 0; kind <= 13; kind++)
            for (int conn = 4; conn <= 8; conn += 4) {
                const int H = s[0], W = s[1];
                const auto f = pattern(kind, H, W);
                g_status = 0;
                const auto want = flood(f, H, W, conn), got = tiled(f, H, W, conn);
                n++;
                if (g_status || memcmp(want.data(), got.data(), want.size() * sizeof(int))) {
                    printf("MISMATCH %d x %d pattern %d connectivity %d status %d\n", H, W, kind, conn, g_status);
                    bad++;
                }
            }
    printf("%d cases, %d bad\n", n, bad);
    return bad != 0;
}
