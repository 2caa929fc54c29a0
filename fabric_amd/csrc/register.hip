// Co-registration of the two dates of a scene: the shift search (bdn_shift_corr: per band, cell and integer shift the six sums of the
// normalised cross-correlation, in double), the peak and the shift field (bdn_shift_peak) and the resampling of date 2 through the field
// (bdn_shift_apply).  include/bidate_hip.h states the semantics and the exact operation order; tests/register_ref.py restates them in numpy.
//
// bdn_shift_corr, two launches whatever the data:
//   corr      grid (P * cells, bands), 256 threads.  Block (p, cell, band) walks its share (T / P, the first T % P partials one more) of the
//             cell's T 32 x 32 tiles in raster order.  Per tile it stages the date-1 tile and the date-2 tile with its halo of R in LDS (20.3 KiB static),
//             an excluded, non-finite or out-of-scene pixel as NaN; thread t owns shifts t, t + 256, ... (NS <= 5 of the (2R + 1)^2) and keeps
//             their count and five double sums in registers.  The date-1 value is one LDS address for the whole block (a broadcast); the
//             date-2 row stride is 33 + 2R = 2R + 1 (mod 32), so the 32 lanes of a half wave, which own consecutive shifts, read consecutive
//             banks across the row breaks of the shift window: no bank conflict.  a, b are float32, so a * a, b * b and a * b are exact in
//             double and fma(a, b, acc) rounds the exact sum once: every term is exact, every sum has one rounding per term.
//   finish    table[band][cell][shift][k] = the P partials added in index order.
// ws: double [bands][cells][P][(2R + 1)^2][6]; P = rg_partials(bands, shifts, cells) does not depend on H or W.  Every word read was written by the same call.
// bdn_shift_peak, one launch: block c < cells scores cell c, block `cells` the whole scene (the cells' tables added in (i, j) order); a cell
//   that falls back to the whole-scene shift (not ok, or ncc < min_ncc) computes the whole-scene peak itself, in the same order and so to
//   the same bits: no block waits for another.
// bdn_shift_apply, one launch: one thread per pixel, the channels in a loop.
#include "common.hpp"
#include <float.h>
#include <math.h>

constexpr int RG_T = 32;                                     // tile side of date 1
constexpr int RG_MAXR = 16, RG_MAXCELLS = 64, RG_MAXBANDS = 64, RG_MAXDIM = 32767, RG_MAXC = 65535;
constexpr int RG_BH = RG_T + 2 * RG_MAXR, RG_BW = RG_T + 2 * RG_MAXR + 1;          // date-2 tile with halo: rows, padded row stride

// partial accumulators per (band, cell): cells * P <= 1024 blocks per band fill the device for a coarse grid, a fine grid takes one; capped so
// that the workspace (P tables) stays within 256 MiB wherever one table does.  Never a function of H, W.
static inline int rg_partials(int n_b, int S2, int cells) {
    const size_t table = sizeof(double) * 6 * (size_t)S2 * (size_t)cells * (size_t)n_b;
    size_t p = 1024 / (size_t)cells, cap = ((size_t)256 << 20) / table;
    if (p > cap) p = cap;
    return p < 1 ? 1 : (int)p;
}
__host__ __device__ static inline int rg_cell_lo(int i, int n, int extent) { return (int)((long long)i * extent / n); }

static bool rg_grid_ok(int H, int W, int ny, int nx) {
    return H >= 1 && W >= 1 && H <= RG_MAXDIM && W <= RG_MAXDIM && ny >= 1 && nx >= 1 && ny <= RG_MAXCELLS && nx <= RG_MAXCELLS && ny <= H && nx <= W;
}

// one rounding per operation (the caller's contraction is not inherited): what numpy float64 / float32 does
__device__ __forceinline__ double rg_dmul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double rg_dsub(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double rg_dadd(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float rg_fmul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float rg_fadd(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float rg_fsub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// ---------------------------------------------------------------- the correlation table
__device__ __forceinline__ float rg_clean(const float* __restrict__ plane, const uint8_t* __restrict__ excl, int exv, size_t idx) {
    const float v = plane[idx];
    if (excl && excl[idx] == exv) return NAN;
    return fabsf(v) <= FLT_MAX ? v : NAN;                    // NaN and +-inf leave the sums
}

template <int NS>
__global__ __launch_bounds__(256) void shift_corr_kernel(const float* __restrict__ d1, const float* __restrict__ d2,
                                                         const int32_t* __restrict__ bands, const uint8_t* __restrict__ excl, int exv,
                                                         double* __restrict__ part, int C, int H, int W, int R, int ny, int nx, int P) {
    __shared__ float sA[RG_T * RG_T];
    __shared__ float sB[RG_BH * RG_BW];
    const int tid = threadIdx.x;
    const int S = 2 * R + 1, S2 = S * S, BW = RG_T + 2 * R + 1;
    const int cells = ny * nx, p = blockIdx.x / cells, cell = blockIdx.x - p * cells;      // p-major: see the tile split below
    const int ci = cell / nx, cj = cell - ci * nx;
    const int r0 = rg_cell_lo(ci, ny, H), r1 = rg_cell_lo(ci + 1, ny, H), c0 = rg_cell_lo(cj, nx, W), c1 = rg_cell_lo(cj + 1, nx, W);
    const int tiles_x = (c1 - c0 + RG_T - 1) / RG_T, tiles_y = (r1 - r0 + RG_T - 1) / RG_T, T = tiles_x * tiles_y;
    // partial p takes T / P tiles, the first T % P partials one more: with T < P the busy blocks are blocks 0 .. T cells - 1 of the grid,
    // consecutive, so the hardware's round-robin over the XCDs spreads them evenly (busy blocks at a stride of P / T landed on 2 XCDs of 8)
    const int tq = T / P, tr = T - tq * P;
    const int t_lo = p * tq + min(p, tr), t_hi = t_lo + tq + (p < tr ? 1 : 0);
    const int band = bands[blockIdx.y];
    const bool band_ok = band >= 0 && band < C;              // an index outside the stack reads nothing: its table is all zero
    const size_t plane = (size_t)(band_ok ? band : 0) * H * W;
    const float* a_pl = d1 + plane;
    const float* b_pl = d2 + plane;

    int off[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) {
        const int s = tid + 256 * k, sc = s < S2 ? s : 0;    // a thread without a shift follows shift 0 and writes nothing
        off[k] = (sc / S) * BW + sc % S;
    }
    double acc[NS][5];
    unsigned cnt[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) { cnt[k] = 0; for (int q = 0; q < 5; q++) acc[k][q] = 0.0; }

    for (int t = t_lo; t < t_hi; t++) {
        const int ty = t / tiles_x, tx = t - ty * tiles_x;
        const int y0 = r0 + ty * RG_T, x0 = c0 + tx * RG_T;
        const int th = min(RG_T, r1 - y0), tw = min(RG_T, c1 - x0);
        __syncthreads();                                     // the previous tile has been read
        for (int e = tid; e < RG_T * RG_T; e += 256) {
            const int ly = e / RG_T, lx = e % RG_T;
            float v = NAN;
            if (ly < th && lx < tw && band_ok) v = rg_clean(a_pl, excl, exv, (size_t)(y0 + ly) * W + (x0 + lx));
            sA[e] = v;
        }
        const int bh = th + 2 * R, bw = tw + 2 * R;
        for (int e = tid; e < bh * BW; e += 256) {            // bh * BW <= RG_BH * RG_BW
            const int ly = e / BW, lx = e - ly * BW;
            const int gy = y0 - R + ly, gx = x0 - R + lx;
            float v = NAN;
            if (lx < bw && gy >= 0 && gy < H && gx >= 0 && gx < W && band_ok) v = rg_clean(b_pl, excl, exv, (size_t)gy * W + gx);
            sB[e] = v;
        }
        __syncthreads();
        for (int ly = 0; ly < th; ly++) {
            for (int lx = 0; lx < tw; lx++) {
                const float a = sA[ly * RG_T + lx];
                if (a != a) continue;                        // (uniform: one address for the block)
                const double da = (double)a, daa = da * da;
                const float* bp = sB + ly * BW + lx;         // off[k] <= 2R BW + 2R: the last read is (th - 1 + 2R) BW + tw - 1 + 2R < bh BW
#pragma unroll
                for (int k = 0; k < NS; k++) {
                    const float b = bp[off[k]];
                    const bool m = b == b;
                    const double db = m ? (double)b : 0.0, am = m ? da : 0.0, aam = m ? daa : 0.0;
                    cnt[k] += m ? 1u : 0u;
                    acc[k][0] += am;
                    acc[k][1] += db;
                    acc[k][2] += aam;
                    acc[k][3] = fma(db, db, acc[k][3]);
                    acc[k][4] = fma(am, db, acc[k][4]);
                }
            }
        }
    }
    double* o = part + ((((size_t)blockIdx.y * cells + cell) * P + p) * S2) * 6;       // [band][cell][p][shift][6]
#pragma unroll
    for (int k = 0; k < NS; k++) {
        const int s = tid + 256 * k;
        if (s < S2) {
            double* e = o + (size_t)s * 6;
            e[0] = (double)cnt[k];
#pragma unroll
            for (int q = 0; q < 5; q++) e[1 + q] = acc[k][q];
        }
    }
}

__global__ __launch_bounds__(256) void shift_corr_finish_kernel(const double* __restrict__ part, double* __restrict__ table,
                                                                long long total, int row, int P) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long bc = i / row; const int r = (int)(i - bc * row);
    const double* q = part + (size_t)bc * P * row + r;
    double s = 0.0;
    int p = 0;
    for (; p + 16 <= P; p += 16) {                           // sixteen loads in flight, then their additions in index order
        double v[16];
#pragma unroll
        for (int k = 0; k < 16; k++) v[k] = q[(size_t)(p + k) * row];
#pragma unroll
        for (int k = 0; k < 16; k++) s = rg_dadd(s, v[k]);
    }
    for (; p < P; p++) s = rg_dadd(s, q[(size_t)p * row]);
    table[i] = s;
}

extern "C" size_t bdn_shift_corr_workspace_bytes(int n_b, int H, int W, int R, int ny, int nx) {
    if (n_b < 1 || n_b > RG_MAXBANDS || R < 1 || R > RG_MAXR || !rg_grid_ok(H, W, ny, nx)) return 0;
    const size_t S = 2 * (size_t)R + 1, cells = (size_t)ny * nx;
    return sizeof(double) * 6 * S * S * cells * (size_t)rg_partials(n_b, (int)(S * S), (int)cells) * (size_t)n_b;
}

extern "C" int bdn_shift_corr(const float* d1, const float* d2, const int32_t* bands, int n_b, const uint8_t* exclude, int exclude_value,
                              int R, int ny, int nx, double* table, void* ws, int C, int H, int W, void* stream) {
    if (!d1 || !d2 || !bands || !table || !ws) BDN_FAIL(BDN_E_ARG, "shift_corr: null pointer");
    if (n_b < 1 || n_b > RG_MAXBANDS) BDN_FAIL(BDN_E_ARG, "shift_corr: n_b=%d band indices (1..%d)", n_b, RG_MAXBANDS);
    if (R < 1 || R > RG_MAXR) BDN_FAIL(BDN_E_ARG, "shift_corr: search radius R=%d (1..%d)", R, RG_MAXR);
    if (C < 1 || C > RG_MAXC) BDN_FAIL(BDN_E_ARG, "shift_corr: C=%d channels (1..%d)", C, RG_MAXC);
    if (!rg_grid_ok(H, W, ny, nx))
        BDN_FAIL(BDN_E_ARG, "shift_corr: bad grid %d x %d on a %d x %d scene (1 <= H, W <= %d; 1 <= ny <= min(%d, H), nx alike)", ny, nx, H, W,
                 RG_MAXDIM, RG_MAXCELLS);
    if (exclude && (exclude_value < 0 || exclude_value > 255)) BDN_FAIL(BDN_E_ARG, "shift_corr: exclude_value=%d must be a byte value (0..255)", exclude_value);
    if (((uintptr_t)d1 & 3) || ((uintptr_t)d2 & 3) || ((uintptr_t)bands & 3) || ((uintptr_t)table & 7) || ((uintptr_t)ws & 15))
        BDN_FAIL(BDN_E_ARG, "shift_corr: d1, d2 and bands must be 4-byte aligned, table 8-byte and ws 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int S2 = (2 * R + 1) * (2 * R + 1), cells = ny * nx, P = rg_partials(n_b, S2, cells), NS = (S2 + 255) / 256;
    const dim3 grid((unsigned)(cells * P), (unsigned)n_b);
    double* part = (double*)ws;
#define RG_LAUNCH(ns) hipLaunchKernelGGL(shift_corr_kernel<ns>, grid, dim3(256), 0, st, d1, d2, bands, exclude, exclude_value, part, C, H, W, R, ny, nx, P)
    switch (NS) {
        case 1: RG_LAUNCH(1); break;
        case 2: RG_LAUNCH(2); break;
        case 3: RG_LAUNCH(3); break;
        case 4: RG_LAUNCH(4); break;
        default: RG_LAUNCH(5); break;                         // R = 16: 1089 shifts
    }
#undef RG_LAUNCH
    BDN_CHECK_LAUNCH("shift_corr");
    const int row = S2 * 6;
    const long long total = (long long)n_b * cells * row;    // <= 64 * 4096 * 1089 * 6 < 2^31
    hipLaunchKernelGGL(shift_corr_finish_kernel, dim3(grid_for((size_t)total)), dim3(256), 0, st, part, table, total, row, P);
    BDN_CHECK_LAUNCH("shift_corr_finish");
    return BDN_OK;
}

// ---------------------------------------------------------------- the peak and the field
struct RgPeak { double dy, dx, ncc; int ok; };

// sc[s] = the mean NCC of the bands at shift s of cell `cell` (cell == cells: the whole scene), -2 where no band is defined
__device__ void rg_scores(const double* __restrict__ table, int n_b, int cells, int S2, int cell, double* sc) {
    for (int s = threadIdx.x; s < S2; s += blockDim.x) {
        double acc = 0.0; int cnt = 0;
        for (int b = 0; b < n_b; b++) {
            double v[6];
            if (cell < cells) {
                const double* e = table + (((size_t)b * cells + cell) * S2 + s) * 6;
#pragma unroll
                for (int k = 0; k < 6; k++) v[k] = e[k];
            } else {
#pragma unroll
                for (int k = 0; k < 6; k++) v[k] = 0.0;
                for (int c = 0; c < cells; c++) {
                    const double* e = table + (((size_t)b * cells + c) * S2 + s) * 6;
#pragma unroll
                    for (int k = 0; k < 6; k++) v[k] = rg_dadd(v[k], e[k]);
                }
            }
            const double n = v[0], sa = v[1], sb = v[2], saa = v[3], sbb = v[4], sab = v[5];
            const double va = rg_dsub(rg_dmul(n, saa), rg_dmul(sa, sa)), vb = rg_dsub(rg_dmul(n, sbb), rg_dmul(sb, sb));
            const double cov = rg_dsub(rg_dmul(n, sab), rg_dmul(sa, sb));
            if (n >= 2.0 && va > 0.0 && vb > 0.0) {
                acc = rg_dadd(acc, __ddiv_rn(cov, __dsqrt_rn(rg_dmul(va, vb))));
                cnt++;
            }
        }
        sc[s] = cnt > 0 ? __ddiv_rn(acc, (double)cnt) : -2.0;
    }
}

__device__ double rg_parabola(double cm, double c0, double cp, bool border) {
    if (border || cm == -2.0 || cp == -2.0) return 0.0;
    const double den = rg_dadd(rg_dsub(cm, rg_dmul(2.0, c0)), cp);
    if (!(den < 0.0)) return 0.0;
    const double d = __ddiv_rn(rg_dmul(0.5, rg_dsub(cm, cp)), den);
    return fmin(fmax(d, -0.5), 0.5);
}

__device__ RgPeak rg_peak(const double* sc, int R) {        // one thread: the first maximum in raster order, then the two parabolas
    const int S = 2 * R + 1, S2 = S * S;
    int best = 0;
    for (int s = 1; s < S2; s++) if (sc[s] > sc[best]) best = s;
    RgPeak r;
    r.ncc = sc[best];
    r.ok = r.ncc > -2.0 ? 1 : 0;
    r.dy = 0.0; r.dx = 0.0;
    if (r.ok) {
        const int py = best / S, px = best - py * S;
        const bool by = py == 0 || py == S - 1, bx = px == 0 || px == S - 1;
        r.dy = rg_dadd((double)(py - R), rg_parabola(by ? 0.0 : sc[best - S], sc[best], by ? 0.0 : sc[best + S], by));
        r.dx = rg_dadd((double)(px - R), rg_parabola(bx ? 0.0 : sc[best - 1], sc[best], bx ? 0.0 : sc[best + 1], bx));
    }
    return r;
}

__global__ __launch_bounds__(256) void shift_peak_kernel(const double* __restrict__ table, int n_b, int R, int ny, int nx, double min_ncc,
                                                         double* __restrict__ report, float* __restrict__ field) {
    __shared__ double sc[(2 * RG_MAXR + 1) * (2 * RG_MAXR + 1)];
    __shared__ RgPeak pk[2];
    const int cells = ny * nx, cell = blockIdx.x, S2 = (2 * R + 1) * (2 * R + 1);
    rg_scores(table, n_b, cells, S2, cell, sc);
    __syncthreads();
    if (threadIdx.x == 0) pk[0] = rg_peak(sc, R);
    __syncthreads();
    const RgPeak own = pk[0];
    if (cell == cells) {
        if (threadIdx.x == 0) { double* e = report + 4 * (size_t)cell; e[0] = own.dy; e[1] = own.dx; e[2] = own.ncc; e[3] = (double)own.ok; }
        return;
    }
    const bool fallback = !own.ok || own.ncc < min_ncc;       // (uniform)
    if (fallback) {                                          // the whole-scene peak, formed as block `cells` forms it
        rg_scores(table, n_b, cells, S2, cells, sc);          // (every thread passed the barrier above: pk[0] has been read)
        __syncthreads();
        if (threadIdx.x == 0) pk[1] = rg_peak(sc, R);
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* e = report + 4 * (size_t)cell;
        e[0] = own.dy; e[1] = own.dx; e[2] = own.ncc; e[3] = (double)own.ok;
        double fy = own.dy, fx = own.dx;
        if (fallback) { fy = pk[1].ok ? pk[1].dy : 0.0; fx = pk[1].ok ? pk[1].dx : 0.0; }
        field[2 * (size_t)cell] = (float)fy;
        field[2 * (size_t)cell + 1] = (float)fx;
    }
}

extern "C" int bdn_shift_peak(const double* table, int n_b, int R, int ny, int nx, double min_ncc, double* report, float* field, void* stream) {
    if (!table || !report || !field) BDN_FAIL(BDN_E_ARG, "shift_peak: null pointer");
    if (n_b < 1 || n_b > RG_MAXBANDS) BDN_FAIL(BDN_E_ARG, "shift_peak: n_b=%d bands (1..%d)", n_b, RG_MAXBANDS);
    if (R < 1 || R > RG_MAXR) BDN_FAIL(BDN_E_ARG, "shift_peak: search radius R=%d (1..%d)", R, RG_MAXR);
    if (ny < 1 || nx < 1 || ny > RG_MAXCELLS || nx > RG_MAXCELLS) BDN_FAIL(BDN_E_ARG, "shift_peak: bad grid %d x %d (1..%d each)", ny, nx, RG_MAXCELLS);
    if (min_ncc != min_ncc) BDN_FAIL(BDN_E_ARG, "shift_peak: min_ncc is NaN");
    if (((uintptr_t)table & 7) || ((uintptr_t)report & 7) || ((uintptr_t)field & 3))
        BDN_FAIL(BDN_E_ARG, "shift_peak: table and report must be 8-byte aligned, field 4-byte aligned");
    hipLaunchKernelGGL(shift_peak_kernel, dim3((unsigned)(ny * nx + 1)), dim3(256), 0, (hipStream_t)stream, table, n_b, R, ny, nx, min_ncc,
                       report, field);
    BDN_CHECK_LAUNCH("shift_peak");
    return BDN_OK;
}

// ---------------------------------------------------------------- resampling through the field
// the field along one axis at pixel q of `extent`, cells n: the two cells whose centres bracket q and the weight of the second
__device__ __forceinline__ void rg_axis(int q, int extent, int n, int& i0, int& i1, float& t) {
    if (n == 1) { i0 = i1 = 0; t = 0.f; return; }
    int i = (int)((((long long)q + 1) * n - 1) / extent);     // the cell that owns q
    auto centre = [&](int k) { return rg_fmul(0.5f, (float)(rg_cell_lo(k, n, extent) + rg_cell_lo(k + 1, n, extent) - 1)); };      // exact
    const float qf = (float)q;
    if (centre(i) > qf) i--;                                 // the last centre <= q
    i0 = min(max(i, 0), n - 2); i1 = i0 + 1;
    const float ca = centre(i0), cb = centre(i1);
    t = fminf(fmaxf(__fdiv_rn(rg_fsub(qf, ca), rg_fsub(cb, ca)), 0.f), 1.f);
}
__device__ __forceinline__ float rg_lerp2(float tx, float ty, float v00, float v01, float v10, float v11) {
    const float gx = rg_fsub(1.f, tx), gy = rg_fsub(1.f, ty);
    const float top = rg_fadd(rg_fmul(gx, v00), rg_fmul(tx, v01)), bot = rg_fadd(rg_fmul(gx, v10), rg_fmul(tx, v11));
    return rg_fadd(rg_fmul(gy, top), rg_fmul(ty, bot));
}
__device__ __forceinline__ int rg_tap(float f) { return (int)fminf(fmaxf(f, -1073741824.f), 1073741824.f); }      // floorf's value as an int, saturated

__global__ __launch_bounds__(256) void shift_apply_kernel(const float* __restrict__ src, const float* __restrict__ field, int ny, int nx,
                                                          float* __restrict__ out, uint8_t* __restrict__ oob, int C, int H, int W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    int i0, i1, j0, j1; float ty, tx;
    rg_axis(y, H, ny, i0, i1, ty);
    rg_axis(x, W, nx, j0, j1, tx);
    const float* f00 = field + 2 * ((size_t)i0 * nx + j0); const float* f01 = field + 2 * ((size_t)i0 * nx + j1);
    const float* f10 = field + 2 * ((size_t)i1 * nx + j0); const float* f11 = field + 2 * ((size_t)i1 * nx + j1);
    const float sy = rg_lerp2(tx, ty, f00[0], f01[0], f10[0], f11[0]), sx = rg_lerp2(tx, ty, f00[1], f01[1], f10[1], f11[1]);
    const float yy = rg_fadd((float)y, sy), xx = rg_fadd((float)x, sx);
    const float yf = floorf(yy), xf = floorf(xx);
    const float fy = rg_fsub(yy, yf), fx = rg_fsub(xx, xf);
    const int iy = rg_tap(yf), ix = rg_tap(xf);
    const int ya = min(max(iy, 0), H - 1), yb = min(max(iy + 1, 0), H - 1), xa = min(max(ix, 0), W - 1), xb = min(max(ix + 1, 0), W - 1);
    if (oob) {                                               // a tap of weight 0 (fy == 0: the lower row; fx == 0: the right column) does not count
        const bool in_y = iy >= 0 && (fy > 0.f ? iy + 1 : iy) <= H - 1, in_x = ix >= 0 && (fx > 0.f ? ix + 1 : ix) <= W - 1;
        oob[i] = (in_y && in_x) ? 0 : 1;
    }
    const size_t o00 = (size_t)ya * W + xa, o01 = (size_t)ya * W + xb, o10 = (size_t)yb * W + xa, o11 = (size_t)yb * W + xb;
    const size_t hw = (size_t)H * W;
    for (int c = 0; c < C; c++) {
        const float* s = src + (size_t)c * hw;
        out[(size_t)c * hw + (size_t)i] = rg_lerp2(fx, fy, s[o00], s[o01], s[o10], s[o11]);
    }
}

extern "C" int bdn_shift_apply(const float* src, const float* field, int ny, int nx, float* out, uint8_t* oob, int C, int H, int W, void* stream) {
    if (!src || !field || !out) BDN_FAIL(BDN_E_ARG, "shift_apply: null pointer");
    if (out == src) BDN_FAIL(BDN_E_ARG, "shift_apply: out == src (every output pixel reads four source pixels)");
    if (C < 1 || C > RG_MAXC) BDN_FAIL(BDN_E_ARG, "shift_apply: C=%d channels (1..%d)", C, RG_MAXC);
    if (!rg_grid_ok(H, W, ny, nx))
        BDN_FAIL(BDN_E_ARG, "shift_apply: bad grid %d x %d on a %d x %d scene (1 <= H, W <= %d; 1 <= ny <= min(%d, H), nx alike)", ny, nx, H, W,
                 RG_MAXDIM, RG_MAXCELLS);
    if (((uintptr_t)src & 3) || ((uintptr_t)out & 3) || ((uintptr_t)field & 3)) BDN_FAIL(BDN_E_ARG, "shift_apply: src, out and field must be 4-byte aligned");
    hipLaunchKernelGGL(shift_apply_kernel, dim3(grid_for((size_t)H * W)), dim3(256), 0, (hipStream_t)stream, src, field, ny, nx, out, oob, C, H, W);
    BDN_CHECK_LAUNCH("shift_apply");
    return BDN_OK;
}
