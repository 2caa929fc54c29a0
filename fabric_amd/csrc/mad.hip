// IR-MAD (iteratively reweighted multivariate alteration detection, Nielsen 2007) between the two dates of a scene: the unweighted centre
// (bdn_mad_centre), the weighted moments up to order two of the 2 n_b centred values of a pixel (bdn_mad_moments), the canonical
// correlation problem on them (bdn_mad_solve), the chi-square statistic with its no-change probability (bdn_mad_chi2) and the
// invariant-pixel mask (bdn_mad_mask).  include/bidate_hip.h states the semantics; tests/mad_ref.py restates them in numpy float64.
//
// bdn_mad_moments, the kernel design (the LDS-tile form, not the f64 matrix-core form): the vector of a pixel is augmented with a constant
// one, v = (z_0 .. z_{D-1}, 1), D = 2 n_b, so that S2, S1 and S0 are the upper triangle of one (D + 1)^2 matrix sum w v v^T.  That matrix is
// cut into 4 x 4 register tiles: T = ceil((D + 1) / 4) tile rows, NT = T (T + 1) / 2 tiles on or above the diagonal (13 bands: 28).  A
// block of 256 threads stages 64 pixels at a time in LDS as doubles (z already centred, w = 0 for an invalid pixel); thread
// (tile, slice g) walks the pixels g, g + G, .. of the staged tile, G = min(64, 256 / NT) slices, with 16 accumulators: per pixel two
// 32-byte LDS reads, four products w z_k and sixteen fused multiply-adds.  A block runs over the tiles blockIdx, blockIdx + grid, ..; at
// its end the slices are added in slice order and the block partial goes to the workspace; a second launch adds the partials in block
// order.  The grid is min(tiles, 768), a function of the shape alone, so every sum is a chain of double additions in an order fixed by
// (n_b, H, W).  The f64 MFMA (v_mfma_f64_16x16x4_f64) would cut the VALU work by four, but with K = pixels it needs the operands laid out
// pixel-major per lane and its own C/D map, and at 13 bands the pass is bound by the staging rather than by the 378 sums (the centre
// pass, which has no products, takes four fifths of its time: DESIGN.md section 25), so the simpler form ships.
// bdn_mad_centre is the same staging with w = 1 and no centre: thread (column, slice) adds one column; the count of valid pixels is the
// augmented column.
// bdn_mad_solve is one wave: lane i owns row i (or column i) of the n_b x n_b blocks in LDS; dot products across lanes are xor-butterfly
// sums, which give every lane the same bits.  One-sided Jacobi (Hestenes) on the columns of K.
#include "common.hpp"
#include <float.h>
#include <math.h>

constexpr int MAD_MAXB = 32, MAD_MAXDIM = 32767, MAD_MAXC = 65535;
constexpr int MAD_P = 64;                                    // pixels of a staged tile
constexpr int MAD_ZSMAX = 68;                                // 2 * 32 + 1, rounded up to a multiple of 4
constexpr int MAD_MAXBLK = 768;                              // three resident blocks on each of 256 compute units
constexpr int MAD_LD = 33;                                   // leading dimension of the solve's LDS blocks (odd: rows on different banks)
constexpr int MAD_SWEEPS = 60;

struct MadDims { int D, T, ZS, NT, NE, G; };
static inline __host__ __device__ MadDims mad_dims(int n_b) {
    MadDims m;
    m.D = 2 * n_b;
    m.T = (m.D + 4) / 4;                                     // ceil((D + 1) / 4)
    m.ZS = 4 * m.T;
    m.NT = m.T * (m.T + 1) / 2;
    m.NE = m.NT * 16;
    m.G = 256 / m.NT > MAD_P ? MAD_P : 256 / m.NT;
    return m;
}
static inline unsigned mad_tiles(int H, int W) { return ((unsigned)H * (unsigned)W + MAD_P - 1) / MAD_P; }
static inline unsigned mad_blocks(int H, int W) { const unsigned t = mad_tiles(H, W); return t < (unsigned)MAD_MAXBLK ? t : (unsigned)MAD_MAXBLK; }
// tile number -> (tile row, tile column), row <= column, rows first
__host__ __device__ __forceinline__ void mad_tile_rc(int pair, int T, int& ti, int& tj) {
    ti = 0;
    int left = pair;
    while (left >= T - ti) { left -= T - ti; ti++; }
    tj = ti + left;
}

struct MadScene { const float* d1; const float* d2; const int32_t* bands; const uint8_t* excl; int exv, n_b, C; unsigned npix; };

// the band list into LDS; false when an index lies outside the stack (then every pixel is invalid and nothing is read)
__device__ __forceinline__ bool mad_stage_bands(const MadScene& s, int* sb) {
    int bad = 0;
    if ((int)threadIdx.x < s.n_b) {
        const int b = s.bands[threadIdx.x];
        sb[threadIdx.x] = b;
        bad = (b < 0 || b >= s.C) ? 1 : 0;
    }
    return !__syncthreads_or(bad);
}

// ---------------------------------------------------------------- centre and moments
struct MadMomArgs { MadScene s; const float* weight; const double* centre; const double* state; double* ws; unsigned ntiles; };

template <bool CENTRE>
__global__ __launch_bounds__(256) void mad_moments_kernel(const MadMomArgs a) {
    __shared__ double zs[MAD_P * MAD_ZSMAX];
    __shared__ double wv[MAD_P];
    __shared__ double cen[2 * MAD_MAXB];
    __shared__ int sb[MAD_MAXB];
    __shared__ int bad[MAD_P];
    if (!CENTRE && a.state && a.state[2] != 0.0) return;     // (uniform) converged: this launch writes nothing
    const int tid = threadIdx.x, n = a.s.n_b;
    const MadDims m = mad_dims(n);
    const bool bands_ok = mad_stage_bands(a.s, sb);
    if (tid < m.D) cen[tid] = CENTRE ? 0.0 : a.centre[tid];
    int ti = 0, tj = 0, g = 0;
    bool worker;
    if (CENTRE) {
        ti = tid % m.ZS; g = tid / m.ZS;                     // ti: the column
        const int gc = 256 / m.ZS > MAD_P ? MAD_P : 256 / m.ZS;
        worker = g < gc;
    } else {
        mad_tile_rc(tid % m.NT, m.T, ti, tj); g = tid / m.NT;
        worker = g < m.G;
    }
    const int G = CENTRE ? (256 / m.ZS > MAD_P ? MAD_P : 256 / m.ZS) : m.G;
    double acc[16];
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.0;
    if (tid < MAD_P) bad[tid] = 0;
    __syncthreads();
    // The values of a tile travel global -> registers -> LDS: thread tid holds pixel tid & 63 of the bands (tid >> 6) + 4 i, and threads
    // 0..63 hold the pixel's exclusion and weight.  The next tile is fetched into the registers before the staged one is walked, so the
    // global latency lies under the arithmetic.
    const int pix = tid & (MAD_P - 1), k0 = tid >> 6;
    float pv[MAD_MAXB / 2];
    int pflag = 0;
    float pw = 1.f;
    auto fetch = [&](unsigned tile) {
        const unsigned p = tile * (unsigned)MAD_P + (unsigned)pix;
        const bool in = bands_ok && p < a.s.npix;
#pragma unroll
        for (int i = 0; i < MAD_MAXB / 2; i++) {
            const int k = k0 + 4 * i;
            pv[i] = (in && k < m.D) ? (k < n ? a.s.d1 : a.s.d2)[(size_t)sb[k < n ? k : k - n] * a.s.npix + p] : 0.f;
        }
        if (tid < MAD_P) {
            pflag = in ? 0 : 1;
            if (in && a.s.excl) pflag = a.s.excl[p] == a.s.exv ? 1 : 0;
            pw = 1.f;
            if (!CENTRE && a.weight && !pflag) pw = a.weight[p];
        }
    };
    if (blockIdx.x < a.ntiles) fetch(blockIdx.x);
    for (unsigned tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {   // (uniform)
        if (tid < MAD_P && pflag) bad[tid] = 1;
#pragma unroll
        for (int i = 0; i < MAD_MAXB / 2; i++) {
            const int k = k0 + 4 * i;
            if (k < m.D) {
                const float v = pv[i];
                double z = 0.0;
                if (fabsf(v) <= FLT_MAX) z = (double)v - cen[k];
                else bad[pix] = 1;                           // several threads may store the same 1
                zs[pix * m.ZS + k] = z;                      // finite always: with w = 0 an invalid pixel adds zeros, never a NaN times 0
            }
        }
        const float wf = pw;
        __syncthreads();
        if (tid < MAD_P) {
            const int b = bad[tid];
            bad[tid] = 0;                                    // for the next tile: its flags are set behind the barrier that ends this one
            wv[tid] = (!b && wf >= 0.f && wf <= FLT_MAX) ? (double)wf : 0.0;
            for (int k = m.D; k < m.ZS; k++) zs[tid * m.ZS + k] = (k == m.D && !b) ? 1.0 : 0.0;
        }
        if (tile + gridDim.x < a.ntiles) fetch(tile + gridDim.x);
        __syncthreads();
        if (worker) {
            if (CENTRE) {
                for (int p = g; p < MAD_P; p += G) acc[0] = fma(wv[p], zs[p * m.ZS + ti], acc[0]);      // w is 0 or 1: the value or nothing
            } else {
                for (int p = g; p < MAD_P; p += G) {
                    const double w = wv[p];
                    const double* zr = zs + p * m.ZS;
                    double zl[4], wz[4];
#pragma unroll
                    for (int i = 0; i < 4; i++) { wz[i] = w * zr[4 * ti + i]; zl[i] = zr[4 * tj + i]; }
#pragma unroll
                    for (int i = 0; i < 4; i++)
#pragma unroll
                        for (int j = 0; j < 4; j++) acc[i * 4 + j] = fma(wz[i], zl[j], acc[i * 4 + j]);
                }
            }
        }
        __syncthreads();                                     // the tile has been read before the next one is staged
    }
    // the slices in slice order, then the block partial
    const int ne = CENTRE ? m.ZS : m.NE;
    if (worker) {
        if (CENTRE) zs[g * m.ZS + ti] = acc[0];
        else {
            const int pair = tid % m.NT;
#pragma unroll
            for (int i = 0; i < 16; i++) zs[g * m.NE + pair * 16 + i] = acc[i];
        }
    }
    __syncthreads();
    for (int e = tid; e < ne; e += 256) {
        double s = 0.0;
        for (int q = 0; q < G; q++) s += zs[q * ne + e];
        a.ws[(size_t)blockIdx.x * ne + e] = s;
    }
}

// the block partials in block order; entry (k, l), k <= l <= D, of the augmented matrix -> S0, S1, S2 (packed upper triangle, rows first)
__global__ __launch_bounds__(256) void mad_moments_finish_kernel(const double* __restrict__ ws, int nblk, int n_b, const double* __restrict__ state,
                                                                 double* __restrict__ mom) {
    if (state && state[2] != 0.0) return;
    const MadDims m = mad_dims(n_b);
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= m.NE) return;
    int ti, tj;
    mad_tile_rc(e >> 4, m.T, ti, tj);
    const int k = 4 * ti + ((e >> 2) & 3), l = 4 * tj + (e & 3);
    if (k > l || l > m.D) return;
    double s = 0.0;
    for (int b = 0; b < nblk; b++) s += ws[(size_t)b * m.NE + e];
    if (l == m.D) mom[k == m.D ? 0 : 1 + k] = s;
    else mom[1 + m.D + k * m.D - k * (k - 1) / 2 + (l - k)] = s;
}

__global__ __launch_bounds__(256) void mad_centre_finish_kernel(const double* __restrict__ ws, int nblk, int n_b, double* __restrict__ centre,
                                                                long long* __restrict__ n_valid) {
    __shared__ double tot[MAD_ZSMAX];
    const MadDims m = mad_dims(n_b);
    const int k = threadIdx.x;
    if (k <= m.D) {
        double s = 0.0;
        for (int b = 0; b < nblk; b++) s += ws[(size_t)b * m.ZS + k];
        tot[k] = s;
    }
    __syncthreads();
    const double cnt = tot[m.D];                             // a sum of ones below 2^30: exact
    if (k < m.D) centre[k] = cnt > 0.0 ? __ddiv_rn(tot[k], cnt) : 0.0;
    if (k == m.D) *n_valid = (long long)cnt;
}

// ---------------------------------------------------------------- the solve
__device__ __forceinline__ double mad_wave_sum(double v) {  // xor butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double mad_wave_max(double v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// A = L L^T in place (lower triangle), by one wave; false (uniform) at a pivot <= 1e-12 times its original diagonal entry
__device__ bool mad_chol(double* A, const double* dg, int n, int t) {
    for (int j = 0; j < n; j++) {
        const double d = A[j * MAD_LD + j];
        if (!(d > 1e-12 * dg[j])) return false;
        const double ljj = sqrt(d);
        __syncthreads();
        if (t == j) A[j * MAD_LD + j] = ljj;
        if (t > j && t < n) A[t * MAD_LD + j] = A[t * MAD_LD + j] / ljj;
        __syncthreads();
        if (t > j && t < n) {
            const double lij = A[t * MAD_LD + j];
            for (int k = j + 1; k <= t; k++) A[t * MAD_LD + k] -= lij * A[k * MAD_LD + j];
        }
        __syncthreads();
    }
    return true;
}

struct MadSolveArgs { const double* mom; const double* centre; const long long* n_valid; int n, first; double tol, min_var; double* state; };

__global__ __launch_bounds__(64) void mad_solve_kernel(const MadSolveArgs q) {
    __shared__ double A[MAD_MAXB * MAD_LD], B[MAD_MAXB * MAD_LD], K[MAD_MAXB * MAD_LD], V[MAD_MAXB * MAD_LD];
    __shared__ double mz[2 * MAD_MAXB], dgx[MAD_MAXB], dgy[MAD_MAXB], sg[MAD_MAXB], rn[MAD_MAXB];
    const int t = threadIdx.x, n = q.n, D = 2 * n;
    double* st = q.state;
    if (!q.first && st[2] != 0.0) {                          // (uniform) converged before: mark the skip, nothing else
        if (t == 0) st[3] = 1.0;
        return;
    }
    const double it0 = q.first ? 0.0 : st[0];
    const double prev = (t < n && !q.first) ? st[BDN_MAD_STATE_RHO + t] : 0.0;
    double* rho = st + BDN_MAD_STATE_RHO;
    double* var = rho + n;
    double* mean = var + n;
    double* cen = mean + D;
    double* av = cen + D;
    double* bv = av + n * n;
    const double S0 = q.mom[0];
    const long long nv = *q.n_valid;
    bool ok = S0 > 0.0 && S0 <= DBL_MAX && nv >= (long long)(D + 1);
    if (t < D) mz[t] = ok ? q.mom[1 + t] / S0 : (double)NAN;
    __syncthreads();
    if (ok) {
        if (t < D) {
            for (int l = 0; l < D; l++) {
                const int kk = t < l ? t : l, ll = t < l ? l : t;
                const double c = q.mom[1 + D + kk * D - kk * (kk - 1) / 2 + (ll - kk)] / S0 - mz[t] * mz[l];
                if (t < n && l < n) A[t * MAD_LD + l] = c;
                else if (t >= n && l >= n) B[(t - n) * MAD_LD + (l - n)] = c;
                else if (t < n) K[t * MAD_LD + (l - n)] = c;
            }
        }
        __syncthreads();
        if (t < n) { dgx[t] = A[t * MAD_LD + t]; dgy[t] = B[t * MAD_LD + t]; }
        __syncthreads();
        ok = mad_chol(A, dgx, n, t);
        if (ok) ok = mad_chol(B, dgy, n, t);
    }
    __syncthreads();
    if (ok) {
        if (t < n) {                                         // column t of Lx^-1 Sxy
            for (int i = 0; i < n; i++) {
                double s = K[i * MAD_LD + t];
                for (int k = 0; k < i; k++) s -= A[i * MAD_LD + k] * K[k * MAD_LD + t];
                K[i * MAD_LD + t] = s / A[i * MAD_LD + i];
            }
        }
        __syncthreads();
        if (t < n) {                                         // row t of (Lx^-1 Sxy) Ly^-T, and V = I
            for (int i = 0; i < n; i++) {
                double s = K[t * MAD_LD + i];
                for (int k = 0; k < i; k++) s -= B[i * MAD_LD + k] * K[t * MAD_LD + k];
                K[t * MAD_LD + i] = s / B[i * MAD_LD + i];
            }
            for (int i = 0; i < n; i++) V[t * MAD_LD + i] = i == t ? 1.0 : 0.0;
        }
        __syncthreads();
        // one-sided Jacobi: lane t owns row t of K and of V; the columns of K are rotated until they are orthogonal, K V = U diag(sigma)
        for (int sweep = 0; sweep < MAD_SWEEPS; sweep++) {
            int rotated = 0;
            for (int p = 0; p < n - 1; p++) {
                for (int c = p + 1; c < n; c++) {
                    const double kp = t < n ? K[t * MAD_LD + p] : 0.0, kc = t < n ? K[t * MAD_LD + c] : 0.0;
                    const double al = mad_wave_sum(kp * kp), be = mad_wave_sum(kc * kc), ga = mad_wave_sum(kp * kc);
                    if (!(fabs(ga) > 1e-14 * (sqrt(al) * sqrt(be)))) continue;          // (uniform) orthogonal already
                    rotated = 1;
                    const double zeta = (be - al) / (2.0 * ga);
                    const double tt = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
                    if (t < n) {
                        K[t * MAD_LD + p] = cs * kp - sn * kc;
                        K[t * MAD_LD + c] = sn * kp + cs * kc;
                        const double vp = V[t * MAD_LD + p], vc = V[t * MAD_LD + c];
                        V[t * MAD_LD + p] = cs * vp - sn * vc;
                        V[t * MAD_LD + c] = sn * vp + cs * vc;
                    }
                }
            }
            if (!rotated) break;
        }
        __syncthreads();
        double sgn = 1.0;
        if (t < n) {                                         // from here lane t owns COLUMN t: the variate before ordering
            double s = 0.0;
            for (int i = 0; i < n; i++) s += K[i * MAD_LD + t] * K[i * MAD_LD + t];
            const double sigma = sqrt(s);
            sg[t] = sigma;
            for (int i = 0; i < n; i++) K[i * MAD_LD + t] = sigma > 0.0 ? K[i * MAD_LD + t] / sigma : 0.0;
            // the sign: sum_k (Sxx a)[k] / sqrt(Sxx[k][k]) with Sxx a = Lx u
            double corr = 0.0;
            for (int k = 0; k < n; k++) {
                double r = 0.0;
                for (int j = 0; j <= k; j++) r += A[k * MAD_LD + j] * K[j * MAD_LD + t];
                corr += r / sqrt(dgx[k]);
            }
            if (corr < 0.0) sgn = -1.0;
            for (int r = n - 1; r >= 0; r--) {               // a = Lx^-T u and b = Ly^-T v, in place
                double s1 = K[r * MAD_LD + t], s2 = V[r * MAD_LD + t];
                for (int k = r + 1; k < n; k++) { s1 -= A[k * MAD_LD + r] * K[k * MAD_LD + t]; s2 -= B[k * MAD_LD + r] * V[k * MAD_LD + t]; }
                K[r * MAD_LD + t] = s1 / A[r * MAD_LD + r];
                V[r * MAD_LD + t] = s2 / B[r * MAD_LD + r];
            }
        }
        __syncthreads();
        if (t < n) {
            int rank = 0;
            for (int i = 0; i < n; i++) rank += (sg[i] > sg[t] || (sg[i] == sg[t] && i < t)) ? 1 : 0;
            const double r = sg[t] < 1.0 ? sg[t] : 1.0;
            rn[rank] = r;
            rho[rank] = r;
            const double v = 2.0 * (1.0 - r);
            var[rank] = v > q.min_var ? v : q.min_var;
            for (int k = 0; k < n; k++) { av[rank * n + k] = sgn * K[k * MAD_LD + t]; bv[rank * n + k] = sgn * V[k * MAD_LD + t]; }
        }
        __syncthreads();
    } else if (t < n) {
        rho[t] = NAN; var[t] = NAN;
        for (int k = 0; k < n; k++) { av[t * n + k] = NAN; bv[t * n + k] = NAN; }
    }
    double delta = (double)NAN;
    if (ok) {
        delta = mad_wave_max(t < n ? fabs(rn[t] - prev) : 0.0);
        if (q.first) delta = (double)INFINITY;
    }
    if (t < D) { mean[t] = q.centre[t] + mz[t]; cen[t] = q.centre[t]; }
    if (t == 0) {
        st[BDN_MAD_STATE_ITER] = it0 + 1.0;
        st[BDN_MAD_STATE_OK] = ok ? 1.0 : 0.0;
        st[BDN_MAD_STATE_CONVERGED] = (!ok || delta < q.tol) ? 1.0 : 0.0;
        st[BDN_MAD_STATE_SKIP] = 0.0;
        st[BDN_MAD_STATE_DELTA] = delta;
        st[BDN_MAD_STATE_S0] = S0;
        st[BDN_MAD_STATE_NVALID] = (double)nv;
    }
}

// ---------------------------------------------------------------- the statistic
// Q(n_b / 2, chi2 / 2) by its finite closed form.  The terms carry one factor e^(-t/2) and the sum is multiplied by the other, so that a
// tail above 1e-308 never passes through a denormal e^-t; every term stays below 2^16.
__device__ double mad_q(int n_b, double chi2) {
    const double t = 0.5 * chi2;
    if (!(t <= DBL_MAX)) return t > 0.0 ? 0.0 : (double)NAN;
    if (!(t > 0.0)) return 1.0;
    const int m = n_b >> 1;
    const double h = exp(-0.5 * t);
    double sum = 0.0, q;
    if (n_b & 1) {
        const double r = sqrt(t);
        double term = h * r * 1.1283791670955126;            // 2 / sqrt(pi) = 1 / Gamma(3/2)
        for (int k = 1; k <= m; k++) { sum += term; term *= t / ((double)k + 0.5); }
        q = erfc(r) + sum * h;
    } else {
        double term = h;
        for (int k = 1; k <= m; k++) { sum += term; term *= t / (double)k; }
        q = sum * h;
    }
    return q < 1.0 ? q : 1.0;
}

struct MadChiArgs { MadScene s; const double* state; float* chi2; float* proba; float* variates; };

template <int NV>
__global__ __launch_bounds__(256) void mad_chi2_kernel(const MadChiArgs a) {
    __shared__ double at[MAD_MAXB * NV];                     // [k][i] = a_i[k]
    __shared__ double bt[MAD_MAXB * NV];                     // [k][i] = -b_i[k]
    __shared__ double mx[MAD_MAXB], my[MAD_MAXB], vr[NV];
    __shared__ int sb[MAD_MAXB];
    if (a.state[BDN_MAD_STATE_SKIP] != 0.0) return;          // (uniform) the run has converged: this launch writes nothing
    const int tid = threadIdx.x, n = a.s.n_b;
    const bool ok = a.state[BDN_MAD_STATE_OK] == 1.0;
    const bool bands_ok = mad_stage_bands(a.s, sb);
    const unsigned npix = a.s.npix;
    if (ok) {
        const double* rho = a.state + BDN_MAD_STATE_RHO;
        const double* var = rho + n;
        const double* mean = var + n;
        const double* av = mean + 4 * n;
        const double* bv = av + n * n;
        for (int e = tid; e < n * NV; e += 256) {
            const int k = e / NV, i = e % NV;
            at[e] = i < n ? av[i * n + k] : 0.0;
            bt[e] = i < n ? -bv[i * n + k] : 0.0;
        }
        if (tid < n) { mx[tid] = mean[tid]; my[tid] = mean[n + tid]; }
        if (tid < NV) vr[tid] = tid < n ? var[tid] : 1.0;
    }
    __syncthreads();
    for (unsigned p = blockIdx.x * 256u + (unsigned)tid; p < npix; p += gridDim.x * 256u) {
        if (!ok) {
            a.chi2[p] = NAN; a.proba[p] = NAN; a.proba[(size_t)npix + p] = NAN;
            if (a.variates) for (int i = 0; i < n; i++) a.variates[(size_t)i * npix + p] = NAN;
            continue;
        }
        bool valid = bands_ok && !(a.s.excl && a.s.excl[p] == a.s.exv);
        double M[NV];
#pragma unroll
        for (int i = 0; i < NV; i++) M[i] = 0.0;
        if (bands_ok) {
            for (int k = 0; k < n; k++) {
                const float x = a.s.d1[(size_t)sb[k] * npix + p];
                valid = valid && fabsf(x) <= FLT_MAX;
                const double dx = (double)x - mx[k];
#pragma unroll
                for (int i = 0; i < NV; i++) M[i] = fma(at[k * NV + i], dx, M[i]);
            }
            for (int k = 0; k < n; k++) {
                const float y = a.s.d2[(size_t)sb[k] * npix + p];
                valid = valid && fabsf(y) <= FLT_MAX;
                const double dy = (double)y - my[k];
#pragma unroll
                for (int i = 0; i < NV; i++) M[i] = fma(bt[k * NV + i], dy, M[i]);
            }
        }
        double c = 0.0;
#pragma unroll
        for (int i = 0; i < NV; i++) if (i < n) c += M[i] * M[i] / vr[i];
        float cf = 0.f, q0 = 1.f, q1 = 0.f;
        if (valid) {
            const double q = mad_q(n, c);
            cf = (float)c; q0 = (float)q; q1 = (float)(1.0 - q);
        }
        a.chi2[p] = cf; a.proba[p] = q0; a.proba[(size_t)npix + p] = q1;
        if (a.variates) {
#pragma unroll
            for (int i = 0; i < NV; i++) if (i < n) a.variates[(size_t)i * npix + p] = valid ? (float)M[i] : 0.f;
        }
    }
}

struct MadMaskArgs { MadScene s; const float* proba; float thr; int out_bad; uint8_t* mask; };

__global__ __launch_bounds__(256) void mad_mask_kernel(const MadMaskArgs a) {
    __shared__ int sb[MAD_MAXB];
    const bool bands_ok = mad_stage_bands(a.s, sb);
    const unsigned npix = a.s.npix;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < npix; p += gridDim.x * 256u) {
        bool valid = bands_ok && !(a.s.excl && a.s.excl[p] == a.s.exv);
        if (valid) {
            for (int k = 0; k < a.s.n_b; k++) {
                const float x = a.s.d1[(size_t)sb[k] * npix + p], y = a.s.d2[(size_t)sb[k] * npix + p];
                valid = valid && fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX;
            }
        }
        a.mask[p] = !valid ? (uint8_t)a.out_bad : (a.proba[p] < a.thr ? (uint8_t)1 : (uint8_t)0);   // a NaN fails the comparison: 0
    }
}

// ---------------------------------------------------------------- entries
static bool mad_scene_ok(int C, int H, int W) { return C >= 1 && C <= MAD_MAXC && H >= 1 && W >= 1 && H <= MAD_MAXDIM && W <= MAD_MAXDIM; }

#define MAD_CHECK_SCENE(name)                                                                                                              \
    if (!d1 || !d2 || !bands) BDN_FAIL(BDN_E_ARG, name ": null pointer");                                                                 \
    if (n_b < 1 || n_b > MAD_MAXB) BDN_FAIL(BDN_E_ARG, name ": n_b=%d band indices (1..%d)", n_b, MAD_MAXB);                               \
    if (!mad_scene_ok(C, H, W)) BDN_FAIL(BDN_E_ARG, name ": bad scene %d x %d x %d (1 <= C <= %d; 1 <= H, W <= %d)", C, H, W, MAD_MAXC, MAD_MAXDIM); \
    if (exclude && (exclude_value < 0 || exclude_value > 255)) BDN_FAIL(BDN_E_ARG, name ": exclude_value=%d must be a byte value (0..255)", exclude_value); \
    if (((uintptr_t)d1 & 3) || ((uintptr_t)d2 & 3) || ((uintptr_t)bands & 3)) BDN_FAIL(BDN_E_ARG, name ": d1, d2 and bands must be 4-byte aligned")

extern "C" size_t bdn_mad_workspace_bytes(int n_b, int H, int W) {
    if (n_b < 1 || n_b > MAD_MAXB || !mad_scene_ok(1, H, W)) return 0;
    return (size_t)mad_blocks(H, W) * (size_t)mad_dims(n_b).NE * sizeof(double);
}

extern "C" int bdn_mad_centre(const float* d1, const float* d2, const int32_t* bands, int n_b, const uint8_t* exclude, int exclude_value,
                              double* centre, long long* n_valid, void* ws, int C, int H, int W, void* stream) {
    MAD_CHECK_SCENE("mad_centre");
    if (!centre || !n_valid || !ws) BDN_FAIL(BDN_E_ARG, "mad_centre: null pointer");
    if (((uintptr_t)centre & 7) || ((uintptr_t)n_valid & 7) || ((uintptr_t)ws & 15))
        BDN_FAIL(BDN_E_ARG, "mad_centre: centre and n_valid must be 8-byte aligned, ws 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nblk = mad_blocks(H, W);
    MadMomArgs a{{d1, d2, bands, exclude, exclude_value, n_b, C, (unsigned)H * (unsigned)W}, nullptr, nullptr, nullptr, (double*)ws, mad_tiles(H, W)};
    hipLaunchKernelGGL(mad_moments_kernel<true>, dim3(nblk), dim3(256), 0, st, a);
    BDN_CHECK_LAUNCH("mad_centre");
    hipLaunchKernelGGL(mad_centre_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, (int)nblk, n_b, centre, n_valid);
    BDN_CHECK_LAUNCH("mad_centre_finish");
    return BDN_OK;
}

extern "C" int bdn_mad_moments(const float* d1, const float* d2, const int32_t* bands, int n_b, const uint8_t* exclude, int exclude_value,
                               const float* weight, const double* centre, const double* state, double* moments, void* ws, int C, int H, int W,
                               void* stream) {
    MAD_CHECK_SCENE("mad_moments");
    if (!centre || !moments || !ws) BDN_FAIL(BDN_E_ARG, "mad_moments: null pointer");
    if (((uintptr_t)weight & 3) || ((uintptr_t)centre & 7) || ((uintptr_t)state & 7) || ((uintptr_t)moments & 7) || ((uintptr_t)ws & 15))
        BDN_FAIL(BDN_E_ARG, "mad_moments: weight must be 4-byte aligned, centre, state and moments 8-byte and ws 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned nblk = mad_blocks(H, W);
    MadMomArgs a{{d1, d2, bands, exclude, exclude_value, n_b, C, (unsigned)H * (unsigned)W}, weight, centre, state, (double*)ws, mad_tiles(H, W)};
    hipLaunchKernelGGL(mad_moments_kernel<false>, dim3(nblk), dim3(256), 0, st, a);
    BDN_CHECK_LAUNCH("mad_moments");
    hipLaunchKernelGGL(mad_moments_finish_kernel, dim3(grid_for((size_t)mad_dims(n_b).NE)), dim3(256), 0, st, (const double*)ws, (int)nblk, n_b,
                       state, moments);
    BDN_CHECK_LAUNCH("mad_moments_finish");
    return BDN_OK;
}

extern "C" int bdn_mad_solve(const double* moments, const double* centre, const long long* n_valid, int n_b, int first, double tol, double min_var,
                             double* state, void* stream) {
    if (!moments || !centre || !n_valid || !state) BDN_FAIL(BDN_E_ARG, "mad_solve: null pointer");
    if (n_b < 1 || n_b > MAD_MAXB) BDN_FAIL(BDN_E_ARG, "mad_solve: n_b=%d band indices (1..%d)", n_b, MAD_MAXB);
    if (first != 0 && first != 1) BDN_FAIL(BDN_E_ARG, "mad_solve: first=%d must be 0 or 1", first);
    if (!(tol >= 0.0) || !(tol <= DBL_MAX)) BDN_FAIL(BDN_E_ARG, "mad_solve: tol=%g must be a finite number >= 0", tol);
    if (!(min_var > 0.0) || !(min_var <= DBL_MAX)) BDN_FAIL(BDN_E_ARG, "mad_solve: min_var=%g must be a finite number > 0", min_var);
    if (((uintptr_t)moments & 7) || ((uintptr_t)centre & 7) || ((uintptr_t)n_valid & 7) || ((uintptr_t)state & 7))
        BDN_FAIL(BDN_E_ARG, "mad_solve: moments, centre, n_valid and state must be 8-byte aligned");
    MadSolveArgs q{moments, centre, n_valid, n_b, first, tol, min_var, state};
    hipLaunchKernelGGL(mad_solve_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, q);
    BDN_CHECK_LAUNCH("mad_solve");
    return BDN_OK;
}

extern "C" int bdn_mad_chi2(const float* d1, const float* d2, const int32_t* bands, int n_b, const uint8_t* exclude, int exclude_value,
                            const double* state, float* chi2, float* proba, float* variates, int C, int H, int W, void* stream) {
    MAD_CHECK_SCENE("mad_chi2");
    if (!state || !chi2 || !proba) BDN_FAIL(BDN_E_ARG, "mad_chi2: null pointer");
    if (((uintptr_t)state & 7) || ((uintptr_t)chi2 & 3) || ((uintptr_t)proba & 3) || ((uintptr_t)variates & 3))
        BDN_FAIL(BDN_E_ARG, "mad_chi2: state must be 8-byte aligned, chi2, proba and variates 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const unsigned npix = (unsigned)H * (unsigned)W;
    unsigned gx = grid_for(npix);
    if (gx > 4096u) gx = 4096u;
    MadChiArgs a{{d1, d2, bands, exclude, exclude_value, n_b, C, npix}, state, chi2, proba, variates};
    if (n_b <= 4) hipLaunchKernelGGL(mad_chi2_kernel<4>, dim3(gx), dim3(256), 0, st, a);
    else if (n_b <= 8) hipLaunchKernelGGL(mad_chi2_kernel<8>, dim3(gx), dim3(256), 0, st, a);
    else if (n_b <= 16) hipLaunchKernelGGL(mad_chi2_kernel<16>, dim3(gx), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(mad_chi2_kernel<32>, dim3(gx), dim3(256), 0, st, a);
    BDN_CHECK_LAUNCH("mad_chi2");
    return BDN_OK;
}

extern "C" int bdn_mad_mask(const float* proba, const float* d1, const float* d2, const int32_t* bands, int n_b, const uint8_t* exclude,
                            int exclude_value, float threshold, int excluded_out, uint8_t* mask, int C, int H, int W, void* stream) {
    MAD_CHECK_SCENE("mad_mask");
    if (!proba || !mask) BDN_FAIL(BDN_E_ARG, "mad_mask: null pointer");
    if (!(threshold >= 0.f && threshold <= 1.f)) BDN_FAIL(BDN_E_ARG, "mad_mask: threshold=%g must lie in [0, 1]", (double)threshold);
    if (excluded_out < 0 || excluded_out > 255) BDN_FAIL(BDN_E_ARG, "mad_mask: excluded_out=%d must be a byte value (0..255)", excluded_out);
    if ((uintptr_t)proba & 3) BDN_FAIL(BDN_E_ARG, "mad_mask: proba must be 4-byte aligned");
    const unsigned npix = (unsigned)H * (unsigned)W;
    unsigned gx = grid_for(npix);
    if (gx > 4096u) gx = 4096u;
    MadMaskArgs a{{d1, d2, bands, exclude, exclude_value, n_b, C, npix}, proba, threshold, excluded_out, mask};
    hipLaunchKernelGGL(mad_mask_kernel, dim3(gx), dim3(256), 0, (hipStream_t)stream, a);
    BDN_CHECK_LAUNCH("mad_mask");
    return BDN_OK;
}
