// libbidate_hip: thresholds without labels.  A change statistic (IR-MAD's chi2, a scene's change probability) becomes a mask at a number
// that, without labels, somebody has to choose.  Here the number is selected from the histogram of the statistic itself: bdn_raster_hist
// counts a scene-sized float raster into caller-given bin edges (comparisons only: the counts are exact and the same bits on every run),
// bdn_hist_threshold applies Otsu's, Kittler and Illingworth's, Rosin's and the two-Gaussian EM rule to the counts in one single-block
// launch, and bdn_raster_mask thresholds the raster at a number that lives in device memory, so that the chain has no host read.
// Everything summed across threads of the raster kernels is an integer; the floating-point sums of the selection run in a fixed order
// (bin order inside a thread's chunk of bins, chunk partials in chunk order), without contraction into fused multiply-adds, so that the
// numpy restatement in tests/thresholds_ref.py performs the same roundings apart from log and exp.
#include "common.hpp"
#include "hist_core.hpp"
#include <float.h>

#pragma clang fp contract(off)

constexpr int RH_THREADS = 256;
constexpr int RH_MAX_BLOCKS = 2048;                     // curve.hip's grid: 8 blocks per CU, the rest is grid-strided
constexpr int RH_MIN_ITEMS = 4;
constexpr int RH_MAX_BINS = 4096;
constexpr long long RH_MAX_PIXELS = 1LL << 40;          // a block then counts < 2^32 pixels into its 32-bit LDS cells whatever the grid

__device__ __forceinline__ bool finite_f(float v) { return fabsf(v) <= FLT_MAX; }      // false for NaN and +-inf

// ============================================================ raster_hist
struct RasterHistArgs {
    const float* raster; const uint8_t* exclude; const float* edges; unsigned long long* hist;
    long long total;                                    // items: HW / PER
    int exclude_value, n_bins;
};

// The cell of one value: n_bins + 2 skipped, n_bins below, n_bins + 1 above, otherwise max{i < n_bins : ed[i] <= v} by bisection.  mid
// stays in [1, n_bins - 1] and the loop ends after at most 12 steps whatever the table holds, sorted or not.
__device__ __forceinline__ int raster_cell(const float* ed, int n_bins, float v, bool skip) {
    if (skip) return n_bins + 2;
    if (v < ed[0]) return n_bins;
    if (v > ed[n_bins]) return n_bins + 1;
    int lo = 0, hi = n_bins - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (ed[mid] <= v) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// An item is PER consecutive pixels (PER = 4: one 16-byte load, four exclude bytes in one load; taken when HW % 4 == 0 and the pointers
// are aligned).  The loop's trip count is the same for every thread of a block (the ballots of wave_hist_add need whole waves), lanes
// past the end carry no pixel.
template <int PER>
__global__ __launch_bounds__(RH_THREADS) void raster_hist_kernel(const RasterHistArgs a) {
    extern __shared__ unsigned rh_lds[];                // [n_bins + 3] counts of this block, then [n_bins + 1] edges
    const int tid = threadIdx.x, lane = tid & 63, n_bins = a.n_bins;
    unsigned* cnt = rh_lds;
    float* ed = reinterpret_cast<float*>(rh_lds + n_bins + 3);
    for (int i = tid; i < n_bins + 3; i += RH_THREADS) cnt[i] = 0;
    for (int i = tid; i <= n_bins; i += RH_THREADS) ed[i] = a.edges[i];
    __syncthreads();
    const long long stride = (long long)gridDim.x * RH_THREADS, base0 = (long long)blockIdx.x * RH_THREADS;
    long long idx = base0 + tid;
    for (long long base = base0; base < a.total; base += stride, idx += stride) {
        int key[PER];
#pragma unroll
        for (int p = 0; p < PER; p++) key[p] = -1;
        if (idx < a.total) {
            float v[PER];
            int ex[PER];
            PixVec<PER>::load(a.raster + idx * PER, v);
            if (a.exclude) PixVec<PER>::labels(a.exclude + idx * PER, ex);
            else {
#pragma unroll
                for (int p = 0; p < PER; p++) ex[p] = -1;
            }
#pragma unroll
            for (int p = 0; p < PER; p++) key[p] = raster_cell(ed, n_bins, v[p], ex[p] == a.exclude_value || !finite_f(v[p]));
        }
#pragma unroll
        for (int p = 0; p < PER; p++) wave_hist_add(cnt, key[p], lane);
    }
    __syncthreads();
    for (int i = tid; i < n_bins + 3; i += RH_THREADS) {
        const unsigned c = cnt[i];
        if (c) atomicAdd(&a.hist[i], (unsigned long long)c);      // one 64-bit integer add per occupied cell and block
    }
}

static inline bool byte_value(int v) { return v >= 0 && v <= 255; }

extern "C" int bdn_raster_hist(const float* raster, const uint8_t* exclude, int exclude_value, const float* edges, int n_bins,
                               unsigned long long* hist, long long HW, void* stream) {
    if (!raster || !edges || !hist) BDN_FAIL(BDN_E_ARG, "raster_hist: null pointer");
    if ((uintptr_t)raster % 4 || (uintptr_t)edges % 4 || (uintptr_t)hist % 8) BDN_FAIL(BDN_E_ARG, "raster_hist: raster / edges must be 4-byte, hist 8-byte aligned");
    if (!byte_value(exclude_value)) BDN_FAIL(BDN_E_ARG, "raster_hist: exclude_value must be a byte 0..255, got %d", exclude_value);
    if (n_bins < 2 || n_bins > RH_MAX_BINS) BDN_FAIL(BDN_E_ARG, "raster_hist: n_bins must be in 2..%d, got %d", RH_MAX_BINS, n_bins);
    if (HW < 1 || HW > RH_MAX_PIXELS) BDN_FAIL(BDN_E_ARG, "raster_hist: need 1 <= HW <= 2^40, got %lld", HW);
    const bool vec = HW % 4 == 0 && (uintptr_t)raster % 16 == 0 && (uintptr_t)exclude % 4 == 0;
    RasterHistArgs a;
    a.raster = raster; a.exclude = exclude; a.edges = edges; a.hist = hist;
    a.total = vec ? HW / 4 : HW; a.exclude_value = exclude_value; a.n_bins = n_bins;
    const long long want = (a.total + RH_THREADS * RH_MIN_ITEMS - 1) / (RH_THREADS * RH_MIN_ITEMS);
    const unsigned blocks = (unsigned)(want < RH_MAX_BLOCKS ? want : RH_MAX_BLOCKS);
    const size_t lds = (2 * (size_t)n_bins + 4) * sizeof(unsigned);          // at most 32 784 bytes
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(raster_hist_kernel<4>, dim3(blocks), dim3(RH_THREADS), lds, st, a);
    else hipLaunchKernelGGL(raster_hist_kernel<1>, dim3(blocks), dim3(RH_THREADS), lds, st, a);
    BDN_CHECK_LAUNCH("raster_hist");
    return BDN_OK;
}

// ============================================================ hist_threshold
// One block of 256 threads.  Thread t owns the `per` = ceil(n_bins / 256) consecutive bins [t per, (t + 1) per) (none past n_bins).  A sum
// over the bins is formed as: every thread adds its bins in ascending order starting from 0, then the 256 thread partials are added in
// thread order starting from 0 (by every thread for itself, from LDS: all threads hold the same bits).  A prefix sum at bin b is the sum
// of the partials of the threads before b's owner, in thread order from 0, to which the owner adds its bins below b in ascending order.
constexpr int HT_THREADS = 256;
constexpr int HT_K = 7;

struct HtShared {
    double d[HT_K][HT_THREADS];
    unsigned long long u[2][HT_THREADS];
    long long best_v[HT_THREADS];
    int best_i[HT_THREADS];
};

struct HtCtx {
    const unsigned long long* hist; const double* coord; const float* edges;
    int n_bins, b_lo, b_hi;
    double M;                                            // the centre the coordinates are taken from: the mean coordinate of all counts
    unsigned long long N;
};

template <int K>
__device__ void block_sums(HtShared& sh, const double (&mine)[K], double (&total)[K], double (&before)[K]) {
    const int t = threadIdx.x;
    __syncthreads();                                     // the readers of the previous call are done
#pragma unroll
    for (int k = 0; k < K; k++) sh.d[k][t] = mine[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        double s = 0.0, p = 0.0;
        for (int j = 0; j < HT_THREADS; j++) { if (j == t) p = s; s += sh.d[k][j]; }
        total[k] = s; before[k] = p;
    }
}

template <int K>
__device__ void block_counts(HtShared& sh, const unsigned long long (&mine)[K], unsigned long long (&total)[K], unsigned long long (&before)[K]) {
    const int t = threadIdx.x;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) sh.u[k][t] = mine[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        unsigned long long s = 0, p = 0;
        for (int j = 0; j < HT_THREADS; j++) { if (j == t) p = s; s += sh.u[k][j]; }
        total[k] = s; before[k] = p;
    }
}

// The candidate (v, i) of the lowest thread that holds the extreme v (strict comparisons in thread order: with every thread offering the
// first extreme of its ascending chunk, the first extreme over all bins).  i < 0: the thread has no candidate.  Returns i, or -1.
template <typename T> __device__ __forceinline__ long long ht_bits(T v);
template <> __device__ __forceinline__ long long ht_bits<double>(double v) { return __double_as_longlong(v); }
template <> __device__ __forceinline__ long long ht_bits<long long>(long long v) { return v; }
template <typename T> __device__ __forceinline__ T ht_value(long long b);
template <> __device__ __forceinline__ double ht_value<double>(long long b) { return __longlong_as_double(b); }
template <> __device__ __forceinline__ long long ht_value<long long>(long long b) { return b; }

template <typename T>
__device__ int block_first_best(HtShared& sh, int i, T v, bool maximise, T* v_out) {
    const int t = threadIdx.x;
    __syncthreads();
    sh.best_v[t] = ht_bits<T>(v); sh.best_i[t] = i;
    __syncthreads();
    int I = -1;
    T V = T(0);
    for (int j = 0; j < HT_THREADS; j++) {
        const int ij = sh.best_i[j];
        if (ij < 0) continue;
        const T vj = ht_value<T>(sh.best_v[j]);
        if (I < 0 || (maximise ? vj > V : vj < V)) { I = ij; V = vj; }
    }
    *v_out = V;
    return I;
}

// max (or min) of one int per thread
__device__ int block_extreme_int(HtShared& sh, int v, bool maximise) {
    const int t = threadIdx.x;
    __syncthreads();
    sh.best_i[t] = v;
    __syncthreads();
    int r = sh.best_i[0];
    for (int j = 1; j < HT_THREADS; j++) { const int x = sh.best_i[j]; r = maximise ? (x > r ? x : r) : (x < r ? x : r); }
    return r;
}

struct HtClasses { unsigned long long n[2]; double a[2], q[2]; };      // per class: count, sum c y, sum c y^2 with y = coord - M

// The two classes of split s (bins < s, bins >= s), each summed for itself.
__device__ HtClasses class_sums(HtShared& sh, const HtCtx& c, int s) {
    unsigned long long n[2] = {0, 0}, nt[2], nb[2];
    double m[4] = {0.0, 0.0, 0.0, 0.0}, mt[4], mb[4];
    for (int b = c.b_lo; b < c.b_hi; b++) {
        const unsigned long long cb = c.hist[b];
        const int k = b >= s;
        const double cy = (double)cb * (c.coord[b] - c.M);
        n[k] += cb; m[k] += cy; m[2 + k] += cy * (c.coord[b] - c.M);
    }
    block_counts<2>(sh, n, nt, nb);
    block_sums<4>(sh, m, mt, mb);
    HtClasses r;
    r.n[0] = nt[0]; r.n[1] = nt[1]; r.a[0] = mt[0]; r.a[1] = mt[1]; r.q[0] = mt[2]; r.q[1] = mt[3];
    return r;
}

__device__ __forceinline__ double class_mean(const HtClasses& k, int i) { return k.n[i] ? k.a[i] / (double)k.n[i] : 0.0; }
__device__ __forceinline__ double class_var(const HtClasses& k, int i) {
    if (!k.n[i]) return 0.0;
    const double m = k.a[i] / (double)k.n[i];
    return k.q[i] / (double)k.n[i] - m * m;
}

struct HtRow { double crit, mean0, mean1, sd0, sd1, w1, iters, loglik; unsigned long long n0, n1; };

__device__ void write_row(const HtCtx& c, double* table, float* thr, int row, int bin, const HtRow& r) {
    if (threadIdx.x != 0) return;
    double* o = table + row * BDN_THR_COLS;
    o[BDN_THR_COL_OK] = 1.0; o[BDN_THR_COL_BIN] = (double)bin; o[BDN_THR_COL_VALUE] = (double)c.edges[bin]; o[BDN_THR_COL_CRIT] = r.crit;
    o[BDN_THR_COL_N0] = (double)r.n0; o[BDN_THR_COL_N1] = (double)r.n1; o[BDN_THR_COL_MEAN0] = r.mean0; o[BDN_THR_COL_MEAN1] = r.mean1;
    o[BDN_THR_COL_SD0] = r.sd0; o[BDN_THR_COL_SD1] = r.sd1; o[BDN_THR_COL_W1] = r.w1; o[BDN_THR_COL_ITERS] = r.iters; o[BDN_THR_COL_LOGLIK] = r.loglik;
    o[BDN_THR_COL_N] = (double)c.N; o[BDN_THR_COL_BELOW] = (double)c.hist[c.n_bins]; o[BDN_THR_COL_ABOVE] = (double)c.hist[c.n_bins + 1];
    thr[row] = c.edges[bin];
}

// the row of a split found by a criterion on the classes themselves (Otsu, Kittler, Rosin)
__device__ void write_split_row(HtShared& sh, const HtCtx& c, double* table, float* thr, int row, int bin, double crit) {
    const HtClasses k = class_sums(sh, c, bin);
    HtRow r;
    r.crit = crit; r.n0 = k.n[0]; r.n1 = k.n[1];
    r.mean0 = class_mean(k, 0) + c.M; r.mean1 = class_mean(k, 1) + c.M;
    r.sd0 = sqrt(fmax(class_var(k, 0), 0.0)); r.sd1 = sqrt(fmax(class_var(k, 1), 0.0));
    r.w1 = (double)k.n[1] / (double)c.N; r.iters = 0.0; r.loglik = 0.0;
    write_row(c, table, thr, row, bin, r);
}

__device__ __forceinline__ bool finite_d(double v) { return fabs(v) <= DBL_MAX; }

__global__ __launch_bounds__(HT_THREADS) void hist_threshold_kernel(const unsigned long long* __restrict__ hist, const double* __restrict__ coord,
                                                                    const float* __restrict__ edges, int n_bins, int methods, int em_iters,
                                                                    double em_tol, double* __restrict__ table, float* __restrict__ thr) {
    __shared__ HtShared sh;
    const int t = threadIdx.x;
    if (t == 0) {                                        // a method that fails or was not requested leaves exactly this
        for (int i = 0; i < 4 * BDN_THR_COLS; i++) table[i] = 0.0;
        for (int i = 0; i < 4; i++) thr[i] = __uint_as_float(0x7fc00000u);
    }
    HtCtx c;
    c.hist = hist; c.coord = coord; c.edges = edges; c.n_bins = n_bins;
    const int per = (n_bins + HT_THREADS - 1) / HT_THREADS;
    c.b_lo = t * per < n_bins ? t * per : n_bins;
    c.b_hi = c.b_lo + per < n_bins ? c.b_lo + per : n_bins;

    // ---- N, the occupied bins, the centre M
    {
        unsigned long long n[2] = {0, 0}, nt[2], nb[2];
        double a[1] = {0.0}, at[1], ab[1];
        for (int b = c.b_lo; b < c.b_hi; b++) {
            const unsigned long long cb = hist[b];
            n[0] += cb; n[1] += cb != 0;
            a[0] += (double)cb * coord[b];
        }
        block_counts<2>(sh, n, nt, nb);
        block_sums<1>(sh, a, at, ab);
        c.N = nt[0];
        if (nt[1] < 2) return;                           // block-uniform: nothing to split
        c.M = at[0] / (double)c.N;
    }
    const double dN = (double)c.N;

    // ---- Otsu and Kittler in one ascending walk over the splits
    int otsu_bin = -1, kit_bin = -1;
    if (methods & (BDN_THR_OTSU | BDN_THR_KITTLER | BDN_THR_EM)) {
        unsigned long long n[1] = {0}, nt[1], nb[1];
        double m[2] = {0.0, 0.0}, mt[2], mb[2];
        for (int b = c.b_lo; b < c.b_hi; b++) {
            const unsigned long long cb = hist[b];
            const double y = coord[b] - c.M, cy = (double)cb * y;
            n[0] += cb; m[0] += cy; m[1] += cy * y;
        }
        block_counts<1>(sh, n, nt, nb);
        block_sums<2>(sh, m, mt, mb);
        unsigned long long n0 = nb[0];
        double a0 = mb[0], q0 = mb[1];
        int io = -1, ik = -1;
        double vo = 0.0, vk = 0.0;
        for (int b = c.b_lo; b < c.b_hi; b++) {
            const unsigned long long n1 = c.N - n0;
            if (b >= 1 && n0 && n1) {
                const double d0 = (double)n0, d1 = (double)n1, a1 = mt[0] - a0, q1 = mt[1] - q0;
                const double m0 = a0 / d0, m1 = a1 / d1, dm = m0 - m1;
                const double otsu = (d0 * d1) * (dm * dm);
                if (finite_d(otsu) && (io < 0 || otsu > vo)) { io = b; vo = otsu; }
                const double v0 = q0 / d0 - m0 * m0, v1 = q1 / d1 - m1 * m1;
                if (v0 > 0.0 && v1 > 0.0) {
                    const double P0 = d0 / dN, P1 = d1 / dN;
                    const double J = (1.0 + (P0 * log(v0) + P1 * log(v1))) - 2.0 * (P0 * log(P0) + P1 * log(P1));
                    if (finite_d(J) && (ik < 0 || J < vk)) { ik = b; vk = J; }
                }
            }
            const unsigned long long cb = hist[b];
            const double y = coord[b] - c.M, cy = (double)cb * y;
            n0 += cb; a0 += cy; q0 += cy * y;
        }
        double best_o, best_k;
        otsu_bin = block_first_best<double>(sh, io, vo, true, &best_o);
        kit_bin = block_first_best<double>(sh, ik, vk, false, &best_k);
        if ((methods & BDN_THR_OTSU) && otsu_bin >= 0) write_split_row(sh, c, table, thr, 0, otsu_bin, best_o);
        if ((methods & BDN_THR_KITTLER) && kit_bin >= 0) write_split_row(sh, c, table, thr, 1, kit_bin, best_k);
    }

    // ---- Rosin: the point of the histogram's right flank farthest from the chord peak -> last occupied bin, in 64-bit integers
    if ((methods & BDN_THR_ROSIN) && c.N < (1ULL << 49)) {
        int ip = -1, ie = -1;
        long long vp = 0;
        for (int b = c.b_lo; b < c.b_hi; b++) {
            const long long cb = (long long)hist[b];
            if (ip < 0 || cb > vp) { ip = b; vp = cb; }
            if (cb) ie = b;
        }
        long long cp;
        const int p = block_first_best<long long>(sh, ip, vp, true, &cp);
        const int e = block_extreme_int(sh, ie, true);
        if (p >= 0 && e >= p + 2) {
            const long long ce = (long long)hist[e], w = e - p;
            int id = -1;
            long long vd = 0;
            for (int b = c.b_lo; b < c.b_hi; b++) {
                if (b <= p || b >= e) continue;
                const long long d = (ce - cp) * (long long)(b - p) - w * ((long long)hist[b] - cp);
                if (id < 0 || d > vd) { id = b; vd = d; }
            }
            long long best_d;
            const int bin = block_first_best<long long>(sh, id, vd, true, &best_d);
            if (bin >= 0) write_split_row(sh, c, table, thr, 2, bin, (double)best_d);
        }
    }

    // ---- EM of two Gaussians on the histogram, started from Kittler's split (Otsu's without one)
    if (!(methods & BDN_THR_EM)) return;
    const int start = kit_bin >= 0 ? kit_bin : otsu_bin;
    if (start < 0) return;
    double vfloor;
    {
        int is = -1;
        double vs = 0.0;
        for (int b = c.b_lo; b < c.b_hi; b++) {
            if (b + 1 >= n_bins) continue;
            const double s = coord[b + 1] - coord[b];
            if (s > 0.0 && (is < 0 || s < vs)) { is = b; vs = s; }
        }
        double smin;
        if (block_first_best<double>(sh, is, vs, false, &smin) < 0) return;
        vfloor = (smin * smin) / 12.0;
    }
    double w[2], mu[2], var[2];
    {
        const HtClasses k = class_sums(sh, c, start);
        for (int i = 0; i < 2; i++) {
            w[i] = (double)k.n[i] / dN; mu[i] = class_mean(k, i); var[i] = fmax(class_var(k, i), vfloor);
        }
    }
    const double TWO_PI = 6.283185307179586;
    double loglik = 0.0, prev = 0.0;
    int iters = 0;
    for (int it = 1; it <= em_iters; it++) {
        const double k0 = log(w[0]) - 0.5 * log(TWO_PI * var[0]), k1 = log(w[1]) - 0.5 * log(TWO_PI * var[1]);
        double acc[HT_K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, tot[HT_K], bef[HT_K];
        for (int b = c.b_lo; b < c.b_hi; b++) {
            const unsigned long long cb = hist[b];
            if (!cb) continue;
            const double cd = (double)cb, y = coord[b] - c.M, e0 = y - mu[0], e1 = y - mu[1];
            const double l0 = k0 - (e0 * e0) / (2.0 * var[0]), l1 = k1 - (e1 * e1) / (2.0 * var[1]);
            const double mx = fmax(l0, l1), x0 = exp(l0 - mx), x1 = exp(l1 - mx), s = x0 + x1;
            const double g0 = cd * (x0 / s), g1 = cd * (x1 / s);
            acc[0] += cd * (mx + log(s));
            acc[1] += g0; acc[2] += g0 * y; acc[3] += (g0 * y) * y;
            acc[4] += g1; acc[5] += g1 * y; acc[6] += (g1 * y) * y;
        }
        block_sums<HT_K>(sh, acc, tot, bef);
        loglik = tot[0]; iters = it;
        if (!finite_d(loglik) || !(tot[1] > 0.0) || !(tot[4] > 0.0)) return;      // block-uniform: every thread holds the same sums
        if (it > 1 && fabs(loglik - prev) <= em_tol * fabs(loglik)) break;
        prev = loglik;
        for (int i = 0; i < 2; i++) {
            const double R = tot[1 + 3 * i];
            w[i] = R / dN; mu[i] = tot[2 + 3 * i] / R; var[i] = fmax(tot[3 + 3 * i] / R - mu[i] * mu[i], vfloor);
        }
    }
    if (!(mu[1] > mu[0]) || !finite_d(mu[0]) || !finite_d(mu[1])) return;
    {
        const double k0 = log(w[0]) - 0.5 * log(TWO_PI * var[0]), k1 = log(w[1]) - 0.5 * log(TWO_PI * var[1]);
        int i0 = -1, i1 = -1;                            // the last bin of this chunk whose coordinate is <= mean 0 / mean 1
        for (int b = c.b_lo; b < c.b_hi; b++) {
            const double y = coord[b] - c.M;
            if (y <= mu[0]) i0 = b;
            if (y <= mu[1]) i1 = b;
        }
        int b0 = block_extreme_int(sh, i0, true), b1 = block_extreme_int(sh, i1, true);
        if (b0 < 0) b0 = 0;
        int first = n_bins;
        for (int b = c.b_lo; b < c.b_hi; b++) {
            if (b <= b0 || b > b1) continue;
            const double y = coord[b] - c.M, e0 = y - mu[0], e1 = y - mu[1];
            const double l0 = k0 - (e0 * e0) / (2.0 * var[0]), l1 = k1 - (e1 * e1) / (2.0 * var[1]);
            if (l1 >= l0) { first = b; break; }
        }
        const int bin = block_extreme_int(sh, first, false);
        if (bin >= n_bins) return;
        const HtClasses k = class_sums(sh, c, bin);
        HtRow r;
        r.crit = loglik; r.n0 = k.n[0]; r.n1 = k.n[1]; r.mean0 = mu[0] + c.M; r.mean1 = mu[1] + c.M;
        r.sd0 = sqrt(var[0]); r.sd1 = sqrt(var[1]); r.w1 = w[1]; r.iters = (double)iters; r.loglik = loglik;
        write_row(c, table, thr, 3, bin, r);
    }
}

extern "C" int bdn_hist_threshold(const unsigned long long* hist, const double* coord, const float* edges, int n_bins, int methods,
                                  int em_iters, double em_tol, double* table, float* thr, void* stream) {
    if (!hist || !coord || !edges || !table || !thr) BDN_FAIL(BDN_E_ARG, "hist_threshold: null pointer");
    if ((uintptr_t)hist % 8 || (uintptr_t)coord % 8 || (uintptr_t)table % 8 || (uintptr_t)edges % 4 || (uintptr_t)thr % 4)
        BDN_FAIL(BDN_E_ARG, "hist_threshold: hist / coord / table must be 8-byte, edges / thr 4-byte aligned");
    if (n_bins < 2 || n_bins > RH_MAX_BINS) BDN_FAIL(BDN_E_ARG, "hist_threshold: n_bins must be in 2..%d, got %d", RH_MAX_BINS, n_bins);
    if (methods < 1 || methods > (BDN_THR_OTSU | BDN_THR_KITTLER | BDN_THR_ROSIN | BDN_THR_EM))
        BDN_FAIL(BDN_E_ARG, "hist_threshold: methods must be a non-empty mask of BDN_THR_*, got %d", methods);
    if (em_iters < 1 || em_iters > 1000) BDN_FAIL(BDN_E_ARG, "hist_threshold: em_iters must be in 1..1000, got %d", em_iters);
    if (!(em_tol >= 0.0 && em_tol <= DBL_MAX)) BDN_FAIL(BDN_E_ARG, "hist_threshold: em_tol must be finite and >= 0, got %g", em_tol);
    hipLaunchKernelGGL(hist_threshold_kernel, dim3(1), dim3(HT_THREADS), 0, (hipStream_t)stream, hist, coord, edges, n_bins, methods, em_iters,
                       em_tol, table, thr);
    BDN_CHECK_LAUNCH("hist_threshold");
    return BDN_OK;
}

// ============================================================ raster_mask
// mask[i] = raster[i] >= *thr (below: < *thr) for a finite raster[i], 0 for a non-finite one, excluded_out where exclude[i] == exclude_value.
// Every comparison with a NaN threshold is false.  Four pixels per thread where HW and the pointers allow, one otherwise.
template <int PER>
__global__ __launch_bounds__(256) void raster_mask_kernel(const float* __restrict__ raster, const uint8_t* __restrict__ exclude, int exclude_value,
                                                          const float* __restrict__ thr, int below, int excluded_out,
                                                          uint8_t* __restrict__ mask, long long n_items) {
    const float th = *thr;
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_items; i += stride) {
        float v[PER];
        int ex[PER];
        PixVec<PER>::load(raster + i * PER, v);
        if (exclude) PixVec<PER>::labels(exclude + i * PER, ex);
        else {
#pragma unroll
            for (int p = 0; p < PER; p++) ex[p] = -1;
        }
        uint32_t o[PER];
#pragma unroll
        for (int p = 0; p < PER; p++)
            o[p] = ex[p] == exclude_value ? (uint32_t)excluded_out : (uint32_t)(finite_f(v[p]) && (below ? v[p] < th : v[p] >= th));
        if constexpr (PER == 4) reinterpret_cast<uint32_t*>(mask)[i] = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
        else mask[i] = (uint8_t)o[0];
    }
}

extern "C" int bdn_raster_mask(const float* raster, const uint8_t* exclude, int exclude_value, const float* thr, int below, int excluded_out,
                               uint8_t* mask, long long HW, void* stream) {
    if (!raster || !thr || !mask) BDN_FAIL(BDN_E_ARG, "raster_mask: null pointer");
    if ((uintptr_t)raster % 4 || (uintptr_t)thr % 4) BDN_FAIL(BDN_E_ARG, "raster_mask: raster and thr must be 4-byte aligned");
    if (!byte_value(exclude_value)) BDN_FAIL(BDN_E_ARG, "raster_mask: exclude_value must be a byte 0..255, got %d", exclude_value);
    if (!byte_value(excluded_out)) BDN_FAIL(BDN_E_ARG, "raster_mask: excluded_out must be a byte 0..255, got %d", excluded_out);
    if (below != 0 && below != 1) BDN_FAIL(BDN_E_ARG, "raster_mask: below must be 0 or 1, got %d", below);
    if (HW < 1 || HW > RH_MAX_PIXELS) BDN_FAIL(BDN_E_ARG, "raster_mask: need 1 <= HW <= 2^40, got %lld", HW);
    const bool vec = HW % 4 == 0 && (uintptr_t)raster % 16 == 0 && (uintptr_t)exclude % 4 == 0 && (uintptr_t)mask % 4 == 0;
    const long long n_items = vec ? HW / 4 : HW, want = (n_items + 255) / 256;
    const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(raster_mask_kernel<4>, dim3(blocks), dim3(256), 0, st, raster, exclude, exclude_value, thr, below, excluded_out, mask, n_items);
    else hipLaunchKernelGGL(raster_mask_kernel<1>, dim3(blocks), dim3(256), 0, st, raster, exclude, exclude_value, thr, below, excluded_out, mask, n_items);
    BDN_CHECK_LAUNCH("raster_mask");
    return BDN_OK;
}
