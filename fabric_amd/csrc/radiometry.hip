// Radiometric matching of the two dates of a scene: exact order statistics per band at many ranks at once (bdn_band_quantiles), the
// pointwise piecewise-linear transfer between two knot tables (bdn_transfer_apply) and the percentile stretch to bytes (bdn_stretch_u8).
// include/bidate_hip.h states the semantics and the exact operation order; tests/radiometry_ref.py restates them in numpy.
//
// bdn_band_quantiles: a radix select over the monotone 32-bit key of a float32 (common.hpp: topk_key) in three levels of 11 + 11 + 10 bits,
// for the 2 n_q ranks {lo, hi} of the n_q probabilities of every band together.  Integer histograms only: a histogram is a sum of ones, so
// the order of the atomic adds cannot change it.  Per group of bands (rq_group: as many bands as fit a 128 MiB workspace), seven launches
// whatever the data:
//   memset    the three histogram levels of the group
//   hist<0>   grid (blocks, bands): a 2048-bin LDS histogram of key >> 21 over the valid pixels of the block's chunks, flushed with one
//             global add per non-empty bin
//   select0   one block per band: n = the histogram's total -> count; per rank entry j (2 q: lo, 2 q + 1: hi) the top digit and the
//             rank that remains inside it; map0[digit] = the smallest entry j that wants the digit (its slot), NONE elsewhere
//   hist<1>   a pixel whose top digit has a slot adds one to hist1[slot][(key >> 10) & 2047]
//   select1   grid (2 n_q slots, bands): the block of a slot in use scans its histogram, advances the entries of the slot by the second
//             digit and OVERWRITES the slot's histogram with map1[digit] = the smallest entry that wants (top digit, digit), NONE elsewhere
//   hist<2>   a pixel whose 22-bit prefix has a slot adds one to hist2[slot][key & 1023]
//   final     grid (n_q, bands): scans the (at most two) level-2 histograms of lo and hi, forms the keys, writes order and value
// No block waits for another; every word of the workspace that is read was written by the same call.
// Ties: a wave first gathers the lanes that add to the same counter (rq_peel: one ballot per distinct counter), so a constant band or a
// nodata area costs one add per wave, not 64 on one address; leaders that stand for two lanes or more go through a small LDS table
// (counter -> count) that the block flushes once, so a band of few distinct values costs a block as many global adds as it has values.
// bdn_transfer_apply, one launch: grid (blocks, C); the block of a named band stages its two knot tables in LDS (8 KiB at K = 1024).
// bdn_stretch_u8, one launch.
#include "common.hpp"
#include <float.h>
#include <math.h>

constexpr int RQ_MAXQ = 1024, RQ_MAXBANDS = 64, RQ_MAXDIM = 32767, RQ_MAXC = 65535, RQ_MAXK = 1024;
constexpr int RQ_B0 = 2048, RQ_B1 = 2048, RQ_B2 = 1024;      // bins of the three levels: 11 + 11 + 10 bits
constexpr unsigned RQ_NONE = 0xFFFFFFFFu;
constexpr size_t RQ_WS_CAP = (size_t)128 << 20;
constexpr int RQ_HT = 1024;                                  // entries of the block's tie table

// bytes of one band in the workspace: hist0, hist1 (later map1), hist2, map0, and the entries after select0 and after select1
static inline size_t rq_band_bytes(int n_q) {
    const size_t S = 2 * (size_t)n_q;
    return sizeof(unsigned) * (RQ_B0 + S * RQ_B1 + S * RQ_B2 + RQ_B0) + 2 * S * sizeof(uint2);
}
// bands per group: the whole list if it fits the cap, never fewer than one (one band at n_q = 1024 takes 24.1 MiB)
static inline int rq_group(int n_b, int n_q) {
    size_t g = RQ_WS_CAP / rq_band_bytes(n_q);
    if (g < 1) g = 1;
    return g > (size_t)n_b ? n_b : (int)g;
}
struct RqLayout { unsigned* hist0; unsigned* hist1; unsigned* hist2; unsigned* map0; uint2* rk0; uint2* rk1; size_t hist_bytes; };
static inline RqLayout rq_layout(void* ws, int G, int n_q) {
    const size_t S = 2 * (size_t)n_q;
    RqLayout l;
    l.hist0 = (unsigned*)ws;
    l.hist1 = l.hist0 + (size_t)G * RQ_B0;
    l.hist2 = l.hist1 + (size_t)G * S * RQ_B1;
    l.map0 = l.hist2 + (size_t)G * S * RQ_B2;
    l.hist_bytes = (size_t)((char*)l.map0 - (char*)ws);
    l.rk0 = (uint2*)(l.map0 + (size_t)G * RQ_B0);            // an even number of words lies in front: 8-byte aligned
    l.rk1 = l.rk0 + (size_t)G * S;
    return l;
}

// one rounding per operation (the caller's contraction is not inherited): what numpy float64 / float32 does
__device__ __forceinline__ double rq_dmul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double rq_dsub(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double rq_dadd(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float rq_fmul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float rq_fadd(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float rq_fsub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// ---------------------------------------------------------------- the histograms
// The lanes of the wave that hold the same `what` (among the `active` ones) elect the lowest of them: it returns how many they are, the
// others 0.  One ballot per distinct value in the wave.  Every lane of the wave must call it.
__device__ __forceinline__ unsigned rq_peel(unsigned what, bool active) {
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long todo = __ballot(active);
    unsigned mine = 0;
    while (todo) {
        const int l = __ffsll((long long)todo) - 1;
        const unsigned w = (unsigned)__builtin_amdgcn_readlane((int)what, l);
        const unsigned long long m = __ballot(active && what == w);
        if (lane == l) mine = (unsigned)__popcll(m);
        todo &= ~m;
    }
    return mine;
}

// add c to counter `idx` of the global histogram g through the block's tie table (keys, counts in LDS); a full neighbourhood falls through
__device__ __forceinline__ void rq_table_add(unsigned* hk, unsigned* hc, unsigned* __restrict__ g, unsigned idx, unsigned c) {
    unsigned h = (idx * 2654435761u) >> 22;                  // 10 bits: RQ_HT entries
#pragma unroll 1
    for (int probe = 0; probe < 4; probe++) {
        const unsigned old = atomicCAS(&hk[h], RQ_NONE, idx);
        if (old == RQ_NONE || old == idx) { atomicAdd(&hc[h], c); return; }
        h = (h + 1) & (RQ_HT - 1);
    }
    atomicAdd(&g[idx], c);
}

struct RqHistArgs {
    const float* scene; const int32_t* bands; const uint8_t* excl; int exv, positive_only;
    unsigned* hist; const unsigned* map0; const unsigned* map1;
    int C, S; unsigned npix, nchunks;
};

template <int LEVEL>
__global__ __launch_bounds__(256) void rq_hist_kernel(const RqHistArgs a) {
    __shared__ unsigned sm[RQ_B0];                           // level 0: the block's histogram; levels 1, 2: map0 of the band
    __shared__ unsigned hk[LEVEL == 0 ? 1 : RQ_HT];
    __shared__ unsigned hc[LEVEL == 0 ? 1 : RQ_HT];
    const int tid = threadIdx.x, b = blockIdx.y;
    const int band = a.bands[b];
    if (band < 0 || band >= a.C) return;                     // (uniform) an index outside the stack reads nothing: its count is 0
    const float* plane = a.scene + (size_t)band * a.npix;
    unsigned* g;
    const unsigned* m1 = nullptr;
    if constexpr (LEVEL == 0) {
        g = a.hist + (size_t)b * RQ_B0;
        for (int i = tid; i < RQ_B0; i += 256) sm[i] = 0;
    } else {
        g = a.hist + (size_t)b * a.S * (LEVEL == 1 ? RQ_B1 : RQ_B2);
        for (int i = tid; i < RQ_B0; i += 256) sm[i] = a.map0[(size_t)b * RQ_B0 + i];
        for (int i = tid; i < RQ_HT; i += 256) { hk[i] = RQ_NONE; hc[i] = 0; }
        if constexpr (LEVEL == 2) m1 = a.map1 + (size_t)b * a.S * RQ_B1;
    }
    __syncthreads();
    for (unsigned chunk = blockIdx.x; chunk < a.nchunks; chunk += gridDim.x) {       // (uniform) a chunk is 1024 consecutive pixels
        float v[4]; bool ok[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const unsigned p = chunk * 1024u + (unsigned)k * 256u + (unsigned)tid;   // < 2^30 + 1024
            ok[k] = p < a.npix;
            v[k] = ok[k] ? plane[p] : 0.f;
            if (ok[k] && a.excl) ok[k] = a.excl[p] != a.exv;
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            bool act = ok[k] && fabsf(v[k]) <= FLT_MAX && (!a.positive_only || v[k] > 0.f);
            const unsigned key = topk_key(v[k]);
            if constexpr (LEVEL == 0) {
                const unsigned d = key >> 21;
                const unsigned long long am = __ballot(act);
                const int first = am ? __ffsll((long long)am) - 1 : 0;
                const unsigned d0 = (unsigned)__builtin_amdgcn_readlane((int)d, first);  // the first valid lane's bin
                if (am && __ballot(act && d == d0) == am) {  // every valid lane of the wave in one bin: one add
                    if ((int)(threadIdx.x & 63) == first) atomicAdd(&sm[d], (unsigned)__popcll(am));
                } else if (act) atomicAdd(&sm[d], 1u);
            } else {
                unsigned idx = 0;
                if (act) {
                    const unsigned s0 = sm[key >> 21];
                    act = s0 != RQ_NONE;
                    if constexpr (LEVEL == 1) {
                        if (act) idx = s0 * RQ_B1 + ((key >> 10) & (RQ_B1 - 1));
                    } else {
                        if (act) {
                            const unsigned s1 = m1[(size_t)s0 * RQ_B1 + ((key >> 10) & (RQ_B1 - 1))];
                            act = s1 != RQ_NONE;
                            if (act) idx = s1 * RQ_B2 + (key & (RQ_B2 - 1));
                        }
                    }
                }
                const unsigned c = rq_peel(idx, act);
                if (c >= 2) rq_table_add(hk, hc, g, idx, c);
                else if (c == 1) atomicAdd(&g[idx], 1u);
            }
        }
    }
    __syncthreads();
    if constexpr (LEVEL == 0) {
        for (int i = tid; i < RQ_B0; i += 256) { const unsigned c = sm[i]; if (c) atomicAdd(&g[i], c); }
    } else {
        for (int i = tid; i < RQ_HT; i += 256) { const unsigned k = hk[i]; if (k != RQ_NONE) atomicAdd(&g[k], hc[i]); }
    }
}

// ---------------------------------------------------------------- the selects
// cum[0 .. NB] = the exclusive prefix sums of the NB counts at src (cum[NB] = their total), by a block of 256 threads
template <int NB>
__device__ void rq_scan(const unsigned* __restrict__ src, unsigned* cum, unsigned* part) {
    constexpr int PER = NB / 256;
    const int tid = threadIdx.x;
    unsigned c[PER], s = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) { c[k] = src[tid * PER + k]; s += c[k]; }
    part[tid] = s;
    __syncthreads();
    if (tid == 0) { unsigned run = 0; for (int i = 0; i < 256; i++) { const unsigned t = part[i]; part[i] = run; run += t; } cum[NB] = run; }
    __syncthreads();
    unsigned run = part[tid];
#pragma unroll
    for (int k = 0; k < PER; k++) { cum[tid * PER + k] = run; run += c[k]; }
    __syncthreads();
}
// the last d in [0, NB) with cum[d] <= r, for r < cum[NB]: the bin that holds rank r (its count is not 0)
template <int NB>
__device__ __forceinline__ unsigned rq_find(const unsigned* cum, unsigned r) {
    unsigned lo = 0, hi = NB - 1;
    while (lo < hi) { const unsigned mid = (lo + hi + 1) >> 1; if (cum[mid] <= r) lo = mid; else hi = mid - 1; }
    return lo;
}
// the rank of entry j (2 q: lo, 2 q + 1: hi) among n valid pixels, and t = h - lo; false when p lies outside [0, 1] (NaN included)
__device__ __forceinline__ bool rq_rank(double p, unsigned n, int j, unsigned& r, double& t) {
    if (n == 0 || !(p >= 0.0 && p <= 1.0)) return false;
    const double h = rq_dmul(p, (double)(n - 1));
    const double fl = floor(h);
    const unsigned lo = (unsigned)fl, hi = lo + 1 < n ? lo + 1 : n - 1;
    t = rq_dsub(h, fl);
    r = (j & 1) ? hi : lo;
    return true;
}

__global__ __launch_bounds__(256) void rq_select0_kernel(const unsigned* __restrict__ hist0, const double* __restrict__ probs, int n_q,
                                                         unsigned* __restrict__ map0, uint2* __restrict__ rk0, long long* __restrict__ count) {
    __shared__ unsigned cum[RQ_B0 + 1];
    __shared__ unsigned slot[RQ_B0];
    __shared__ unsigned part[256];
    const int tid = threadIdx.x, b = blockIdx.x, S = 2 * n_q;
    for (int i = tid; i < RQ_B0; i += 256) slot[i] = RQ_NONE;
    rq_scan<RQ_B0>(hist0 + (size_t)b * RQ_B0, cum, part);
    const unsigned n = cum[RQ_B0];
    if (tid == 0) count[b] = (long long)n;
    for (int j = tid; j < S; j += 256) {
        unsigned r; double t;
        uint2 e = make_uint2(0u, RQ_NONE);
        if (rq_rank(probs[j >> 1], n, j, r, t)) {
            const unsigned d = rq_find<RQ_B0>(cum, r);
            e = make_uint2(d << 21, r - cum[d]);
            atomicMin(&slot[d], (unsigned)j);
        }
        rk0[(size_t)b * S + j] = e;
    }
    __syncthreads();
    for (int i = tid; i < RQ_B0; i += 256) map0[(size_t)b * RQ_B0 + i] = slot[i];
}

__global__ __launch_bounds__(256) void rq_select1_kernel(unsigned* __restrict__ hist1, const unsigned* __restrict__ map0,
                                                         const uint2* __restrict__ rk0, uint2* __restrict__ rk1, int n_q) {
    __shared__ unsigned cum[RQ_B1 + 1];
    __shared__ unsigned slot[RQ_B1];
    __shared__ unsigned part[256];
    const int tid = threadIdx.x, s = blockIdx.x, b = blockIdx.y, S = 2 * n_q;
    const unsigned* m0 = map0 + (size_t)b * RQ_B0;
    const uint2* in = rk0 + (size_t)b * S;
    const uint2 own = in[s];
    if (own.y == RQ_NONE || m0[own.x >> 21] != (unsigned)s) return;            // (uniform) not a slot in use
    unsigned* h = hist1 + ((size_t)b * S + s) * RQ_B1;
    for (int i = tid; i < RQ_B1; i += 256) slot[i] = RQ_NONE;
    rq_scan<RQ_B1>(h, cum, part);                            // every count is in registers or LDS behind its barriers
    for (int j = tid; j < S; j += 256) {
        const uint2 e = in[j];
        if (e.y == RQ_NONE || m0[e.x >> 21] != (unsigned)s) continue;
        const unsigned d = rq_find<RQ_B1>(cum, e.y);         // e.y < cum[RQ_B1]: the slot's histogram holds every key of the top digit
        rk1[(size_t)b * S + j] = make_uint2(e.x | (d << 10), e.y - cum[d]);
        atomicMin(&slot[d], (unsigned)j);
    }
    __syncthreads();
    for (int i = tid; i < RQ_B1; i += 256) h[i] = slot[i];  // the slot's histogram becomes its map
}

__global__ __launch_bounds__(256) void rq_final_kernel(const unsigned* __restrict__ hist0, const unsigned* __restrict__ hist2,
                                                       const unsigned* __restrict__ map0, const unsigned* __restrict__ map1,
                                                       const uint2* __restrict__ rk0, const uint2* __restrict__ rk1,
                                                       const double* __restrict__ probs, int n_q, const long long* __restrict__ count,
                                                       double* __restrict__ value, float* __restrict__ order) {
    __shared__ unsigned cum[RQ_B2 + 1];
    __shared__ unsigned part[256];
    __shared__ unsigned found[2];
    const int tid = threadIdx.x, q = blockIdx.x, b = blockIdx.y, S = 2 * n_q;
    const unsigned n = (unsigned)count[b];
    unsigned r; double t = 0.0;
    const bool ok = rq_rank(probs[q], n, 0, r, t);           // (uniform)
    if (!ok) {
        if (tid == 0) {
            value[(size_t)b * n_q + q] = (double)NAN;
            order[((size_t)b * n_q + q) * 2] = NAN; order[((size_t)b * n_q + q) * 2 + 1] = NAN;
        }
        return;
    }
    if (tid < 2) found[tid] = RQ_NONE;                       // (the key of a NaN) ordered before the writes below by rq_scan's barriers
    for (int e = 0; e < 2; e++) {
        const uint2 k = rk1[(size_t)b * S + 2 * q + e];
        const unsigned s0 = map0[(size_t)b * RQ_B0 + (k.x >> 21)];
        const unsigned s1 = map1[((size_t)b * S + s0) * RQ_B1 + ((k.x >> 10) & (RQ_B1 - 1))];
        __syncthreads();                                     // the previous entry's cum has been read
        rq_scan<RQ_B2>(hist2 + ((size_t)b * S + s1) * RQ_B2, cum, part);
        for (int d = tid * 4; d < tid * 4 + 4; d++)
            if (cum[d] <= k.y && k.y < cum[d + 1]) found[e] = k.x | (unsigned)d;         // one bin of the 1024 holds the rank
    }
    __syncthreads();
    if (tid == 0) {
        const float lo = topk_unkey(found[0]), hi = topk_unkey(found[1]);
        order[((size_t)b * n_q + q) * 2] = lo; order[((size_t)b * n_q + q) * 2 + 1] = hi;
        const double a = (double)lo, c = (double)hi;
        value[(size_t)b * n_q + q] = rq_dadd(a, rq_dmul(rq_dsub(c, a), t));
    }
}

static bool rq_scene_ok(int C, int H, int W) { return C >= 1 && C <= RQ_MAXC && H >= 1 && W >= 1 && H <= RQ_MAXDIM && W <= RQ_MAXDIM; }

extern "C" size_t bdn_band_quantiles_workspace_bytes(int n_b, int n_q, int H, int W) {
    if (n_b < 1 || n_b > RQ_MAXBANDS || n_q < 1 || n_q > RQ_MAXQ || !rq_scene_ok(1, H, W)) return 0;
    return (size_t)rq_group(n_b, n_q) * rq_band_bytes(n_q);
}

extern "C" int bdn_band_quantiles(const float* scene, const int32_t* bands, int n_b, const uint8_t* exclude, int exclude_value, int positive_only,
                                  const double* probs, int n_q, double* value, float* order, long long* count, void* ws, int C, int H, int W,
                                  void* stream) {
    if (!scene || !bands || !probs || !value || !order || !count || !ws) BDN_FAIL(BDN_E_ARG, "band_quantiles: null pointer");
    if (n_b < 1 || n_b > RQ_MAXBANDS) BDN_FAIL(BDN_E_ARG, "band_quantiles: n_b=%d band indices (1..%d)", n_b, RQ_MAXBANDS);
    if (n_q < 1 || n_q > RQ_MAXQ) BDN_FAIL(BDN_E_ARG, "band_quantiles: n_q=%d probabilities (1..%d)", n_q, RQ_MAXQ);
    if (!rq_scene_ok(C, H, W)) BDN_FAIL(BDN_E_ARG, "band_quantiles: bad scene %d x %d x %d (1 <= C <= %d; 1 <= H, W <= %d)", C, H, W, RQ_MAXC, RQ_MAXDIM);
    if (exclude && (exclude_value < 0 || exclude_value > 255)) BDN_FAIL(BDN_E_ARG, "band_quantiles: exclude_value=%d must be a byte value (0..255)", exclude_value);
    if (positive_only != 0 && positive_only != 1) BDN_FAIL(BDN_E_ARG, "band_quantiles: positive_only=%d must be 0 or 1", positive_only);
    if (((uintptr_t)scene & 3) || ((uintptr_t)bands & 3) || ((uintptr_t)order & 3) || ((uintptr_t)probs & 7) || ((uintptr_t)value & 7) ||
        ((uintptr_t)count & 7) || ((uintptr_t)ws & 15))
        BDN_FAIL(BDN_E_ARG, "band_quantiles: scene, bands and order must be 4-byte aligned, probs, value and count 8-byte and ws 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int G = rq_group(n_b, n_q), S = 2 * n_q;
    const RqLayout l = rq_layout(ws, G, n_q);
    const unsigned npix = (unsigned)H * (unsigned)W, nchunks = (npix + 1023u) / 1024u;
    for (int b0 = 0; b0 < n_b; b0 += G) {
        const int g = n_b - b0 < G ? n_b - b0 : G;
        if (hipMemsetAsync(ws, 0, l.hist_bytes, st) != hipSuccess) BDN_FAIL(BDN_E_HIP, "band_quantiles: memset failed");
        unsigned gx = 4096u / (unsigned)g;
        if (gx > nchunks) gx = nchunks;
        RqHistArgs a{scene, bands + b0, exclude, exclude_value, positive_only, l.hist0, l.map0, l.hist1, C, S, npix, nchunks};
        hipLaunchKernelGGL(rq_hist_kernel<0>, dim3(gx, (unsigned)g), dim3(256), 0, st, a);
        BDN_CHECK_LAUNCH("band_quantiles_hist0");
        hipLaunchKernelGGL(rq_select0_kernel, dim3((unsigned)g), dim3(256), 0, st, l.hist0, probs, n_q, l.map0, l.rk0, count + b0);
        BDN_CHECK_LAUNCH("band_quantiles_select0");
        a.hist = l.hist1;
        hipLaunchKernelGGL(rq_hist_kernel<1>, dim3(gx, (unsigned)g), dim3(256), 0, st, a);
        BDN_CHECK_LAUNCH("band_quantiles_hist1");
        hipLaunchKernelGGL(rq_select1_kernel, dim3((unsigned)S, (unsigned)g), dim3(256), 0, st, l.hist1, l.map0, l.rk0, l.rk1, n_q);
        BDN_CHECK_LAUNCH("band_quantiles_select1");
        a.hist = l.hist2;
        hipLaunchKernelGGL(rq_hist_kernel<2>, dim3(gx, (unsigned)g), dim3(256), 0, st, a);
        BDN_CHECK_LAUNCH("band_quantiles_hist2");
        hipLaunchKernelGGL(rq_final_kernel, dim3((unsigned)n_q, (unsigned)g), dim3(256), 0, st, l.hist0, l.hist2, l.map0, l.hist1, l.rk0, l.rk1,
                           probs, n_q, count + b0, value + (size_t)b0 * n_q, order + (size_t)b0 * n_q * 2);
        BDN_CHECK_LAUNCH("band_quantiles_final");
    }
    return BDN_OK;
}

// ---------------------------------------------------------------- the transfer
__device__ __forceinline__ float rq_offset(float x, float s, float t) {
    const float d = rq_fsub(t, s);
    return d == 0.f ? x : rq_fadd(x, d);                     // a zero offset returns the bits (-0.0 stays -0.0)
}
__device__ __forceinline__ float rq_segment(float x, const float* sk, const float* tk, int k) {
    const float s0 = sk[k], s1 = sk[k + 1], t0 = tk[k], t1 = tk[k + 1];
    if (s0 == t0 && s1 == t1) return x;                      // an identity segment returns the bits
    return rq_fadd(t0, rq_fmul(rq_fsub(x, s0), __fdiv_rn(rq_fsub(t1, t0), rq_fsub(s1, s0))));
}

__global__ __launch_bounds__(256) void rq_transfer_kernel(const float* __restrict__ src, float* __restrict__ out, const int32_t* __restrict__ bands,
                                                          int n_b, const float* __restrict__ s_knots, const float* __restrict__ t_knots, int K,
                                                          int slope, const uint8_t* __restrict__ exact, unsigned npix) {
    __shared__ float sk[RQ_MAXK];
    __shared__ float tk[RQ_MAXK];
    const int tid = threadIdx.x, c = blockIdx.y;
    int b = -1;
    for (int i = 0; i < n_b; i++) if (bands[i] == c) { b = i; break; }        // (uniform) the first row that names the band
    const float* sp = src + (size_t)c * npix;
    float* op = out + (size_t)c * npix;
    const unsigned step = gridDim.x * 256u;
    int through = b < 0 || (exact && exact[b]) ? 1 : 0;
    if (b >= 0) {                                            // (uniform)
        int bad = 0;
        for (int i = tid; i < K; i += 256) {
            const float s = s_knots[(size_t)b * K + i], t = t_knots[(size_t)b * K + i];
            sk[i] = s; tk[i] = t;
            bad |= (s != s || t != t) ? 1 : 0;
        }
        through |= __syncthreads_or(bad);                    // a band without valid pixels in either date has NaN knots: it passes through
    }
    if (through) {
        if (out != src) for (unsigned p = blockIdx.x * 256u + tid; p < npix; p += step) op[p] = sp[p];
        return;
    }
    const float s_lo = sk[0], s_hi = sk[K - 1];
    for (unsigned p = blockIdx.x * 256u + tid; p < npix; p += step) {
        const float x = sp[p];
        float y = x;
        if (fabsf(x) <= FLT_MAX) {
            if (x < s_lo) y = (slope && sk[1] > sk[0]) ? rq_segment(x, sk, tk, 0) : rq_offset(x, sk[0], tk[0]);
            else if (x >= s_hi) y = (slope && sk[K - 1] > sk[K - 2]) ? rq_segment(x, sk, tk, K - 2) : rq_offset(x, sk[K - 1], tk[K - 1]);
            else {
                int lo = 0, hi = K - 2;                      // the last k with sk[k] <= x; sk[0] <= x < sk[K - 1]
                while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (sk[mid] <= x) lo = mid; else hi = mid - 1; }
                y = rq_segment(x, sk, tk, lo);
            }
        }
        op[p] = y;
    }
}

extern "C" int bdn_transfer_apply(const float* src, float* out, const int32_t* bands, int n_b, const float* s_knots, const float* t_knots, int K,
                                  int extrapolate, const uint8_t* exact, int C, int H, int W, void* stream) {
    if (!src || !out || !bands || !s_knots || !t_knots) BDN_FAIL(BDN_E_ARG, "transfer_apply: null pointer");
    if (n_b < 1 || n_b > RQ_MAXBANDS) BDN_FAIL(BDN_E_ARG, "transfer_apply: n_b=%d band indices (1..%d)", n_b, RQ_MAXBANDS);
    if (K < 2 || K > RQ_MAXK) BDN_FAIL(BDN_E_ARG, "transfer_apply: K=%d knots (2..%d)", K, RQ_MAXK);
    if (extrapolate != BDN_EXTRAPOLATE_OFFSET && extrapolate != BDN_EXTRAPOLATE_SLOPE)
        BDN_FAIL(BDN_E_ARG, "transfer_apply: extrapolate=%d is neither BDN_EXTRAPOLATE_OFFSET (0) nor BDN_EXTRAPOLATE_SLOPE (1)", extrapolate);
    if (!rq_scene_ok(C, H, W)) BDN_FAIL(BDN_E_ARG, "transfer_apply: bad scene %d x %d x %d (1 <= C <= %d; 1 <= H, W <= %d)", C, H, W, RQ_MAXC, RQ_MAXDIM);
    if (((uintptr_t)src & 3) || ((uintptr_t)out & 3) || ((uintptr_t)bands & 3) || ((uintptr_t)s_knots & 3) || ((uintptr_t)t_knots & 3))
        BDN_FAIL(BDN_E_ARG, "transfer_apply: src, out, bands and the knot tables must be 4-byte aligned");
    const unsigned npix = (unsigned)H * (unsigned)W;
    unsigned gx = grid_for(npix);
    if (gx > 1024u) gx = 1024u;
    hipLaunchKernelGGL(rq_transfer_kernel, dim3(gx, (unsigned)C), dim3(256), 0, (hipStream_t)stream, src, out, bands, n_b, s_knots, t_knots, K,
                       extrapolate == BDN_EXTRAPOLATE_SLOPE ? 1 : 0, exact, npix);
    BDN_CHECK_LAUNCH("transfer_apply");
    return BDN_OK;
}

// ---------------------------------------------------------------- the stretch to bytes
template <typename T>
__global__ __launch_bounds__(256) void rq_stretch_kernel(const T* __restrict__ src, const double* __restrict__ cd, uint8_t* __restrict__ out,
                                                         unsigned npix) {
    const int c = blockIdx.y;
    const double lo = cd[2 * c], scale = __ddiv_rn(255.0, rq_dsub(cd[2 * c + 1], lo));
    const T* sp = src + (size_t)c * npix;
    uint8_t* op = out + (size_t)c * npix;
    for (unsigned p = blockIdx.x * 256u + threadIdx.x; p < npix; p += gridDim.x * 256u) {
        const double v = rq_dmul(rq_dsub((double)sp[p], lo), scale);
        op[p] = v > 255.0 ? (uint8_t)255 : v > 0.0 ? (uint8_t)(int)v : (uint8_t)0;       // NaN fails both comparisons: 0
    }
}

extern "C" int bdn_stretch_u8(const void* src, int src_is_u16, const double* cd, uint8_t* out, int C, int H, int W, void* stream) {
    if (!src || !cd || !out) BDN_FAIL(BDN_E_ARG, "stretch_u8: null pointer");
    if (src_is_u16 != 0 && src_is_u16 != 1) BDN_FAIL(BDN_E_ARG, "stretch_u8: src_is_u16=%d must be 0 (float32) or 1 (uint16)", src_is_u16);
    if (!rq_scene_ok(C, H, W)) BDN_FAIL(BDN_E_ARG, "stretch_u8: bad scene %d x %d x %d (1 <= C <= %d; 1 <= H, W <= %d)", C, H, W, RQ_MAXC, RQ_MAXDIM);
    if (((uintptr_t)src & (src_is_u16 ? 1 : 3)) || ((uintptr_t)cd & 7))
        BDN_FAIL(BDN_E_ARG, "stretch_u8: src must be aligned to its element (4 bytes float32, 2 bytes uint16), cd 8-byte aligned");
    const unsigned npix = (unsigned)H * (unsigned)W;
    unsigned gx = grid_for(npix);
    if (gx > 1024u) gx = 1024u;
    if (src_is_u16)
        hipLaunchKernelGGL(rq_stretch_kernel<uint16_t>, dim3(gx, (unsigned)C), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)src, cd, out, npix);
    else
        hipLaunchKernelGGL(rq_stretch_kernel<float>, dim3(gx, (unsigned)C), dim3(256), 0, (hipStream_t)stream, (const float*)src, cd, out, npix);
    BDN_CHECK_LAUNCH("stretch_u8");
    return BDN_OK;
}
