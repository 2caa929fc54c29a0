// Lovasz-Softmax (Berman, Rahman Triki, Blaschko, CVPR 2018; batch level, per_image = False) on the classifier's float32 NCHW logits and
// uint8 labels: bdn_lovasz_softmax, the add-on term of the criterion family of loss.hip (include/bidate_hip.h states the semantics).
//
// For every class the valid pixels are sorted by err = |fg - p_c| descending -- a stable LSD radix sort of (key, pixel index) pairs,
// four passes of eight bits -- and the loss is the dot product of the sorted errors with the increments of the Jaccard index along the
// order.  The sort key of a valid pixel is ~topk_key(err) (common.hpp): ascending sort keys are descending topk keys.  err carries a
// clear sign bit (it is an absolute value, NaN included), so topk_key(err) >= 0x80000000 and the sort key is <= 0x7FFFFFFF; an
// ignored pixel gets the sort key 0xFFFFFFFF and lands behind every valid one.  The pairs start in pixel-index order and every pass is
// stable, so equal keys keep the lower pixel index first.  The payload is the pixel index (< 2^31) with the foreground bit on top; key
// and payload travel as one 8-byte pair (one scattered store per element and pass).
//
// Launches (all classes in one grid, the class as grid.y; TILE = 4096 elements per block = 4 waves x 16 rounds x 64 lanes):
//   prep      softmax once per pixel -> the pairs of every class, the digit histogram of pass 0 per (class, tile), the valid count per
//             tile, pixel_errors
//   per pass  hist (passes 1..3: digit counts per (class, tile), LDS integer atomics), rowscan (one wave per (class, digit): exclusive scan
//             of that digit's counts over the tiles, and the digit's total), scatter (the block scans the 256 digit totals, a wave ranks its
//             1024 consecutive elements by digit with ballots, round by round; the destination order inside a digit is tile, wave, round,
//             lane = the source order)
//   fgcount   foreground pixels per tile of the sorted order
//   rowscan   the same kernel over the tile counts (a class's total is G), and n = the sum of the tiles' valid counts
//   coef      per sorted element: c_prev from a block scan, the coefficient g in double from the integers I and U, err * g summed in
//             double (thread-serial over 16 consecutive ranks, then an LDS tree: a fixed order), g with its sign scattered to the pixel,
//             ranks
//   finish    the tiles' partials per class in a fixed order, the included classes, term, loss, the per-class gradient scale 1 / m
//   grad      dlogit_j = weight p_j (q_j - sum_c q_c p_c), written or added once per element (none with dlogits == NULL)
// 17 launches with a gradient, whatever the data; LDS integer atomics only, no float atomics, no host read-back, no block waits for
// another; every workspace byte that is read has been written by an earlier launch of the same call.
// ws (N' = N rounded up to 4, nt = tiles, nt' = nt rounded up to 4): [pairs A C*N' x 8 B][pairs B C*N' x 8 B -- its front holds the scattered
//     coefficients after the sort][hist C*256*nt' u32][digit totals C*256 u32][tile fg counts C*nt' u32][tile valid counts nt i32]
//     [partials C*nt f64][G per class, n: 16 x u32][class scales 8 x f32], every part padded to 16 bytes: 16 bytes per pixel and class.
#include "common.hpp"

constexpr int LV_TILE = 4096, LV_ROUNDS = 16;             // 256 threads x 16 elements
constexpr unsigned LV_IGNORED = 0xFFFFFFFFu;              // sort key of an ignored pixel: behind every valid key (<= 0x7FFFFFFF)
constexpr unsigned LV_FG = 0x80000000u;                   // payload: pixel index | LV_FG at a foreground pixel of the class

static inline size_t lv_up16(size_t v) { return (v + 15) / 16 * 16; }
struct LovaszPlan { int npix, nt, nt4; size_t cs, o_kpA, o_kpB, o_hist, o_dtot, o_tfg, o_pval, o_part, o_meta, o_scale, total; };
static LovaszPlan lovasz_plan(int B, int ncls, int H, int W) {
    LovaszPlan p;
    p.npix = B * H * W;
    p.nt = (p.npix + LV_TILE - 1) / LV_TILE;
    p.nt4 = (p.nt + 3) / 4 * 4;                            // row stride of the per-tile tables: rows stay 16-byte aligned
    p.cs = ((size_t)p.npix + 3) / 4 * 4;                   // elements between the classes of a per-pixel array, for the same reason
    const size_t arr = sizeof(uint2) * (size_t)ncls * p.cs;
    p.o_kpA = 0; p.o_kpB = arr;
    p.o_hist = 2 * arr;
    p.o_dtot = p.o_hist + sizeof(unsigned) * (size_t)ncls * 256 * p.nt4;
    p.o_tfg = p.o_dtot + sizeof(unsigned) * (size_t)ncls * 256;
    p.o_pval = p.o_tfg + sizeof(unsigned) * (size_t)ncls * p.nt4;
    p.o_part = lv_up16(p.o_pval + sizeof(int32_t) * (size_t)p.nt);
    p.o_meta = p.o_part + sizeof(double) * (size_t)ncls * p.nt;
    p.o_scale = p.o_meta + sizeof(unsigned) * 16;
    p.total = lv_up16(p.o_scale + sizeof(float) * 8);
    return p;
}

// one count per active lane into an LDS histogram.  AGG (the top digit: sign, exponent and a mantissa bit of an error in [0, 1] take a
// handful of values, and same-address LDS atomics serialise): lanes of a wave that share a digit add once, as loss.hip's topk_hist_kernel
// does; the lower digits are spread over the bins and go lane by lane.
template <bool AGG>
__device__ __forceinline__ void lv_hist_add(unsigned* lh, unsigned digit, bool active, int lane) {
    if constexpr (AGG) {
        for (int round = 0; round < 4; round++) {
            const unsigned long long am = __ballot(active);
            if (am == 0) break;                            // wave-uniform
            const int leader = __ffsll((long long)am) - 1;
            const unsigned d0 = __shfl(digit, leader);
            const bool same = active && digit == d0;
            const unsigned long long sm = __ballot(same);
            if (lane == leader) atomicAdd(&lh[d0], (unsigned)__popcll(sm));
            active = active && !same;
        }
    }
    if (active) atomicAdd(&lh[digit], 1u);
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ unsigned lv_wave_scan(unsigned v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const unsigned u = __shfl_up(v, off); if (lane >= off) v += u; }
    return v;
}

// exclusive scan of one value per thread over a block of 256 threads (thread order); total = the block's sum
__device__ __forceinline__ unsigned lv_block_scan(unsigned v, unsigned& total) {
    __shared__ unsigned wsum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned inc = lv_wave_scan(v, lane);
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    unsigned pre = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) { const unsigned s = wsum[w]; if (w < wave) pre += s; tot += s; }
    __syncthreads();                                       // (wsum is free for the next call)
    total = tot;
    return pre + inc - v;
}

// ---------------------------------------------------------------- prep: errors -> pairs, pass-0 histogram, valid counts
__global__ __launch_bounds__(256) void lovasz_prep_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels, int ignore,
                                                          uint2* __restrict__ kp, unsigned* __restrict__ hist, int32_t* __restrict__ pval,
                                                          float* __restrict__ pixel_errors, int npix, size_t cs, int ncls, int nt4, FastDiv dhw) {
    __shared__ unsigned lh[OUTC_MAXCLS * 256];
    __shared__ int s_valid;
    const int tid = threadIdx.x, lane = tid & 63, tile = blockIdx.x;
    for (int i = tid; i < ncls * 256; i += 256) lh[i] = 0;
    if (tid == 0) s_valid = 0;
    __syncthreads();
    const size_t hw = (size_t)dhw.d;
    int nvalid = 0;
    for (int r = 0; r < LV_ROUNDS; r++) {
        const long long e = (long long)tile * LV_TILE + r * 256 + tid;
        const bool in = e < npix;
        const int t = in ? (int)labels[e] : ignore;
        const bool valid = in && t != ignore;              // an ignored pixel: none of its logits is read
        float p[OUTC_MAXCLS];
        if (valid) {
            int b, q; dhw.divmod((int)e, b, q);
            float m = -INFINITY;
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { p[k] = logits[((size_t)b * ncls + k) * hw + q]; m = fmaxf(m, p[k]); }
            float den = 0.f;
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { p[k] = expf(p[k] - m); den += p[k]; }
            const float inv = 1.f / den;                   // softmax as the criterion's statistics pass forms it
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) p[k] *= inv;
            nvalid++;
        }
#pragma unroll
        for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) {
            unsigned sk = LV_IGNORED, pl = (unsigned)e;
            float err = 0.f;
            if (valid) {
                const bool fg = t == k;
                err = __uint_as_float(__float_as_uint((fg ? 1.f : 0.f) - p[k]) & 0x7FFFFFFFu);      // |fg - p|, the sign bit clear whatever p holds
                sk = ~topk_key(err);
                if (fg) pl |= LV_FG;
            }
            if (in) {
                kp[(size_t)k * cs + (size_t)e] = make_uint2(sk, pl);
                if (pixel_errors) pixel_errors[(size_t)k * npix + (size_t)e] = err;
            }
            lv_hist_add<false>(lh + k * 256, sk & 255u, in, lane);
        }
    }
    if (nvalid) atomicAdd(&s_valid, nvalid);
    __syncthreads();
    for (int i = tid; i < ncls * 256; i += 256) hist[(size_t)i * nt4 + tile] = lh[i];
    if (tid == 0) pval[tile] = s_valid;
}

// ---------------------------------------------------------------- hist: digit counts of one pass per (class, tile)
template <bool TOP>
__global__ __launch_bounds__(256) void lovasz_hist_kernel(const uint2* __restrict__ kp, unsigned* __restrict__ hist, int npix, size_t cs, int nt4,
                                                          int shift) {
    __shared__ unsigned lh[256];
    const int tid = threadIdx.x, lane = tid & 63, tile = blockIdx.x, c = blockIdx.y;
    lh[tid] = 0;
    __syncthreads();
    const uint2* kc = kp + (size_t)c * cs;
    for (int r = 0; r < LV_ROUNDS; r++) {
        const long long e = (long long)tile * LV_TILE + r * 256 + tid;
        const bool in = e < npix;
        const unsigned k = in ? kc[e].x : 0u;
        lv_hist_add<TOP>(lh, (k >> shift) & 255u, in, lane);
    }
    __syncthreads();
    hist[((size_t)c * 256 + tid) * nt4 + tile] = lh[tid];
}

// ---------------------------------------------------------------- rowscan: one wave per row of `len` counts: in-place exclusive scan, the row's total
// rows of `stride` (a multiple of 4) elements.  pval / meta_n: the wave of row 0 also adds the nt tile valid counts (integers: any order).
__global__ __launch_bounds__(256) void lovasz_rowscan_kernel(unsigned* __restrict__ data, int rows, int stride, int len, unsigned* __restrict__ totals,
                                                             const int32_t* __restrict__ pval, unsigned* __restrict__ meta_n) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;                               // (wave-uniform; no block barrier below)
    unsigned* a = data + (size_t)row * stride;             // 16-byte aligned: the base is, and stride is a multiple of 4
    unsigned carry = 0;                                    // (every sum stays below 2^31: B*H*W does)
    for (int base = 0; base < len; base += 256) {
        const int i0 = base + lane * 4;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (i0 < len) v = *reinterpret_cast<const uint4*>(a + i0);      // (i0 + 3 < stride; what lies behind len is unwritten: masked here)
        if (i0 + 1 >= len) v.y = 0;
        if (i0 + 2 >= len) v.z = 0;
        if (i0 + 3 >= len) v.w = 0;
        const unsigned s = v.x + v.y + v.z + v.w;
        const unsigned inc = lv_wave_scan(s, lane);
        const unsigned ex = carry + inc - s;
        if (i0 < len) *reinterpret_cast<uint4*>(a + i0) = make_uint4(ex, ex + v.x, ex + v.x + v.y, ex + v.x + v.y + v.z);
        carry += __shfl(inc, 63);
    }
    if (lane == 0) totals[row] = carry;
    if (pval && row == 0) {
        unsigned s = 0;
        for (int i = lane; i < len; i += 64) s += (unsigned)pval[i];
        s = lv_wave_scan(s, lane);
        if (lane == 63) meta_n[0] = s;
    }
}

// ---------------------------------------------------------------- scatter: one stable pass
// Wave w of the block owns the elements [tile*4096 + w*1024, + 1024) in 16 rounds of 64 consecutive ones.  A round: the lanes that share
// a digit find each other with eight ballots; the first of them takes the wave's running count of that digit from LDS and advances it
// (a wave's LDS accesses execute in program order; the counts of a wave are touched by that wave alone until the barrier).  After the
// rounds thread d turns the four waves' counts of digit d into their bases: the scan of the digit totals + the digit's count in the
// tiles in front.
__global__ __launch_bounds__(256) void lovasz_scatter_kernel(const uint2* __restrict__ kp_in, uint2* __restrict__ kp_out,
                                                             const unsigned* __restrict__ hist, const unsigned* __restrict__ dtot,
                                                             int npix, size_t cs, int nt4, int shift) {
    __shared__ unsigned wcnt[4][256];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x, c = blockIdx.y;
    const size_t cb = (size_t)c * cs;
    uint2 kp[LV_ROUNDS]; unsigned lrank[LV_ROUNDS];
    const long long e0 = (long long)tile * LV_TILE + wave * 1024 + lane;
#pragma unroll
    for (int r = 0; r < LV_ROUNDS; r++) kp[r] = e0 + r * 64 < npix ? kp_in[cb + e0 + r * 64] : make_uint2(0, 0);
#pragma unroll
    for (int w = 0; w < 4; w++) wcnt[w][tid] = 0;
    unsigned tot;
    const unsigned dbase = lv_block_scan(dtot[c * 256 + tid], tot) + hist[((size_t)c * 256 + tid) * nt4 + tile];      // (its barriers order the zeroing too)
    volatile unsigned* mine = wcnt[wave];
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int r = 0; r < LV_ROUNDS; r++) {
        const bool in = e0 + r * 64 < npix;
        const unsigned d = (kp[r].x >> shift) & 255u;
        unsigned long long m = __ballot(in);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const unsigned long long bal = __ballot(in && bit);
            m &= bit ? bal : ~bal;
        }                                                  // m: the lanes of this round with this lane's digit (its own included)
        const int leader = in ? __ffsll((long long)m) - 1 : lane;
        unsigned old = 0;
        if (in && lane == leader) { old = mine[d]; mine[d] = old + (unsigned)__popcll(m); }
        old = __shfl(old, leader);
        lrank[r] = old + (unsigned)__popcll(m & below);
    }
    __syncthreads();
    {
        const unsigned c0 = wcnt[0][tid], c1 = wcnt[1][tid], c2 = wcnt[2][tid];
        wcnt[0][tid] = dbase; wcnt[1][tid] = dbase + c0; wcnt[2][tid] = dbase + c0 + c1; wcnt[3][tid] = dbase + c0 + c1 + c2;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < LV_ROUNDS; r++) {
        if (e0 + r * 64 < npix) {
            const unsigned dest = wcnt[wave][(kp[r].x >> shift) & 255u] + lrank[r];
            if (dest < (unsigned)npix) kp_out[cb + dest] = kp[r];      // (always, by the histogram: the test keeps a store in bounds whatever happens)
        }
    }
}

// ---------------------------------------------------------------- fgcount: foreground pixels per tile of the sorted order
__global__ __launch_bounds__(256) void lovasz_fgcount_kernel(const uint2* __restrict__ kp, unsigned* __restrict__ tfg, int npix, size_t cs, int nt4) {
    __shared__ unsigned s_cnt;
    const int tid = threadIdx.x, tile = blockIdx.x, c = blockIdx.y;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const uint2* pc = kp + (size_t)c * cs;
    unsigned n = 0;
    for (int r = 0; r < LV_ROUNDS; r++) {
        const long long e = (long long)tile * LV_TILE + r * 256 + tid;
        if (e < npix) n += pc[e].y >> 31;
    }
    if (n) atomicAdd(&s_cnt, n);
    __syncthreads();
    if (tid == 0) tfg[(size_t)c * nt4 + tile] = s_cnt;
}

// ---------------------------------------------------------------- coef: coefficients along the order, the class term's partials
// rank r, c_prev foreground pixels in front of it:  I = G - c_prev, U = G + r - c_prev;  g = 1/U (foreground), I / (U (U + 1)) otherwise,
// 1 when U = 0: the increment of the Jaccard index, from integers in double.  meta[c] = G, meta[8] = n (the valid pixels).
__global__ __launch_bounds__(256) void lovasz_coef_kernel(const uint2* __restrict__ kp, const unsigned* __restrict__ tfg,
                                                          const unsigned* __restrict__ meta, float* __restrict__ q, double* __restrict__ part,
                                                          int32_t* __restrict__ ranks, int npix, size_t cs, int nt, int nt4) {
    __shared__ double dred[256];
    const int tid = threadIdx.x, tile = blockIdx.x, c = blockIdx.y;
    const size_t cb = (size_t)c * cs, rb = (size_t)c * npix;
    const long long r0 = (long long)tile * LV_TILE + tid * 16;
    unsigned k[16], p[16], s = 0;
    if (r0 + 16 <= npix) {                                 // 128 consecutive bytes per thread (cb + r0 is a multiple of 4 pairs)
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint4 a = *reinterpret_cast<const uint4*>(kp + cb + r0 + 2 * j);
            k[2 * j] = a.x; p[2 * j] = a.y; k[2 * j + 1] = a.z; p[2 * j + 1] = a.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint2 a = r0 + j < npix ? kp[cb + r0 + j] : make_uint2(LV_IGNORED, 0u);
            k[j] = a.x; p[j] = a.y;
        }
    }
#pragma unroll
    for (int j = 0; j < 16; j++) s += p[j] >> 31;
    unsigned tot;
    const long long G = meta[c], n = meta[8];
    long long c_prev = (long long)tfg[(size_t)c * nt4 + tile] + lv_block_scan(s, tot);
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const long long r = r0 + j;
        if (r >= npix) break;
        const unsigned idx = p[j] & ~LV_FG;
        if (idx >= (unsigned)npix) continue;               // (never: the payloads are a permutation of the pixel indices)
        if (r < n) {
            const bool fg = (p[j] >> 31) != 0;
            const long long I = G - c_prev, U = G + r - c_prev;
            const double g = fg ? 1.0 / (double)U : (U == 0 ? 1.0 : (double)I / ((double)U * (double)(U + 1)));
            acc += (double)topk_unkey(~k[j]) * g;
            q[cb + idx] = fg ? -(float)g : (float)g;
            if (ranks) ranks[rb + idx] = (int32_t)r;
            c_prev += fg;
        } else if (ranks) ranks[rb + idx] = -1;            // behind the valid pixels: the ignored ones
    }
    dred[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) { if (tid < h) dred[tid] += dred[tid + h]; __syncthreads(); }
    if (tid == 0) part[(size_t)c * nt + tile] = dred[0];
}

// ---------------------------------------------------------------- finish: class terms, the mean over the included classes, loss
__global__ __launch_bounds__(256) void lovasz_finish_kernel(const double* __restrict__ part, const unsigned* __restrict__ meta, int ncls, int nt,
                                                            int classes_all, float weight, int accumulate, float* __restrict__ loss,
                                                            float* __restrict__ term, float* __restrict__ scale) {
    __shared__ double dred[256];
    __shared__ double lc[OUTC_MAXCLS];
    const int tid = threadIdx.x;
    for (int c = 0; c < ncls; c++) {
        double a = 0.0;
        for (int i = tid; i < nt; i += 256) a += part[(size_t)c * nt + i];
        dred[tid] = a;
        __syncthreads();
        for (int h = 128; h > 0; h >>= 1) { if (tid < h) dred[tid] += dred[tid + h]; __syncthreads(); }
        if (tid == 0) lc[c] = dred[0];
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned n = meta[8];
        int m = 0; double sum = 0.0;
        for (int c = 0; c < ncls; c++) if (n > 0 && (classes_all || meta[c] > 0)) { m++; sum += lc[c]; }
        const float t = m ? (float)(sum / m) : 0.f;
        for (int c = 0; c < OUTC_MAXCLS; c++)
            scale[c] = (c < ncls && n > 0 && (classes_all || meta[c] > 0)) ? (float)(1.0 / m) : 0.f;
        if (term) *term = t;
        const float wt = __fmul_rn(weight, t);
        *loss = accumulate ? *loss + wt : wt;
    }
}

// ---------------------------------------------------------------- grad: q_c = (fg ? -g : +g) / m, dlogit_j = weight p_j (q_j - sum_c q_c p_c)
__global__ __launch_bounds__(256) void lovasz_grad_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels, int ignore,
                                                          const float* __restrict__ q, const float* __restrict__ scale, float weight,
                                                          int accumulate, float* __restrict__ dlogits, int npix, size_t cs, int ncls, FastDiv dhw) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= npix) return;
    const size_t hw = (size_t)dhw.d;
    int b, qi; dhw.divmod((int)e, b, qi);
    if ((int)labels[e] == ignore) {                        // nothing of this pixel's logits is read; an accumulated gradient stays as it is
        if (!accumulate) {
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) dlogits[((size_t)b * ncls + k) * hw + qi] = 0.f;
        }
        return;
    }
    float p[OUTC_MAXCLS], qq[OUTC_MAXCLS]; float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { p[k] = logits[((size_t)b * ncls + k) * hw + qi]; m = fmaxf(m, p[k]); }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { p[k] = expf(p[k] - m); den += p[k]; }
    const float inv = 1.f / den;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) {
        p[k] *= inv;
        const float sc = scale[k];
        qq[k] = sc != 0.f ? q[(size_t)k * cs + (size_t)e] * sc : 0.f;          // a class that is not included is selected out
        dot += qq[k] * p[k];
    }
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) {
        const size_t o = ((size_t)b * ncls + k) * hw + qi;
        const float v = __fmul_rn(weight, p[k] * (qq[k] - dot));               // rounded before the add: accumulate = 1 is one float32 add of accumulate = 0's value
        dlogits[o] = accumulate ? dlogits[o] + v : v;
    }
}

extern "C" size_t bdn_lovasz_workspace_bytes(int B, int ncls, int H, int W) {
    if (B <= 0 || H <= 0 || W <= 0 || ncls < 2 || ncls > OUTC_MAXCLS || (size_t)B * H * W >= ((size_t)1 << 31)) return 0;
    return lovasz_plan(B, ncls, H, W).total;
}

extern "C" int bdn_lovasz_softmax(const float* logits, const uint8_t* labels, int ignore_label, int classes_all, float weight, int accumulate,
                                  void* ws, float* loss, float* term, float* dlogits, float* pixel_errors, int32_t* ranks,
                                  int B, int ncls, int H, int W, void* stream) {
    if (!logits || !labels || !ws || !loss) BDN_FAIL(BDN_E_ARG, "lovasz_softmax: null pointer");
    if (ignore_label < -1 || ignore_label > 255) BDN_FAIL(BDN_E_ARG, "lovasz_softmax: ignore_label=%d is neither -1 (none) nor a byte value (0..255)", ignore_label);
    if (!(weight >= 0.f)) BDN_FAIL(BDN_E_ARG, "lovasz_softmax: negative weight (%g)", weight);
    if (ncls < 2 || ncls > OUTC_MAXCLS) BDN_FAIL(BDN_E_SHAPE, "lovasz_softmax: ncls=%d unsupported (2..%d)", ncls, OUTC_MAXCLS);
    if (B <= 0 || H <= 0 || W <= 0 || (size_t)B * H * W >= ((size_t)1 << 31)) BDN_FAIL(BDN_E_SHAPE, "lovasz_softmax: bad shape (B*H*W must stay below 2^31)");
    if ((uintptr_t)ws & 15) BDN_FAIL(BDN_E_ARG, "lovasz_softmax: ws must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const LovaszPlan p = lovasz_plan(B, ncls, H, W);
    char* base = (char*)ws;
    uint2* kpA = (uint2*)(base + p.o_kpA); uint2* kpB = (uint2*)(base + p.o_kpB);
    unsigned* hist = (unsigned*)(base + p.o_hist); unsigned* dtot = (unsigned*)(base + p.o_dtot); unsigned* tfg = (unsigned*)(base + p.o_tfg);
    int32_t* pval = (int32_t*)(base + p.o_pval); double* part = (double*)(base + p.o_part);
    unsigned* meta = (unsigned*)(base + p.o_meta); float* scale = (float*)(base + p.o_scale);
    float* q = (float*)kpB;                                // the pairs end in A; B's front then holds the coefficients, C rows of cs floats
    const FastDiv dhw(H * W);
    const dim3 tiles(p.nt, ncls);
    hipLaunchKernelGGL(lovasz_prep_kernel, dim3(p.nt), dim3(256), 0, st, logits, labels, ignore_label, kpA, hist, pval, pixel_errors,
                       p.npix, p.cs, ncls, p.nt4, dhw);
    BDN_CHECK_LAUNCH("lovasz_prep");
    for (int pass = 0; pass < 4; pass++) {                 // A -> B -> A -> B -> A
        const uint2* in = pass & 1 ? kpB : kpA; uint2* out = pass & 1 ? kpA : kpB;
        if (pass == 3) hipLaunchKernelGGL(lovasz_hist_kernel<true>, tiles, dim3(256), 0, st, in, hist, p.npix, p.cs, p.nt4, 24);
        else if (pass) hipLaunchKernelGGL(lovasz_hist_kernel<false>, tiles, dim3(256), 0, st, in, hist, p.npix, p.cs, p.nt4, 8 * pass);
        BDN_CHECK_LAUNCH("lovasz_hist");
        hipLaunchKernelGGL(lovasz_rowscan_kernel, dim3(ncls * 64), dim3(256), 0, st, hist, ncls * 256, p.nt4, p.nt, dtot, (const int32_t*)nullptr,
                           (unsigned*)nullptr);
        BDN_CHECK_LAUNCH("lovasz_rowscan");
        hipLaunchKernelGGL(lovasz_scatter_kernel, tiles, dim3(256), 0, st, in, out, hist, dtot, p.npix, p.cs, p.nt4, 8 * pass);
        BDN_CHECK_LAUNCH("lovasz_scatter");
    }
    hipLaunchKernelGGL(lovasz_fgcount_kernel, tiles, dim3(256), 0, st, kpA, tfg, p.npix, p.cs, p.nt4);
    BDN_CHECK_LAUNCH("lovasz_fgcount");
    hipLaunchKernelGGL(lovasz_rowscan_kernel, dim3((ncls + 3) / 4), dim3(256), 0, st, tfg, ncls, p.nt4, p.nt, meta, pval, meta + 8);
    BDN_CHECK_LAUNCH("lovasz_tile_scan");
    hipLaunchKernelGGL(lovasz_coef_kernel, tiles, dim3(256), 0, st, kpA, tfg, meta, q, part, ranks, p.npix, p.cs, p.nt, p.nt4);
    BDN_CHECK_LAUNCH("lovasz_coef");
    hipLaunchKernelGGL(lovasz_finish_kernel, dim3(1), dim3(256), 0, st, part, meta, ncls, p.nt, classes_all, weight, accumulate, loss, term, scale);
    BDN_CHECK_LAUNCH("lovasz_finish");
    if (dlogits) {
        hipLaunchKernelGGL(lovasz_grad_kernel, dim3(grid_for((size_t)p.npix)), dim3(256), 0, st, logits, labels, ignore_label, q, scale, weight,
                           accumulate, dlogits, p.npix, p.cs, ncls, dhw);
        BDN_CHECK_LAUNCH("lovasz_grad");
    }
    return BDN_OK;
}
