// The criterion of loss.hip on SOFT targets: bdn_criterion_soft (include/bidate_hip.h states the semantics).  Every pixel carries a
// target q_c >= 0 per class and a weight w >= 0; v = [w > 0]:
//   hard labels (FLOAT_T = false)   q_c = hi at the label's class, lo elsewhere (label smoothing; hi = 1, lo = 0 without), q = 0 for a valid
//                                   label >= ncls, w = 0 at the ignore label; the pass reads the label byte, as bdn_criterion_masked does
//   float targets (FLOAT_T = true)  q as given, f32 [B, ncls, H, W]: 4 ncls more bytes per pixel
// and `weights` (NULL or f32 [B, H, W]) multiplies into w.  The three passes mirror bdn_criterion_masked's:
//   stats    softmax once per pixel -> per-block partial sums of TP = w p q, FP = w p (1 - q), FN = w (1 - p) q in float32, the focal
//            partial sum_c [q_c > 0] q_c a_c m_c (-log p_c) times w in double, the five counters; four rows of a lane in flight
//   finish   one block adds the block partials in a fixed order, forms loss and terms, leaves the coefficient tables 1/D and TP/D^2 and
//            the focal scale (1 / valid, or 1) in the workspace
//   grad     w_overlap dO + w_focal dF per pixel, 0.0f for every class where w is not > 0
// A pixel with v = 0 is skipped by a branch before any of its logits or targets is used: inf or NaN there reaches no output.  A class
// with q_c == 0 is selected out of the focal term, never multiplied (0 * log 0 is not formed).  A term with weight 0 is selected out of
// loss and dlogits and reported as 0.  No atomics, no memset, no host read-back: the same bits every run, whatever the workspace held.
// ws: [focal block partials, double, gx*gy, padded to 16 bytes][sums n, then the coefficient tables][part nblk*n][pcounts gx*gy*5]
//     [focal gradient scale, padded to 16 bytes], n = 3 * ncls * (W or 1) -- bdn_criterion_masked's layout.
#include "common.hpp"

__device__ __forceinline__ float soft_mod(float p, float gamma) { return gamma == 0.f ? 1.f : powf(fmaxf(1.f - p, 0.f), gamma); }

struct SoftSrc {
    const uint8_t* labels; const float* targets; const float* weights;         // exactly one of labels / targets; weights or NULL
    int ignore; float hi, lo;                                                  // hard labels: the ignore byte or -1, the smoothed pair
};
struct SoftFocal { const float* calpha; float gamma; };                        // class weights or NULL

// block = 256 threads = RL row lanes x CW columns (CW = min(W rounded up to a power of two, 256)), the column the fast index: a wave reads
// consecutive x;  grid.x = column blocks, grid.y = row blocks.  A lane walks its rows four at a time: the loads of four rows are
// requested before the first is used (one dependent HBM round trip per row otherwise), the rows are accumulated one after the other.
template <int NC, bool FLOAT_T>
__global__ __launch_bounds__(256) void soft_stats_kernel(const float* __restrict__ logits, SoftSrc src, SoftFocal fo, float* __restrict__ part,
                                                         double* __restrict__ fpart, int32_t* __restrict__ pcounts, int B, int ncls, int H,
                                                         int W, int rows_per_block, int We, FastDiv dH) {
    extern __shared__ float sm[];                         // [RL][3*NC][CW]
    const int CW = blockDim.x, RL = blockDim.y;
    const int cl = threadIdx.x, rl = threadIdx.y;
    const int x = blockIdx.x * CW + cl;
    const size_t hw = (size_t)H * W;
    float tp[NC], fp[NC], fn[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) { tp[k] = 0.f; fp[k] = 0.f; fn[k] = 0.f; }
    int c_tp = 0, c_fp = 0, c_fn = 0, c_ok = 0, c_valid = 0;
    double facc = 0.0;
    const int rows = B * H, r_end = min(rows, (int)(blockIdx.y + 1) * rows_per_block);
    if (x < W)
        for (int r0 = blockIdx.y * rows_per_block + rl; r0 < r_end; r0 += 4 * RL) {
            float lv[4][NC], qv[4][FLOAT_T ? NC : 1], wv[4]; int tv[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int r = r0 + u * RL;
                const int rr = r < r_end ? r : r0;
                int b, y; dH.divmod(rr, b, y);
                const size_t q = (size_t)y * W + x;
#pragma unroll
                for (int k = 0; k < NC; k++) lv[u][k] = k < ncls ? logits[((size_t)b * ncls + k) * hw + q] : -INFINITY;
                if constexpr (FLOAT_T) {
#pragma unroll
                    for (int k = 0; k < NC; k++) qv[u][k] = k < ncls ? src.targets[((size_t)b * ncls + k) * hw + q] : 0.f;
                    tv[u] = 0;
                } else {
                    qv[u][0] = 0.f;
                    tv[u] = src.labels[(size_t)b * hw + q];
                }
                wv[u] = src.weights ? src.weights[(size_t)b * hw + q] : 1.f;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (r0 + u * RL >= r_end) break;
                float w = wv[u];
                if constexpr (!FLOAT_T) { if (tv[u] == src.ignore) w = 0.f; }
                if (!(w > 0.f)) continue;                  // an invalid pixel: nothing of it is used
                c_valid++;
                float l[NC]; float m = -INFINITY; int am = 0;
#pragma unroll
                for (int k = 0; k < NC; k++) { l[k] = lv[u][k]; if (l[k] > m) { m = l[k]; am = k; } }
                float den = 0.f;
#pragma unroll
                for (int k = 0; k < NC; k++) { l[k] = k < ncls ? expf(l[k] - m) : 0.f; den += l[k]; }
                const float inv = 1.f / den, logden = logf(den);
                int t = tv[u];                             // the pixel's class: the label, or the first maximum of q
                float qmax = -INFINITY;
                float f = 0.f;
#pragma unroll
                for (int k = 0; k < NC; k++) {
                    if (k < ncls) {
                        float q;
                        if constexpr (FLOAT_T) { q = qv[u][k]; if (q > qmax) { qmax = q; t = k; } }
                        else q = t < ncls ? (t == k ? src.hi : src.lo) : 0.f;
                        const float p = l[k] * inv;
                        tp[k] += w * (p * q); fp[k] += w * (p * (1.f - q)); fn[k] += w * ((1.f - p) * q);
                        if (q > 0.f) {
                            const float a = fo.calpha ? fo.calpha[k] : 1.f;
                            f += -(q * a * soft_mod(p, fo.gamma)) * ((lv[u][k] - m) - logden);
                        }
                    }
                }
                facc += (double)w * (double)f;
                c_tp += (am == 1 && t == 1); c_fp += (am == 1 && t != 1); c_fn += (am != 1 && t == 1); c_ok += (am == t);
            }
        }
#pragma unroll
    for (int k = 0; k < NC; k++) {
        sm[(rl * 3 * NC + 0 * NC + k) * CW + cl] = tp[k];
        sm[(rl * 3 * NC + 1 * NC + k) * CW + cl] = fp[k];
        sm[(rl * 3 * NC + 2 * NC + k) * CW + cl] = fn[k];
    }
    __syncthreads();
    // block partials: part[row block][cell] (cells [3][ncls][W]), or part[block][3*ncls] when the columns are reduced too
    const int nblk_lin = blockIdx.y * gridDim.x + blockIdx.x;
    const int tid = rl * CW + cl;
    if (We == W) {
        if (rl == 0 && x < W)
            for (int k = 0; k < ncls; k++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    float v = 0.f;
                    for (int r = 0; r < RL; r++) v += sm[(r * 3 * NC + j * NC + k) * CW + cl];
                    part[(size_t)blockIdx.y * 3 * ncls * W + (j * ncls + k) * W + x] = v;
                }
    } else if (tid < 3 * NC) {
        float v = 0.f;
        for (int i = 0; i < RL * CW; i++) {
            const int r = i / CW, c = i % CW;
            if (blockIdx.x * CW + c < W) v += sm[(r * 3 * NC + tid) * CW + c];
        }
        const int j = tid / NC, k = tid % NC;
        if (k < ncls) part[(size_t)nblk_lin * 3 * ncls + j * ncls + k] = v;
    }
    int* ism = reinterpret_cast<int*>(sm);                // (256 * 5 ints fit in the 256 * 3 * NC floats of sm)
    __syncthreads();
    ism[tid * 5 + 0] = c_tp; ism[tid * 5 + 1] = c_fp; ism[tid * 5 + 2] = c_fn; ism[tid * 5 + 3] = c_ok; ism[tid * 5 + 4] = c_valid;
    __syncthreads();
    if (tid < 5) { int v = 0; for (int i = 0; i < 256; i++) v += ism[i * 5 + tid]; pcounts[nblk_lin * 5 + tid] = v; }
    double* dsm = reinterpret_cast<double*>(sm);          // the block's focal partial: LDS tree over the 256 lanes, a fixed order
    __syncthreads();
    dsm[tid] = facc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) dsm[tid] += dsm[tid + s]; __syncthreads(); }
    if (tid == 0) fpart[nblk_lin] = dsm[0];
}

// One block: sums[cell] = the nblk block partials in a fixed order (thread = (float4 of cells or one cell, block lane)), the counters, then
// O = 1 - mean TP / (TP + alpha FP + beta FN + eps), F = scale * the focal partials, loss, terms.  Leaves 1/D in sums[0..], TP/D^2 in
// sums[nc..] and the focal scale in *gscale for the gradient pass.  W = the effective width (1 when the columns are reduced too).
__global__ __launch_bounds__(1024) void soft_finish_kernel(float* __restrict__ sums, const float* __restrict__ part, int nblk,
                                                           const int32_t* __restrict__ pcounts, const double* __restrict__ fpart, int ncblk,
                                                           int32_t* __restrict__ counts, float alpha, float beta, float eps, int ncls, int W,
                                                           float w_o, float w_f, int size_average, float* __restrict__ loss,
                                                           float* __restrict__ terms, float* __restrict__ gscale) {
    __shared__ double red[256];
    __shared__ float4 lane_sums[1024];
    __shared__ int nvalid;
    const int n = 3 * ncls * W, tid = threadIdx.x;
    if (n % 4 == 0 && n / 4 <= 1024) {
        const int n4 = n / 4, LN = 1024 / n4 > 16 ? 16 : 1024 / n4;            // block lanes per float4 of cells (>= 1)
        const int q = tid % n4, l = tid / n4;
        float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
        if (l < LN) {
#pragma unroll 8
            for (int b = l; b < nblk; b += LN) {
                const float4 v = *reinterpret_cast<const float4*>(part + (size_t)b * n + 4 * q);
                a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
            }
            lane_sums[tid] = a;
        }
        __syncthreads();
        if (l == 0) {
            for (int k = 1; k < LN; k++) { const float4 v = lane_sums[k * n4 + q]; a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
            *reinterpret_cast<float4*>(sums + 4 * q) = a;
        }
    } else {
        for (int i = tid; i < n; i += 1024) {
            float a = 0.f;
            for (int b = 0; b < nblk; b++) a += part[(size_t)b * n + i];
            sums[i] = a;
        }
    }
    {                                                      // TP / FP / FN / correct / valid: 5 counters x 128 block lanes, LDS tree per counter
        int* ired = reinterpret_cast<int*>(lane_sums);
        __syncthreads();                                   // lane_sums is free again
        const int j = tid >> 7, l = tid & 127;
        if (tid < 640) {
            int v = 0;
            for (int b = l; b < ncblk; b += 128) v += pcounts[b * 5 + j];
            ired[tid] = v;
        }
        __syncthreads();
        for (int s2 = 64; s2 >= 1; s2 >>= 1) { if (tid < 640 && l < s2) ired[tid] += ired[tid + s2]; __syncthreads(); }
        if (tid < 5 && counts) counts[tid] = ired[tid * 128];
        if (tid == 0) nvalid = ired[4 * 128];
    }
    __syncthreads();
    double acc = 0.0;
    const int nc = ncls * W;
    if (tid < 256)
        for (int i = tid; i < nc; i += 256) {
            const float tp = sums[i], fp = sums[nc + i], fn = sums[2 * nc + i];
            const float D = tp + alpha * fp + beta * fn + eps;
            acc += (double)(tp / D);
            sums[i] = 1.f / D; sums[nc + i] = tp / (D * D);
        }
    if (tid < 256) red[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    const float ov = (float)(1.0 - red[0] / nc);
    __syncthreads();                                       // red[0] is read by every thread before it is reused
    double f = 0.0;
    if (tid < 256) { for (int i = tid; i < ncblk; i += 256) f += fpart[i]; red[tid] = f; }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    if (tid == 0) {
        const double scale = size_average && nvalid > 0 ? 1.0 / (double)nvalid : 1.0;
        const float fv = (float)(red[0] * scale);
        const float lo = w_o != 0.f ? w_o * ov : 0.f, lf = w_f != 0.f ? w_f * fv : 0.f;
        *loss = lo + lf;
        if (terms) { terms[0] = w_o != 0.f ? ov : 0.f; terms[1] = w_f != 0.f ? fv : 0.f; }
        *gscale = (float)scale;
    }
}

// dO_k = p_k (g_k - sum_j p_j g_j) with g_k = -(1/n) w (q_k / D - TP / D^2 (q_k + alpha (1 - q_k) - beta q_k));
// dF_k = -scale w (h_k - p_k sum_j h_j) with h_k = [q_k > 0] q_k a_k m_k, m_k a constant.  One pixel per thread.
template <bool FLOAT_T>
__global__ __launch_bounds__(256) void soft_bwd_kernel(const float* __restrict__ logits, SoftSrc src, SoftFocal fo, const float* __restrict__ coef,
                                                       const float* __restrict__ gscale, float alpha, float beta, float w_o, float w_f,
                                                       float* __restrict__ dlogits, int B, int ncls, int H, int Wimg, int W, FastDiv dhw,
                                                       FastDiv dWimg) {
    const size_t hw = (size_t)H * Wimg, npix = (size_t)B * hw;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    int bi, qi, yi, xi; dhw.divmod((int)p, bi, qi); dWimg.divmod(qi, yi, xi);      // (the entry point keeps B*H*W below 2^31)
    const size_t b = bi, q = qi; const int x = W == 1 ? 0 : xi;
    const int n = ncls * W;
    int t = 0;
    float w = src.weights ? src.weights[p] : 1.f;
    if constexpr (!FLOAT_T) { t = src.labels[p]; if (t == src.ignore) w = 0.f; }
    if (!(w > 0.f)) {                                      // nothing of this pixel's logits or targets is read
#pragma unroll
        for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) dlogits[(b * ncls + k) * hw + q] = 0.f;
        return;
    }
    float l[OUTC_MAXCLS], dp[OUTC_MAXCLS], h[OUTC_MAXCLS]; float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { l[k] = logits[(b * ncls + k) * hw + q]; m = fmaxf(m, l[k]); }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { l[k] = expf(l[k] - m); den += l[k]; }
    const float norm = -1.f / (float)n;
    float dot = 0.f, hs = 0.f;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) {
        l[k] /= den;
        float qk;
        if constexpr (FLOAT_T) qk = src.targets[(b * ncls + k) * hw + q];
        else qk = t < ncls ? (t == k ? src.hi : src.lo) : 0.f;
        const float invD = coef[k * W + x], tpD2 = coef[n + k * W + x];
        dp[k] = norm * w * (qk * invD - tpD2 * (qk + alpha * (1.f - qk) - beta * qk));
        dot += l[k] * dp[k];
        h[k] = qk > 0.f ? qk * (fo.calpha ? fo.calpha[k] : 1.f) * soft_mod(l[k], fo.gamma) : 0.f;
        hs += h[k];
    }
    const float c = -gscale[0] * w;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) {
        const float go = w_o != 0.f ? w_o * (l[k] * (dp[k] - dot)) : 0.f;
        const float gf = w_f != 0.f ? w_f * (c * (h[k] - l[k] * hs)) : 0.f;
        dlogits[(b * ncls + k) * hw + q] = go + gf;
    }
}

struct SoftPlan { int We, CW, RL, rpb, gx, gy, nblk, n; size_t o_sums, o_part, o_pcounts, o_gscale, total; };
static inline size_t soft_up16(size_t v) { return (v + 15) / 16 * 16; }
static SoftPlan soft_plan(int B, int ncls, int H, int W, int reduce_w) {
    SoftPlan p;
    p.We = reduce_w ? 1 : W;
    p.CW = 1; while (p.CW < W && p.CW < 256) p.CW *= 2;
    p.RL = 256 / p.CW;
    const int rows = B * H;
    p.rpb = (rows + 255) / 256; if (p.rpb < p.RL) p.rpb = p.RL;                 // ~256 row blocks
    p.gx = (W + p.CW - 1) / p.CW; p.gy = (rows + p.rpb - 1) / p.rpb;
    p.nblk = reduce_w ? p.gx * p.gy : p.gy;                                     // partial rows the finish adds up
    p.n = 3 * ncls * p.We;
    p.o_sums = soft_up16(sizeof(double) * (size_t)p.gx * p.gy);
    p.o_part = p.o_sums + sizeof(float) * p.n;
    p.o_pcounts = p.o_part + sizeof(float) * (size_t)p.nblk * p.n;
    p.o_gscale = p.o_pcounts + sizeof(int32_t) * 5 * (size_t)p.gx * p.gy;
    p.total = p.o_gscale + 16;
    return p;
}

extern "C" size_t bdn_criterion_soft_workspace_bytes(int B, int ncls, int H, int W, int reduce_w) {
    if (B <= 0 || H <= 0 || W <= 0 || ncls < 2 || ncls > OUTC_MAXCLS || (size_t)B * H * W >= ((size_t)1 << 31)) return 0;
    return soft_plan(B, ncls, H, W, reduce_w).total;
}

template <bool FLOAT_T>
static int soft_passes(const float* logits, const SoftSrc& src, const SoftFocal& fo, const SoftPlan& p, char* ws, float w_o, float alpha,
                       float beta, float eps, float w_f, int size_average, float* loss, float* terms, int32_t* counts, float* dlogits,
                       int B, int ncls, int H, int W, hipStream_t st) {
    double* fpart = (double*)ws;
    float* sums = (float*)(ws + p.o_sums); float* part = (float*)(ws + p.o_part);
    int32_t* pcounts = (int32_t*)(ws + p.o_pcounts); float* gscale = (float*)(ws + p.o_gscale);
    const dim3 grid(p.gx, p.gy), block(p.CW, p.RL);
    if (ncls <= 2) hipLaunchKernelGGL((soft_stats_kernel<2, FLOAT_T>), grid, block, sizeof(float) * 256 * 3 * 2, st, logits, src, fo, part, fpart, pcounts, B, ncls, H, W, p.rpb, p.We, FastDiv(H));
    else hipLaunchKernelGGL((soft_stats_kernel<OUTC_MAXCLS, FLOAT_T>), grid, block, sizeof(float) * 256 * 3 * OUTC_MAXCLS, st, logits, src, fo, part, fpart, pcounts, B, ncls, H, W, p.rpb, p.We, FastDiv(H));
    BDN_CHECK_LAUNCH("criterion_soft_stats");
    hipLaunchKernelGGL(soft_finish_kernel, dim3(1), dim3(1024), 0, st, sums, part, p.nblk, pcounts, fpart, p.gx * p.gy, counts, alpha, beta, eps, ncls, p.We, w_o, w_f, size_average, loss, terms, gscale);
    BDN_CHECK_LAUNCH("criterion_soft_finish");
    if (dlogits) {
        hipLaunchKernelGGL((soft_bwd_kernel<FLOAT_T>), dim3(grid_for((size_t)B * H * W)), dim3(256), 0, st, logits, src, fo, sums, gscale, alpha, beta, w_o, w_f, dlogits, B, ncls, H, W, p.We, FastDiv(H * W), FastDiv(W));
        BDN_CHECK_LAUNCH("criterion_soft_bwd");
    }
    return BDN_OK;
}

extern "C" int bdn_criterion_soft(const float* logits, const uint8_t* labels, const float* targets, const float* weights, int ignore_label,
                                  float smoothing, float w_overlap, float alpha, float beta, float eps, int reduce_w, float w_focal,
                                  float gamma, const float* class_alpha, int size_average, void* ws, float* loss, float* terms,
                                  int32_t* counts, float* dlogits, int B, int ncls, int H, int W, void* stream) {
    if (!logits || !ws || !loss) BDN_FAIL(BDN_E_ARG, "criterion_soft: null pointer");
    if ((labels != nullptr) == (targets != nullptr)) BDN_FAIL(BDN_E_ARG, "criterion_soft: exactly one of labels and targets must be given");
    if (!(smoothing >= 0.f && smoothing < 1.f)) BDN_FAIL(BDN_E_ARG, "criterion_soft: smoothing=%g outside [0, 1)", smoothing);
    if (targets && smoothing != 0.f) BDN_FAIL(BDN_E_ARG, "criterion_soft: smoothing=%g with float targets (smooth the targets instead)", smoothing);
    if (ignore_label < -1 || ignore_label > 255) BDN_FAIL(BDN_E_ARG, "criterion_soft: ignore_label=%d is neither -1 (none) nor a byte value (0..255)", ignore_label);
    if (targets && ignore_label != -1) BDN_FAIL(BDN_E_ARG, "criterion_soft: ignore_label=%d with float targets (give a weight of 0 instead)", ignore_label);
    if (!(w_overlap >= 0.f) || !(w_focal >= 0.f)) BDN_FAIL(BDN_E_ARG, "criterion_soft: negative weight (w_overlap=%g, w_focal=%g)", w_overlap, w_focal);
    if (w_overlap == 0.f && w_focal == 0.f) BDN_FAIL(BDN_E_ARG, "criterion_soft: both weights are zero");
    if (!(gamma >= 0.f)) BDN_FAIL(BDN_E_ARG, "criterion_soft: negative gamma");
    if ((uintptr_t)ws & 15) BDN_FAIL(BDN_E_ARG, "criterion_soft: ws must be 16-byte aligned");
    if (((uintptr_t)logits | (uintptr_t)targets | (uintptr_t)weights | (uintptr_t)class_alpha | (uintptr_t)loss | (uintptr_t)terms |
         (uintptr_t)counts | (uintptr_t)dlogits) & 3)
        BDN_FAIL(BDN_E_ARG, "criterion_soft: a float32 / int32 pointer is not 4-byte aligned");
    if (ncls < 2 || ncls > OUTC_MAXCLS) BDN_FAIL(BDN_E_SHAPE, "criterion_soft: ncls=%d unsupported (2..%d)", ncls, OUTC_MAXCLS);
    if (B <= 0 || H <= 0 || W <= 0 || (size_t)B * H * W >= ((size_t)1 << 31)) BDN_FAIL(BDN_E_SHAPE, "criterion_soft: bad shape (B*H*W must stay below 2^31)");
    const SoftPlan p = soft_plan(B, ncls, H, W, reduce_w);
    const float lo = smoothing / (float)ncls;              // one rounding each: what a caller forms with the same float32 operations
    const float one_minus = 1.f - smoothing;
    const float hi = one_minus + lo;
    const SoftSrc src{labels, targets, weights, ignore_label, hi, lo};
    const SoftFocal fo{class_alpha, gamma};
    if (targets) return soft_passes<true>(logits, src, fo, p, (char*)ws, w_overlap, alpha, beta, eps, w_focal, size_average, loss, terms, counts, dlogits, B, ncls, H, W, (hipStream_t)stream);
    return soft_passes<false>(logits, src, fo, p, (char*)ws, w_overlap, alpha, beta, eps, w_focal, size_average, loss, terms, counts, dlogits, B, ncls, H, W, (hipStream_t)stream);
}
