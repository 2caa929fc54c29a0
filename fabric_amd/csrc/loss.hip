// Criteria on the classifier's float32 NCHW logits and uint8 labels: the overlap (Tversky) and focal losses, their weighted sum (bdn_criterion)
// and its forms with an ignore label and with top-k hard-pixel mining.  Block partials are added in a fixed order: no float atomics.
#include "common.hpp"

// ============================================================ Tversky loss (utils/metrics.py:130-171, dims == (0,2))
// sums[k][c][w], k = 0 TP, 1 FP, 2 FN, reduced over batch and H for every (class, column w).
// pass 1: grid (column blocks x row blocks) -> per-block partial sums;  pass 2: single block adds the blocks in a fixed
// order (no float atomics: the loss and dlogits are the same bits every run), then loss + coefficient tables;  pass 3: dlogits.
// FOCAL (bdn_criterion's compound loss, below): the same three passes also carry a focal term -- the statistics pass adds every pixel's
// focal loss from the softmax it has already formed (double per lane, block partials in a fixed order), the finish adds the blocks'
// partials and forms the weighted sum, the gradient pass writes w_overlap dO + w_focal dF.  FOCAL = false is the code as it was.
// MASKED (bdn_criterion_masked, with FOCAL): a pixel whose label equals `ignore` is skipped by a branch before any of its logits is
// used -- it adds to no sum and to no count, so whatever its logits hold (inf, NaN) reaches no output; the statistics pass also counts
// the valid pixels (pcounts[block][5]), the finish forms the focal scale 1/valid from that count and leaves it in device memory for
// the gradient pass, which writes 0.0f at an ignored pixel.  A term with weight 0 contributes nothing (it is selected out, not
// multiplied by 0).  MASKED = false is the code as it was.
// TOPK (bdn_criterion_topk, with FOCAL and MASKED; the section "criterion with top-k hard-pixel mining" below): the statistics pass stores
// every pixel's float32 focal term in the workspace (pterm[(b*H + y)*W + x], 0 at an ignored pixel) instead of summing it; the radix select
// ranks those stored values, the finish takes the kept count K for the valid count in the focal scale, and the gradient pass selects the
// focal part out at a pixel whose kept byte is 0.  TOPK = false is the code as it was.
struct FocalStats { const float* calpha; float gamma; double* part; int ignore; float* pterm; };   // class weights or NULL; partial [gx*gy]
__device__ __forceinline__ float focal_mod(float pt, float gamma) { return gamma == 0.f ? 1.f : powf(fmaxf(1.f - pt, 0.f), gamma); }

template <int NC, bool FOCAL = false, bool MASKED = false, bool TOPK = false>
__global__ void tversky_sums_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                    float* __restrict__ part, int32_t* __restrict__ pcounts, int B, int ncls, int H, int W,
                                    int rows_per_block, int We, FastDiv dH, FocalStats fs = {}) {
    // block = 256 threads = RL row lanes x CW columns (CW = min(W rounded up to a power of two, 256));
    // grid.x = column blocks, grid.y = row blocks
    extern __shared__ float sm[];                         // [RL][3*NC][CW]
    const int CW = blockDim.y, RL = blockDim.x;           // launch: dim3(RL, CW) with x = row lane (slow), see host
    const int cl = threadIdx.y, rl = threadIdx.x;
    const int x = blockIdx.x * CW + cl;
    const size_t hw = (size_t)H * W;
    float tp[NC], fp[NC], fn[NC];
#pragma unroll
    for (int k = 0; k < NC; k++) { tp[k] = 0.f; fp[k] = 0.f; fn[k] = 0.f; }
    int c_tp = 0, c_fp = 0, c_fn = 0, c_ok = 0, c_valid = 0;
    double facc = 0.0;
    const int rows = B * H, r_end = min(rows, (int)(blockIdx.y + 1) * rows_per_block);
    if (x < W)
        // four rows of a lane are requested before the first is used (a lane walks 16 rows at B = 64: one dependent HBM round trip
        // per row made this pass 17.6 us for 9 MB); the rows are still ACCUMULATED one after the other, in the same order
        for (int r0 = blockIdx.y * rows_per_block + rl; r0 < r_end; r0 += 4 * RL) {
            float lv[4][NC]; int tv[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int r = r0 + u * RL;
                const int rr = r < r_end ? r : r0;
                int b, y; dH.divmod(rr, b, y);
                const size_t q = (size_t)y * W + x;
#pragma unroll
                for (int k = 0; k < NC; k++) lv[u][k] = k < ncls ? logits[((size_t)b * ncls + k) * hw + q] : -INFINITY;
                tv[u] = labels[(size_t)b * hw + q];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (r0 + u * RL >= r_end) break;
                if constexpr (TOPK) {
                    if (tv[u] == fs.ignore) {              // (the stored term of an ignored pixel is never ranked: written so that no byte stays unset)
                        int b, y; dH.divmod(r0 + u * RL, b, y);
                        fs.pterm[(size_t)b * hw + (size_t)y * W + x] = 0.f;
                    }
                }
                if constexpr (MASKED) { if (tv[u] == fs.ignore) continue; c_valid++; }      // an ignored pixel: nothing of it is used
                float l[NC]; float m = -INFINITY; int am = 0;
#pragma unroll
                for (int k = 0; k < NC; k++) { l[k] = lv[u][k]; if (l[k] > m) { m = l[k]; am = k; } }
                float den = 0.f;
#pragma unroll
                for (int k = 0; k < NC; k++) { l[k] = k < ncls ? expf(l[k] - m) : 0.f; den += l[k]; }
                const int t = tv[u];
                const float inv = 1.f / den;
                float pt = 0.f;
#pragma unroll
                for (int k = 0; k < NC; k++) {
                    const float p = l[k] * inv;
                    if (t == k) { tp[k] += p; fn[k] += 1.f - p; pt = p; } else fp[k] += p;
                }
                if constexpr (FOCAL) {                     // -(1 - pt)^gamma a[t] log pt on the softmax above (focal_kernel's expression)
                    float ltm = 0.f;                       // l[t] - max
#pragma unroll
                    for (int k = 0; k < NC; k++) if (k < ncls && t == k) ltm = lv[u][k] - m;      // (lv is -inf for k >= ncls: 0 * inf otherwise)
                    const float a = t < ncls ? (fs.calpha ? fs.calpha[t] : 1.f) : 0.f;       // a label >= ncls has no true class: no focal term
                    if constexpr (TOPK) {                  // the same float32 expression, kept per pixel: what the select ranks
                        int b, y; dH.divmod(r0 + u * RL, b, y);
                        fs.pterm[(size_t)b * hw + (size_t)y * W + x] = -focal_mod(pt, fs.gamma) * a * (ltm - logf(den));
                    } else
                    facc += (double)(-focal_mod(pt, fs.gamma) * a * (ltm - logf(den)));
                }
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
    // block partials, no atomics: part[row block][cell] (cells [3][ncls][W]) or part[block][3*NC] when the columns are
    // reduced too; tversky_finish_kernel adds the blocks in a fixed order.  pcounts[block][4] likewise ([5] MASKED: + valid pixels).
    const int nblk_lin = blockIdx.y * gridDim.x + blockIdx.x;
    if (We == W) {
        if (rl == 0 && x < W)
            for (int k = 0; k < ncls; k++)
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    float v = 0.f;
                    for (int r = 0; r < RL; r++) v += sm[(r * 3 * NC + j * NC + k) * CW + cl];
                    part[(size_t)blockIdx.y * 3 * ncls * W + (j * ncls + k) * W + x] = v;
                }
    } else {
        // [B,1,H,W] labels: the reference reduces over the columns too (dims == (0,2,3))
        const int tid = rl + RL * cl;
        if (tid < 3 * NC) {
            float v = 0.f;
            for (int i = 0; i < RL * CW; i++) {
                const int r = i / CW, c = i % CW;
                if (blockIdx.x * CW + c < W) v += sm[(r * 3 * NC + tid) * CW + c];
            }
            const int j = tid / NC, k = tid % NC;
            if (k < ncls) part[(size_t)nblk_lin * 3 * ncls + j * ncls + k] = v;
        }
    }
    {
        int* ism = reinterpret_cast<int*>(sm);
        __syncthreads();
        const int tid = rl * CW + cl;
        constexpr int NCNT = MASKED ? 5 : 4;             // (256 * 5 ints fit in the 256 * 3 * NC floats of sm)
        ism[tid * NCNT + 0] = c_tp; ism[tid * NCNT + 1] = c_fp; ism[tid * NCNT + 2] = c_fn; ism[tid * NCNT + 3] = c_ok;
        if constexpr (MASKED) ism[tid * NCNT + 4] = c_valid;
        __syncthreads();
        if (tid < NCNT) { int v = 0; for (int i = 0; i < 256; i++) v += ism[i * NCNT + tid]; pcounts[nblk_lin * NCNT + tid] = v; }
        if constexpr (FOCAL && !TOPK) {                    // the block's focal partial: LDS tree over the 256 lanes, a fixed order
            double* dsm = reinterpret_cast<double*>(sm);
            __syncthreads();
            dsm[tid] = facc;
            __syncthreads();
            for (int s = 128; s > 0; s >>= 1) { if (tid < s) dsm[tid] += dsm[tid + s]; __syncthreads(); }
            if (tid == 0) fs.part[nblk_lin] = dsm[0];
        }
    }
}

// sums[cell] = sum over the nblk block partials (cell-major rows of `part`), fixed order: thread = (float4 of cells or one
// cell, block lane); then loss = 1 - mean_{c,w} TP/(TP + a FP + b FN + eps).  Overwrites sums[0] with 1/D and sums[1] with TP/D^2.
// FOCAL: also adds the nfp focal block partials (fixed order), loss = w_o overlap + w_f focal, terms = the two unweighted values.
// MASKED: five counters per block; the focal scale is formed here from the valid count (size_average: 1/valid, 1 with no valid pixel --
// the sum is then 0 --; else 1) and left in *gscale for the gradient pass; a term with weight 0 is reported as 0 and adds nothing.
// TOPK: the focal scale is 1/K (K the kept count, state[0] of the select's last level; 1 when K = 0), counts[5] = K, terms[2] = the K-th
// largest term (state[2] holds its key; 0 when K = 0), and `part` holds the nfp block partials of the kept terms.
struct FocalFinish { const double* part; int nfp; double scale; float w_o, w_f; float* terms; int size_average; float* gscale; const long long* kstate; };
template <bool FOCAL = false, bool MASKED = false, bool TOPK = false>
__global__ __launch_bounds__(1024) void tversky_finish_kernel(float* __restrict__ sums, const float* __restrict__ part, int nblk,
                                      const int32_t* __restrict__ pcounts, int ncblk, int32_t* __restrict__ counts,
                                      float alpha, float beta, float eps, int ncls, int W, float* __restrict__ loss,    // W = effective width (1 when the columns are reduced too)
                                      FocalFinish ff = {}) {
    __shared__ double red[256];
    __shared__ float4 lane_sums[1024];
    const int n = 3 * ncls * W, tid = threadIdx.x;
    if (n % 4 == 0 && n / 4 <= 1024) {
        const int n4 = n / 4, LN = 1024 / n4 > 0 ? (1024 / n4 > 16 ? 16 : 1024 / n4) : 1;       // block lanes per float4 of cells
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
    __shared__ int nvalid;                                 // MASKED: the number of valid pixels
    if constexpr (MASKED) {                                // TP / FP / FN / correct / valid: 5 counters x 128 block lanes, LDS tree per counter
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
        if constexpr (TOPK) { if (tid == 5 && counts) counts[5] = (int32_t)ff.kstate[0]; }
        if (tid == 0) nvalid = ired[4 * 128];
    } else
    if (counts) {                                          // TP / FP / FN / correct counts: 256 block lanes x 4 counters, LDS tree (integers: any order)
        int* ired = reinterpret_cast<int*>(lane_sums);
        __syncthreads();                                   // lane_sums is free again
        const int j = tid & 3, l = tid >> 2;
        int v = 0;
        for (int b = l; b < ncblk; b += 256) v += pcounts[b * 4 + j];
        ired[tid] = v;
        __syncthreads();
        for (int s2 = 512; s2 >= 4; s2 >>= 1) { if (tid < s2) ired[tid] += ired[tid + s2]; __syncthreads(); }
        if (tid < 4) counts[tid] = ired[tid];
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
    if constexpr (FOCAL) {
        const float ov = (float)(1.0 - red[0] / nc);
        __syncthreads();                                   // red[0] is read by every thread before it is reused
        double f = 0.0;
        if (tid < 256) { for (int i = tid; i < ff.nfp; i += 256) f += ff.part[i]; red[tid] = f; }
        __syncthreads();
        for (int s = 128; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
        if constexpr (MASKED) {
            if (tid == 0) {
                long long nmean = nvalid;                 // the pixels the focal mean runs over
                if constexpr (TOPK) nmean = ff.kstate[0];
                const double scale = ff.size_average && nmean > 0 ? 1.0 / (double)nmean : 1.0;
                const float fo = (float)(red[0] * scale);
                const float lo = ff.w_o != 0.f ? ff.w_o * ov : 0.f, lf = ff.w_f != 0.f ? ff.w_f * fo : 0.f;
                *loss = lo + lf;
                if (ff.terms) { ff.terms[0] = ff.w_o != 0.f ? ov : 0.f; ff.terms[1] = ff.w_f != 0.f ? fo : 0.f; }
                if constexpr (TOPK) { if (ff.terms) ff.terms[2] = nmean > 0 ? topk_unkey((unsigned)ff.kstate[2]) : 0.f; }
                *ff.gscale = (float)scale;
            }
        } else
        if (tid == 0) {
            const float fo = (float)(red[0] * ff.scale);
            *loss = ff.w_o * ov + ff.w_f * fo;
            if (ff.terms) { ff.terms[0] = ov; ff.terms[1] = fo; }
        }
    } else
    if (tid == 0) *loss = (float)(1.0 - red[0] / nc);
}

// FOCAL: dlogits = w_o dO + w_f dF with dF_k = -(1 - pt)^gamma a[t] gscale ([k == t] - p_k), the factor a constant (focal_kernel)
// MASKED: 0.0f for every class at an ignored pixel (written: the buffer is uninitialised), the focal scale read from *gscale_dev
// TOPK: the focal part is written only where kept[p] != 0 (selected out elsewhere, not multiplied by 0); the overlap part reaches every valid pixel
struct FocalBwd { const float* calpha; float gamma, gscale, w_o, w_f; const float* gscale_dev; int ignore; const uint8_t* kept; };
template <bool FOCAL = false, bool MASKED = false, bool TOPK = false>
__global__ void tversky_bwd_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                                   const float* __restrict__ coef, float alpha, float beta, float* __restrict__ dlogits,
                                   int B, int ncls, int H, int Wimg, int W, FastDiv dhw, FastDiv dWimg, FocalBwd fb = {}) {
    const size_t hw = (size_t)H * Wimg, npix = (size_t)B * hw;
    const size_t p = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    int bi, qi, yi, xi; dhw.divmod((int)p, bi, qi); dWimg.divmod(qi, yi, xi);      // (the entry point keeps B*H*W below 2^31)
    const size_t b = bi, q = qi; const int x = W == 1 ? 0 : xi;
    const int n = ncls * W;
    if constexpr (MASKED) {
        if (labels[p] == fb.ignore) {                      // nothing of this pixel's logits is read
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) dlogits[(b * ncls + k) * hw + q] = 0.f;
            return;
        }
    }
    float l[OUTC_MAXCLS], dp[OUTC_MAXCLS]; float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { l[k] = logits[(b * ncls + k) * hw + q]; m = fmaxf(m, l[k]); }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { l[k] = expf(l[k] - m); den += l[k]; }
    const int t = labels[p];
    const float norm = -1.f / (float)n;
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) {
        l[k] /= den;
        const float invD = coef[k * W + x], tpD2 = coef[n + k * W + x];
        const float tk = t == k ? 1.f : 0.f;
        // d(TP/D)/dp = t/D - TP/D^2 * (t + alpha (1-t) - beta t)
        dp[k] = norm * (tk * invD - tpD2 * (tk + alpha * (1.f - tk) - beta * tk));
        dot += l[k] * dp[k];
    }
    if constexpr (FOCAL) {
        float pt = 0.f;
#pragma unroll
        for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls && k == t) pt = l[k];
        const float a = t < ncls ? (fb.calpha ? fb.calpha[t] : 1.f) : 0.f;                   // a label >= ncls: no focal gradient
        if constexpr (MASKED) {
            const float c = -focal_mod(pt, fb.gamma) * a * fb.gscale_dev[0];
            bool wf = fb.w_f != 0.f;
            if constexpr (TOPK) wf = wf && fb.kept[p] != 0;
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) {
                const float go = fb.w_o != 0.f ? fb.w_o * (l[k] * (dp[k] - dot)) : 0.f;
                const float gf = wf ? fb.w_f * (c * ((k == t ? 1.f : 0.f) - l[k])) : 0.f;
                dlogits[(b * ncls + k) * hw + q] = go + gf;
            }
        } else {
        const float c = -focal_mod(pt, fb.gamma) * a * fb.gscale;
#pragma unroll
        for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls)
            dlogits[(b * ncls + k) * hw + q] = fb.w_o * (l[k] * (dp[k] - dot)) + fb.w_f * (c * ((k == t ? 1.f : 0.f) - l[k]));
        }
    } else {
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) dlogits[(b * ncls + k) * hw + q] = l[k] * (dp[k] - dot);
    }
}

struct OverlapPlan { int We, CW, RL, rpb, gx, gy, nblk, n; };
static OverlapPlan overlap_plan(int B, int ncls, int H, int W, int reduce_w) {
    OverlapPlan p;
    p.We = reduce_w ? 1 : W;
    p.CW = 1; while (p.CW < W && p.CW < 256) p.CW *= 2;
    p.RL = 256 / p.CW;
    const int rows = B * H;
    p.rpb = (rows + 255) / 256; if (p.rpb < p.RL) p.rpb = p.RL;                 // ~256 row blocks
    p.gx = (W + p.CW - 1) / p.CW; p.gy = (rows + p.rpb - 1) / p.rpb;
    p.nblk = reduce_w ? p.gx * p.gy : p.gy;                                     // partial rows the finish kernel adds up
    p.n = 3 * ncls * p.We;
    return p;
}
// The workspace of every entry point below, as byte offsets: [focal block partials, double, nfp of them, padded to 16 bytes][sums n]
// [part nblk*n][pcounts gx*gy*ncnt][focal gradient scale, padded to 16 bytes].  nfp = 0 (no focal term): sums starts the workspace.
// Without a device-side scale the tail is the 8 floats of slack that bdn_overlap_workspace_bytes has always asked for.
static inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }
struct CriterionWs { double* fpart; float* sums; float* part; int32_t* pcounts; float* gscale; };
struct CriterionLayout {
    size_t fpart, sums, part, pcounts, gscale, end;
    CriterionWs carve(void* ws) const {
        char* b = (char*)ws;
        return {(double*)(b + fpart), (float*)(b + sums), (float*)(b + part), (int32_t*)(b + pcounts), (float*)(b + gscale)};
    }
};
static CriterionLayout criterion_layout(const OverlapPlan& p, int nfp, int ncnt, bool has_gscale) {
    CriterionLayout l;
    l.fpart = 0;                                                               // [nfp]
    l.sums = up16(sizeof(double) * nfp);                                       // [n], then the coefficient tables
    l.part = l.sums + sizeof(float) * p.n;                                     // [nblk][n] block partials behind the n final sums
    l.pcounts = l.part + sizeof(float) * (size_t)p.nblk * p.n;                 // [gx*gy][ncnt]
    l.gscale = l.pcounts + sizeof(int32_t) * (size_t)ncnt * p.gx * p.gy;       // the finish writes it, the gradient pass reads it
    l.end = l.gscale + (has_gscale ? 16 : sizeof(float) * 8);
    return l;
}

// The three passes of every entry point below: statistics, finish and, with dlogits, the gradient.  `select` runs between the statistics
// and the finish (bdn_criterion_topk's radix select over the stored terms).
struct OverlapArgs { const float* logits; const uint8_t* labels; float alpha, beta, eps; float* loss; int32_t* counts; float* dlogits; int B, ncls, H, W; };
#define OVERLAP_CHECK_LAUNCH(pass_) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) BDN_FAIL(BDN_E_HIP, "%s_" pass_ ": %s", what, hipGetErrorString(e_)); } while (0)
template <bool FOCAL, bool MASKED, bool TOPK, typename Select = int (*)()>
static int overlap_passes(const char* what, const OverlapArgs& a, const OverlapPlan& p, const CriterionWs& w, const FocalStats& fs,
                          const FocalFinish& ff, const FocalBwd& fb, hipStream_t st, Select select = [] { return (int)BDN_OK; }) {
    dim3 grid(p.gx, p.gy), block(p.RL, p.CW);
    if (a.ncls <= 2) hipLaunchKernelGGL((tversky_sums_kernel<2, FOCAL, MASKED, TOPK>), grid, block, sizeof(float) * 256 * 3 * 2, st, a.logits, a.labels, w.part, w.pcounts, a.B, a.ncls, a.H, a.W, p.rpb, p.We, FastDiv(a.H), fs);
    else hipLaunchKernelGGL((tversky_sums_kernel<OUTC_MAXCLS, FOCAL, MASKED, TOPK>), grid, block, sizeof(float) * 256 * 3 * OUTC_MAXCLS, st, a.logits, a.labels, w.part, w.pcounts, a.B, a.ncls, a.H, a.W, p.rpb, p.We, FastDiv(a.H), fs);
    OVERLAP_CHECK_LAUNCH("stats");
    if (int rc = select()) return rc;
    hipLaunchKernelGGL((tversky_finish_kernel<FOCAL, MASKED, TOPK>), dim3(1), dim3(1024), 0, st, w.sums, w.part, p.nblk, w.pcounts, p.gx * p.gy, a.counts, a.alpha, a.beta, a.eps, a.ncls, p.We, a.loss, ff);
    OVERLAP_CHECK_LAUNCH("finish");
    if (a.dlogits) {
        hipLaunchKernelGGL((tversky_bwd_kernel<FOCAL, MASKED, TOPK>), dim3(grid_for((size_t)a.B * a.H * a.W)), dim3(256), 0, st, a.logits, a.labels, w.sums, a.alpha, a.beta, a.dlogits, a.B, a.ncls, a.H, a.W, p.We,
                           FastDiv(a.H * a.W), FastDiv(a.W), fb);
        OVERLAP_CHECK_LAUNCH("bwd");
    }
    return BDN_OK;
}
#undef OVERLAP_CHECK_LAUNCH

// what bdn_criterion, _masked and _topk check alike, behind their null-pointer test and their own extras
static int criterion_check(const char* what, float w_overlap, float w_focal, float gamma, int B, int ncls, int H, int W, const void* ws) {
    if (!(w_overlap >= 0.f) || !(w_focal >= 0.f)) BDN_FAIL(BDN_E_ARG, "%s: negative weight (w_overlap=%g, w_focal=%g)", what, w_overlap, w_focal);
    if (w_overlap == 0.f && w_focal == 0.f) BDN_FAIL(BDN_E_ARG, "%s: both weights are zero", what);
    if (!(gamma >= 0.f)) BDN_FAIL(BDN_E_ARG, "%s: negative gamma", what);
    if (ncls < 2 || ncls > OUTC_MAXCLS) BDN_FAIL(BDN_E_SHAPE, "%s: ncls=%d unsupported (2..%d)", what, ncls, OUTC_MAXCLS);
    if (B <= 0 || H <= 0 || W <= 0 || (size_t)B * H * W >= ((size_t)1 << 31)) BDN_FAIL(BDN_E_SHAPE, "%s: bad shape (B*H*W must stay below 2^31)", what);
    if ((uintptr_t)ws & 15) BDN_FAIL(BDN_E_ARG, "%s: ws must be 16-byte aligned", what);
    return BDN_OK;
}

extern "C" size_t bdn_overlap_workspace_bytes(int B, int ncls, int H, int W, int reduce_w) {
    if (B <= 0 || H <= 0 || W <= 0 || ncls < 2 || ncls > OUTC_MAXCLS) return 0;          // (B*H*W >= 2^31 is refused by bdn_overlap_loss, not here)
    return criterion_layout(overlap_plan(B, ncls, H, W, reduce_w), 0, 4, false).end;
}

extern "C" int bdn_overlap_loss(const float* logits, const uint8_t* labels, float alpha, float beta, float eps,
                                int reduce_w, float* ws, float* loss, int32_t* counts, float* dlogits,
                                int B, int ncls, int H, int W, void* stream) {
    if (!logits || !labels || !ws || !loss) BDN_FAIL(BDN_E_ARG, "overlap_loss: null pointer");
    if (ncls < 2 || ncls > OUTC_MAXCLS) BDN_FAIL(BDN_E_SHAPE, "overlap_loss: ncls=%d unsupported (2..%d)", ncls, OUTC_MAXCLS);
    if (B <= 0 || H <= 0 || W <= 0 || (size_t)B * H * W >= ((size_t)1 << 31)) BDN_FAIL(BDN_E_SHAPE, "overlap_loss: bad shape");
    const OverlapPlan p = overlap_plan(B, ncls, H, W, reduce_w);
    return overlap_passes<false, false, false>("overlap_loss", {logits, labels, alpha, beta, eps, loss, counts, dlogits, B, ncls, H, W}, p,
                                               criterion_layout(p, 0, 4, false).carve(ws), {}, {}, {}, (hipStream_t)stream);
}

extern "C" int bdn_tversky(const float* logits, const uint8_t* labels, float alpha, float beta, float eps,
                           float* ws, float* loss, int32_t* counts, float* dlogits,
                           int B, int ncls, int H, int W, void* stream) {
    return bdn_overlap_loss(logits, labels, alpha, beta, eps, 0, ws, loss, counts, dlogits, B, ncls, H, W, stream);
}

// ============================================================ Focal loss (utils/metrics.py:8-48)
// loss_i = -(1 - pt)^gamma * a[t] * log pt with pt = softmax(l)[t]; the modulating factor is built from
// `logpt.data.exp()` (:35) and is therefore a constant for the gradient:
//   d loss_i / d l_k = -(1 - pt)^gamma * a[t] * ([k == t] - p_k)   (times 1/N when size_average).
// pass 1: per-pixel loss + dlogits, per-block partial sums (double) -> ws;  pass 2: fixed-order finish.
__global__ void focal_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels,
                             const float* __restrict__ alpha, float gamma, float gscale,
                             double* __restrict__ part, int32_t* __restrict__ counts, float* __restrict__ dlogits,
                             int B, int ncls, size_t hw) {
    __shared__ double red[256];
    __shared__ int ired[256 * 4];
    const size_t npix = (size_t)B * hw;
    double acc = 0.0;
    int c_tp = 0, c_fp = 0, c_fn = 0, c_ok = 0;
    for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < npix; p += (size_t)gridDim.x * 256) {
        const size_t b = p / hw, q = p % hw;
        float l[OUTC_MAXCLS]; float m = -INFINITY; int am = 0;
#pragma unroll
        for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { l[k] = logits[(b * ncls + k) * hw + q]; if (l[k] > m) { m = l[k]; am = k; } }
        float den = 0.f;
#pragma unroll
        for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) den += expf(l[k] - m);
        const int t = labels[p];
        // log-softmax on the maximum-subtracted logits, (l - m) - log(den): forming lse = m + log(den) first rounds log(den) to an ulp of m
        // and makes the loss depend on a common shift of the logits (1e-3 at |l| ~ 8192)
        const float logden = logf(den);
        float ltm = 0.f;
#pragma unroll
        for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls && k == t) ltm = l[k] - m;      // (l[k] is not loaded for k >= ncls)
        const float logpt = ltm - logden, pt = expf(logpt);
        const float a = t < ncls ? (alpha ? alpha[t] : 1.f) : 0.f;     // a label >= ncls has no true class: term and gradient are 0, alpha is not indexed
        const float mod = gamma == 0.f ? 1.f : powf(fmaxf(1.f - pt, 0.f), gamma);
        acc += (double)(-mod * a * logpt);
        if (dlogits) {
            const float c = -mod * a * gscale;
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls)
                dlogits[(b * ncls + k) * hw + q] = c * ((k == t ? 1.f : 0.f) - expf((l[k] - m) - logden));
        }
        c_tp += (am == 1 && t == 1); c_fp += (am == 1 && t != 1); c_fn += (am != 1 && t == 1); c_ok += (am == t);
    }
    red[threadIdx.x] = acc;
    ired[threadIdx.x * 4 + 0] = c_tp; ired[threadIdx.x * 4 + 1] = c_fp; ired[threadIdx.x * 4 + 2] = c_fn; ired[threadIdx.x * 4 + 3] = c_ok;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
    if (counts && threadIdx.x < 4) { int v = 0; for (int i = 0; i < 256; i++) v += ired[i * 4 + threadIdx.x]; atomicAdd(&counts[threadIdx.x], v); }
}

__global__ void focal_finish_kernel(const double* __restrict__ part, int nblk, double scale, float* __restrict__ loss) {
    __shared__ double red[256];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 256) acc += part[i];
    red[threadIdx.x] = acc; __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s]; __syncthreads(); }
    if (threadIdx.x == 0) *loss = (float)(red[0] * scale);
}

extern "C" size_t bdn_focal_workspace_bytes(void) { return sizeof(double) * 1024; }

extern "C" int bdn_focal(const float* logits, const uint8_t* labels, float gamma, const float* alpha, int size_average,
                         void* ws, float* loss, int32_t* counts, float* dlogits,
                         int B, int ncls, int H, int W, void* stream) {
    if (!logits || !labels || !ws || !loss) BDN_FAIL(BDN_E_ARG, "focal: null pointer");
    if (ncls < 2 || ncls > OUTC_MAXCLS) BDN_FAIL(BDN_E_SHAPE, "focal: ncls=%d unsupported (2..%d)", ncls, OUTC_MAXCLS);
    if (B <= 0 || H <= 0 || W <= 0 || gamma < 0.f) BDN_FAIL(BDN_E_SHAPE, "focal: bad shape or negative gamma");
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)B * H * W;
    int nblk = (int)((npix + 255) / 256); if (nblk > 1024) nblk = 1024;
    if (counts && hipMemsetAsync(counts, 0, sizeof(int32_t) * 4, st) != hipSuccess) BDN_FAIL(BDN_E_HIP, "focal: memset failed");
    const double inv = size_average ? 1.0 / (double)npix : 1.0;
    hipLaunchKernelGGL(focal_kernel, dim3(nblk), dim3(256), 0, st, logits, labels, alpha, gamma, (float)inv,
                       (double*)ws, counts, dlogits, B, ncls, (size_t)H * W);
    BDN_CHECK_LAUNCH("focal");
    hipLaunchKernelGGL(focal_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, nblk, inv, loss);
    BDN_CHECK_LAUNCH("focal_finish");
    return BDN_OK;
}

// ============================================================ criterion: w_overlap Overlap + w_focal Focal (utils/helpers.py:303-312)
// One term with weight 1 is the existing entry point, launch for launch (same bits).  Anything else -- the compound losses -- runs the
// overlap loss's three passes in their FOCAL form: statistics (softmax once per pixel -> overlap partial sums, focal partial sums in
// double, argmax counts), the fixed-order finish, and one gradient pass that writes w_overlap dO + w_focal dF.  No atomics, no memset.
// ws: [focal block partials, double, padded to 16 bytes][bdn_overlap_loss's workspace].
__global__ void criterion_terms_kernel(const float* __restrict__ loss, float* __restrict__ terms, int slot) {
    terms[slot] = *loss; terms[1 - slot] = 0.f;
}

extern "C" size_t bdn_criterion_workspace_bytes(int B, int ncls, int H, int W, int reduce_w) {
    if (bdn_overlap_workspace_bytes(B, ncls, H, W, reduce_w) == 0 || (size_t)B * H * W >= ((size_t)1 << 31)) return 0;
    const OverlapPlan p = overlap_plan(B, ncls, H, W, reduce_w);
    const size_t compound = criterion_layout(p, p.gx * p.gy, 4, false).end, focal = bdn_focal_workspace_bytes();
    return compound > focal ? compound : focal;
}

extern "C" int bdn_criterion(const float* logits, const uint8_t* labels, float w_overlap, float alpha, float beta, float eps, int reduce_w,
                             float w_focal, float gamma, const float* class_alpha, int size_average, void* ws, float* loss, float* terms,
                             int32_t* counts, float* dlogits, int B, int ncls, int H, int W, void* stream) {
    if (!logits || !labels || !ws || !loss) BDN_FAIL(BDN_E_ARG, "criterion: null pointer");
    if (int rc = criterion_check("criterion", w_overlap, w_focal, gamma, B, ncls, H, W, ws)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((w_focal == 0.f && w_overlap == 1.f) || (w_overlap == 0.f && w_focal == 1.f)) {
        const int focal = w_overlap == 0.f;
        const int rc = focal ? bdn_focal(logits, labels, gamma, class_alpha, size_average, ws, loss, counts, dlogits, B, ncls, H, W, stream)
                             : bdn_overlap_loss(logits, labels, alpha, beta, eps, reduce_w, (float*)ws, loss, counts, dlogits, B, ncls, H, W, stream);
        if (rc != BDN_OK || !terms) return rc;
        hipLaunchKernelGGL(criterion_terms_kernel, dim3(1), dim3(1), 0, st, loss, terms, focal);
        BDN_CHECK_LAUNCH("criterion_terms");
        return BDN_OK;
    }
    const OverlapPlan p = overlap_plan(B, ncls, H, W, reduce_w);
    const CriterionWs w = criterion_layout(p, p.gx * p.gy, 4, false).carve(ws);
    const double inv = size_average ? 1.0 / (double)((size_t)B * H * W) : 1.0;
    return overlap_passes<true, false, false>("criterion", {logits, labels, alpha, beta, eps, loss, counts, dlogits, B, ncls, H, W}, p, w,
                                              FocalStats{class_alpha, gamma, w.fpart},
                                              FocalFinish{w.fpart, p.gx * p.gy, inv, w_overlap, w_focal, terms},
                                              FocalBwd{class_alpha, gamma, (float)inv, w_overlap, w_focal}, st);
}

// ============================================================ criterion with an ignore label
// bdn_criterion's function over the VALID pixels (label != ignore_label): always the three MASKED launches above, whatever the weights.
// ws: [focal block partials, double, padded to 16 bytes][sums n][part nblk*n][pcounts gx*gy*5][focal gradient scale, padded to 16 bytes].
extern "C" size_t bdn_criterion_masked_workspace_bytes(int B, int ncls, int H, int W, int reduce_w) {
    if (B <= 0 || H <= 0 || W <= 0 || ncls < 2 || ncls > OUTC_MAXCLS || (size_t)B * H * W >= ((size_t)1 << 31)) return 0;
    const OverlapPlan p = overlap_plan(B, ncls, H, W, reduce_w);
    return criterion_layout(p, p.gx * p.gy, 5, true).end;
}

extern "C" int bdn_criterion_masked(const float* logits, const uint8_t* labels, int ignore_label, float w_overlap, float alpha, float beta,
                                    float eps, int reduce_w, float w_focal, float gamma, const float* class_alpha, int size_average,
                                    void* ws, float* loss, float* terms, int32_t* counts, float* dlogits, int B, int ncls, int H, int W,
                                    void* stream) {
    if (!logits || !labels || !ws || !loss) BDN_FAIL(BDN_E_ARG, "criterion_masked: null pointer");
    if (ignore_label < 0 || ignore_label > 255) BDN_FAIL(BDN_E_ARG, "criterion_masked: ignore_label=%d is not a byte value (0..255)", ignore_label);
    if (int rc = criterion_check("criterion_masked", w_overlap, w_focal, gamma, B, ncls, H, W, ws)) return rc;
    const OverlapPlan p = overlap_plan(B, ncls, H, W, reduce_w);
    const CriterionWs w = criterion_layout(p, p.gx * p.gy, 5, true).carve(ws);
    return overlap_passes<true, true, false>("criterion_masked", {logits, labels, alpha, beta, eps, loss, counts, dlogits, B, ncls, H, W}, p, w,
                                             FocalStats{class_alpha, gamma, w.fpart, ignore_label},
                                             FocalFinish{w.fpart, p.gx * p.gy, 1.0, w_overlap, w_focal, terms, size_average, w.gscale},
                                             FocalBwd{class_alpha, gamma, 1.f, w_overlap, w_focal, w.gscale, ignore_label}, (hipStream_t)stream);
}

// ============================================================ criterion with top-k hard-pixel mining
// bdn_criterion_masked's function with the focal term averaged over the K hardest valid pixels only (include/bidate_hip.h states the
// semantics).  The statistics pass stores every pixel's float32 focal term; an exact radix select over the 32-bit keys
//   key = u ^ 0x80000000 (sign bit clear) or ~u (sign bit set), u the term's bit pattern       -- monotone: -0 < +0, +inf on top
// finds the K-th largest key T in three levels of 11 + 11 + 10 bits; ties at T are kept in pixel-index order.  Launches:
//   memset   the three level histograms (20 KB)
//   stats    tversky_sums_kernel<.., TOPK>: overlap partials, counts, pterm[p]
//   hist<0>  histogram of key >> 21 over the valid pixels
//   hist<1>  every block first reduces level 0's histogram to (K, digit, remaining rank) -- block 0 records it --, then histograms
//            (key >> 10) & 2047 among the keys with that top digit
//   hist<2>  the same one level down: key & 1023 among the keys with the 22-bit prefix
//   hist<3>  reduces level 2 to T and the number of ties to keep, then counts the keys == T per chunk of 256 consecutive pixels
//   sum      per block a run of consecutive chunks: the ties before it (sum of the chunk counts), the kept byte of every pixel
//            (key > T, or key == T and fewer than `ties to keep` ties before it in index order), the block's sum of kept terms in double
//   finish   tversky_finish_kernel<.., TOPK>: block partials in a fixed order, 1/K, counts[5] = K, terms[2] = the threshold
//   bwd      tversky_bwd_kernel<.., TOPK>
// Histogram counts are integers (LDS and global integer atomics: their order cannot change a sum); no float atomics, no host read-back.
// ws: [kept-term block partials, double][sums n][part nblk*n][pcounts gx*gy*5][gscale, 16 B][state 3 x 4 int64][hist 2048 + 2048 + 1024]
//     [chunk tie counts][pterm npix f32][kept npix u8], every part padded to 16 bytes.
__host__ __device__ constexpr int topk_bins(int level) { return level < 2 ? 2048 : 1024; }
__host__ __device__ constexpr int topk_shift(int level) { return level == 0 ? 21 : level == 1 ? 10 : 0; }
__host__ __device__ constexpr int topk_hist_off(int level) { return level * 2048; }
constexpr int TOPK_HIST_TOTAL = 5120;
constexpr int TOPK_CHUNK = 256;                    // pixels per tie-count chunk = one block's pass over consecutive pixels

struct TopkPlan { OverlapPlan ov; int npix, nchunks, cpb, nsb, hgrid; CriterionLayout cl; size_t o_state, o_hist, o_tie, o_pterm, o_kept, total; };
static TopkPlan topk_plan(int B, int ncls, int H, int W, int reduce_w) {
    TopkPlan t;
    t.ov = overlap_plan(B, ncls, H, W, reduce_w);
    t.npix = B * H * W;
    t.nchunks = (t.npix + TOPK_CHUNK - 1) / TOPK_CHUNK;
    t.cpb = (t.nchunks + 511) / 512;                                           // chunks per block of the sum pass: at most 512 blocks
    t.nsb = (t.nchunks + t.cpb - 1) / t.cpb;
    t.hgrid = t.nchunks < 1024 ? t.nchunks : 1024;                             // histogram passes: grid-stride over the chunks
    t.cl = criterion_layout(t.ov, t.nsb, 5, true);                             // bdn_criterion_masked's layout behind the nsb kept-term partials
    t.o_state = up16(t.cl.end);
    t.o_hist = t.o_state + sizeof(long long) * 12;
    t.o_tie = t.o_hist + sizeof(unsigned) * TOPK_HIST_TOTAL;
    t.o_pterm = up16(t.o_tie + sizeof(int32_t) * t.nchunks);
    t.o_kept = up16(t.o_pterm + sizeof(float) * (size_t)t.npix);
    t.total = up16(t.o_kept + (size_t)t.npix);
    return t;
}

// The select of one level, by every thread of a 256-thread block: the digit d of the level's histogram with
//   count(bins > d) < rem <= count(bins >= d),   and greater = count(bins > d).
// FIRST: rem is formed here from the histogram's total (= the valid pixels): K = max(1, total * ppm / 1e6), 0 without a valid pixel.
// rem = 0 (no valid pixel) gives digit 0, greater 0.  Bins are walked from the top: thread t owns bins NB-1 - t*PER - j.
template <int NB, bool FIRST>
__device__ void topk_block_select(const unsigned* __restrict__ hist, long long& rem, int ppm, int& digit, long long& greater) {
    constexpr int PER = NB / 256;
    __shared__ unsigned scan[256];
    __shared__ int s_digit; __shared__ unsigned s_greater;
    const int tid = threadIdx.x;
    unsigned c[PER], s = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) { c[j] = hist[NB - 1 - tid * PER - j]; s += c[j]; }
    if (tid == 0) { s_digit = 0; s_greater = 0; }
    scan[tid] = s;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {              // inclusive scan (counts stay below 2^31: B*H*W does)
        const unsigned v = tid >= off ? scan[tid - off] : 0u;
        __syncthreads();
        scan[tid] += v;
        __syncthreads();
    }
    if constexpr (FIRST) {
        const long long total = scan[255];
        const long long k = total * (long long)ppm / 1000000;
        rem = total == 0 ? 0 : (k < 1 ? 1 : k);
    }
    const long long incl = scan[tid], excl = incl - s;
    if (rem > excl && rem <= incl) {                       // one thread at most
        long long run = excl;
#pragma unroll
        for (int j = 0; j < PER; j++) {
            if (run + c[j] >= rem) { s_digit = NB - 1 - tid * PER - j; s_greater = (unsigned)run; break; }
            run += c[j];
        }
    }
    __syncthreads();
    digit = s_digit; greater = s_greater;
    __syncthreads();                                       // (the shared cells are free for a second call)
}

// state[l] = {K, remaining rank after level l, key prefix after level l, unused}; state[2] = {K, ties to keep, T}
// LEVEL 0..2: the histogram of that level's digit; LEVEL 3: the chunk tie counts.
template <int LEVEL>
__global__ __launch_bounds__(256) void topk_hist_kernel(const float* __restrict__ pterm, const uint8_t* __restrict__ labels, int ignore,
                                                        int npix, int nchunks, int ppm, unsigned* __restrict__ hist,
                                                        long long* __restrict__ state, int32_t* __restrict__ tiecnt) {
    constexpr int NB = topk_bins(LEVEL < 3 ? LEVEL : 2);
    __shared__ unsigned lh[NB];
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned prefix = 0;
    if constexpr (LEVEL >= 1) {                            // the level above, reduced by every block alike
        constexpr int PL = LEVEL - 1;
        long long K = 0, rem = 0, greater; int digit;
        if constexpr (PL > 0) { K = state[(PL - 1) * 4 + 0]; rem = state[(PL - 1) * 4 + 1]; prefix = (unsigned)state[(PL - 1) * 4 + 2]; }
        topk_block_select<topk_bins(PL), PL == 0>(hist + topk_hist_off(PL), rem, ppm, digit, greater);
        if constexpr (PL == 0) K = rem;
        rem -= greater;
        prefix |= (unsigned)digit << topk_shift(PL);
        if (blockIdx.x == 0 && tid == 0) { state[PL * 4 + 0] = K; state[PL * 4 + 1] = rem; state[PL * 4 + 2] = prefix; state[PL * 4 + 3] = 0; }
    }
    if constexpr (LEVEL == 3) {
        for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
            const int p = c * TOPK_CHUNK + tid;
            bool tie = false;
            if (p < npix && labels[p] != ignore) tie = topk_key(pterm[p]) == prefix;
            const int n = __syncthreads_count(tie);
            if (tid == 0) tiecnt[c] = n;
        }
    } else {
        for (int i = tid; i < NB; i += 256) lh[i] = 0;
        __syncthreads();
        for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
            const int p = c * TOPK_CHUNK + tid;
            bool active = false; unsigned digit = 0;
            if (p < npix && labels[p] != ignore) {
                const unsigned key = topk_key(pterm[p]);
                if constexpr (LEVEL == 0) active = true;
                else active = (key >> topk_shift(LEVEL - 1)) == (prefix >> topk_shift(LEVEL - 1));
                digit = (key >> topk_shift(LEVEL)) & (NB - 1);
            }
            // the top digit is sign, exponent and two mantissa bits: most of a wave's lanes share a few values, and same-address LDS atomics
            // serialise.  Up to four rounds of "the first active lane's digit, one add of the matching lanes' count"; what is left (many
            // distinct digits: the lower levels) goes lane by lane to different addresses.
            for (int round = 0; round < 4; round++) {
                const unsigned long long am = __ballot(active);
                if (am == 0) break;                        // wave-uniform
                const int leader = __ffsll((long long)am) - 1;
                const unsigned d0 = __shfl(digit, leader);
                const bool same = active && digit == d0;
                const unsigned long long sm = __ballot(same);
                if (lane == leader) atomicAdd(&lh[d0], (unsigned)__popcll(sm));
                active = active && !same;
            }
            if (active) atomicAdd(&lh[digit], 1u);
        }
        __syncthreads();
        unsigned* gh = hist + topk_hist_off(LEVEL < 3 ? LEVEL : 2);
        for (int i = tid; i < NB; i += 256) { const unsigned v = lh[i]; if (v) atomicAdd(&gh[i], v); }
    }
}

// kept bytes and the block partials of the kept terms.  Block b owns chunks [b*cpb, (b+1)*cpb): a thread adds its pixels in chunk order,
// the block's 256 lanes meet in an LDS tree -- a fixed order.
__global__ __launch_bounds__(256) void topk_sum_kernel(const float* __restrict__ pterm, const uint8_t* __restrict__ labels, int ignore,
                                                       int npix, int nchunks, int cpb, const long long* __restrict__ state,
                                                       const int32_t* __restrict__ tiecnt, uint8_t* __restrict__ kept_ws,
                                                       double* __restrict__ part, float* __restrict__ terms_out, uint8_t* __restrict__ kept_out) {
    __shared__ long long lred[256];
    __shared__ double dred[256];
    __shared__ int wcnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long keep_ties = state[2 * 4 + 1];
    const unsigned T = (unsigned)state[2 * 4 + 2];
    const int c0 = blockIdx.x * cpb, c1 = min(nchunks, c0 + cpb);
    long long before = 0;                                  // ties in the chunks in front of this block
    for (int c = tid; c < c0; c += 256) before += tiecnt[c];
    lred[tid] = before;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) lred[tid] += lred[tid + s]; __syncthreads(); }
    before = lred[0];
    double acc = 0.0;
    for (int c = c0; c < c1; c++) {
        const int p = c * TOPK_CHUNK + tid;
        const bool in = p < npix;
        float v = 0.f; bool valid = false;
        if (in) { v = pterm[p]; valid = labels[p] != ignore; }
        const unsigned key = topk_key(v);
        const bool tie = valid && key == T;
        const unsigned long long tm = __ballot(tie);
        if (lane == 0) wcnt[wave] = __popcll(tm);
        __syncthreads();
        long long rank = before + __popcll(tm & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) rank += wcnt[w];
        const bool kept = valid && (key > T || (tie && rank < keep_ties));
        if (in) {
            kept_ws[p] = kept ? 1 : 0;
            if (kept_out) kept_out[p] = kept ? 1 : 0;
            if (terms_out) terms_out[p] = v;
        }
        if (kept) acc += (double)v;
        before += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();                                   // wcnt is rewritten by the next chunk
    }
    dred[tid] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) { if (tid < s) dred[tid] += dred[tid + s]; __syncthreads(); }
    if (tid == 0) part[blockIdx.x] = dred[0];
}

extern "C" size_t bdn_criterion_topk_workspace_bytes(int B, int ncls, int H, int W, int reduce_w) {
    if (B <= 0 || H <= 0 || W <= 0 || ncls < 2 || ncls > OUTC_MAXCLS || (size_t)B * H * W >= ((size_t)1 << 31)) return 0;
    return topk_plan(B, ncls, H, W, reduce_w).total;
}

extern "C" int bdn_criterion_topk(const float* logits, const uint8_t* labels, int ignore_label, float w_overlap, float alpha, float beta,
                                  float eps, int reduce_w, float w_focal, float gamma, const float* class_alpha, int size_average,
                                  int topk_ppm, void* ws, float* loss, float* terms, int32_t* counts, float* dlogits, float* pixel_terms,
                                  uint8_t* kept, int B, int ncls, int H, int W, void* stream) {
    if (!logits || !labels || !ws || !loss) BDN_FAIL(BDN_E_ARG, "criterion_topk: null pointer");
    if (ignore_label < -1 || ignore_label > 255) BDN_FAIL(BDN_E_ARG, "criterion_topk: ignore_label=%d is neither -1 (none) nor a byte value (0..255)", ignore_label);
    if (topk_ppm < 1 || topk_ppm > 1000000) BDN_FAIL(BDN_E_ARG, "criterion_topk: topk_ppm=%d outside 1..1000000", topk_ppm);
    if (!(w_overlap >= 0.f) || !(w_focal > 0.f)) BDN_FAIL(BDN_E_ARG, "criterion_topk: top-k ranks the focal term: w_focal > 0 and w_overlap >= 0 (w_overlap=%g, w_focal=%g)", w_overlap, w_focal);
    if (int rc = criterion_check("criterion_topk", w_overlap, w_focal, gamma, B, ncls, H, W, ws)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const TopkPlan t = topk_plan(B, ncls, H, W, reduce_w);
    const CriterionWs w = t.cl.carve(ws);                                      // fpart: [nsb] block partials of the kept terms
    char* base = (char*)ws;
    long long* state = (long long*)(base + t.o_state);
    unsigned* hist = (unsigned*)(base + t.o_hist);
    int32_t* tiecnt = (int32_t*)(base + t.o_tie);
    float* pterm = (float*)(base + t.o_pterm);
    uint8_t* kept_ws = (uint8_t*)(base + t.o_kept);
    if (hipMemsetAsync(hist, 0, sizeof(unsigned) * TOPK_HIST_TOTAL, st) != hipSuccess) BDN_FAIL(BDN_E_HIP, "criterion_topk: memset failed");
    const auto select = [&]() -> int {
#define TOPK_HIST(L_) hipLaunchKernelGGL(topk_hist_kernel<L_>, dim3(t.hgrid), dim3(256), 0, st, pterm, labels, ignore_label, t.npix, t.nchunks, topk_ppm, hist, state, tiecnt)
        TOPK_HIST(0); BDN_CHECK_LAUNCH("criterion_topk_hist0");
        TOPK_HIST(1); BDN_CHECK_LAUNCH("criterion_topk_hist1");
        TOPK_HIST(2); BDN_CHECK_LAUNCH("criterion_topk_hist2");
        TOPK_HIST(3); BDN_CHECK_LAUNCH("criterion_topk_ties");
#undef TOPK_HIST
        hipLaunchKernelGGL(topk_sum_kernel, dim3(t.nsb), dim3(256), 0, st, pterm, labels, ignore_label, t.npix, t.nchunks, t.cpb, state, tiecnt, kept_ws, w.fpart, pixel_terms, kept);
        BDN_CHECK_LAUNCH("criterion_topk_sum");
        return BDN_OK;
    };
    return overlap_passes<true, true, true>("criterion_topk", {logits, labels, alpha, beta, eps, loss, counts, dlogits, B, ncls, H, W}, t.ov, w,
                                            FocalStats{class_alpha, gamma, nullptr, ignore_label, pterm},
                                            FocalFinish{w.fpart, t.nsb, 1.0, w_overlap, w_focal, terms, size_average, w.gscale, state + 8},
                                            FocalBwd{class_alpha, gamma, 1.f, w_overlap, w_focal, w.gscale, ignore_label, kept_ws}, st, select);
}
