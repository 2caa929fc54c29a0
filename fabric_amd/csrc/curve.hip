// libbidate_hip: threshold-free validation.  The reference judges a model at the argmax only (train.py:96-106 and train.py:151-158: argmax +
// sklearn's precision_recall_fscore_support per batch; train.py:199: the argmax mask of a scene), which for two classes is a probability
// threshold of 0.5.  Here the score s = P(pos_class) of every valid pixel is counted into a fixed-bin histogram, split by label, that is
// accumulated on the device over a whole validation pass (bdn_score_hist); one finishing launch turns it into the precision / recall
// curve, the best-F1 threshold and the average precision (bdn_score_curve); bdn_threshold_mask applies a threshold to a scene's
// probabilities.  Everything that is summed across threads is an integer (LDS and global integer atomics): integer sums do not depend on
// arrival order, so the histogram is the same bits on every run, for any grid and any split of the pixels into calls.  There are no float
// atomics; the curve's floating-point sums run in a fixed order.
#include "common.hpp"
#include "hist_core.hpp"

constexpr int SH_THREADS = 256;
// The grid: one block per 4 x 256 items, at most 2048 blocks (8 per CU; the rest is grid-strided).  Measured at 1024 bins on the training
// shape and on a 10 000^2 scene: fewer, longer-lived blocks save the per-block LDS clear and flush -- up to 2 n_bins
// global adds each, all blocks on one address when the input is skewed -- (one item per thread: 31 -> 18 us on uniform scores), while the
// scene wants the residency (256 / 512 / 1024 / 2048 / 4096 / 8192 blocks: 595 / 320 / 200 / 158 / 152 / 215 us).
constexpr int SH_MAX_BLOCKS = 2048;
constexpr int SH_MIN_ITEMS = 4;
constexpr int SH_MAX_BINS = 4096;
constexpr long long SH_MAX_PIXELS = 1LL << 40;          // a block then counts < 2^32 pixels into its 32-bit LDS cells whatever the grid

// ============================================================ score_hist
// The block histogram is filled by wave_hist_add (hist_core.hpp) with key = label_is_pos * n_bins + bin.
struct ScoreHistArgs {
    const float* x; const uint8_t* labels; unsigned long long* hist; float* scores_out;
    long long HW, Q, total, stride_img, stride_off;      // Q: items per image; total = n_img * Q; the grid's stride over the items, split by Q
    int is_logits, ignore, pos, ncls, n_bins;
};

// An item is PER consecutive pixels of one image (PER = 4: 16-byte loads of every class plane, 4 label bytes in one load, a 16-byte score
// store; taken when HW % 4 == 0 and the pointers are aligned; PER = 1 otherwise).  NC: the class count when it is 2 (logits stay in
// registers), 0 = a.ncls (the planes are read once per pass over the classes, from L1/L2 after the first).  The loop's trip count is the
// same for every thread of a block (the ballots of wave_hist_add need whole waves), lanes past the end carry no pixel.
template <int NC, int PER>
__global__ __launch_bounds__(SH_THREADS) void score_hist_kernel(const ScoreHistArgs a) {
    extern __shared__ unsigned sh_lds[];                  // [2][n_bins] counts of this block, negatives first
    const int tid = threadIdx.x, lane = tid & 63;
    const int ncls = NC ? NC : a.ncls, n_bins = a.n_bins;
    for (int i = tid; i < 2 * n_bins; i += SH_THREADS) sh_lds[i] = 0;
    __syncthreads();
    const long long stride = (long long)gridDim.x * SH_THREADS, base0 = (long long)blockIdx.x * SH_THREADS;
    long long idx = base0 + tid;
    long long img = idx / a.Q, off = idx - img * a.Q;     // the only division; the stride is added in its (image, offset) parts
    const float fb = (float)n_bins;
    for (long long base = base0; base < a.total; base += stride) {
        int key[PER];
#pragma unroll
        for (int p = 0; p < PER; p++) key[p] = -1;
        if (idx < a.total) {
            const long long pix = off * PER;
            const float* xp = a.x + (size_t)img * ncls * a.HW + pix;
            int lab[PER];
            PixVec<PER>::labels(a.labels + (size_t)img * a.HW + pix, lab);
            float s[PER];
            if (a.is_logits) {
                // blend_fold_kernel's expression: m = max_c l_c, e_c = expf(l_c - m), sum in class order, e_pos / sum
                float m[PER], sum[PER], v[PER];
                if constexpr (NC == 2) {
                    float l0[PER], l1[PER];
                    PixVec<PER>::load(xp, l0);
                    PixVec<PER>::load(xp + a.HW, l1);
#pragma unroll
                    for (int p = 0; p < PER; p++) {
                        m[p] = fmaxf(l0[p], l1[p]);
                        const float e0 = expf(l0[p] - m[p]), e1 = expf(l1[p] - m[p]);
                        sum[p] = e0 + e1;
                        s[p] = (a.pos ? e1 : e0) / sum[p];
                    }
                } else {
                    PixVec<PER>::load(xp, m);
                    for (int c = 1; c < ncls; c++) {
                        PixVec<PER>::load(xp + (size_t)c * a.HW, v);
#pragma unroll
                        for (int p = 0; p < PER; p++) m[p] = fmaxf(m[p], v[p]);
                    }
#pragma unroll
                    for (int p = 0; p < PER; p++) sum[p] = 0.f;
                    for (int c = 0; c < ncls; c++) {
                        PixVec<PER>::load(xp + (size_t)c * a.HW, v);
#pragma unroll
                        for (int p = 0; p < PER; p++) sum[p] += expf(v[p] - m[p]);
                    }
                    PixVec<PER>::load(xp + (size_t)a.pos * a.HW, v);
#pragma unroll
                    for (int p = 0; p < PER; p++) s[p] = expf(v[p] - m[p]) / sum[p];
                }
            } else {
                PixVec<PER>::load(xp + (size_t)a.pos * a.HW, s);
            }
#pragma unroll
            for (int p = 0; p < PER; p++) {
                const bool ign = lab[p] == a.ignore;          // nothing of an ignored pixel's logits survives this select
                const float sc = ign ? 0.f : s[p];
                const int bin = sc >= 1.f ? n_bins - 1 : sc > 0.f ? (int)(sc * fb) : 0;      // NaN: bin 0
                key[p] = ign ? -1 : (lab[p] == a.pos ? n_bins : 0) + bin;
                s[p] = sc;
            }
            if (a.scores_out) PixVec<PER>::store(a.scores_out + (size_t)img * a.HW + pix, s);
        }
#pragma unroll
        for (int p = 0; p < PER; p++) wave_hist_add(sh_lds, key[p], lane);
        idx += stride; off += a.stride_off; img += a.stride_img;
        if (off >= a.Q) { off -= a.Q; img++; }
    }
    __syncthreads();
    for (int i = tid; i < 2 * n_bins; i += SH_THREADS) {
        const unsigned c = sh_lds[i];
        if (c) atomicAdd(&a.hist[i], (unsigned long long)c);    // one 64-bit integer add per occupied bin and block
    }
}

static inline bool pow2_bins(int n) { return n >= 2 && n <= SH_MAX_BINS && (n & (n - 1)) == 0; }

extern "C" int bdn_score_hist(const float* x, int x_is_logits, const uint8_t* labels, int ignore_label, int pos_class, int n_img, int ncls,
                              long long HW, int n_bins, unsigned long long* hist, float* scores_out, void* stream) {
    if (!x || !labels || !hist) BDN_FAIL(BDN_E_ARG, "score_hist: null pointer");
    if ((uintptr_t)x % 4 || (uintptr_t)hist % 8 || (uintptr_t)scores_out % 4) BDN_FAIL(BDN_E_ARG, "score_hist: x / scores_out must be 4-byte, hist 8-byte aligned");
    if (x_is_logits != 0 && x_is_logits != 1) BDN_FAIL(BDN_E_ARG, "score_hist: x_is_logits must be 0 or 1, got %d", x_is_logits);
    if (ignore_label < -1 || ignore_label > 255) BDN_FAIL(BDN_E_ARG, "score_hist: ignore_label must be -1 (none) or a label byte 0..255, got %d", ignore_label);
    if (!pow2_bins(n_bins)) BDN_FAIL(BDN_E_ARG, "score_hist: n_bins must be a power of two in 2..%d, got %d", SH_MAX_BINS, n_bins);
    if (n_img <= 0 || ncls < 2 || ncls > 256 || HW <= 0) BDN_FAIL(BDN_E_SHAPE, "score_hist: need n_img > 0, 2 <= ncls <= 256, HW > 0");
    if (pos_class < 0 || pos_class >= ncls) BDN_FAIL(BDN_E_ARG, "score_hist: pos_class must be in 0..%d, got %d", ncls - 1, pos_class);
    if (HW > SH_MAX_PIXELS / n_img) BDN_FAIL(BDN_E_SHAPE, "score_hist: more than 2^40 pixels");
    const bool vec = HW % 4 == 0 && (uintptr_t)x % 16 == 0 && (uintptr_t)labels % 4 == 0 && (uintptr_t)scores_out % 16 == 0;
    ScoreHistArgs a;
    a.x = x; a.labels = labels; a.hist = hist; a.scores_out = scores_out;
    a.HW = HW; a.Q = vec ? HW / 4 : HW; a.total = a.Q * n_img;
    a.is_logits = x_is_logits; a.ignore = ignore_label; a.pos = pos_class; a.ncls = ncls; a.n_bins = n_bins;
    const long long want = (a.total + SH_THREADS * SH_MIN_ITEMS - 1) / (SH_THREADS * SH_MIN_ITEMS);
    const unsigned blocks = (unsigned)(want < SH_MAX_BLOCKS ? want : SH_MAX_BLOCKS);
    const long long stride = (long long)blocks * SH_THREADS;
    a.stride_img = stride / a.Q; a.stride_off = stride % a.Q;
    const size_t lds = 2 * (size_t)n_bins * sizeof(unsigned);
    hipStream_t st = (hipStream_t)stream;
    const bool two = ncls == 2 && x_is_logits;
    if (vec && two) hipLaunchKernelGGL((score_hist_kernel<2, 4>), dim3(blocks), dim3(SH_THREADS), lds, st, a);
    else if (vec) hipLaunchKernelGGL((score_hist_kernel<0, 4>), dim3(blocks), dim3(SH_THREADS), lds, st, a);
    else if (two) hipLaunchKernelGGL((score_hist_kernel<2, 1>), dim3(blocks), dim3(SH_THREADS), lds, st, a);
    else hipLaunchKernelGGL((score_hist_kernel<0, 1>), dim3(blocks), dim3(SH_THREADS), lds, st, a);
    BDN_CHECK_LAUNCH("score_hist");
    return BDN_OK;
}

// ============================================================ score_curve
// One block.  Thread t owns the `per` consecutive bins [t per, (t + 1) per) (per = n_bins / 256, or one bin each for fewer bins): it sums
// its bins, reads the other threads' sums from LDS to get the suffix sums behind its chunk (64-bit integers: exact, any order), then walks
// its chunk from the top bin down.  Every ratio is one double division of two integers below 2^53.  The average precision is summed in
// descending bin order inside a chunk and the chunk partials in descending chunk order by thread 0: a fixed order.
constexpr int SC_THREADS = 256;
__device__ __forceinline__ double ratio(unsigned long long num, unsigned long long den) { return den ? (double)num / (double)den : 0.0; }

__global__ __launch_bounds__(SC_THREADS) void score_curve_kernel(const unsigned long long* __restrict__ hist, int n_bins,
                                                                 double* __restrict__ curve, double* __restrict__ summary) {
    __shared__ unsigned long long tot[2][SC_THREADS];
    __shared__ double ap_part[SC_THREADS], f_best[SC_THREADS];
    __shared__ int i_best[SC_THREADS];
    const int t = threadIdx.x;
    const int per = n_bins >= SC_THREADS ? n_bins / SC_THREADS : 1, active = n_bins / per;
    const int b0 = t * per;
    unsigned long long sneg = 0, spos = 0;
    if (t < active)
        for (int b = b0; b < b0 + per; b++) { sneg += hist[b]; spos += hist[n_bins + b]; }
    tot[0][t] = sneg; tot[1][t] = spos;
    __syncthreads();
    unsigned long long fp = 0, tp = 0, n_neg = 0, n_pos = 0;      // fp, tp: the counts of the bins behind this thread's chunk
    for (int k = 0; k < active; k++) {
        n_neg += tot[0][k]; n_pos += tot[1][k];
        if (k > t) { fp += tot[0][k]; tp += tot[1][k]; }
    }
    double ap = 0.0, fb = -1.0;
    int ib = 0;
    if (t < active) {
        double r_next = ratio(tp, n_pos);                         // R_{i+1} of the chunk's top bin (R_{n_bins} = 0)
        for (int b = b0 + per - 1; b >= b0; b--) {
            fp += hist[b]; tp += hist[n_bins + b];
            const double P = ratio(tp, tp + fp), R = ratio(tp, n_pos), F = ratio(2 * tp, 2 * tp + fp + (n_pos - tp));
            ap += (R - r_next) * P;
            r_next = R;
            if (F >= fb) { fb = F; ib = b; }                      // descending walk: >= leaves the lowest bin of a tie
            if (curve) {
                curve[b] = (double)tp; curve[n_bins + b] = (double)fp;
                curve[2 * n_bins + b] = P; curve[3 * n_bins + b] = R;
            }
        }
    }
    ap_part[t] = ap; f_best[t] = fb; i_best[t] = ib;
    __syncthreads();
    if (t == 0) {
        double AP = 0.0, F = -1.0;
        int I = 0;
        for (int k = active - 1; k >= 0; k--) AP += ap_part[k];
        for (int k = 0; k < active; k++)
            if (f_best[k] > F) { F = f_best[k]; I = i_best[k]; }  // ascending chunks, strict: the first maximum
        unsigned long long TP = 0, FP = 0;                        // the counts at the best threshold, again as integers
        for (int b = I; b < n_bins; b++) { FP += hist[b]; TP += hist[n_bins + b]; }
        summary[0] = F; summary[1] = (double)I / (double)n_bins; summary[2] = (double)I;
        summary[3] = ratio(TP, TP + FP); summary[4] = ratio(TP, n_pos); summary[5] = AP;
        summary[6] = (double)n_pos; summary[7] = (double)n_neg;
    }
}

extern "C" int bdn_score_curve(const unsigned long long* hist, int n_bins, double* curve_out, double* summary, void* stream) {
    if (!hist || !summary) BDN_FAIL(BDN_E_ARG, "score_curve: null pointer");
    if ((uintptr_t)hist % 8 || (uintptr_t)curve_out % 8 || (uintptr_t)summary % 8) BDN_FAIL(BDN_E_ARG, "score_curve: buffers must be 8-byte aligned");
    if (!pow2_bins(n_bins)) BDN_FAIL(BDN_E_ARG, "score_curve: n_bins must be a power of two in 2..%d, got %d", SH_MAX_BINS, n_bins);
    hipLaunchKernelGGL(score_curve_kernel, dim3(1), dim3(SC_THREADS), 0, (hipStream_t)stream, hist, n_bins, curve_out, summary);
    BDN_CHECK_LAUNCH("score_curve");
    return BDN_OK;
}

// ============================================================ threshold_mask
// mask[i] = proba[pos_class][i] >= threshold (a NaN probability gives 0).  Four pixels per thread (one 16-byte load, one 4-byte store) where
// HW and the pointers allow, one otherwise; capped grid, grid-strided.
template <int PER>
__global__ __launch_bounds__(256) void threshold_mask_kernel(const float* __restrict__ p, float thr, uint8_t* __restrict__ mask, long long n_items) {
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n_items; i += stride) {
        if constexpr (PER == 4) {
            const float4 v = reinterpret_cast<const float4*>(p)[i];
            reinterpret_cast<uint32_t*>(mask)[i] = (uint32_t)(v.x >= thr) | (uint32_t)(v.y >= thr) << 8 | (uint32_t)(v.z >= thr) << 16 | (uint32_t)(v.w >= thr) << 24;
        } else {
            mask[i] = p[i] >= thr;
        }
    }
}

extern "C" int bdn_threshold_mask(const float* proba, int pos_class, float threshold, uint8_t* mask, int ncls, long long HW, void* stream) {
    if (!proba || !mask) BDN_FAIL(BDN_E_ARG, "threshold_mask: null pointer");
    if ((uintptr_t)proba % 4) BDN_FAIL(BDN_E_ARG, "threshold_mask: proba must be 4-byte aligned");
    if (!(threshold >= 0.f && threshold <= 1.f)) BDN_FAIL(BDN_E_ARG, "threshold_mask: threshold must be in [0, 1], got %g", (double)threshold);
    if (ncls < 2 || ncls > 256 || HW <= 0 || HW > SH_MAX_PIXELS) BDN_FAIL(BDN_E_SHAPE, "threshold_mask: need 2 <= ncls <= 256, 0 < HW <= 2^40");
    if (pos_class < 0 || pos_class >= ncls) BDN_FAIL(BDN_E_ARG, "threshold_mask: pos_class must be in 0..%d, got %d", ncls - 1, pos_class);
    const float* p = proba + (size_t)pos_class * HW;
    const bool vec = HW % 4 == 0 && (uintptr_t)p % 16 == 0 && (uintptr_t)mask % 4 == 0;
    const long long n_items = vec ? HW / 4 : HW, want = (n_items + 255) / 256;
    const unsigned blocks = (unsigned)(want < 2048 ? want : 2048);
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(threshold_mask_kernel<4>, dim3(blocks), dim3(256), 0, st, p, threshold, mask, n_items);
    else hipLaunchKernelGGL(threshold_mask_kernel<1>, dim3(blocks), dim3(256), 0, st, p, threshold, mask, n_items);
    BDN_CHECK_LAUNCH("threshold_mask");
    return BDN_OK;
}
