// Boundary kernels: NCHW<->NHWC / weight packing, the 1x1 classifier, the Tversky loss and the SGD
// update.  All activations NHWC, 16-byte vector access
// along channels; per-channel reductions go through per-block partials (deterministic, no atomics).
#include "common.hpp"

static inline unsigned grid_for(size_t n, int block = 256) { return (unsigned)((n + block - 1) / block); }

// ============================================================ pack_input
// reference boundary: BiDateNet.forward(x_d1, x_d2), models/bidate_model.py:22 (NCHW f32)
// One thread per (pixel, 16-byte output unit): the band planes are read coalesced along x, every store is 16 bytes
// (the first version wrote Cpad scalars per thread: 100 us for 176 MB).
template <typename T>
__global__ void pack_input_kernel(const float* __restrict__ x1, const float* __restrict__ x2, T* __restrict__ out,
                                  int B, int C, int H, int W, int Cpad, FastDiv dhw, FastDiv dupp) {
    constexpr int EPU = ET<T>::EPU;
    const int upp = Cpad / EPU;
    const size_t hw = (size_t)H * W, total = (size_t)2 * B * hw * upp;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    // the unit index is the slow coordinate inside an image so that a wave reads 64 consecutive pixels of one plane set
    int ti, pi, n, u; dhw.divmod((int)i, ti, pi); dupp.divmod(ti, n, u);        // (total < 2^31: the entry point keeps the tensor below 4 GB)
    const size_t p = pi;
    const float* src = (n < B ? x1 + (size_t)n * C * hw : x2 + (size_t)(n - B) * C * hw) + p;
    float f[EPU];
#pragma unroll
    for (int e = 0; e < EPU; e++) { const int c = u * EPU + e; f[e] = c < C ? src[(size_t)c * hw] : 0.f; }
    *reinterpret_cast<uint4*>(out + ((size_t)n * hw + p) * Cpad + u * EPU) = Unit<T>::pack(f);
}

// bf16x3: the packed input leaves directly as the [hi | lo] bf16 operand of the first convolution ([2B,H,W,2 Cpad]: bdn_split_pack's layout)
__global__ void pack_input_split_kernel(const float* __restrict__ x1, const float* __restrict__ x2, bf16s* __restrict__ out,
                                        int B, int C, int H, int W, int Cpad, FastDiv dhw, FastDiv dupp) {
    // eight channels per thread: the hi and the lo unit leave as one 16-byte store each (four channels per thread wrote 8 bytes at a 64-byte
    // stride: 88.7 us for 243 MB at B = 64)
    const int upp = Cpad / 8;
    const size_t hw = (size_t)H * W, total = (size_t)2 * B * hw * upp;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int ti, pi, n, u; dhw.divmod((int)i, ti, pi); dupp.divmod(ti, n, u);
    const size_t p = pi;
    const float* src = (n < B ? x1 + (size_t)n * C * hw : x2 + (size_t)(n - B) * C * hw) + p;
    float f[8], h[8], r[8];
#pragma unroll
    for (int e = 0; e < 8; e++) { const int c = u * 8 + e; f[e] = c < C ? src[(size_t)c * hw] : 0.f; }
    const uint4 hi = Unit<bf16s>::pack(f);                     // bdn_split_pack's arithmetic: hi = bf16(x), lo = bf16(x - hi)
    Unit<bf16s>::unpack(hi, h);
#pragma unroll
    for (int e = 0; e < 8; e++) r[e] = f[e] - h[e];
    bf16s* dst = out + ((size_t)n * hw + p) * 2 * Cpad + u * 8;
    *reinterpret_cast<uint4*>(dst) = hi;
    *reinterpret_cast<uint4*>(dst + Cpad) = Unit<bf16s>::pack(r);
}

extern "C" int bdn_pack_input(int dtype, const float* x_d1, const float* x_d2, void* out,
                              int B, int C, int H, int W, int Cpad, void* stream) {
    if (!x_d1 || !x_d2 || !out) BDN_FAIL(BDN_E_ARG, "pack_input: null pointer");
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || Cpad < C || Cpad % 16) BDN_FAIL(BDN_E_SHAPE, "pack_input: bad shape");
    hipStream_t st = (hipStream_t)stream;
    const size_t npix = (size_t)2 * B * H * W;
    if (npix * (Cpad / 4) >= ((size_t)1 << 31)) BDN_FAIL(BDN_E_SHAPE, "pack_input: 2*B*H*W*Cpad/4 = %zu reaches 2^31; split the batch", npix * (Cpad / 4));
    if (dtype == BDN_BF16) hipLaunchKernelGGL(pack_input_kernel<bf16s>, dim3(grid_for(npix * (Cpad / 8))), dim3(256), 0, st, x_d1, x_d2, (bf16s*)out, B, C, H, W, Cpad, FastDiv(H * W), FastDiv(Cpad / 8));
    else if (dtype == BDN_F32) hipLaunchKernelGGL(pack_input_kernel<float>, dim3(grid_for(npix * (Cpad / 4))), dim3(256), 0, st, x_d1, x_d2, (float*)out, B, C, H, W, Cpad, FastDiv(H * W), FastDiv(Cpad / 4));
    else if (dtype == BDN_BF16X3) hipLaunchKernelGGL(pack_input_split_kernel, dim3(grid_for(npix * (Cpad / 8))), dim3(256), 0, st, x_d1, x_d2, (bf16s*)out, B, C, H, W, Cpad, FastDiv(H * W), FastDiv(Cpad / 8));
    else BDN_FAIL(BDN_E_ARG, "pack_input: bad dtype");
    BDN_CHECK_LAUNCH("pack_input");
    return BDN_OK;
}

// ============================================================ pack_weights
// forward image:        W_f(co, tap, ci) = w[co][ci][r][c]               (tap = 3r+c)
// data-gradient image:  W_d(ci, tap, co) = w[co][ci][2-r][2-c]  i.e. the transposed filter with taps rotated 180 deg
// both stored in MFMA fragment order (common.hpp: wfrag_index); Cout and Cin_pad are multiples of 32 / 16.
template <typename T>
__global__ void pack_weights_kernel(const float* __restrict__ w, T* __restrict__ wf, T* __restrict__ wd,
                                    int Cout, int Cin, int Cinp) {
    const size_t total = (size_t)Cout * 9 * Cinp;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ci = i % Cinp; const size_t t = i / Cinp; const int tap = t % 9; const int co = t / 9;
    const float v = ci < Cin ? w[((size_t)co * Cin + ci) * 9 + tap] : 0.f;
    if (wf) wf[wfrag_index<T>(co, tap, ci, Cinp)] = from_f<T>(v);
    if (wd) wd[wfrag_index<T>(ci, 8 - tap, co, Cout)] = from_f<T>(v);
}

extern "C" int bdn_pack_weights(int dtype, const float* w_oihw, void* wf, void* wd,
                                int Cout, int Cin, int Cin_pad, void* stream) {
    if (!w_oihw || (!wf && !wd)) BDN_FAIL(BDN_E_ARG, "pack_weights: null pointer");
    if (Cout <= 0 || Cin <= 0 || Cin_pad < Cin || Cout % 32 || Cin_pad % 16 || (wd && Cin_pad % 32))
        BDN_FAIL(BDN_E_SHAPE, "pack_weights: Cout must be a multiple of 32, Cin_pad of 16 (32 with a data-gradient image)");
    hipStream_t st = (hipStream_t)stream;
    const size_t total = (size_t)Cout * 9 * Cin_pad;
    if (dtype == BDN_BF16X3) return bdn_pack_weights_x3(w_oihw, wf, wd, Cout, Cin, Cin_pad, st);   // images of 3x the reduction length (x3.hip)
    if (dtype == BDN_BF16) hipLaunchKernelGGL(pack_weights_kernel<bf16s>, dim3(grid_for(total)), dim3(256), 0, st, w_oihw, (bf16s*)wf, (bf16s*)wd, Cout, Cin, Cin_pad);
    else if (dtype == BDN_F32) hipLaunchKernelGGL(pack_weights_kernel<float>, dim3(grid_for(total)), dim3(256), 0, st, w_oihw, (float*)wf, (float*)wd, Cout, Cin, Cin_pad);
    else BDN_FAIL(BDN_E_ARG, "pack_weights: bad dtype");
    BDN_CHECK_LAUNCH("pack_weights");
    return BDN_OK;
}

// all layers in one launch: desc[l] = {w, wf, wd, Cout, Cin, Cin_pad}; grid.y = layer
// one thread per OUTPUT element (coalesced 2/4-byte writes in fragment order; the strided reads of the
// 54 MB fp32 master hit L2)
template <typename T>
__global__ void pack_weights_multi_kernel(const PackDesc* __restrict__ desc) {
    constexpr int EPU = 16 / (int)sizeof(T), KCH = 32 / (int)sizeof(T), REC = 64 * EPU;
    const PackDesc d = desc[blockIdx.y];
    const size_t total = (size_t)d.Cout * 9 * d.Cinp;
    T* wf = reinterpret_cast<T*>(d.wf); T* wd = reinterpret_cast<T*>(d.wd);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e = i % EPU, lane = (i / EPU) % 64; const size_t rec = i / REC;
        if (wf) {       // rec = (cb*9 + tap)*(Cinp/KCH) + kgi
            const int kgi = rec % (d.Cinp / KCH); const size_t t = rec / (d.Cinp / KCH); const int tap = t % 9, cb = t / 9;
            const int co = cb * 32 + (lane & 31), ci = kgi * KCH + (lane >> 5) * EPU + e;
            wf[i] = from_f<T>(ci < d.Cin ? d.w[((size_t)co * d.Cin + ci) * 9 + tap] : 0.f);
        }
        if (wd) {       // roles swapped: "cout" = ci (padded), "cin" = co; taps rotated by 180 degrees
            const int kgi = rec % (d.Cout / KCH); const size_t t = rec / (d.Cout / KCH); const int tap = t % 9, cb = t / 9;
            const int ci = cb * 32 + (lane & 31), co = kgi * KCH + (lane >> 5) * EPU + e;
            wd[i] = from_f<T>(ci < d.Cin ? d.w[((size_t)co * d.Cin + ci) * 9 + (8 - tap)] : 0.f);
        }
    }
}

// Regular layers (bf16, Cin a multiple of 64 and unpadded, Cout of 32 -- 17 of BiDateNet's 18) go through LDS instead: a block
// takes 32 output channels x 64 input channels x 9 taps, reads them as 32 contiguous 2304-byte rows of the OIHW master
// (16-byte loads), and writes complete 1 KB fragment records of both images with 16-byte stores.  The element-wise kernel
// above gathers 4-byte values 36 bytes apart and stores 2 bytes per lane: 61 us for the 107 MB of the step, and that
// sits alone at the start of every step.
__device__ __forceinline__ bool pack_regular(const PackDesc& d) { return d.Cin == d.Cinp && d.Cin % 64 == 0 && d.Cout % 32 == 0; }
__global__ __launch_bounds__(256) void pack_weights_tiles_kernel(const PackDesc* __restrict__ desc, int n_layers) {
    constexpr int ROW = 9 * 64 + 8;                            // LDS elements per output channel: [tap][ci] + 16 bytes of padding
    __shared__ __attribute__((aligned(16))) bf16s t[32 * ROW];
    const int tid = threadIdx.x;
    for (int item = blockIdx.x;; item += gridDim.x) {
        // which (layer, 32-co block, 64-ci block) is this item?
        int l = 0, local = item;
        for (; l < n_layers; l++) {
            const int cnt = pack_regular(desc[l]) ? (desc[l].Cout / 32) * (desc[l].Cin / 64) : 0;
            if (local < cnt) break;
            local -= cnt;
        }
        if (l == n_layers) return;                             // uniform for the block
        const PackDesc d = desc[l];
        const int ncc = d.Cin / 64, cb = local / ncc, cc = local % ncc, co0 = cb * 32, ci0 = cc * 64;
        __syncthreads();                                       // the previous item's LDS reads are done
        for (int q = tid; q < 32 * 144; q += 256) {            // 144 float4 per output-channel row
            const int r = q / 144, o4 = (q % 144) * 4;
            const float4 v = *reinterpret_cast<const float4*>(d.w + ((size_t)(co0 + r) * d.Cin + ci0) * 9 + o4);
            const float f[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int o = o4 + e, ci = o / 9, tap = o % 9;
                t[r * ROW + tap * 64 + ci] = from_f<bf16s>(f[e]);
            }
        }
        __syncthreads();
        bf16s* wf = reinterpret_cast<bf16s*>(d.wf); bf16s* wd = reinterpret_cast<bf16s*>(d.wd);
        for (int u = tid; u < 36 * 64; u += 256) {             // 36 records x 64 lanes, 16 bytes each
            const int rec_l = u >> 6, lane = u & 63;
            if (wf) {      // record (tap, kq): lane = co & 31 + 32 * (ci % 16) / 8, 8 consecutive ci
                const int tap = rec_l >> 2, kq = rec_l & 3;
                const size_t rec = ((size_t)cb * 9 + tap) * (d.Cin / 16) + (ci0 / 16 + kq);
                *reinterpret_cast<uint4*>(wf + rec * 512 + lane * 8) =
                    *reinterpret_cast<const uint4*>(t + (lane & 31) * ROW + tap * 64 + kq * 16 + (lane >> 5) * 8);
            }
            if (wd) {      // roles swapped, taps rotated: record (ci block, 8 - tap, co group of 16): 8 consecutive co
                const int cbi = rec_l / 18, rem = rec_l % 18, tap = rem >> 1, kg = rem & 1;
                const int ci = cbi * 32 + (lane & 31), co8 = kg * 16 + (lane >> 5) * 8;
                unsigned short h[8];
#pragma unroll
                for (int e = 0; e < 8; e++) h[e] = t[(co8 + e) * ROW + tap * 64 + ci];
                const size_t rec = ((size_t)(ci0 / 32 + cbi) * 9 + (8 - tap)) * (d.Cout / 16) + (co0 / 16 + kg);
                *reinterpret_cast<uint4*>(wd + rec * 512 + lane * 8) =
                    make_uint4(h[0] | ((unsigned)h[1] << 16), h[2] | ((unsigned)h[3] << 16), h[4] | ((unsigned)h[5] << 16), h[6] | ((unsigned)h[7] << 16));
            }
        }
    }
}
// the element-wise kernel restricted to the layers the tile kernel does not take
__global__ void pack_weights_irregular_kernel(const PackDesc* __restrict__ desc) {
    if (pack_regular(desc[blockIdx.y])) return;
    constexpr int EPU = 8, KCH = 16, REC = 64 * EPU;
    const PackDesc d = desc[blockIdx.y];
    const size_t total = (size_t)d.Cout * 9 * d.Cinp;
    bf16s* wf = reinterpret_cast<bf16s*>(d.wf); bf16s* wd = reinterpret_cast<bf16s*>(d.wd);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int e = i % EPU, lane = (i / EPU) % 64; const size_t rec = i / REC;
        if (wf) {
            const int kgi = rec % (d.Cinp / KCH); const size_t t = rec / (d.Cinp / KCH); const int tap = t % 9, cb = t / 9;
            const int co = cb * 32 + (lane & 31), ci = kgi * KCH + (lane >> 5) * EPU + e;
            wf[i] = from_f<bf16s>(ci < d.Cin ? d.w[((size_t)co * d.Cin + ci) * 9 + tap] : 0.f);
        }
        if (wd) {
            const int kgi = rec % (d.Cout / KCH); const size_t t = rec / (d.Cout / KCH); const int tap = t % 9, cb = t / 9;
            const int ci = cb * 32 + (lane & 31), co = kgi * KCH + (lane >> 5) * EPU + e;
            wd[i] = from_f<bf16s>(ci < d.Cin ? d.w[((size_t)co * d.Cin + ci) * 9 + (8 - tap)] : 0.f);
        }
    }
}

extern "C" int bdn_pack_weights_multi(int dtype, const void* desc, int n_layers, void* stream) {
    if (!desc || n_layers <= 0) BDN_FAIL(BDN_E_ARG, "pack_weights_multi: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BDN_BF16) {
        hipLaunchKernelGGL(pack_weights_tiles_kernel, dim3(1024), dim3(256), 0, st, (const PackDesc*)desc, n_layers);
        hipLaunchKernelGGL(pack_weights_irregular_kernel, dim3(32, n_layers), dim3(256), 0, st, (const PackDesc*)desc);
    }
    else if (dtype == BDN_F32) hipLaunchKernelGGL(pack_weights_multi_kernel<float>, dim3(256, n_layers), dim3(256), 0, st, (const PackDesc*)desc);
    else if (dtype == BDN_BF16X3) return bdn_pack_weights_x3_multi((const PackDesc*)desc, n_layers, st);      // images of 3x the reduction length (x3.hip)
    else BDN_FAIL(BDN_E_ARG, "pack_weights_multi: bad dtype");
    BDN_CHECK_LAUNCH("pack_weights_multi");
    return BDN_OK;
}

// ============================================================ outconv 1x1 (unet_parts.py:86)
constexpr int OUTC_MAXCLS = 8;
constexpr int OUTC_ITERS = 16;      // pixels per thread in the classifier forward
constexpr int OUTC_BWD_ITERS = 32;  // ... and backward: every block ends with 130 same-address global atomics, which
                                    // serialise per address, so fewer, fatter blocks (2048 -> 1024 at full resolution: 117 -> 88 us)
// NC = compile-time class-count bound (2 for the change / no-change head, 8 generic): loops over classes unroll
// without runtime predicates.  CU = C/EPU consecutive lanes share one pixel (each reads 16 contiguous bytes ->
// fully coalesced), partial dot products are combined with xor-shuffles inside the CU-lane group.
// CUC: the lanes per pixel as a compile-time constant (8 or 16: the 64-channel head in bf16 / float32), 0 = run-time.  With it the
// partial dot products of a pixel meet in its first lane by DPP row shifts (same association as the xor butterfly: 4, 2, 1 -- the
// same bits) instead of ds_bpermute round trips in a run-time loop, and the next four pixels of a lane are requested before the
// current four are reduced (round 5: 42 -> 3x us at B = 64).
// (dpp_row_shl / first_lane_sum: common.hpp -- the eval-mode convolution epilogue sums a pixel's classifier terms the same way)
template <typename T, int NC, int CUC = 0>
__global__ __launch_bounds__(256) void outc_fwd_kernel(const T* __restrict__ z, const float* __restrict__ bn, const float* __restrict__ w,
                                const float* __restrict__ bias, float* __restrict__ logits, int npix, int hw, int C, int ncls, FastDiv dhw) {
    constexpr int EPU = ET<T>::EPU;
    const int CU = CUC ? CUC : C / EPU, rows = 256 / CU, tid = threadIdx.x, cu = tid % CU, row = tid / CU, c = cu * EPU;
    float sc[EPU], sh[EPU], wk[NC][EPU], bk[NC];
#pragma unroll
    for (int i = 0; i < EPU; i++) { sc[i] = bn_row(bn, 0, 2, C)[c + i]; sh[i] = bn_row(bn, 0, 3, C)[c + i]; }
#pragma unroll
    for (int k = 0; k < NC; k++) {
        const int kk = k < ncls ? k : 0;                                           // unconditional loads, selected afterwards
        const float bv = bias[kk];
        bk[k] = k < ncls ? bv : 0.f;
#pragma unroll
        for (int i = 0; i < EPU; i++) { const float wv = w[kk * C + c + i]; wk[k][i] = k < ncls ? wv : 0.f; }
    }
    const int p_begin = blockIdx.x * rows * OUTC_ITERS, p_end = min(npix, p_begin + rows * OUTC_ITERS);
    // four pixels of a lane are requested before the first is used (with one 16-byte load in flight per lane the pass ran at 3.6 TB/s),
    // and the following four before these are reduced.  RAGGED_ = false: the block's whole range lies inside the tensor (every block
    // but possibly the last) -- no per-pixel bounds tests
    uint4 u[4], un[4];
#define OUTC_LOAD4(dst_, p0_, RAGGED_)                                                                   \
    _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                      \
        const int p_ = (p0_) + j * rows + row;                                                          \
        dst_[j] = *reinterpret_cast<const uint4*>(z + (size_t)(!(RAGGED_) || p_ < p_end ? p_ : (p0_)) * C + c); \
    }
#define OUTC_RUN(RAGGED_)                                                                                \
    {                                                                                                   \
        OUTC_LOAD4(u, p_begin, RAGGED_)                                                                 \
        for (int p0 = p_begin; p0 < p_end; p0 += 4 * rows) {                      /* block-uniform trip count */ \
            const bool more = p0 + 4 * rows < p_end;                                                    \
            /* unconditional (the last trip re-requests its own pixels): a branch here makes the compiler wait for ALL loads, */ \
            /* the new ones included, before the first use of the current four */                        \
            { const int pn_ = more ? p0 + 4 * rows : p0; OUTC_LOAD4(un, pn_, RAGGED_) }                  \
            _Pragma("unroll") for (int j = 0; j < 4; j++) {                                              \
                const int p = p0 + j * rows + row;                                                      \
                if ((RAGGED_) && p0 + j * rows >= p_end) break;                   /* block-uniform */   \
                const bool in_ = !(RAGGED_) || p < p_end;                                               \
                float f[EPU], acc[NC];                                                                  \
                _Pragma("unroll") for (int k = 0; k < NC; k++) acc[k] = 0.f;                             \
                Unit<T>::unpack(u[j], f);                                                               \
                _Pragma("unroll") for (int i = 0; i < EPU; i++) {                                        \
                    const float a = to_f(from_f<T>(fmaxf(fmaf(f[i], sc[i], sh[i]), 0.f)));              \
                    _Pragma("unroll") for (int k = 0; k < NC; k++) acc[k] = fmaf(a, wk[k][i], acc[k]);   \
                }                                                                                       \
                if constexpr (CUC != 0) {                                                               \
                    _Pragma("unroll") for (int k = 0; k < NC; k++) acc[k] = first_lane_sum<CUC ? CUC : 8>(acc[k]); \
                } else {                                                                                \
                    _Pragma("unroll") for (int k = 0; k < NC; k++)                                       \
                        for (int off = CU >> 1; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off);  \
                }                                                                                       \
                if (cu == 0 && in_) {                                                                   \
                    int b, q; dhw.divmod(p, b, q);                                                      \
                    _Pragma("unroll") for (int k = 0; k < NC; k++) if (k < ncls) logits[((size_t)b * ncls + k) * hw + q] = acc[k] + bk[k]; \
                }                                                                                       \
            }                                                                                           \
            _Pragma("unroll") for (int j = 0; j < 4; j++) u[j] = un[j];                                  \
        }                                                                                               \
    }
    if (p_begin >= p_end) return;
    if (p_begin + rows * OUTC_ITERS <= npix) OUTC_RUN(false) else OUTC_RUN(true)
#undef OUTC_RUN
#undef OUTC_LOAD4
}

extern "C" int bdn_outc_fwd(int dtype, const void* z, const float* bn, const float* w, const float* b,
                            float* logits, int B, int H, int W, int C, int ncls, void* stream) {
    if (!z || !bn || !w || !b || !logits) BDN_FAIL(BDN_E_ARG, "outc_fwd: null pointer");
    if (ncls < 1 || ncls > OUTC_MAXCLS || C % 16 || C > 512 || 512 % C) BDN_FAIL(BDN_E_SHAPE, "outc_fwd: ncls=%d (max %d), C=%d", ncls, OUTC_MAXCLS, C);
    hipStream_t st = (hipStream_t)stream; const int npix = B * H * W, hw = H * W;
    if (dtype == BDN_BF16) {
        const int per = 256 / (C / 8) * OUTC_ITERS; const unsigned grid = (npix + per - 1) / per;
        if (ncls <= 2 && C == 64) hipLaunchKernelGGL((outc_fwd_kernel<bf16s, 2, 8>), dim3(grid), dim3(256), 0, st, (const bf16s*)z, bn, w, b, logits, npix, hw, C, ncls, FastDiv(hw));
        else if (ncls <= 2) hipLaunchKernelGGL((outc_fwd_kernel<bf16s, 2>), dim3(grid), dim3(256), 0, st, (const bf16s*)z, bn, w, b, logits, npix, hw, C, ncls, FastDiv(hw));
        else hipLaunchKernelGGL((outc_fwd_kernel<bf16s, OUTC_MAXCLS>), dim3(grid), dim3(256), 0, st, (const bf16s*)z, bn, w, b, logits, npix, hw, C, ncls, FastDiv(hw));
    } else if (dtype == BDN_F32) {
        const int per = 256 / (C / 4) * OUTC_ITERS; const unsigned grid = (npix + per - 1) / per;
        if (ncls <= 2 && C == 64) hipLaunchKernelGGL((outc_fwd_kernel<float, 2, 16>), dim3(grid), dim3(256), 0, st, (const float*)z, bn, w, b, logits, npix, hw, C, ncls, FastDiv(hw));
        else if (ncls <= 2) hipLaunchKernelGGL((outc_fwd_kernel<float, 2>), dim3(grid), dim3(256), 0, st, (const float*)z, bn, w, b, logits, npix, hw, C, ncls, FastDiv(hw));
        else hipLaunchKernelGGL((outc_fwd_kernel<float, OUTC_MAXCLS>), dim3(grid), dim3(256), 0, st, (const float*)z, bn, w, b, logits, npix, hw, C, ncls, FastDiv(hw));
    }
    else BDN_FAIL(BDN_E_ARG, "outc_fwd: bad dtype");
    BDN_CHECK_LAUNCH("outc_fwd");
    return BDN_OK;
}

// backward: dA[p][c] = sum_k dl[k][p] w[k][c];  dw[k][c] = sum_p dl[k][p] a[p][c];  db[k] = sum_p dl[k][p]
// Thread t owns channel unit t % CU (its filter taps, BN constants and dw accumulators live in registers)
// and walks pixels t / CU, +rows, ...; the block partials of dw/db go to a workspace and are summed in a fixed order by
// outc_dw_reduce_kernel (the first version added them with float atomics: the only non-deterministic bits of a step).
template <typename T, int NC, int CUC = 0>          // CUC: lanes per pixel at compile time (see outc_fwd_kernel), 0 = run-time
__global__ __launch_bounds__(256) void outc_bwd_kernel(const float* __restrict__ dl, const T* __restrict__ z, const float* __restrict__ bn,
                                const float* __restrict__ w, T* __restrict__ dA, float* __restrict__ wpart,
                                float* __restrict__ bs_partial, int npix, int hw, int C, int ncls, FastDiv dhw) {
    constexpr int EPU = ET<T>::EPU;
    extern __shared__ float sm[];                             // [ncls][C+1] block sums + [256][EPU][2] reduction scratch
    const int CU = CUC ? CUC : C / EPU, rows = 256 / CU, tid = threadIdx.x, cu = tid % CU, row = tid / CU, c = cu * EPU;
    for (int i = tid; i < ncls * (C + 1); i += 256) sm[i] = 0.f;
    float sc[EPU], sh[EPU], wk[NC][EPU], acc[NC][EPU], accb[NC], t0[EPU], t1[EPU];
#pragma unroll
    for (int i = 0; i < EPU; i++) { sc[i] = bn_row(bn, 0, 2, C)[c + i]; sh[i] = bn_row(bn, 0, 3, C)[c + i]; t0[i] = 0.f; t1[i] = 0.f; }
    const bool bs = bs_partial != nullptr;
#pragma unroll
    for (int k = 0; k < NC; k++) {
        accb[k] = 0.f;
        const int kk = k < ncls ? k : 0;
#pragma unroll
        for (int i = 0; i < EPU; i++) { const float wv = w[kk * C + c + i]; wk[k][i] = k < ncls ? wv : 0.f; acc[k][i] = 0.f; }
    }
    __syncthreads();
    const int p_begin = blockIdx.x * rows * OUTC_BWD_ITERS, p_end = min(npix, p_begin + rows * OUTC_BWD_ITERS);
    // four pixels of a lane are requested before the first is used, and the following four before these are consumed (unconditionally:
    // the last trip re-requests its own -- a branch around the requests makes the compiler drain them all before the first use); the
    // pixels are still accumulated one after the other, in order
    uint4 zu[4], zn[4]; float gv[4][NC], gn[4][NC];
#define OUTC_BLOAD4(zd_, gd_, p0_)                                                                       \
    _Pragma("unroll") for (int j = 0; j < 4; j++) {                                                      \
        const int pj_ = (p0_) + j * rows + row < p_end ? (p0_) + j * rows + row : p_begin + row;          \
        int b_, q_; dhw.divmod(pj_, b_, q_);                                                            \
        _Pragma("unroll") for (int k = 0; k < NC; k++) gd_[j][k] = dl[((size_t)b_ * ncls + (k < ncls ? k : 0)) * hw + q_]; \
        zd_[j] = *reinterpret_cast<const uint4*>(z + (size_t)pj_ * C + c);                              \
    }
    if (p_begin + row < p_end) {                              // (a block's first row of pixels is inside the tensor whenever the block has work)
        OUTC_BLOAD4(zu, gv, p_begin)
        for (int p0 = p_begin; p0 < p_end; p0 += 4 * rows) {  // block-uniform trip count
            { const int pn_ = p0 + 4 * rows < p_end ? p0 + 4 * rows : p0; OUTC_BLOAD4(zn, gn, pn_) }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int p = p0 + j * rows + row;
                if (p < p_end) {
                    float g[NC], f[EPU], o[EPU];
#pragma unroll
                    for (int k = 0; k < NC; k++) g[k] = k < ncls ? gv[j][k] : 0.f;
                    Unit<T>::unpack(zu[j], f);
#pragma unroll
                    for (int i = 0; i < EPU; i++) {
                        const float a = to_f(from_f<T>(fmaxf(fmaf(f[i], sc[i], sh[i]), 0.f)));
                        float s = 0.f;
#pragma unroll
                        for (int k = 0; k < NC; k++) if (k < ncls) { s = fmaf(g[k], wk[k][i], s); acc[k][i] = fmaf(g[k], a, acc[k][i]); }
                        o[i] = s;
                    }
                    if (cu == 0) {
#pragma unroll
                        for (int k = 0; k < NC; k++) accb[k] += g[k];
                    }
                    const uint4 uo = Unit<T>::pack(o);
                    if (dA) *reinterpret_cast<uint4*>(dA + (size_t)p * C + c) = uo;
                    if (bs) {                                             // BatchNorm-backward partial sums of this layer on the stored gradient
                        Unit<T>::unpack(uo, o);
#pragma unroll
                        for (int i = 0; i < EPU; i++) {
                            const float gm = fmaf(f[i], sc[i], sh[i]) > 0.f ? o[i] : 0.f;
                            t0[i] += gm; t1[i] = fmaf(gm, f[i], t1[i]);
                        }
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                zu[j] = zn[j];
#pragma unroll
                for (int k = 0; k < NC; k++) gv[j][k] = gn[j][k];
            }
        }
    }
#undef OUTC_BLOAD4
    // block sums of dw / db in a fixed order: per class every thread parks its partials in LDS, then one thread per
    // channel adds the block's `rows` pixel rows in order (LDS atomics would make the last bits depend on wave timing)
    {
        float* red = sm + ncls * (C + 1);                     // [256][EPU] dw partials + [rows] db partials
#pragma unroll
        for (int k = 0; k < NC; k++) {
            if (k < ncls) {
                __syncthreads();
#pragma unroll
                for (int i = 0; i < EPU; i++) red[tid * EPU + i] = acc[k][i];
                if (cu == 0) red[256 * EPU + row] = accb[k];
                __syncthreads();
                for (int o = tid; o <= C; o += 256) {
                    float v = 0.f;
                    if (o < C) { const int ccu = o / EPU, i = o % EPU; for (int r = 0; r < rows; r++) v += red[(r * CU + ccu) * EPU + i]; }
                    else for (int r = 0; r < rows; r++) v += red[256 * EPU + r];
                    sm[k * (C + 1) + o] = v;
                }
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < ncls * (C + 1); i += 256)        // block partial [ncls][C+1]; outc_dw_reduce_kernel sums the blocks in order
        wpart[(size_t)blockIdx.x * ncls * (C + 1) + i] = sm[i];
    if (bs) {                                                 // bs_partial[block][2][C], fixed order
        float* sred = sm + ncls * (C + 1);
#pragma unroll
        for (int i = 0; i < EPU; i++) { sred[(tid * EPU + i) * 2] = t0[i]; sred[(tid * EPU + i) * 2 + 1] = t1[i]; }
        __syncthreads();
        for (int o = tid; o < C * 2; o += 256) {
            const int k = o & 1, cc = o >> 1, ccu = cc / EPU, i = cc % EPU;
            float v = 0.f;
            for (int r = 0; r < rows; r++) v += sred[((r * CU + ccu) * EPU + i) * 2 + k];
            bs_partial[((size_t)blockIdx.x * 2 + k) * C + cc] = v;
        }
    }
}

// dw[k][c] / db[k] = sum over the blocks' partials, fixed order: one block per output value, 256 lanes stride the rows,
// then an LDS tree.
__global__ __launch_bounds__(256) void outc_dw_reduce_kernel(const float* __restrict__ wpart, int rows, int C, int ncls,
                                                             float* __restrict__ dw, float* __restrict__ db) {
    __shared__ float sm[256];
    const int o = blockIdx.x, n = ncls * (C + 1);
    float a = 0.f;
    for (int r = threadIdx.x; r < rows; r += 256) a += wpart[(size_t)r * n + o];
    sm[threadIdx.x] = a;
    __syncthreads();
    for (int st = 128; st >= 1; st >>= 1) {
        if ((int)threadIdx.x < st) sm[threadIdx.x] += sm[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int k = o / (C + 1), cc = o % (C + 1);
        if (cc < C) dw[k * C + cc] = sm[0]; else db[k] = sm[0];
    }
}

extern "C" int bdn_outc_bwd_rows(int dtype, int B, int H, int W, int C) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 16 || C > 1024 || 1024 % C) return 0;
    const int per = 256 / (C / (dtype == BDN_BF16 ? 8 : 4)) * OUTC_BWD_ITERS;
    return (B * H * W + per - 1) / per;
}

extern "C" size_t bdn_outc_bwd_workspace_bytes(int dtype, int B, int H, int W, int C, int ncls) {
    const int rows = bdn_outc_bwd_rows(dtype, B, H, W, C);
    if (rows <= 0 || ncls < 1 || ncls > OUTC_MAXCLS) return 0;
    return (size_t)rows * ncls * (C + 1) * sizeof(float);
}

extern "C" int bdn_outc_bwd(int dtype, const float* dlogits, const void* z, const float* bn, const float* w,
                            void* dA, float* dw, float* db, float* bs_partial, float* ws, int B, int H, int W, int C, int ncls, void* stream) {
    if (!dlogits || !z || !bn || !w || !dw || !db || !ws) BDN_FAIL(BDN_E_ARG, "outc_bwd: null pointer");
    if (!dA && !bs_partial) BDN_FAIL(BDN_E_ARG, "outc_bwd: dA may be omitted only together with bs_partial (bdn_outc_bn_bwd_apply recomputes it)");
    if (ncls < 1 || ncls > OUTC_MAXCLS || C % 16 || C > 1024 || 1024 % C) BDN_FAIL(BDN_E_SHAPE, "outc_bwd: bad shape");
    hipStream_t st = (hipStream_t)stream; const int npix = B * H * W;
    const unsigned grid = bdn_outc_bwd_rows(dtype, B, H, W, C);
    const size_t smem = sizeof(float) * (ncls * (C + 1) + 256 * (dtype == BDN_BF16 ? 8 : 4) * 2);
    if (dtype == BDN_BF16) {
        if (ncls <= 2 && C == 64) hipLaunchKernelGGL((outc_bwd_kernel<bf16s, 2, 8>), dim3(grid), dim3(256), smem, st, dlogits, (const bf16s*)z, bn, w, (bf16s*)dA, ws, bs_partial, npix, H * W, C, ncls, FastDiv(H * W));
        else if (ncls <= 2) hipLaunchKernelGGL((outc_bwd_kernel<bf16s, 2>), dim3(grid), dim3(256), smem, st, dlogits, (const bf16s*)z, bn, w, (bf16s*)dA, ws, bs_partial, npix, H * W, C, ncls, FastDiv(H * W));
        else hipLaunchKernelGGL((outc_bwd_kernel<bf16s, OUTC_MAXCLS>), dim3(grid), dim3(256), smem, st, dlogits, (const bf16s*)z, bn, w, (bf16s*)dA, ws, bs_partial, npix, H * W, C, ncls, FastDiv(H * W));
    } else if (dtype == BDN_F32) {
        if (ncls <= 2 && C == 64) hipLaunchKernelGGL((outc_bwd_kernel<float, 2, 16>), dim3(grid), dim3(256), smem, st, dlogits, (const float*)z, bn, w, (float*)dA, ws, bs_partial, npix, H * W, C, ncls, FastDiv(H * W));
        else if (ncls <= 2) hipLaunchKernelGGL((outc_bwd_kernel<float, 2>), dim3(grid), dim3(256), smem, st, dlogits, (const float*)z, bn, w, (float*)dA, ws, bs_partial, npix, H * W, C, ncls, FastDiv(H * W));
        else hipLaunchKernelGGL((outc_bwd_kernel<float, OUTC_MAXCLS>), dim3(grid), dim3(256), smem, st, dlogits, (const float*)z, bn, w, (float*)dA, ws, bs_partial, npix, H * W, C, ncls, FastDiv(H * W));
    } else BDN_FAIL(BDN_E_ARG, "outc_bwd: bad dtype");
    BDN_CHECK_LAUNCH("outc_bwd");
    hipLaunchKernelGGL(outc_dw_reduce_kernel, dim3(ncls * (C + 1)), dim3(256), 0, st, ws, (int)grid, C, ncls, dw, db);
    BDN_CHECK_LAUNCH("outc_dw_reduce");
    return BDN_OK;
}

// BatchNorm+ReLU backward of the layer in front of the classifier, with the classifier's data gradient RECOMPUTED from
// dlogits (ncls values per pixel) instead of read back: dA = round_T(sum_k dl[k] w[k][c]) exactly as outc_bwd forms and
// rounds it, then bn_bwd_apply's expression.  outc_bwd then need not store dA at all: 2 x B*H*W*C elements of HBM traffic
// less, at a point of the step where nothing else runs.
template <typename T, int NC, bool SPLIT = false>
__global__ __launch_bounds__(256) void outc_bn_bwd_apply_kernel(const float* __restrict__ dl, const float* __restrict__ w,
                                const T* __restrict__ z, const float* __restrict__ bn, const float* __restrict__ sums,
                                T* __restrict__ dz, int npix, int hw, int pix_per_group, int pix_per_block, int C, int ncls, FastDiv dhw, FastDiv dppg) {
    constexpr int EPU = ET<T>::EPU;
    const int CU = C / EPU, rows = 256 / CU, tid = threadIdx.x, cu = tid % CU, row = tid / CU, c = cu * EPU;
    const int p_begin = blockIdx.x * pix_per_block, p_end = min(npix, p_begin + pix_per_block);
    if (p_begin >= p_end) return;
    const float invM = 1.f / (float)pix_per_group;
    int gcur = -1;
    float mean[EPU], inv[EPU], sc[EPU], sh[EPU], k0[EPU], k1[EPU], wk[NC][EPU];
#pragma unroll
    for (int k = 0; k < NC; k++)
#pragma unroll
        for (int i = 0; i < EPU; i++) wk[k][i] = k < ncls ? w[k * C + c + i] : 0.f;
    for (int pb = p_begin + row; pb < p_end; pb += 4 * rows) {
        // four pixels of a lane are requested before the first is used
        uint4 zu[4]; float gv[4][NC];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int pj = pb + j * rows < p_end ? pb + j * rows : pb;
            int b, q; dhw.divmod(pj, b, q);
#pragma unroll
            for (int k = 0; k < NC; k++) gv[j][k] = k < ncls ? dl[((size_t)b * ncls + k) * hw + q] : 0.f;
            zu[j] = *reinterpret_cast<const uint4*>(z + (size_t)pj * C + c);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int p = pb + j * rows;
            if (p >= p_end) break;
            const int g = dppg.div(p);
            if (g != gcur) {                                   // (blocks never straddle groups in practice; correct if they do)
                gcur = g;
#pragma unroll
                for (int i = 0; i < EPU; i++) {
                    mean[i] = bn_row(bn, g, 0, C)[c + i]; inv[i] = bn_row(bn, g, 1, C)[c + i];
                    sc[i] = bn_row(bn, g, 2, C)[c + i]; sh[i] = bn_row(bn, g, 3, C)[c + i];
                    k0[i] = sums[((size_t)g * 2 + 0) * C + c + i] * invM;
                    k1[i] = sums[((size_t)g * 2 + 1) * C + c + i] * invM;
                }
            }
            float fz[EPU], o[EPU];
            Unit<T>::unpack(zu[j], fz);
#pragma unroll
            for (int i = 0; i < EPU; i++) {
                float s = 0.f;
#pragma unroll
                for (int k = 0; k < NC; k++) if (k < ncls) s = fmaf(gv[j][k], wk[k][i], s);
                o[i] = s;
            }
            Unit<T>::unpack(Unit<T>::pack(o), o);              // the gradient as outc_bwd would have stored it
#pragma unroll
            for (int i = 0; i < EPU; i++) {
                const float gm = fmaf(fz[i], sc[i], sh[i]) > 0.f ? o[i] : 0.f;
                const float xhat = (fz[i] - mean[i]) * inv[i];
                o[i] = sc[i] * (gm - k0[i] - xhat * k1[i]);
            }
            if constexpr (SPLIT) {                             // bf16x3: dz leaves as the [hi | lo] operand of its two consumers ([pixel][2C])
                const SplitOut so = {reinterpret_cast<bf16s*>(dz), 2 * C, 0, C};
                store_split4(so, (size_t)p, c, o);
            } else
            *reinterpret_cast<uint4*>(dz + (size_t)p * C + c) = Unit<T>::pack(o);
        }
    }
}

extern "C" int bdn_outc_bn_bwd_apply(int dtype, const float* dlogits, const float* w, const void* z, const float* bn,
                                     int imgs_per_group, const float* sums, void* dz, int B, int H, int W, int C, int ncls, void* stream) {
    if (!dlogits || !w || !z || !bn || !sums || !dz) BDN_FAIL(BDN_E_ARG, "outc_bn_bwd_apply: null pointer");
    if (ncls < 1 || ncls > OUTC_MAXCLS || C % 16 || C > 1024 || 1024 % C || B <= 0 || H <= 0 || W <= 0 || imgs_per_group <= 0 || B % imgs_per_group)
        BDN_FAIL(BDN_E_SHAPE, "outc_bn_bwd_apply: bad shape");
    hipStream_t st = (hipStream_t)stream;
    const int npix = B * H * W, epu = dtype == BDN_BF16 ? 8 : 4, rows = 256 / (C / epu);
    int ppb = (npix + 2047) / 2048; if (ppb < 2 * rows) ppb = 2 * rows; ppb = (ppb + rows - 1) / rows * rows;
    const unsigned grid = (npix + ppb - 1) / ppb;
    if (dtype == BDN_BF16X3) {                 // float32 z, dz stored as the split operand
#define OUTC_APPLY_S(NC_) hipLaunchKernelGGL((outc_bn_bwd_apply_kernel<float, NC_, true>), dim3(grid), dim3(256), 0, st, dlogits, w, (const float*)z, bn, sums, \
                                               (float*)dz, npix, H * W, imgs_per_group * H * W, ppb, C, ncls, FastDiv(H * W), FastDiv(imgs_per_group * H * W))
        if (ncls <= 2) OUTC_APPLY_S(2); else OUTC_APPLY_S(OUTC_MAXCLS);
#undef OUTC_APPLY_S
        BDN_CHECK_LAUNCH("outc_bn_bwd_apply");
        return BDN_OK;
    }
#define OUTC_APPLY(T_, NC_) hipLaunchKernelGGL((outc_bn_bwd_apply_kernel<T_, NC_>), dim3(grid), dim3(256), 0, st, dlogits, w, (const T_*)z, bn, sums, \
                                               (T_*)dz, npix, H * W, imgs_per_group * H * W, ppb, C, ncls, FastDiv(H * W), FastDiv(imgs_per_group * H * W))
    if (dtype == BDN_BF16) { if (ncls <= 2) OUTC_APPLY(bf16s, 2); else OUTC_APPLY(bf16s, OUTC_MAXCLS); }
    else if (dtype == BDN_F32) { if (ncls <= 2) OUTC_APPLY(float, 2); else OUTC_APPLY(float, OUTC_MAXCLS); }
    else BDN_FAIL(BDN_E_ARG, "outc_bn_bwd_apply: bad dtype");
#undef OUTC_APPLY
    BDN_CHECK_LAUNCH("outc_bn_bwd_apply");
    return BDN_OK;
}

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
__device__ __forceinline__ unsigned topk_key(float v) { const unsigned u = __float_as_uint(v); return (u & 0x80000000u) ? ~u : (u ^ 0x80000000u); }
__device__ __forceinline__ float topk_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k); }
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
extern "C" size_t bdn_overlap_workspace_bytes(int B, int ncls, int H, int W, int reduce_w) {
    if (B <= 0 || H <= 0 || W <= 0 || ncls < 2 || ncls > OUTC_MAXCLS) return 0;
    const OverlapPlan p = overlap_plan(B, ncls, H, W, reduce_w);
    return sizeof(float) * ((size_t)p.n * (p.nblk + 1) + 8) + sizeof(int32_t) * 4 * p.gx * p.gy;
}

extern "C" int bdn_overlap_loss(const float* logits, const uint8_t* labels, float alpha, float beta, float eps,
                                int reduce_w, float* ws, float* loss, int32_t* counts, float* dlogits,
                                int B, int ncls, int H, int W, void* stream) {
    if (!logits || !labels || !ws || !loss) BDN_FAIL(BDN_E_ARG, "overlap_loss: null pointer");
    if (ncls < 2 || ncls > OUTC_MAXCLS) BDN_FAIL(BDN_E_SHAPE, "overlap_loss: ncls=%d unsupported (2..%d)", ncls, OUTC_MAXCLS);
    if (B <= 0 || H <= 0 || W <= 0 || (size_t)B * H * W >= ((size_t)1 << 31)) BDN_FAIL(BDN_E_SHAPE, "overlap_loss: bad shape");
    hipStream_t st = (hipStream_t)stream;
    const OverlapPlan p = overlap_plan(B, ncls, H, W, reduce_w);
    const int We = p.We;
    float* part = ws + p.n;                                                    // [nblk][n] block partials behind the n final sums
    int32_t* pcounts = reinterpret_cast<int32_t*>(part + (size_t)p.nblk * p.n);  // [gx*gy][4]
    dim3 grid(p.gx, p.gy), block(p.RL, p.CW);
    if (ncls <= 2) hipLaunchKernelGGL((tversky_sums_kernel<2, false>), grid, block, sizeof(float) * 256 * 3 * 2, st, logits, labels, part, pcounts, B, ncls, H, W, p.rpb, We, FastDiv(H), FocalStats{});
    else hipLaunchKernelGGL((tversky_sums_kernel<OUTC_MAXCLS, false>), grid, block, sizeof(float) * 256 * 3 * OUTC_MAXCLS, st, logits, labels, part, pcounts, B, ncls, H, W, p.rpb, We, FastDiv(H), FocalStats{});
    BDN_CHECK_LAUNCH("tversky_sums");
    hipLaunchKernelGGL(tversky_finish_kernel<false>, dim3(1), dim3(1024), 0, st, ws, part, p.nblk, pcounts, p.gx * p.gy, counts, alpha, beta, eps, ncls, We, loss, FocalFinish{});
    BDN_CHECK_LAUNCH("tversky_finish");
    if (dlogits) {
        hipLaunchKernelGGL(tversky_bwd_kernel<false>, dim3(grid_for((size_t)B * H * W)), dim3(256), 0, st, logits, labels, ws, alpha, beta, dlogits, B, ncls, H, W, We, FastDiv(H * W), FastDiv(W), FocalBwd{});
        BDN_CHECK_LAUNCH("tversky_bwd");
    }
    return BDN_OK;
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
    if (counts) hipMemsetAsync(counts, 0, sizeof(int32_t) * 4, st);
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

static inline size_t criterion_focal_part_bytes(const OverlapPlan& p) { return (sizeof(double) * p.gx * p.gy + 15) / 16 * 16; }

extern "C" size_t bdn_criterion_workspace_bytes(int B, int ncls, int H, int W, int reduce_w) {
    const size_t ov = bdn_overlap_workspace_bytes(B, ncls, H, W, reduce_w);
    if (ov == 0 || (size_t)B * H * W >= ((size_t)1 << 31)) return 0;
    const size_t compound = criterion_focal_part_bytes(overlap_plan(B, ncls, H, W, reduce_w)) + ov, focal = bdn_focal_workspace_bytes();
    return compound > focal ? compound : focal;
}

extern "C" int bdn_criterion(const float* logits, const uint8_t* labels, float w_overlap, float alpha, float beta, float eps, int reduce_w,
                             float w_focal, float gamma, const float* class_alpha, int size_average, void* ws, float* loss, float* terms,
                             int32_t* counts, float* dlogits, int B, int ncls, int H, int W, void* stream) {
    if (!logits || !labels || !ws || !loss) BDN_FAIL(BDN_E_ARG, "criterion: null pointer");
    if (!(w_overlap >= 0.f) || !(w_focal >= 0.f)) BDN_FAIL(BDN_E_ARG, "criterion: negative weight (w_overlap=%g, w_focal=%g)", w_overlap, w_focal);
    if (w_overlap == 0.f && w_focal == 0.f) BDN_FAIL(BDN_E_ARG, "criterion: both weights are zero");
    if (!(gamma >= 0.f)) BDN_FAIL(BDN_E_ARG, "criterion: negative gamma");
    if (ncls < 2 || ncls > OUTC_MAXCLS) BDN_FAIL(BDN_E_SHAPE, "criterion: ncls=%d unsupported (2..%d)", ncls, OUTC_MAXCLS);
    if (B <= 0 || H <= 0 || W <= 0 || (size_t)B * H * W >= ((size_t)1 << 31)) BDN_FAIL(BDN_E_SHAPE, "criterion: bad shape (B*H*W must stay below 2^31)");
    if ((uintptr_t)ws & 15) BDN_FAIL(BDN_E_ARG, "criterion: ws must be 16-byte aligned");
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
    double* fpart = (double*)ws;                                               // [gx*gy]
    float* sums = (float*)((char*)ws + criterion_focal_part_bytes(p));         // bdn_overlap_loss's layout from here on
    float* part = sums + p.n;
    int32_t* pcounts = reinterpret_cast<int32_t*>(part + (size_t)p.nblk * p.n);
    const double inv = size_average ? 1.0 / (double)((size_t)B * H * W) : 1.0;
    const FocalStats fs{class_alpha, gamma, fpart};
    dim3 grid(p.gx, p.gy), block(p.RL, p.CW);
    if (ncls <= 2) hipLaunchKernelGGL((tversky_sums_kernel<2, true>), grid, block, sizeof(float) * 256 * 3 * 2, st, logits, labels, part, pcounts, B, ncls, H, W, p.rpb, p.We, FastDiv(H), fs);
    else hipLaunchKernelGGL((tversky_sums_kernel<OUTC_MAXCLS, true>), grid, block, sizeof(float) * 256 * 3 * OUTC_MAXCLS, st, logits, labels, part, pcounts, B, ncls, H, W, p.rpb, p.We, FastDiv(H), fs);
    BDN_CHECK_LAUNCH("criterion_stats");
    hipLaunchKernelGGL(tversky_finish_kernel<true>, dim3(1), dim3(1024), 0, st, sums, part, p.nblk, pcounts, p.gx * p.gy, counts, alpha, beta, eps, ncls, p.We, loss,
                       FocalFinish{fpart, p.gx * p.gy, inv, w_overlap, w_focal, terms});
    BDN_CHECK_LAUNCH("criterion_finish");
    if (dlogits) {
        hipLaunchKernelGGL(tversky_bwd_kernel<true>, dim3(grid_for((size_t)B * H * W)), dim3(256), 0, st, logits, labels, sums, alpha, beta, dlogits, B, ncls, H, W, p.We,
                           FastDiv(H * W), FastDiv(W), FocalBwd{class_alpha, gamma, (float)inv, w_overlap, w_focal});
        BDN_CHECK_LAUNCH("criterion_bwd");
    }
    return BDN_OK;
}

// ============================================================ criterion with an ignore label
// bdn_criterion's function over the VALID pixels (label != ignore_label): always the three MASKED launches above, whatever the weights.
// ws: [focal block partials, double, padded to 16 bytes][sums n][part nblk*n][pcounts gx*gy*5][focal gradient scale, padded to 16 bytes].
extern "C" size_t bdn_criterion_masked_workspace_bytes(int B, int ncls, int H, int W, int reduce_w) {
    if (B <= 0 || H <= 0 || W <= 0 || ncls < 2 || ncls > OUTC_MAXCLS || (size_t)B * H * W >= ((size_t)1 << 31)) return 0;
    const OverlapPlan p = overlap_plan(B, ncls, H, W, reduce_w);
    return criterion_focal_part_bytes(p) + sizeof(float) * (size_t)p.n * (p.nblk + 1) + sizeof(int32_t) * 5 * p.gx * p.gy + 16;
}

extern "C" int bdn_criterion_masked(const float* logits, const uint8_t* labels, int ignore_label, float w_overlap, float alpha, float beta,
                                    float eps, int reduce_w, float w_focal, float gamma, const float* class_alpha, int size_average,
                                    void* ws, float* loss, float* terms, int32_t* counts, float* dlogits, int B, int ncls, int H, int W,
                                    void* stream) {
    if (!logits || !labels || !ws || !loss) BDN_FAIL(BDN_E_ARG, "criterion_masked: null pointer");
    if (ignore_label < 0 || ignore_label > 255) BDN_FAIL(BDN_E_ARG, "criterion_masked: ignore_label=%d is not a byte value (0..255)", ignore_label);
    if (!(w_overlap >= 0.f) || !(w_focal >= 0.f)) BDN_FAIL(BDN_E_ARG, "criterion_masked: negative weight (w_overlap=%g, w_focal=%g)", w_overlap, w_focal);
    if (w_overlap == 0.f && w_focal == 0.f) BDN_FAIL(BDN_E_ARG, "criterion_masked: both weights are zero");
    if (!(gamma >= 0.f)) BDN_FAIL(BDN_E_ARG, "criterion_masked: negative gamma");
    if (ncls < 2 || ncls > OUTC_MAXCLS) BDN_FAIL(BDN_E_SHAPE, "criterion_masked: ncls=%d unsupported (2..%d)", ncls, OUTC_MAXCLS);
    if (B <= 0 || H <= 0 || W <= 0 || (size_t)B * H * W >= ((size_t)1 << 31)) BDN_FAIL(BDN_E_SHAPE, "criterion_masked: bad shape (B*H*W must stay below 2^31)");
    if ((uintptr_t)ws & 15) BDN_FAIL(BDN_E_ARG, "criterion_masked: ws must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const OverlapPlan p = overlap_plan(B, ncls, H, W, reduce_w);
    double* fpart = (double*)ws;                                               // [gx*gy]
    float* sums = (float*)((char*)ws + criterion_focal_part_bytes(p));         // [n], then the coefficient tables
    float* part = sums + p.n;                                                  // [nblk][n]
    int32_t* pcounts = reinterpret_cast<int32_t*>(part + (size_t)p.nblk * p.n);  // [gx*gy][5]
    float* gscale = reinterpret_cast<float*>(pcounts + (size_t)5 * p.gx * p.gy); // the finish writes it, the gradient pass reads it
    const FocalStats fs{class_alpha, gamma, fpart, ignore_label};
    dim3 grid(p.gx, p.gy), block(p.RL, p.CW);
    if (ncls <= 2) hipLaunchKernelGGL((tversky_sums_kernel<2, true, true>), grid, block, sizeof(float) * 256 * 3 * 2, st, logits, labels, part, pcounts, B, ncls, H, W, p.rpb, p.We, FastDiv(H), fs);
    else hipLaunchKernelGGL((tversky_sums_kernel<OUTC_MAXCLS, true, true>), grid, block, sizeof(float) * 256 * 3 * OUTC_MAXCLS, st, logits, labels, part, pcounts, B, ncls, H, W, p.rpb, p.We, FastDiv(H), fs);
    BDN_CHECK_LAUNCH("criterion_masked_stats");
    hipLaunchKernelGGL((tversky_finish_kernel<true, true>), dim3(1), dim3(1024), 0, st, sums, part, p.nblk, pcounts, p.gx * p.gy, counts, alpha, beta, eps, ncls, p.We, loss,
                       FocalFinish{fpart, p.gx * p.gy, 1.0, w_overlap, w_focal, terms, size_average, gscale});
    BDN_CHECK_LAUNCH("criterion_masked_finish");
    if (dlogits) {
        hipLaunchKernelGGL((tversky_bwd_kernel<true, true>), dim3(grid_for((size_t)B * H * W)), dim3(256), 0, st, logits, labels, sums, alpha, beta, dlogits, B, ncls, H, W, p.We,
                           FastDiv(H * W), FastDiv(W), FocalBwd{class_alpha, gamma, 1.f, w_overlap, w_focal, gscale, ignore_label});
        BDN_CHECK_LAUNCH("criterion_masked_bwd");
    }
    return BDN_OK;
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

struct TopkPlan { OverlapPlan ov; int npix, nchunks, cpb, nsb, hgrid; size_t o_sums, o_state, o_hist, o_tie, o_pterm, o_kept, total; };
static inline size_t up16(size_t v) { return (v + 15) / 16 * 16; }
static TopkPlan topk_plan(int B, int ncls, int H, int W, int reduce_w) {
    TopkPlan t;
    t.ov = overlap_plan(B, ncls, H, W, reduce_w);
    t.npix = B * H * W;
    t.nchunks = (t.npix + TOPK_CHUNK - 1) / TOPK_CHUNK;
    t.cpb = (t.nchunks + 511) / 512;                                           // chunks per block of the sum pass: at most 512 blocks
    t.nsb = (t.nchunks + t.cpb - 1) / t.cpb;
    t.hgrid = t.nchunks < 1024 ? t.nchunks : 1024;                             // histogram passes: grid-stride over the chunks
    t.o_sums = up16(sizeof(double) * t.nsb);
    t.o_state = up16(t.o_sums + sizeof(float) * (size_t)t.ov.n * (t.ov.nblk + 1) + sizeof(int32_t) * 5 * t.ov.gx * t.ov.gy + 16);
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
    if (!(gamma >= 0.f)) BDN_FAIL(BDN_E_ARG, "criterion_topk: negative gamma");
    if (ncls < 2 || ncls > OUTC_MAXCLS) BDN_FAIL(BDN_E_SHAPE, "criterion_topk: ncls=%d unsupported (2..%d)", ncls, OUTC_MAXCLS);
    if (B <= 0 || H <= 0 || W <= 0 || (size_t)B * H * W >= ((size_t)1 << 31)) BDN_FAIL(BDN_E_SHAPE, "criterion_topk: bad shape (B*H*W must stay below 2^31)");
    if ((uintptr_t)ws & 15) BDN_FAIL(BDN_E_ARG, "criterion_topk: ws must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const TopkPlan t = topk_plan(B, ncls, H, W, reduce_w);
    const OverlapPlan& p = t.ov;
    char* base = (char*)ws;
    double* fpart = (double*)base;                                             // [nsb] block partials of the kept terms
    float* sums = (float*)(base + t.o_sums);                                   // bdn_criterion_masked's layout from here to gscale
    float* part = sums + p.n;
    int32_t* pcounts = reinterpret_cast<int32_t*>(part + (size_t)p.nblk * p.n);
    float* gscale = reinterpret_cast<float*>(pcounts + (size_t)5 * p.gx * p.gy);
    long long* state = (long long*)(base + t.o_state);
    unsigned* hist = (unsigned*)(base + t.o_hist);
    int32_t* tiecnt = (int32_t*)(base + t.o_tie);
    float* pterm = (float*)(base + t.o_pterm);
    uint8_t* kept_ws = (uint8_t*)(base + t.o_kept);
    if (hipMemsetAsync(hist, 0, sizeof(unsigned) * TOPK_HIST_TOTAL, st) != hipSuccess) BDN_FAIL(BDN_E_HIP, "criterion_topk: memset failed");
    const FocalStats fs{class_alpha, gamma, nullptr, ignore_label, pterm};
    dim3 grid(p.gx, p.gy), block(p.RL, p.CW);
    if (ncls <= 2) hipLaunchKernelGGL((tversky_sums_kernel<2, true, true, true>), grid, block, sizeof(float) * 256 * 3 * 2, st, logits, labels, part, pcounts, B, ncls, H, W, p.rpb, p.We, FastDiv(H), fs);
    else hipLaunchKernelGGL((tversky_sums_kernel<OUTC_MAXCLS, true, true, true>), grid, block, sizeof(float) * 256 * 3 * OUTC_MAXCLS, st, logits, labels, part, pcounts, B, ncls, H, W, p.rpb, p.We, FastDiv(H), fs);
    BDN_CHECK_LAUNCH("criterion_topk_stats");
#define TOPK_HIST(L_) hipLaunchKernelGGL(topk_hist_kernel<L_>, dim3(t.hgrid), dim3(256), 0, st, pterm, labels, ignore_label, t.npix, t.nchunks, topk_ppm, hist, state, tiecnt)
    TOPK_HIST(0); BDN_CHECK_LAUNCH("criterion_topk_hist0");
    TOPK_HIST(1); BDN_CHECK_LAUNCH("criterion_topk_hist1");
    TOPK_HIST(2); BDN_CHECK_LAUNCH("criterion_topk_hist2");
    TOPK_HIST(3); BDN_CHECK_LAUNCH("criterion_topk_ties");
#undef TOPK_HIST
    hipLaunchKernelGGL(topk_sum_kernel, dim3(t.nsb), dim3(256), 0, st, pterm, labels, ignore_label, t.npix, t.nchunks, t.cpb, state, tiecnt, kept_ws, fpart, pixel_terms, kept);
    BDN_CHECK_LAUNCH("criterion_topk_sum");
    hipLaunchKernelGGL((tversky_finish_kernel<true, true, true>), dim3(1), dim3(1024), 0, st, sums, part, p.nblk, pcounts, p.gx * p.gy, counts, alpha, beta, eps, ncls, p.We, loss,
                       FocalFinish{fpart, t.nsb, 1.0, w_overlap, w_focal, terms, size_average, gscale, state + 8});
    BDN_CHECK_LAUNCH("criterion_topk_finish");
    if (dlogits) {
        hipLaunchKernelGGL((tversky_bwd_kernel<true, true, true>), dim3(grid_for((size_t)B * H * W)), dim3(256), 0, st, logits, labels, sums, alpha, beta, dlogits, B, ncls, H, W, p.We,
                           FastDiv(H * W), FastDiv(W), FocalBwd{class_alpha, gamma, 1.f, w_overlap, w_focal, gscale, ignore_label, kept_ws});
        BDN_CHECK_LAUNCH("criterion_topk_bwd");
    }
    return BDN_OK;
}

// ============================================================ SGD (train.py:55,95)
__global__ void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float step, size_t n4, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n4) {
        float4 a = reinterpret_cast<float4*>(p)[i]; const float4 b = reinterpret_cast<const float4*>(g)[i];
        a.x -= step * b.x; a.y -= step * b.y; a.z -= step * b.z; a.w -= step * b.w;
        reinterpret_cast<float4*>(p)[i] = a;
    }
    if (i == 0) for (size_t k = n4 * 4; k < n; k++) p[k] -= step * g[k];
}

extern "C" int bdn_sgd_step(float* params, const float* grads, float lr, float grad_scale, size_t n, void* stream) {
    if (!params || !grads) BDN_FAIL(BDN_E_ARG, "sgd_step: null pointer");
    if (((uintptr_t)params | (uintptr_t)grads) & 15) BDN_FAIL(BDN_E_ARG, "sgd_step: buffers must be 16-byte aligned");
    if (n == 0) return BDN_OK;
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(sgd_kernel, dim3(grid_for(n4 > 0 ? n4 : 1)), dim3(256), 0, (hipStream_t)stream, params, grads, lr * grad_scale, n4, n);
    BDN_CHECK_LAUNCH("sgd_step");
    return BDN_OK;
}

// ============================================================ momentum SGD / Adam / AdamW (train.py:55-56,95)
// torch.optim's single-tensor update rules over the flat f32 buffers, one element per lane and OPT_VEC float4s in flight per
// thread (every load of a pass is issued before the first store).  Memory-bound: the grid is capped at 8 blocks per CU of the
// 256 and grid-strides the rest.  No LDS, no atomics: every element's result depends only on its own inputs (bit-reproducible).
// IEEE division and sqrt (hipcc's default correctly rounded f32 divide / sqrt).
constexpr int OPT_VEC = 4;

static inline unsigned opt_grid(size_t n4) {
    const size_t b = (n4 + 256 * OPT_VEC - 1) / (256 * OPT_VEC);
    return (unsigned)(b == 0 ? 1 : (b < 2048 ? b : 2048));
}

struct SgdmParams { float lr, grad_scale, momentum, damp1 /* 1 - dampening */, weight_decay; int first, nesterov; };

// SGD (torch 2.10 _single_tensor_sgd): g = s*grad (+ wd*p); buf = g on the first step, momentum*buf + (1-dampening)*g after it;
// g = g + momentum*buf (nesterov) or buf; p -= lr*g.  MOM = false: no momentum buffer is read or written.
template <bool MOM>
__device__ __forceinline__ void sgdm_elem(float& p, float gr, float& buf, const SgdmParams& a) {
    float g = a.grad_scale * gr;
    if (a.weight_decay != 0.f) g = g + a.weight_decay * p;
    if (MOM) {
        buf = a.first ? g : a.momentum * buf + a.damp1 * g;
        g = a.nesterov ? g + a.momentum * buf : buf;
    }
    p = p - a.lr * g;
}

template <bool MOM>
__global__ void __launch_bounds__(256) sgdm_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                   SgdmParams a, size_t n4, size_t n) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256 + threadIdx.x; base < n4; base += stride * OPT_VEC) {
        float4 P[OPT_VEC], G[OPT_VEC], M[OPT_VEC] = {};
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = base + u * stride;
            if (i < n4) {
                P[u] = reinterpret_cast<const float4*>(p)[i]; G[u] = reinterpret_cast<const float4*>(g)[i];
                if (MOM && !a.first) M[u] = reinterpret_cast<const float4*>(buf)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = base + u * stride;
            if (i < n4) {
                sgdm_elem<MOM>(P[u].x, G[u].x, M[u].x, a); sgdm_elem<MOM>(P[u].y, G[u].y, M[u].y, a);
                sgdm_elem<MOM>(P[u].z, G[u].z, M[u].z, a); sgdm_elem<MOM>(P[u].w, G[u].w, M[u].w, a);
                reinterpret_cast<float4*>(p)[i] = P[u];
                if (MOM) reinterpret_cast<float4*>(buf)[i] = M[u];
            }
        }
    }
    // the n % 4 trailing elements (never for a FlatLayout buffer: every tensor is padded to 4 floats)
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const size_t k = n4 * 4 + threadIdx.x;
        float m = (MOM && !a.first) ? buf[k] : 0.f, q = p[k];
        sgdm_elem<MOM>(q, g[k], m, a);
        p[k] = q;
        if (MOM) buf[k] = m;
    }
}

extern "C" int bdn_sgd_momentum_step(float* params, const float* grads, float* momentum_buf, float lr, float grad_scale, float momentum,
                                     float dampening, float weight_decay, int nesterov, int first_step, size_t n, void* stream) {
    if (!params || !grads) BDN_FAIL(BDN_E_ARG, "sgd_momentum_step: null pointer");
    if ((momentum != 0.f) != (momentum_buf != nullptr))
        BDN_FAIL(BDN_E_ARG, "sgd_momentum_step: momentum_buf must be given iff momentum != 0");
    if (nesterov && (momentum <= 0.f || dampening != 0.f))
        BDN_FAIL(BDN_E_ARG, "sgd_momentum_step: nesterov needs momentum > 0 and zero dampening");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf) & 15)
        BDN_FAIL(BDN_E_ARG, "sgd_momentum_step: buffers must be 16-byte aligned");
    if (n == 0) return BDN_OK;
    const size_t n4 = n / 4;
    const SgdmParams a{lr, grad_scale, momentum, (float)(1.0 - (double)dampening), weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
    if (momentum_buf)
        hipLaunchKernelGGL(sgdm_kernel<true>, dim3(opt_grid(n4)), dim3(256), 0, (hipStream_t)stream, params, grads, momentum_buf, a, n4, n);
    else
        hipLaunchKernelGGL(sgdm_kernel<false>, dim3(opt_grid(n4)), dim3(256), 0, (hipStream_t)stream, params, grads, momentum_buf, a, n4, n);
    BDN_CHECK_LAUNCH("sgd_momentum_step");
    return BDN_OK;
}

struct AdamParams { float grad_scale, w1 /* lerp weight 1 - beta1 */, beta2, c2 /* 1 - beta2 */, eps, l2 /* Adam's coupled weight
                    decay */, decay /* AdamW: 1 - lr*wd */, step_size /* lr / bc1 */, bc2_sqrt; int lerp_hi; };

// Adam / AdamW (torch 2.10 _single_tensor_adam): g = s*grad; AdamW p *= 1 - lr*wd, Adam g += wd*p; m = lerp(m, g, 1-beta1);
// v = beta2*v + (1-beta2)*g*g; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps).  lerp as torch evaluates it: weight < 0.5 ? m + w*(g-m)
// : g - (g-m)*(1-w).
__device__ __forceinline__ void adam_elem(float& p, float gr, float& m, float& v, const AdamParams& a) {
    float g = a.grad_scale * gr;
    p = p * a.decay;
    if (a.l2 != 0.f) g = g + a.l2 * p;
    m = a.lerp_hi ? g - (g - m) * (1.f - a.w1) : m + a.w1 * (g - m);
    v = a.beta2 * v + a.c2 * g * g;
    const float den = sqrtf(v) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / den);
}

__global__ void __launch_bounds__(256) adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, AdamParams a, size_t n4, size_t n) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256 + threadIdx.x; base < n4; base += stride * OPT_VEC) {
        float4 P[OPT_VEC], G[OPT_VEC], M[OPT_VEC], V[OPT_VEC];
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = base + u * stride;
            if (i < n4) {
                P[u] = reinterpret_cast<const float4*>(p)[i]; G[u] = reinterpret_cast<const float4*>(g)[i];
                M[u] = reinterpret_cast<const float4*>(m)[i]; V[u] = reinterpret_cast<const float4*>(v)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = base + u * stride;
            if (i < n4) {
                adam_elem(P[u].x, G[u].x, M[u].x, V[u].x, a); adam_elem(P[u].y, G[u].y, M[u].y, V[u].y, a);
                adam_elem(P[u].z, G[u].z, M[u].z, V[u].z, a); adam_elem(P[u].w, G[u].w, M[u].w, V[u].w, a);
                reinterpret_cast<float4*>(p)[i] = P[u]; reinterpret_cast<float4*>(m)[i] = M[u]; reinterpret_cast<float4*>(v)[i] = V[u];
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {
        const size_t k = n4 * 4 + threadIdx.x;
        float q = p[k], mk = m[k], vk = v[k];
        adam_elem(q, g[k], mk, vk, a);
        p[k] = q; m[k] = mk; v[k] = vk;
    }
}

extern "C" int bdn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float lr, float grad_scale,
                             double beta1, double beta2, float eps, float weight_decay, int decoupled_weight_decay, long long step,
                             size_t n, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq) BDN_FAIL(BDN_E_ARG, "adam_step: null pointer");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15)
        BDN_FAIL(BDN_E_ARG, "adam_step: buffers must be 16-byte aligned");
    if (step < 1) BDN_FAIL(BDN_E_ARG, "adam_step: step must be >= 1 (1-based, counted after the increment), got %lld", step);
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0))
        BDN_FAIL(BDN_E_ARG, "adam_step: betas must lie in [0, 1)");
    if (n == 0) return BDN_OK;
    // 1 - beta and the bias corrections in double on the host, as torch computes them from Python floats: no device sync
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    const float w1 = (float)(1.0 - beta1);
    const bool dec = decoupled_weight_decay != 0;
    const AdamParams a{grad_scale, w1, (float)beta2, (float)(1.0 - beta2), eps, dec ? 0.f : weight_decay,
                       dec ? (float)(1.0 - (double)lr * (double)weight_decay) : 1.f, (float)((double)lr / bc1), (float)std::sqrt(bc2),
                       w1 >= 0.5f ? 1 : 0};
    const size_t n4 = n / 4;
    hipLaunchKernelGGL(adam_kernel, dim3(opt_grid(n4)), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg, exp_avg_sq, a, n4, n);
    BDN_CHECK_LAUNCH("adam_step");
    return BDN_OK;
}

// ============================================================ the same rules with parameter groups and frozen tensors (train.py:55-56,95)
// One launch over the flat buffers in which every float4 takes the hyperparameters of the group its tensor belongs to, or is skipped
// (frozen: neither read nor written).  FlatLayout pads every tensor to 4 floats, so a float4 never straddles two tensors.  The layout is
// a segment table in device memory -- sorted segment ends in float4 units and one group id per segment, OPT_FROZEN for a frozen one --
// staged in LDS once per block; the per-group hyperparameters travel by value in the kernel arguments and are staged beside it.  A
// block's 256 consecutive vectors almost always lie in one segment: one lookup of the first vector then serves the block (the lookup is
// per lane otherwise).  A vector behind the last segment end or with a group id outside [0, n_groups) is skipped, so a wrong table can
// not move an access out of the buffers.  The element formulas are sgd's p -= step*g, sgdm_elem and adam_elem above; the pass keeps
// their shape (OPT_VEC float4s per thread, every load issued before the first store, no reductions, no atomics).
constexpr int OPT_MAX_GROUPS = 8;
constexpr int OPT_MAX_SEGS = 256;
constexpr int OPT_FROZEN = -1;

struct SegTable { const uint32_t* end; const int32_t* group; int n_seg, n_groups; };
template <typename P> struct GroupArgs { P g[OPT_MAX_GROUPS]; };

struct RuleSgd {                                        // plain SGD: bdn_sgd_step's p -= (lr * grad_scale) * g
    using Params = float;
    static constexpr int NS = 0;
    static constexpr bool GRAD = true;
    static __device__ __forceinline__ void scale(Params& step, float s) { step *= s; }
    static __device__ __forceinline__ bool reads_state(const Params&) { return false; }
    static __device__ __forceinline__ void elem(float& p, float g, float&, float&, const Params& step) { p -= step * g; }
};
template <bool MOM> struct RuleSgdm {
    using Params = SgdmParams;
    static constexpr int NS = MOM ? 1 : 0;
    static constexpr bool GRAD = true;
    static __device__ __forceinline__ void scale(Params& a, float s) { a.grad_scale *= s; }
    static __device__ __forceinline__ bool reads_state(const Params& a) { return MOM && !a.first; }
    static __device__ __forceinline__ void elem(float& p, float g, float& buf, float&, const Params& a) { sgdm_elem<MOM>(p, g, buf, a); }
};
struct RuleAdam {
    using Params = AdamParams;
    static constexpr int NS = 2;
    static constexpr bool GRAD = true;
    static __device__ __forceinline__ void scale(Params& a, float s) { a.grad_scale *= s; }
    static __device__ __forceinline__ bool reads_state(const Params&) { return true; }
    static __device__ __forceinline__ void elem(float& p, float g, float& m, float& v, const Params& a) { adam_elem(p, g, m, v, a); }
};

// One halving step of the lookup "first s with end[s] > i" over the LDS table, which is padded with UINT32_MAX to `cap` entries, a power
// of two: branch-free, so the OPT_VEC lookups of a pass advance side by side (their LDS reads are independent) and lanes never diverge.
__device__ __forceinline__ void seg_step(const uint32_t* s_end, int h, uint32_t i, int& s) {
    if (s_end[s + h - 1] <= i) s += h;
}

template <typename Rule>
__global__ void __launch_bounds__(256) grouped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                      float* __restrict__ s1, SegTable t, GroupArgs<typename Rule::Params> a,
                                                      const float* __restrict__ dev_scale, size_t n4) {
    __shared__ uint32_t s_end[OPT_MAX_SEGS];
    __shared__ int s_grp[OPT_MAX_SEGS];
    __shared__ typename Rule::Params s_par[OPT_MAX_GROUPS];
    int cap = 1;
    while (cap < t.n_seg) cap <<= 1;
    for (int k = threadIdx.x; k < cap; k += 256) {
        s_end[k] = k < t.n_seg ? t.end[k] : 0xffffffffu;
        s_grp[k] = k < t.n_seg ? t.group[k] : (t.n_seg == 0 ? 0 : OPT_FROZEN);      // no table (bdn_ema_update): one segment of group 0
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < OPT_MAX_GROUPS; k++) s_par[k] = a.g[k];
        if (dev_scale) {                                     // the _ex entry points: grad_scale * *dev_scale, formed once per block
            const float ds = *dev_scale;
#pragma unroll
            for (int k = 0; k < OPT_MAX_GROUPS; k++) Rule::scale(s_par[k], ds);
        }
    }
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t b0 = (size_t)blockIdx.x * 256; b0 < n4; b0 += stride * OPT_VEC) {
        int gid[OPT_VEC], seg[OPT_VEC] = {};
        for (int h = cap >> 1; h > 0; h >>= 1) {             // the segment of each pass's first vector (clamped: a pass past the end is skipped below)
#pragma unroll
            for (int u = 0; u < OPT_VEC; u++) {
                const size_t first = b0 + u * stride;
                seg_step(s_end, h, (uint32_t)(first < n4 ? first : n4 - 1), seg[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t first = b0 + u * stride, i = first + threadIdx.x;
            int grp = OPT_FROZEN;
            if (i < n4) {
                const size_t last = first + 255 < n4 ? first + 255 : n4 - 1;
                int s = seg[u];
                if (!(s_end[s] > last)) {                    // the block's 256 vectors span a boundary (or lie behind the table): per lane
                    s = 0;
                    for (int h = cap >> 1; h > 0; h >>= 1) seg_step(s_end, h, (uint32_t)i, s);
                }
                if (s_end[s] > i) grp = s_grp[s];
            }
            gid[u] = (unsigned)grp < (unsigned)t.n_groups ? grp : OPT_FROZEN;
        }
        float4 P[OPT_VEC], G[OPT_VEC], S0[OPT_VEC] = {}, S1[OPT_VEC] = {};
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = b0 + u * stride + threadIdx.x;
            if (gid[u] != OPT_FROZEN) {
                P[u] = reinterpret_cast<const float4*>(p)[i];
                if (Rule::GRAD) G[u] = reinterpret_cast<const float4*>(g)[i];
                if (Rule::NS > 0 && Rule::reads_state(s_par[0])) S0[u] = reinterpret_cast<const float4*>(s0)[i];
                if (Rule::NS > 1) S1[u] = reinterpret_cast<const float4*>(s1)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = b0 + u * stride + threadIdx.x;
            if (gid[u] != OPT_FROZEN) {
                const typename Rule::Params q = s_par[gid[u]];
                float4 g4 = {};                              // a rule without `g` never loaded G[u]: it is not read either
                if constexpr (Rule::GRAD) g4 = G[u];
                Rule::elem(P[u].x, g4.x, S0[u].x, S1[u].x, q); Rule::elem(P[u].y, g4.y, S0[u].y, S1[u].y, q);
                Rule::elem(P[u].z, g4.z, S0[u].z, S1[u].z, q); Rule::elem(P[u].w, g4.w, S0[u].w, S1[u].w, q);
                reinterpret_cast<float4*>(p)[i] = P[u];
                if (Rule::NS > 0) reinterpret_cast<float4*>(s0)[i] = S0[u];
                if (Rule::NS > 1) reinterpret_cast<float4*>(s1)[i] = S1[u];
            }
        }
    }
}

static int grouped_check(const char* what, const void* params, const void* grads, const void* s0, const void* s1, const uint32_t* seg_end,
                         const int32_t* seg_group, int n_seg, int n_groups, const float* lr, size_t n) {
    if (!params || !grads || !seg_end || !seg_group || !lr) BDN_FAIL(BDN_E_ARG, "%s: null pointer", what);
    if (n_groups < 1 || n_groups > OPT_MAX_GROUPS)
        BDN_FAIL(BDN_E_ARG, "%s: %d groups (1..%d: their hyperparameters travel in the kernel arguments)", what, n_groups, OPT_MAX_GROUPS);
    if (n_seg < 1 || n_seg > OPT_MAX_SEGS) BDN_FAIL(BDN_E_ARG, "%s: %d segments (1..%d)", what, n_seg, OPT_MAX_SEGS);
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)s0 | (uintptr_t)s1) & 15) BDN_FAIL(BDN_E_ARG, "%s: buffers must be 16-byte aligned", what);
    if (((uintptr_t)seg_end | (uintptr_t)seg_group) & 3) BDN_FAIL(BDN_E_ARG, "%s: segment table must be 4-byte aligned", what);
    if (n % 4 != 0 || n / 4 > 0xffffffffull)
        BDN_FAIL(BDN_E_ARG, "%s: n = %zu must be a multiple of 4 (tensors padded to a float4) below 2^34", what, n);
    return BDN_OK;
}

// The grouped entry points and their _ex forms share one launcher each: dev_scale == nullptr is the plain form (the kernel then never
// touches the staged parameters, so its bits are those it always gave), a device pointer the _ex form.
static int ex_check(const char* what, const float* dev_scale) {
    if (!dev_scale) BDN_FAIL(BDN_E_ARG, "%s: null pointer (dev_scale)", what);
    if ((uintptr_t)dev_scale & 3) BDN_FAIL(BDN_E_ARG, "%s: dev_scale must be 4-byte aligned", what);
    return BDN_OK;
}

static int sgd_grouped_launch(const char* what, float* params, const float* grads, const uint32_t* seg_end, const int32_t* seg_group,
                              int n_seg, int n_groups, const float* lr, float grad_scale, const float* dev_scale, size_t n, void* stream) {
    if (int rc = grouped_check(what, params, grads, nullptr, nullptr, seg_end, seg_group, n_seg, n_groups, lr, n)) return rc;
    if (n == 0) return BDN_OK;
    GroupArgs<float> a{};
    for (int k = 0; k < n_groups; k++) a.g[k] = lr[k] * grad_scale;
    const SegTable t{seg_end, seg_group, n_seg, n_groups};
    hipLaunchKernelGGL(grouped_kernel<RuleSgd>, dim3(opt_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, params, grads, (float*)nullptr,
                       (float*)nullptr, t, a, dev_scale, n / 4);
    BDN_CHECK_LAUNCH(what);
    return BDN_OK;
}

extern "C" int bdn_sgd_step_grouped(float* params, const float* grads, const uint32_t* seg_end, const int32_t* seg_group, int n_seg,
                                    int n_groups, const float* lr, float grad_scale, size_t n, void* stream) {
    return sgd_grouped_launch("sgd_step_grouped", params, grads, seg_end, seg_group, n_seg, n_groups, lr, grad_scale, nullptr, n, stream);
}

extern "C" int bdn_sgd_step_grouped_ex(float* params, const float* grads, const uint32_t* seg_end, const int32_t* seg_group, int n_seg,
                                       int n_groups, const float* lr, float grad_scale, const float* dev_scale, size_t n, void* stream) {
    if (int rc = ex_check("sgd_step_grouped_ex", dev_scale)) return rc;
    return sgd_grouped_launch("sgd_step_grouped_ex", params, grads, seg_end, seg_group, n_seg, n_groups, lr, grad_scale, dev_scale, n, stream);
}

static int sgdm_grouped_launch(const char* what, float* params, const float* grads, float* momentum_buf, const uint32_t* seg_end,
                               const int32_t* seg_group, int n_seg, int n_groups, const float* lr, const float* weight_decay,
                               float grad_scale, const float* dev_scale, float momentum, float dampening, int nesterov, int first_step,
                               size_t n, void* stream) {
    if (int rc = grouped_check(what, params, grads, momentum_buf, nullptr, seg_end, seg_group, n_seg, n_groups, lr, n)) return rc;
    if (!weight_decay) BDN_FAIL(BDN_E_ARG, "%s: null pointer", what);
    if ((momentum != 0.f) != (momentum_buf != nullptr)) BDN_FAIL(BDN_E_ARG, "%s: momentum_buf must be given iff momentum != 0", what);
    if (nesterov && (momentum <= 0.f || dampening != 0.f)) BDN_FAIL(BDN_E_ARG, "%s: nesterov needs momentum > 0 and zero dampening", what);
    if (n == 0) return BDN_OK;
    GroupArgs<SgdmParams> a{};
    for (int k = 0; k < n_groups; k++)
        a.g[k] = SgdmParams{lr[k], grad_scale, momentum, (float)(1.0 - (double)dampening), weight_decay[k], first_step ? 1 : 0, nesterov ? 1 : 0};
    for (int k = n_groups; k < OPT_MAX_GROUPS; k++) a.g[k].first = first_step ? 1 : 0;        // reads_state() asks entry 0 only; keep all alike
    const SegTable t{seg_end, seg_group, n_seg, n_groups};
    if (momentum_buf)
        hipLaunchKernelGGL(grouped_kernel<RuleSgdm<true>>, dim3(opt_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, params, grads,
                           momentum_buf, (float*)nullptr, t, a, dev_scale, n / 4);
    else
        hipLaunchKernelGGL(grouped_kernel<RuleSgdm<false>>, dim3(opt_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, params, grads,
                           (float*)nullptr, (float*)nullptr, t, a, dev_scale, n / 4);
    BDN_CHECK_LAUNCH(what);
    return BDN_OK;
}

extern "C" int bdn_sgd_momentum_step_grouped(float* params, const float* grads, float* momentum_buf, const uint32_t* seg_end,
                                             const int32_t* seg_group, int n_seg, int n_groups, const float* lr, const float* weight_decay,
                                             float grad_scale, float momentum, float dampening, int nesterov, int first_step, size_t n,
                                             void* stream) {
    return sgdm_grouped_launch("sgd_momentum_step_grouped", params, grads, momentum_buf, seg_end, seg_group, n_seg, n_groups, lr,
                               weight_decay, grad_scale, nullptr, momentum, dampening, nesterov, first_step, n, stream);
}

extern "C" int bdn_sgd_momentum_step_grouped_ex(float* params, const float* grads, float* momentum_buf, const uint32_t* seg_end,
                                                const int32_t* seg_group, int n_seg, int n_groups, const float* lr,
                                                const float* weight_decay, float grad_scale, const float* dev_scale, float momentum,
                                                float dampening, int nesterov, int first_step, size_t n, void* stream) {
    if (int rc = ex_check("sgd_momentum_step_grouped_ex", dev_scale)) return rc;
    return sgdm_grouped_launch("sgd_momentum_step_grouped_ex", params, grads, momentum_buf, seg_end, seg_group, n_seg, n_groups, lr,
                               weight_decay, grad_scale, dev_scale, momentum, dampening, nesterov, first_step, n, stream);
}

static int adam_grouped_launch(const char* what, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                               const uint32_t* seg_end, const int32_t* seg_group, int n_seg, int n_groups, const float* lr,
                               const float* weight_decay, float grad_scale, const float* dev_scale, double beta1, double beta2, float eps,
                               int decoupled_weight_decay, long long step, size_t n, void* stream) {
    if (int rc = grouped_check(what, params, grads, exp_avg, exp_avg_sq, seg_end, seg_group, n_seg, n_groups, lr, n)) return rc;
    if (!exp_avg || !exp_avg_sq || !weight_decay) BDN_FAIL(BDN_E_ARG, "%s: null pointer", what);
    if (step < 1) BDN_FAIL(BDN_E_ARG, "%s: step must be >= 1 (1-based, counted after the increment), got %lld", what, step);
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) BDN_FAIL(BDN_E_ARG, "%s: betas must lie in [0, 1)", what);
    if (n == 0) return BDN_OK;
    // 1 - beta and the bias corrections in double on the host, exactly as bdn_adam_step forms them
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    const float w1 = (float)(1.0 - beta1);
    const bool dec = decoupled_weight_decay != 0;
    GroupArgs<AdamParams> a{};
    for (int k = 0; k < n_groups; k++)
        a.g[k] = AdamParams{grad_scale, w1, (float)beta2, (float)(1.0 - beta2), eps, dec ? 0.f : weight_decay[k],
                            dec ? (float)(1.0 - (double)lr[k] * (double)weight_decay[k]) : 1.f, (float)((double)lr[k] / bc1),
                            (float)std::sqrt(bc2), w1 >= 0.5f ? 1 : 0};
    const SegTable t{seg_end, seg_group, n_seg, n_groups};
    hipLaunchKernelGGL(grouped_kernel<RuleAdam>, dim3(opt_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, params, grads, exp_avg,
                       exp_avg_sq, t, a, dev_scale, n / 4);
    BDN_CHECK_LAUNCH(what);
    return BDN_OK;
}

extern "C" int bdn_adam_step_grouped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint32_t* seg_end,
                                     const int32_t* seg_group, int n_seg, int n_groups, const float* lr, const float* weight_decay,
                                     float grad_scale, double beta1, double beta2, float eps, int decoupled_weight_decay, long long step,
                                     size_t n, void* stream) {
    return adam_grouped_launch("adam_step_grouped", params, grads, exp_avg, exp_avg_sq, seg_end, seg_group, n_seg, n_groups, lr,
                               weight_decay, grad_scale, nullptr, beta1, beta2, eps, decoupled_weight_decay, step, n, stream);
}

extern "C" int bdn_adam_step_grouped_ex(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint32_t* seg_end,
                                        const int32_t* seg_group, int n_seg, int n_groups, const float* lr, const float* weight_decay,
                                        float grad_scale, const float* dev_scale, double beta1, double beta2, float eps,
                                        int decoupled_weight_decay, long long step, size_t n, void* stream) {
    if (int rc = ex_check("adam_step_grouped_ex", dev_scale)) return rc;
    return adam_grouped_launch("adam_step_grouped_ex", params, grads, exp_avg, exp_avg_sq, seg_end, seg_group, n_seg, n_groups, lr,
                               weight_decay, grad_scale, dev_scale, beta1, beta2, eps, decoupled_weight_decay, step, n, stream);
}

// ============================================================ averaged weights: EMA / SWA (torch.optim.swa_utils.AveragedModel)
// avg = lerp(avg, p, w) as torch evaluates it (ATen lerp: w < 0.5 ? avg + w*(p - avg) : p - (p - avg)*(1 - w)), or avg = p for the first
// update, and the in-place exchange of two flat buffers.  Both are rules of grouped_kernel above -- its LDS-staged segment lookup, its pass
// shape (one float4 per lane, OPT_VEC in flight, every load issued before the first store), no atomics -- in which `p` is the average and
// `g` the parameters (RuleEma), or `p` and `s0` the two buffers and no `g` at all (RuleSwap).  Every group id 0..7 counts alike: only
// frozen vectors and vectors behind the table's end are skipped, in every buffer.
struct EmaParams { float w; int copy, hi; };

__device__ __forceinline__ void ema_elem(float& a, float p, const EmaParams& q) {
    if (q.copy) a = p;
    else a = q.hi ? p - (p - a) * (1.f - q.w) : a + q.w * (p - a);
}

struct RuleEma {
    using Params = EmaParams;
    static constexpr int NS = 0;
    static constexpr bool GRAD = true;
    static __device__ __forceinline__ void scale(Params&, float) {}
    static __device__ __forceinline__ bool reads_state(const Params&) { return false; }
    static __device__ __forceinline__ void elem(float& a, float p, float&, float&, const Params& q) { ema_elem(a, p, q); }
};
struct RuleSwap {                                       // bits are moved, never computed
    using Params = int;
    static constexpr int NS = 1;
    static constexpr bool GRAD = false;
    static __device__ __forceinline__ void scale(Params&, float) {}
    static __device__ __forceinline__ bool reads_state(const Params&) { return true; }
    static __device__ __forceinline__ void elem(float& a, float, float& b, float&, const Params&) { const float t = a; a = b; b = t; }
};

static int segments_check(const char* what, const void* a, const void* b, const uint32_t* seg_end, const int32_t* seg_group, int n_seg, size_t n) {
    if (!a || !b) BDN_FAIL(BDN_E_ARG, "%s: null pointer", what);
    if (n_seg < 0 || n_seg > OPT_MAX_SEGS) BDN_FAIL(BDN_E_ARG, "%s: %d segments (0..%d; 0: no table, every vector counts)", what, n_seg, OPT_MAX_SEGS);
    if (n_seg > 0 && (!seg_end || !seg_group)) BDN_FAIL(BDN_E_ARG, "%s: null pointer (segment table of %d segments)", what, n_seg);
    if (((uintptr_t)a | (uintptr_t)b) & 15) BDN_FAIL(BDN_E_ARG, "%s: buffers must be 16-byte aligned", what);
    if (n_seg > 0 && (((uintptr_t)seg_end | (uintptr_t)seg_group) & 3)) BDN_FAIL(BDN_E_ARG, "%s: segment table must be 4-byte aligned", what);
    if (n % 4 != 0 || n / 4 > 0xffffffffull)
        BDN_FAIL(BDN_E_ARG, "%s: n = %zu must be a multiple of 4 (tensors padded to a float4) below 2^34", what, n);
    return BDN_OK;
}

static int ema_params(const char* what, float weight, int copy, EmaParams& q) {
    if (!(weight >= 0.f && weight <= 1.f)) BDN_FAIL(BDN_E_ARG, "%s: weight = %g must lie in [0, 1]", what, (double)weight);
    if (copy != 0 && copy != 1) BDN_FAIL(BDN_E_ARG, "%s: copy must be 0 or 1, got %d", what, copy);
    q = EmaParams{weight, copy, weight >= 0.5f ? 1 : 0};
    return BDN_OK;
}

extern "C" int bdn_ema_update(float* avg, const float* params, const uint32_t* seg_end, const int32_t* seg_group, int n_seg, float weight,
                              int copy, size_t n, void* stream) {
    if (int rc = segments_check("ema_update", avg, params, seg_end, seg_group, n_seg, n)) return rc;
    EmaParams q;
    if (int rc = ema_params("ema_update", weight, copy, q)) return rc;
    if (n == 0) return BDN_OK;
    GroupArgs<EmaParams> a{};
    for (int k = 0; k < OPT_MAX_GROUPS; k++) a.g[k] = q;
    const SegTable t{seg_end, seg_group, n_seg, OPT_MAX_GROUPS};
    hipLaunchKernelGGL(grouped_kernel<RuleEma>, dim3(opt_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, avg, params, (float*)nullptr,
                       (float*)nullptr, t, a, (const float*)nullptr, n / 4);
    BDN_CHECK_LAUNCH("ema_update");
    return BDN_OK;
}

extern "C" int bdn_swap_segments(float* a, float* b, const uint32_t* seg_end, const int32_t* seg_group, int n_seg, size_t n, void* stream) {
    if (int rc = segments_check("swap_segments", a, b, seg_end, seg_group, n_seg, n)) return rc;
    if (a == b) BDN_FAIL(BDN_E_ARG, "swap_segments: a and b are the same buffer");
    if (n == 0) return BDN_OK;
    const SegTable t{seg_end, seg_group, n_seg, OPT_MAX_GROUPS};
    hipLaunchKernelGGL(grouped_kernel<RuleSwap>, dim3(opt_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, a, (const float*)nullptr, b,
                       (float*)nullptr, t, GroupArgs<int>{}, (const float*)nullptr, n / 4);
    BDN_CHECK_LAUNCH("swap_segments");
    return BDN_OK;
}

// The same rule over a device table of small tensors (the BatchNorm running statistics) in one launch: block row y owns tensor y and
// grid-strides it, a float4 body where both pointers are 16-byte aligned and one element per lane for the rest.
struct EmaDesc { float* avg; const float* src; int len, pad_; };
constexpr int EMA_MULTI_MAX_BLOCKS = 64;

__global__ void __launch_bounds__(256) ema_multi_kernel(const EmaDesc* __restrict__ desc, EmaParams q) {
    const EmaDesc d = desc[blockIdx.y];
    const int stride = gridDim.x * 256, tid = blockIdx.x * 256 + threadIdx.x;
    const int n4 = ((((uintptr_t)d.avg | (uintptr_t)d.src) & 15) == 0 && d.len > 0) ? d.len / 4 : 0;
    for (int i = tid; i < n4; i += stride) {
        float4 a = reinterpret_cast<float4*>(d.avg)[i];
        const float4 p = reinterpret_cast<const float4*>(d.src)[i];
        ema_elem(a.x, p.x, q); ema_elem(a.y, p.y, q); ema_elem(a.z, p.z, q); ema_elem(a.w, p.w, q);
        reinterpret_cast<float4*>(d.avg)[i] = a;
    }
    for (int i = n4 * 4 + tid; i < d.len; i += stride) {
        float a = d.avg[i];
        ema_elem(a, d.src[i], q);
        d.avg[i] = a;
    }
}

extern "C" int bdn_ema_update_multi(const void* desc_dev, int n_tensors, int max_len, float weight, int copy, void* stream) {
    if (!desc_dev) BDN_FAIL(BDN_E_ARG, "ema_update_multi: null pointer");
    if ((uintptr_t)desc_dev & 7) BDN_FAIL(BDN_E_ARG, "ema_update_multi: the descriptor table must be 8-byte aligned");
    if (n_tensors < 0 || n_tensors > 65535 || max_len < 0) BDN_FAIL(BDN_E_SHAPE, "ema_update_multi: n_tensors=%d (0..65535) max_len=%d", n_tensors, max_len);
    EmaParams q;
    if (int rc = ema_params("ema_update_multi", weight, copy, q)) return rc;
    if (n_tensors == 0 || max_len == 0) return BDN_OK;
    const int want = (max_len + 1023) / 1024;
    hipLaunchKernelGGL(ema_multi_kernel, dim3(want < EMA_MULTI_MAX_BLOCKS ? want : EMA_MULTI_MAX_BLOCKS, n_tensors), dim3(256), 0,
                       (hipStream_t)stream, static_cast<const EmaDesc*>(desc_dev), q);
    BDN_CHECK_LAUNCH("ema_update_multi");
    return BDN_OK;
}

// ============================================================ gradient accumulation and the global gradient norm (clip_grad_norm_)
// Two memory-bound passes on the path between backward and the update, in the update kernels' shape (float4, OPT_VEC loads in flight).
//
// bdn_grad_accumulate: dst = src (add = 0) or dst = dst + src (add = 1), one IEEE float32 add per element; a micro-step's gradients go
// into the accumulator, the last micro-step's come out of it, and no zero-fill is ever needed.
//
// bdn_grad_norm: out[0] = grad_scale * sqrt(sum g^2) over the vectors that count, out[1] = torch's clip coefficient of it.  Every float32
// is converted to double before it is squared and everything is accumulated in double (a square neither overflows nor underflows; the
// sum of 2^32 vectors errs by ~n 2^-53).  Stage 1: block b owns the NORM_CHUNK consecutive vectors [b NORM_CHUNK, (b + 1) NORM_CHUNK) --
// the block count is a function of n alone -- each lane sums its vectors in index order, a wave64 butterfly (__shfl_xor, the same tree in
// every wave) sums the lanes, thread 0 adds the four wave sums in wave order and writes ONE double.  Stage 2: one thread adds the partials
// in index order (staged through LDS 1024 at a time) and forms norm and coefficient.  No atomics, no memset, the same bits on any device.
// With a segment table (the update kernels') a vector of a frozen segment, or behind the table's end, is not read.
__device__ __forceinline__ float4 add4(const float4& a, const float4& b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// A pass whose OPT_VEC vectors are all in range issues its loads without a bounds test (named registers: hipcc moved a conditionally
// loaded float4[OPT_VEC] of the copy form into LDS and waited for every load in turn); the last, partial pass goes vector by vector.
template <bool ADD>
__global__ void __launch_bounds__(256) grad_accumulate_kernel(float* __restrict__ dst, const float* __restrict__ src, size_t n4, size_t n) {
    static_assert(OPT_VEC == 4, "four loads in flight, written out");
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(src);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(dst);
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t base = (size_t)blockIdx.x * 256 + threadIdx.x; base < n4; base += stride * OPT_VEC) {
        if (base + 3 * stride < n4) {
            float4 a0 = s4[base], a1 = s4[base + stride], a2 = s4[base + 2 * stride], a3 = s4[base + 3 * stride];
            if (ADD) {
                const float4 c0 = d4[base], c1 = d4[base + stride], c2 = d4[base + 2 * stride], c3 = d4[base + 3 * stride];
                a0 = add4(c0, a0); a1 = add4(c1, a1); a2 = add4(c2, a2); a3 = add4(c3, a3);
            }
            d4[base] = a0; d4[base + stride] = a1; d4[base + 2 * stride] = a2; d4[base + 3 * stride] = a3;
        } else {
            for (size_t i = base; i < n4; i += stride) {
                float4 v = s4[i];
                if (ADD) v = add4(d4[i], v);
                d4[i] = v;
            }
        }
    }
    if (blockIdx.x == 0 && threadIdx.x < n - n4 * 4) {       // the n % 4 trailing elements
        const size_t k = n4 * 4 + threadIdx.x;
        dst[k] = ADD ? dst[k] + src[k] : src[k];
    }
}

extern "C" int bdn_grad_accumulate(float* dst, const float* src, size_t n, int add, void* stream) {
    if (!dst || !src) BDN_FAIL(BDN_E_ARG, "grad_accumulate: null pointer");
    if (((uintptr_t)dst | (uintptr_t)src) & 15) BDN_FAIL(BDN_E_ARG, "grad_accumulate: buffers must be 16-byte aligned");
    if (add != 0 && add != 1) BDN_FAIL(BDN_E_ARG, "grad_accumulate: add must be 0 or 1, got %d", add);
    if (n == 0) return BDN_OK;
    const size_t n4 = n / 4;
    if (add) hipLaunchKernelGGL(grad_accumulate_kernel<true>, dim3(opt_grid(n4)), dim3(256), 0, (hipStream_t)stream, dst, src, n4, n);
    else hipLaunchKernelGGL(grad_accumulate_kernel<false>, dim3(opt_grid(n4)), dim3(256), 0, (hipStream_t)stream, dst, src, n4, n);
    BDN_CHECK_LAUNCH("grad_accumulate");
    return BDN_OK;
}

constexpr int NORM_ROUNDS = 4;                                   // passes of OPT_VEC float4s per thread
constexpr size_t NORM_CHUNK = (size_t)256 * OPT_VEC * NORM_ROUNDS;   // vectors per block and per partial: 4096 (64 KiB of gradients)

static inline size_t norm_blocks(size_t n4) { return (n4 + NORM_CHUNK - 1) / NORM_CHUNK; }

__device__ __forceinline__ double sq_acc(double acc, const float4& v) {
    const double x = (double)v.x, y = (double)v.y, z = (double)v.z, w = (double)v.w;
    acc = fma(x, x, acc); acc = fma(y, y, acc); acc = fma(z, z, acc); acc = fma(w, w, acc);
    return acc;
}

__global__ void __launch_bounds__(256) grad_norm_partial_kernel(const float* __restrict__ g, const uint32_t* __restrict__ seg_end,
                                                                const int32_t* __restrict__ seg_group, int n_seg,
                                                                double* __restrict__ part, size_t n4) {
    __shared__ uint32_t s_end[OPT_MAX_SEGS];
    __shared__ int s_grp[OPT_MAX_SEGS];
    __shared__ double s_wave[4];
    int cap = 1;
    if (n_seg > 0) {
        while (cap < n_seg) cap <<= 1;
        for (int k = threadIdx.x; k < cap; k += 256) {
            s_end[k] = k < n_seg ? seg_end[k] : 0xffffffffu;
            s_grp[k] = k < n_seg ? seg_group[k] : OPT_FROZEN;
        }
        __syncthreads();
    }
    const size_t c0 = (size_t)blockIdx.x * NORM_CHUNK;
    // A block's 4096 consecutive vectors almost always lie in one segment: one lookup of its first and of its last vector then serves the
    // block (a frozen block reads nothing at all); a block that spans a boundary looks every vector up.  The sums are the same either way.
    bool per_lane = false, whole = true;
    if (n_seg > 0) {
        const size_t last = (c0 + NORM_CHUNK < n4 ? c0 + NORM_CHUNK : n4) - 1;
        int s_lo = 0, s_hi = 0;
        for (int h = cap >> 1; h > 0; h >>= 1) { seg_step(s_end, h, (uint32_t)c0, s_lo); seg_step(s_end, h, (uint32_t)last, s_hi); }
        per_lane = s_lo != s_hi;
        whole = s_end[s_lo] > last && s_grp[s_lo] != OPT_FROZEN;
    }
    double acc = 0.0;
    for (int r = 0; r < NORM_ROUNDS; r++) {
        bool take[OPT_VEC];
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = c0 + (size_t)(r * OPT_VEC + u) * 256 + threadIdx.x;
            take[u] = i < n4 && (per_lane || whole);
            if (take[u] && per_lane) {                       // first segment whose end lies behind i
                int s = 0;
                for (int h = cap >> 1; h > 0; h >>= 1) seg_step(s_end, h, (uint32_t)i, s);
                take[u] = s_end[s] > i && s_grp[s] != OPT_FROZEN;
            }
        }
        float4 G[OPT_VEC] = {};
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = c0 + (size_t)(r * OPT_VEC + u) * 256 + threadIdx.x;
            if (take[u]) G[u] = reinterpret_cast<const float4*>(g)[i];
        }
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) acc = sq_acc(acc, G[u]);           // a vector not taken adds +0.0: the sum is unchanged
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) acc += __shfl_xor(acc, m);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

__global__ void __launch_bounds__(256) grad_norm_finish_kernel(const double* __restrict__ part, size_t nblk, float grad_scale, float max_norm,
                                                               float* __restrict__ out) {
    __shared__ double s_part[1024];
    double sum = 0.0;
    for (size_t b0 = 0; b0 < nblk; b0 += 1024) {
        const size_t m = nblk - b0 < 1024 ? nblk - b0 : 1024;
        for (size_t k = threadIdx.x; k < m; k += 256) s_part[k] = part[b0 + k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (size_t k = 0; k < m; k++) sum += s_part[k];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float norm32 = (float)((double)grad_scale * sqrt(sum));
        // torch.nn.utils.clip_grad_norm_: clamp(max_norm / (norm + 1e-6), max = 1), the quotient as torch evaluates a Python float over a
        // tensor (Tensor.__rtruediv__): reciprocal, then product
        float coef = (1.0f / (norm32 + 1e-6f)) * max_norm;
        if (coef > 1.0f) coef = 1.0f;                        // a comparison, not fminf: a NaN norm keeps its NaN coefficient
        out[0] = norm32;
        out[1] = coef;
    }
}

extern "C" size_t bdn_grad_norm_workspace_bytes(size_t n) {
    const size_t nb = norm_blocks(n / 4);
    return ((nb ? nb : 1) * sizeof(double) + 15) / 16 * 16;
}

extern "C" int bdn_grad_norm(const float* grads, const uint32_t* seg_end, const int32_t* seg_group, int n_seg, float grad_scale,
                             float max_norm, void* workspace, float* out, size_t n, void* stream) {
    if (!grads || !workspace || !out) BDN_FAIL(BDN_E_ARG, "grad_norm: null pointer");
    if (n_seg < 0 || n_seg > OPT_MAX_SEGS) BDN_FAIL(BDN_E_ARG, "grad_norm: %d segments (0..%d; 0: no table, every element counts)", n_seg, OPT_MAX_SEGS);
    if (n_seg > 0 && (!seg_end || !seg_group)) BDN_FAIL(BDN_E_ARG, "grad_norm: null pointer (segment table of %d segments)", n_seg);
    if ((uintptr_t)grads & 15) BDN_FAIL(BDN_E_ARG, "grad_norm: buffers must be 16-byte aligned");
    if ((uintptr_t)workspace & 7) BDN_FAIL(BDN_E_ARG, "grad_norm: workspace must be 8-byte aligned");
    if ((uintptr_t)out & 3) BDN_FAIL(BDN_E_ARG, "grad_norm: out must be 4-byte aligned");
    if (n_seg > 0 && (((uintptr_t)seg_end | (uintptr_t)seg_group) & 3)) BDN_FAIL(BDN_E_ARG, "grad_norm: segment table must be 4-byte aligned");
    if (n % 4 != 0 || n / 4 > 0xffffffffull)
        BDN_FAIL(BDN_E_ARG, "grad_norm: n = %zu must be a multiple of 4 (tensors padded to a float4) below 2^34", n);
    if (!(max_norm >= 0.f)) BDN_FAIL(BDN_E_ARG, "grad_norm: max_norm = %g must be >= 0 (+inf: measure only)", (double)max_norm);
    const size_t n4 = n / 4, nblk = norm_blocks(n4);
    if (nblk) {
        hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, grads, seg_end, seg_group, n_seg,
                           (double*)workspace, n4);
        BDN_CHECK_LAUNCH("grad_norm");
    }
    hipLaunchKernelGGL(grad_norm_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)workspace, nblk, grad_scale, max_norm, out);
    BDN_CHECK_LAUNCH("grad_norm_finish");
    return BDN_OK;
}

// ============================================================ misc
static thread_local char g_err[512] = "";
void bdn_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
extern "C" const char* bdn_last_error(void) { return g_err; }
extern "C" int bdn_version(void) { return 1; }

// ============================================================ streams of the training step
// The step runs on THREE HIP streams per device -- the dependency chain (high priority), the weight-gradient GEMMs, the host -> device
// copies -- which must sit on three distinct hardware queues: two streams that share a queue serialise, and the step is 8-14 %
// slower (round 2: successive TrainStep instances took whatever the next pool streams of the host framework were, and some of those
// share a queue).  The library creates them itself, once per role, so their placement does not depend on how many streams the host
// program created before.  priority: 0 = normal, 1 = high (mapped onto hipDeviceGetStreamPriorityRange).
extern "C" int bdn_stream_create(int priority, void** stream_out) {
    if (!stream_out) BDN_FAIL(BDN_E_ARG, "stream_create: null pointer");
    if (priority != 0 && priority != 1) BDN_FAIL(BDN_E_ARG, "stream_create: priority must be 0 (normal) or 1 (high)");
    int least = 0, greatest = 0;
    hipError_t e = hipDeviceGetStreamPriorityRange(&least, &greatest);
    if (e != hipSuccess) BDN_FAIL(BDN_E_HIP, "stream_create: hipDeviceGetStreamPriorityRange: %s", hipGetErrorString(e));
    hipStream_t s = nullptr;
    e = hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority ? greatest : 0);
    if (e != hipSuccess) BDN_FAIL(BDN_E_HIP, "stream_create: hipStreamCreateWithPriority: %s", hipGetErrorString(e));
    *stream_out = reinterpret_cast<void*>(s);
    return BDN_OK;
}

extern "C" int bdn_stream_destroy(void* stream) {
    if (!stream) BDN_FAIL(BDN_E_ARG, "stream_destroy: null pointer");
    const hipError_t e = hipStreamDestroy(reinterpret_cast<hipStream_t>(stream));
    if (e != hipSuccess) BDN_FAIL(BDN_E_HIP, "stream_destroy: %s", hipGetErrorString(e));
    return BDN_OK;
}

// Events for stream-to-stream hand-offs on ONE device (the chain releases a layer's weight-gradient GEMM to the second stream 17 times
// per backward).  Created with hipEventDisableTiming | hipEventDisableSystemFence: the default event performs a SYSTEM-scope release
// when it is recorded -- a cache write-back / invalidate that makes device memory visible to the host and to other devices -- which
// showed as a 6.5 us bubble on the recording stream at every hand-off; a consumer stream on the same device needs none of it.
// NOT for host-side synchronisation (hipEventSynchronize on such an event does not make device writes visible to the host).
extern "C" int bdn_event_create(void** event_out) {
    if (!event_out) BDN_FAIL(BDN_E_ARG, "event_create: null pointer");
    hipEvent_t e = nullptr;
    const hipError_t rc = hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventDisableSystemFence);
    if (rc != hipSuccess) BDN_FAIL(BDN_E_HIP, "event_create: %s", hipGetErrorString(rc));
    *event_out = reinterpret_cast<void*>(e);
    return BDN_OK;
}
extern "C" int bdn_event_destroy(void* event) {
    if (!event) BDN_FAIL(BDN_E_ARG, "event_destroy: null pointer");
    const hipError_t rc = hipEventDestroy(reinterpret_cast<hipEvent_t>(event));
    if (rc != hipSuccess) BDN_FAIL(BDN_E_HIP, "event_destroy: %s", hipGetErrorString(rc));
    return BDN_OK;
}
// record `event` on `stream`, resp. make `stream` wait for the event's most recent record (both asynchronous)
extern "C" int bdn_event_record(void* event, void* stream) {
    if (!event) BDN_FAIL(BDN_E_ARG, "event_record: null pointer");
    const hipError_t rc = hipEventRecord(reinterpret_cast<hipEvent_t>(event), reinterpret_cast<hipStream_t>(stream));
    if (rc != hipSuccess) BDN_FAIL(BDN_E_HIP, "event_record: %s", hipGetErrorString(rc));
    return BDN_OK;
}
extern "C" int bdn_stream_wait_event(void* stream, void* event) {
    if (!event) BDN_FAIL(BDN_E_ARG, "stream_wait_event: null pointer");
    const hipError_t rc = hipStreamWaitEvent(reinterpret_cast<hipStream_t>(stream), reinterpret_cast<hipEvent_t>(event), 0);
    if (rc != hipSuccess) BDN_FAIL(BDN_E_HIP, "stream_wait_event: %s", hipGetErrorString(rc));
    return BDN_OK;
}
