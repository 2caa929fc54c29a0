/*
 * bidate_hip.h -- C ABI of libbidate_hip.so: hand-written gfx950 (MI355X / CDNA4)
 * kernels for the bi-date Siamese U-Net training path of granularai/fabric.
 *
 * The reference has no FFI: its hot path is a set of ATen call sites reached from
 * Python.  Each entry point below names the reference call site(s)
 * (file:line relative to the reference root) whose arithmetic it replaces.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (PyTorch caching
 *     allocator); the library never allocates, frees or synchronises;
 *   - every call enqueues on `stream` (a hipStream_t passed as void*) and returns;
 *   - return value: 0 = ok, negative = error (BDN_E_*); bdn_last_error() gives a
 *     thread-local message.  No C++ exception crosses the boundary;
 *   - activations are NHWC; `dtype` selects the element type of activations and
 *     packed weights: BDN_F32 (f32 storage, v_mfma_f32_32x32x2_f32: the
 *     "fp32-equivalent" parity setting) or BDN_BF16 (bf16 storage,
 *     v_mfma_f32_32x32x16_bf16, fp32 accumulate: the throughput setting);
 *   - BatchNorm statistics are kept per *group* (= date): images
 *     [g*imgs_per_group, (g+1)*imgs_per_group) of a batch form group g
 *     (models/bidate_model.py:23-33 runs the shared BN modules once per date).
 */
#ifndef BIDATE_HIP_H
#define BIDATE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum { BDN_F32 = 0, BDN_BF16 = 1, BDN_BF16X3 = 2,     /* BDN_BF16X3: float32 tensors, GEMM operands split into bf16 hi + lo (3 MFMAs per product) */
       BDN_BF16X2 = 3 };  /* the BACKWARD GEMMs of the bf16x3 setting with two of the three terms, on the same operands and filter images as
                           * BDN_BF16X3 -- bdn_conv3x3 / bdn_conv3x3_dgrad_bs (data gradient): K = [dz_hi | dz_lo] against [w_hi | w_hi], i.e. the
                           * filter rounded to bf16, dz in full; bdn_conv3x3_wgrad_ex / bdn_wgrad_workspace_bytes_ex: dz_hi x [a_hi | a_lo], i.e.
                           * dz rounded, the activations in full (autograd of models/unet_parts.py:13,16 to ~1e-3 relative instead of ~2e-5).
                           * Accepted by those entry points only. */
enum { BDN_OK = 0, BDN_E_ARG = -1, BDN_E_SHAPE = -2, BDN_E_HIP = -3 };
enum { BDN_IN_PLAIN = 0, BDN_IN_BNRELU = 1 };
/* How the two dates' features of an encoder level meet in its skip (the `fusion` argument of the entry points that carry it):
 * BDN_FUSE_PRODUCT  relu(x_d2 * x_d1), the reference's models/bidate_model.py:35-38;
 * BDN_FUSE_ABSDIFF  |x_d2 - x_d1| at the same call sites (FC-Siam-diff, Daudt et al., ICIP 2018): one float32 subtraction of the two
 *                   rounded activations, the absolute value, one rounding to the storage type.  Backward: dA_d1 = dF * s,
 *                   dA_d2 = -(dF * s) with s = sign(a_d1 - a_d2) in {-1, 0, +1}; exactly 0 at a_d1 == a_d2 (torch.abs's rule). */
enum { BDN_FUSE_PRODUCT = 0, BDN_FUSE_ABSDIFF = 1 };

const char* bdn_last_error(void);
int bdn_version(void);

/* ---- streams of the training step (reference: none -- train.py:83-101 runs on PyTorch's default stream) ----
 * A HIP stream on the calling thread's current device, created by the library so that its hardware-queue placement does not
 * depend on the host framework's stream pool: the step's dependency chain (priority 1 = high), its weight-gradient GEMMs and
 * its host -> device copies (priority 0) each get one, shared by every step object of the process (fabric_amd/streams.py).
 * The caller owns the stream and destroys it with bdn_stream_destroy. */
int bdn_stream_create(int priority, void** stream_out);
int bdn_stream_destroy(void* stream);
/* Events for hand-offs between two streams of ONE device (the chain releases each layer's weight-gradient GEMM to the second stream):
 * created with hipEventDisableTiming | hipEventDisableSystemFence -- a default event performs a system-scope release (cache write-back /
 * invalidate towards the host) every time it is recorded.  Not for host-side synchronisation.  bdn_event_record(event, stream) and
 * bdn_stream_wait_event(stream, event) enqueue and return. */
int bdn_event_create(void** event_out);
int bdn_event_destroy(void* event);
int bdn_event_record(void* event, void* stream);
int bdn_stream_wait_event(void* stream, void* event);

/* ---- layout converters (boundary of BiDateNet.forward, models/bidate_model.py:22) ---- */
/* x_d1, x_d2: [B,C,H,W] f32 NCHW  ->  out: [2B,H,W,Cpad] (date-1 images first), channels >= C zeroed.
 * dtype BDN_BF16X3: out is the first convolution's split operand [2B,H,W,2 Cpad] bf16 = hi | lo (bdn_split_pack of the float32 image). */
int bdn_pack_input(int dtype, const float* x_d1, const float* x_d2, void* out,
                   int B, int C, int H, int W, int Cpad, void* stream);
/* OIHW f32 [Cout,Cin,3,3] -> forward GEMM image wf [Cout][9][Cin_pad] and the data-gradient image
 * wd [Cin_pad][9][Cout] (taps rotated by 180 degrees); either output may be NULL. */
int bdn_pack_weights(int dtype, const float* w_oihw, void* wf, void* wd,
                     int Cout, int Cin, int Cin_pad, void* stream);

/* The same for n_layers filters in one launch.  desc: DEVICE array of n_layers records
 * { const float* w_oihw; void* wf; void* wd; int32 Cout, Cin, Cin_pad, reserved; } (40 bytes each).  dtype BDN_BF16X3: the split images of
 * bdn_pack_weights(BDN_BF16X3) for every record. */
int bdn_pack_weights_multi(int dtype, const void* desc, int n_layers, void* stream);

/* ---- 3x3 convolution, stride 1, zero padding 1: nn.Conv2d(ci,co,3,padding=1), models/unet_parts.py:13,16 ----
 * Implicit GEMM on MFMA.  The A operand is gathered from in0 (channels [0,C0)) and optionally in1
 * (channels [C0,C0+C1), the never-materialised torch.cat of models/unet_parts.py:78).
 * in_mode BDN_IN_BNRELU applies relu(z*scale+shift) (BatchNorm2d+ReLU of the producing layer,
 * models/unet_parts.py:14-15,17-18) while loading in0; in_bn is that layer's [G][4][C0] f32 table
 * written by bdn_bn_finalize / bdn_bn_eval.
 * w: packed [Cout][9][C0+C1]; bias: [Cout] f32 or NULL.
 * out: [N,H,W,Cout].  stats_partial: NULL or [bdn_conv3x3_num_mtiles][2][Cout] f32 receiving
 * per-tile sum / sum-of-squares of the (bias-included, f32) outputs for the BatchNorm that follows.
 * The same entry point computes the data gradient when given wd and dz.
 * Every tensor must stay below 4 GB (the kernels address with one base + a 32-bit byte offset): BDN_E_SHAPE otherwise. */
int bdn_conv3x3(int dtype, const void* in0, int C0, const void* in1, int C1,
                int in_mode, const float* in_bn, int imgs_per_group,
                const void* w, const float* bias, void* out, float* stats_partial,
                int N, int H, int W, int Cout, void* stream);
int bdn_conv3x3_num_mtiles(int N, int H, int W, int Cout, int imgs_per_group);
/* The same by operand type: BDN_BF16X3 / BDN_BF16X2 launches with C0 (logical operand channels) a multiple of 64 run the kernels that fuse the
 * split product into one reduction (two LDS patches per chunk), which have their own tile plan; every other case equals bdn_conv3x3_num_mtiles. */
int bdn_conv3x3_num_mtiles_ex(int dtype, int N, int H, int W, int C0, int Cout, int imgs_per_group);
/* Name of the kernel instantiation bdn_conv3x3 runs for a shape, e.g. "conv3x3_kernel<bf16,128,8,16,1,128,1,4,false,bf16,false,false>"
 * (the rocprofv3 name with `unsigned short` spelled bf16); "" for an unsupported shape.  Thread-local buffer. */
const char* bdn_conv3x3_variant(int dtype, int N, int H, int W, int C0, int C1, int Cout, int imgs_per_group);
/* Test hook: while on (non-zero), every conv3x3 launch of the calling thread -- forward, data gradient, eval mode -- takes the kernels' general
 * path: no interior-tile staging, no full-tile copy-out.  Both paths compute the same bits; the tests compare
 * them.  Thread-local, off by default; returns the previous setting. */
int bdn_conv3x3_force_general(int on);

/* bf16x3 / bf16x2 convolution straight from a FLOAT32 operand (reference: models/unet_parts.py:14-16, BatchNorm -> ReLU -> Conv2d of a
 * double_conv's second half; round 6).  Equals bdn_split_pack(in, in_mode, in_bn) followed by bdn_conv3x3(dtype, ...) bit for bit, in one
 * launch: relu(z * scale + shift) and the bf16 hi / lo split are applied while the tile is staged, no split pass runs in front of the
 * convolution.  in [N,H,W,C0] float32, C0 a multiple of 64 and <= 512; w the bdn_pack_weights(BDN_BF16X3) forward image; out float32;
 * stats_partial as bdn_conv3x3 with bdn_conv3x3_num_mtiles_ex(dtype, ...) rows.
 * split_out: NULL, or [N,H,W,2 C0] bf16 that receives exactly bdn_split_pack's output (the layer's weight-gradient GEMM reads it later). */
int bdn_conv3x3_x3src(int dtype, const float* in, int C0, int in_mode, const float* in_bn, int imgs_per_group,
                      const void* w, const float* bias, float* out, float* stats_partial, void* split_out,
                      int N, int H, int W, int Cout, void* stream);
/* Name of the kernel instantiation bdn_conv3x3_x3src runs for a shape (as bdn_conv3x3_variant); "" for an unsupported shape. */
const char* bdn_conv3x3_x3src_variant(int dtype, int N, int H, int W, int C0, int Cout, int imgs_per_group);

/* Data gradient of nn.Conv2d(ci,co,3,padding=1) (autograd of models/unet_parts.py:13,16) with the BatchNorm-backward
 * statistics of the PRODUCING layer fused into the epilogue: dz [N,H,W,C0] x rotated filter image w_dgrad ->
 * dA [N,H,W,Cout] (gradient wrt relu(bn(z_prev))), and bs_partial [bdn_conv3x3_num_mtiles(N,H,W,Cout,ipg)][2][Cout] =
 * per-tile sum g, sum g*z_prev with g = dA * [scale*z_prev + shift > 0] (z_prev [N,H,W,Cout], bn_prev [G][4][Cout]).
 * What is STORED to dA is g, the masked gradient (zero where relu(bn(z_prev)) is off): every BatchNorm-backward consumer applies the
 * same mask again (idempotent), and bdn_conv3x3_dgrad_bb expects it.  The same holds for bdn_enc_skip_bwd (with bs_partial) and
 * bdn_upsample2x_bwd_bs.  Tiles are image-major, so a statistic group owns num_mtiles/G consecutive rows: feed bdn_bn_bwd_apply(raw_moment=1). */
int bdn_conv3x3_dgrad_bs(int dtype, const void* dz, int C0, const void* w_dgrad, void* dA,
                         const void* z_prev, const float* bn_prev, int imgs_per_group, float* bs_partial,
                         int N, int H, int W, int Cout, void* stream);

/* Data gradient of layer L's convolution with L's BatchNorm+ReLU backward (autograd of models/unet_parts.py:14-15,17-18) applied while the
 * operand is staged: dA [N,H,W,C0] = the MASKED gradient g = dA*[scale z + shift > 0] as the fused producers store it (see
 * bdn_conv3x3_dgrad_bs), z [N,H,W,C0], bn [G][4][C0], sums [G][2][C0] from bdn_bn_bwd_finalize; the kernel forms
 * dz = a g + b z + c with a = scale, b = -scale invstd s1/M, c = -scale s0/M - b mean (= bdn_bn_bwd_apply's scale*(g - s0/M - xhat*s1/M)
 * up to rounding: two FMAs per element, three per-channel constants, no compare), convolves it with w_dgrad into dA_prev [N,H,W,Cout]
 * and stores dz [N,H,W,C0] to dz_out (NULL: not stored) for the weight-gradient GEMM -- bdn_bn_bwd_apply's pass over dA, z and dz does
 * not run.  z_prev / bn_prev / bs_partial: as bdn_conv3x3_dgrad_bs, or all NULL.
 * bf16, C0 = 64 (a single channel chunk: the staging then runs once, in the kernel's prologue), maps larger than 8x8. */
int bdn_conv3x3_dgrad_bb(int dtype, const void* dA, int C0, const void* z, const float* bn, const float* sums, int imgs_per_group,
                         const void* w_dgrad, void* dA_prev, const void* z_prev, const float* bn_prev, float* bs_partial,
                         void* dz_out, int N, int H, int W, int Cout, void* stream);

/* Name of the kernel instantiation bdn_conv3x3_dgrad_bb runs for a shape (its dispatcher picks its own tile configurations); "" for an
 * unsupported shape.  Thread-local buffer, as bdn_conv3x3_variant. */
const char* bdn_conv3x3_dgrad_bb_variant(int N, int H, int W, int Cout, int imgs_per_group);

/* ---- 3x3x3 convolution, stride 1, zero padding 1 (BASELINE configs[3]: the multi-date 3-D U-Net stack) ----
 * The reference tree holds NO source for that model (UNetLSTM/ is an empty sub-module, README.md:5): parity is UNPINNED, the
 * oracle is torch.nn.functional.conv3d.  Implicit GEMM with K = 27 Cin on the 2-D kernels: tensors are [N,D,H,W,C] (the D
 * slices of a sample are consecutive NHWC images), a 3x3x3 window is three 3x3 windows on slices d-1, d, d+1 = three sources
 * of one reduction, a slice outside the sample is a zero mask.  No depth padding, no im2col.
 *   w      bdn_pack_weights image (wf) of the OIHW view [Cout][3 C][3][3] whose input channel kd*C + c holds w3d[co][c][kd][.][.]
 *          (data gradient: the same entry point on dz with the view [C][3 Cout][3][3], channel s*Cout + co = w3d[co][c][2-s][2-kh][2-kw])
 *   in_mode / in_bn / stats_partial / bias as in bdn_conv3x3; imgs_per_group counts samples;
 *   stats_partial rows: bdn_conv3d_num_mtiles(N, D, H, W).  dtype: BDN_BF16, BDN_F32, or BDN_BF16X3 (round 4) -- then `in` is the bf16
 *   operand [N,D,H,W,C] whose C = 3 x the logical width holds [hi | lo | hi] of the float32 tensor (bdn_split_pack's [hi | lo] plus its hi
 *   half again), `w` the plain BDN_BF16 image of the view with channels [w_hi | w_hi | w_lo] per depth tap, in_mode PLAIN, out float32.
 * bdn_conv3d_wgrad: dw [Cout][Cin_real][3][3][3] f32 from dz [N,D,H,W,Cout] and the PLAIN input [N,D,H,W,C];
 *   partial: bdn_wgrad_workspace_bytes_ex(dtype, N*D, H, W, Cout, C, 0, 1, BDN_IN_PLAIN, 0) bytes.
 *   BDN_BF16X3: dz [N,D,H,W,2 Cout] and in [N,D,H,W,2 C] are bdn_split_pack operands; partial: the BDN_BF16 size for (2 Cout, 2 C) plus
 *   4*Cout*C*27 floats (the doubled-operand tile the three quadrants are summed from). */
int bdn_conv3d_num_mtiles(int N, int D, int H, int W);
int bdn_conv3d(int dtype, const void* in, int C, int in_mode, const float* in_bn, int imgs_per_group,
               const void* w, const float* bias, void* out, float* stats_partial,
               int N, int D, int H, int W, int Cout, void* stream);
int bdn_conv3d_wgrad(int dtype, const void* dz, int Cout, const void* in, int C,
                     float* partial, float* dw_oidhw, int Cin_real, int N, int D, int H, int W, void* stream);

/* ---- bf16x3 operand split (dtype BDN_BF16X3 of bdn_conv3x3 / bdn_conv3x3_dgrad_bs / bdn_conv3x3_wgrad* / bdn_pack_weights) ----
 * The 1e-3-parity setting at matrix-core speed: tensors stay float32; a GEMM operand x is fed as hi = bf16(x) and
 * lo = bf16(x - hi) and a product keeps a_hi*w_hi + a_lo*w_hi + a_hi*w_lo (float32 accumulate).  bdn_split_pack builds the
 * operand every BDN_BF16X3 entry point expects: out [N,H,W,2(C0+C1)] bf16 = hi(a) | lo(a), a = cat(src0, src1) (f32 NHWC;
 * src1 may be NULL) with relu(bn(.)) applied to src0 when in_mode == BDN_IN_BNRELU (models/unet_parts.py:14-15,78).
 * With BDN_BF16X3: bdn_conv3x3 takes in0 = that tensor, C0 = the logical channel count, in1 = NULL, in_mode PLAIN, w from
 * bdn_pack_weights(BDN_BF16X3) (wf: [Cout][9][3 Cin_pad] bf16, wd: [Cin_pad][9][3 Cout]), and writes float32 out / statistics;
 * bdn_conv3x3_wgrad* take dz and in0 both split-packed and write the float32 OIHW gradient.
 * Rounding: hi and lo are round-to-nearest-even conversions (ties to the even bf16 mantissa, carries into the next binade included);
 * float32 subnormals are NOT flushed -- they convert to bf16 subnormals and x - hi is formed with subnormals kept -- and the sign of a
 * zero survives: the output equals torch's CPU conversion bit for bit on every finite input (tests/test_gpu_conditioning.py, E).  The
 * same holds for bdn_pack_input and bdn_pack_weights.  With BDN_IN_BNRELU an input that is off is stored as +0.0. */
int bdn_split_pack(const float* src0, int C0, const float* src1, int C1, int in_mode, const float* in_bn,
                   int imgs_per_group, void* out, int N, int H, int W, void* stream);

/* ---- weight gradient of the same convolution (autograd of models/unet_parts.py:13,16) ----
 * dz: [N,H,W,Cout]; inputs as in bdn_conv3x3.  partial: workspace of bdn_wgrad_workspace_bytes().
 * dw_oihw: f32 [Cout,Cin_real,3,3] (overwritten; channels >= Cin_real of a padded input are dropped).
 * bdn_wgrad_workspace_bytes is pure: it covers every dtype / source split / input mode of the shape under default flags. */
size_t bdn_wgrad_workspace_bytes(int N, int H, int W, int Cout, int Cin, int imgs_per_group);
int bdn_conv3x3_wgrad(int dtype, const void* dz, int Cout,
                      const void* in0, int C0, const void* in1, int C1,
                      int in_mode, const float* in_bn, int imgs_per_group,
                      float* partial, float* dw_oihw, int Cin_real,
                      int N, int H, int W, void* stream);
/* The same with a per-call `flags` word (there is no process-wide tuning state):
 *   bits 0-1   phases: bit 0 = split-K GEMM into `partial`, bit 1 = fixed-order reduction into dw_oihw (a profiler can
 *              bracket the GEMM alone by issuing the phases apart);
 *   bits 8-11  kernel override (0 = the library's choice): BDN_WG_SIMPLE forces the one-chunk-at-a-time kernel
 *              (bdn_conv3x3_wgrad_variant says what a call will run: BDN_WG_SIMPLE or BDN_WG_ROLE);
 *   bits 16-28 target number of blocks of the GEMM (0 = default 128: half the CUs, the GEMM shares the chip with the dz chain).
 * With non-default flags `partial` must hold bdn_wgrad_workspace_bytes_ex(same arguments).  Results are deterministic
 * for fixed flags; different plans differ only in the summation order of the partial tiles. */
#define BDN_WG_SIMPLE 1      /* one-chunk-at-a-time kernel (any dtype, first layer, 8x8 maps) */
#define BDN_WG_ROLE   5      /* role-split bf16 kernel (64-channel tiles, 8x16 spatial tiles): four MFMA waves fed by four staging waves --
                                dz tile by LDS-DMA, halo patch by LDS-DMA (plain) or through registers with BatchNorm+ReLU on load; 3 LDS buffers.
                                (2-4 were the round-1/2 kernels it replaced: tools/experimental/wgrad_v2_v6.hip.inc) */
#define BDN_WG_FLAGS(phases, kernel, blocks) ((phases) | ((kernel) << 8) | ((blocks) << 16))
size_t bdn_wgrad_workspace_bytes_ex(int dtype, int N, int H, int W, int Cout, int C0, int C1, int imgs_per_group,
                                    int in_mode, int flags);
int bdn_conv3x3_wgrad_ex(int dtype, const void* dz, int Cout,
                         const void* in0, int C0, const void* in1, int C1,
                         int in_mode, const float* in_bn, int imgs_per_group,
                         float* partial, float* dw_oihw, int Cin_real,
                         int N, int H, int W, int flags, void* stream);
int bdn_conv3x3_wgrad_variant(int dtype, int N, int H, int W, int Cout, int C0, int C1, int imgs_per_group,
                              int in_mode, int flags);
/* The kernels bdn_conv3x3_wgrad_ex launches for these arguments and this flags word, '+'-joined in launch order, e.g.
 * "wgrad7_kernel<true>+wgrad_reduce_kernel<8>" or "wgrad_kernel<bf16,8,8,2,false>+wgrad_reduce_kernel<1>+wgrad_x3_combine_kernel":
 * the entry point's own code path with the launches replaced by their names (host only, no device needed), so the GEMM instantiation,
 * the bf16x3 / bf16x2 route (fused wgrad7x_kernel or doubled operands + combine) and the split lanes of the reduction all come from the
 * code that launches.  Phase bits as in `flags` (1: the GEMM alone; 2: the reduction, and the combine where there is one; 0 is read as
 * 3).  "" where bdn_conv3x3_wgrad_ex refuses the arguments.  The string is thread-local and valid until the thread's next query. */
const char* bdn_conv3x3_wgrad_kernels(int dtype, int N, int H, int W, int Cout, int C0, int C1, int imgs_per_group,
                                      int in_mode, int flags);
/* Weight gradient of the FIRST convolution (inc.conv.conv.0, models/unet_parts.py:13 via unet_model.py inconv) with the
 * BatchNorm+ReLU backward of its own output (unet_parts.py:14-15) fused into the staging: the layer has no data gradient,
 * so dz = bn_bwd(dA, z) is never written -- the kernel reads dA [N,H,W,ldA>=64] and z [N,H,W,64], applies
 * bdn_bn_bwd_apply's expression with `sums` from bdn_bn_bwd_finalize, rounds to bf16 and multiplies with the input patches
 * in0 [N,H,W,16].  The result equals bdn_bn_bwd_apply + bdn_conv3x3_wgrad up to the summation order of the partial tiles.
 * Shape class: Cout = 64, C0 = 16 (bdn_conv3x3_wgrad_bnbwd_supported); partial: bdn_wgrad_workspace_bytes().
 * dtype BDN_BF16X3 / BDN_BF16X2 (round 6): dA [N,H,W,ldA] and z [N,H,W,64] float32, in0 = the input's split operand [N,H,W,32] bf16 =
 * hi(16) | lo(16) (bdn_pack_input(BDN_BF16X3) / bdn_split_pack); dz is formed in float32, split into bf16 hi + lo inside the staging and the
 * three (two: dz rounded) terms of the split product go into one accumulator: equals bdn_bn_bwd_apply_split + bdn_conv3x3_wgrad(dtype) up to
 * summation order, without the pass over dA and z and without the split dz. */
int bdn_conv3x3_wgrad_bnbwd_supported(int dtype, int N, int H, int W, int Cout, int C0, int imgs_per_group);
int bdn_conv3x3_wgrad_bnbwd(int dtype, const void* dA, int ldA, const void* z, const float* bn, const float* sums,
                            int imgs_per_group, int Cout, const void* in0, int C0,
                            float* partial, float* dw_oihw, int Cin_real, int N, int H, int W, void* stream);
/* Its kernels, as bdn_conv3x3_wgrad_kernels ("wgrad_first_kernel+wgrad_reduce_kernel<16>"); "" outside bdn_conv3x3_wgrad_bnbwd_supported. */
const char* bdn_conv3x3_wgrad_bnbwd_kernels(int dtype, int N, int H, int W, int Cout, int C0, int imgs_per_group);
/* Data gradient of the FIRST convolution (inc.conv.conv.0, models/unet_parts.py:13 in models/bidate_model.py:22-30): the gradient on the
 * two input images.  dA [2B,H,W,ldA >= 64], z [2B,H,W,64] of the shared encoder's 2B images (date 1 first: bdn_pack_input's order),
 * dz formed on load with bdn_bn_bwd_apply's expression from bn [G][4][64] and sums [G][2][64] (bdn_bn_bwd_finalize: batch statistics;
 * bdn_bn_bwd_finalize_frozen on a bdn_bn_eval table: running statistics); z == NULL: dA is dz itself (bn, sums unused).  w_oihw: the
 * float32 master weight [64][Cin_real][3][3].  Writes dx1, dx2 float32 NCHW [B,Cin_real,H,W] (date 1, date 2) directly; nothing else.
 * dtype BDN_BF16: bf16 dA / z, dz and filter rounded to bf16; BDN_F32: float32 dA / z, three-term split bf16 product. */
int bdn_conv3x3_dgrad_first(int dtype, const void* dA, int ldA, const void* z, const float* bn, const float* sums,
                            int imgs_per_group, const float* w_oihw, int Cin_real,
                            float* dx1, float* dx2, int B, int H, int W, void* stream);

/* ---- BatchNorm2d training statistics: nn.BatchNorm2d, models/unet_parts.py:14,17 ----
 * Reduces the conv's per-tile partials and produces, per group g and channel c,
 * bn[g][0..3][c] = {mean, invstd, scale = gamma*invstd, shift = beta - mean*scale}  (layout [G][4][C]),
 * then updates running_mean/var (momentum 0.1, unbiased variance) once per group in order g=0,1,..
 * and adds G to num_batches_tracked -- the reference calls the module once per date.
 * running_mean and running_var NULL together, and num_batches_tracked NULL: that buffer is left alone; with all three NULL the call
 * only writes bn (a forward on batch statistics that moves no running statistics: the second pass of a SAM step).
 * ws: scratch of bdn_bn_finalize_workspace_bytes() (double partial sums of the two-stage reduction).
 * Limit of the one-pass statistic.  The partials are per-tile float32 sums of z and z*z (bdn_conv3x3: stats_partial); they are added
 * in double and var = s1/count - mean^2, clamped at 0, so invstd <= 1/sqrt(eps) and a constant channel gives invstd = 1/sqrt(eps) or
 * whatever the rounding of its sum of squares leaves above 0.  The subtraction loses (mean/std)^2 of the float32 sums' precision:
 * error of the normalised output about 3e-6 of its magnitude at |mean|/std = 4, 4e-5 at 16, 8e-4 at 64, 1.5e-2 at 256 (measured; DESIGN.md
 * 12), where torch.native_batch_norm in float32 stays below 1.3e-5.  The reference network stays below |mean|/std = 4.1 in every layer; the suite
 * requires the float32 bar (5e-5) up to twice that.  The raw-moment backward half (bdn_bn_bwd_apply, raw_moment = 1: sum g*z converted
 * to sum g*xhat; bdn_conv3x3_dgrad_bb: dz = a g + b z + c) cancels in the same way but only linearly in mean/std: dgamma is off by
 * 2e-5 of its magnitude at 256 and dz stays at its storage rounding. */
size_t bdn_bn_finalize_workspace_bytes(int n_mtiles, int G, int C);
int bdn_bn_finalize(const float* stats_partial, int n_mtiles, int G, int C, int count_per_group,
                    const float* gamma, const float* beta, float eps, float momentum,
                    float* running_mean, float* running_var, int64_t* num_batches_tracked,
                    float* bn, void* ws, void* stream);
/* Eval mode: bn[0][..] from the running buffers (mean=rm, invstd=rsqrt(rv+eps)), replicated for G groups. */
int bdn_bn_eval(const float* gamma, const float* beta, const float* running_mean,
                const float* running_var, float eps, int G, int C, float* bn, void* stream);

/* ---- eval-mode stages (round 6): nothing depends on batch statistics, so conv -> BatchNorm -> ReLU is ONE launch ----
 * Reference: model.eval() forward of double_conv, models/unet_parts.py:13-18, as validation (train.py:125-172) and full-scene
 * inference (train.py:182-205, utils/inference.py:134-236) run it.
 *
 * bdn_bn_eval_fold_multi: per layer  scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale  (bdn_bn_eval's values),
 *   out[0][c] = scale, out[1][c] = conv_bias[c] * scale + shift, for n_layers layers in one launch.  desc: DEVICE array of records
 *   { const float* gamma, *beta, *running_mean, *running_var, *conv_bias (may be NULL); float* out (= [2][C] floats); int32 C, reserved; }
 *   (56 bytes each); max_C = the largest C among them.
 *
 * bdn_conv3x3_eval: out = relu(conv3x3(in0 | in1) * ep_scale + ep_shift) as [N,H,W,Cout]; operands are PLAIN activations (what such a
 *   launch stores), w the bdn_pack_weights forward image.  Optional fused consumers (either may be NULL):
 *     mul  [N,H,W,Cout]     the other date's activation of the same layer: `out` then receives relu(x_d2 * x_d1) = a * mul
 *                           (models/bidate_model.py:35-38; both factors are rounded activations >= 0) instead of a;
 *     pool [N,H/2,W/2,Cout] nn.MaxPool2d(2) of a (models/unet_parts.py:40, floor mode).
 * bdn_conv3x3_eval_cls: the last double_conv stage (Cout = 64) with the 1x1 classifier (models/unet_parts.py:88-89, ncls <= 2) in its
 *   epilogue: logits [N,ncls,H,W] f32 (NULL: not stored; bit-identical to bdn_outc_fwd on the stored activation), mask = argmax over
 *   classes (first maximum wins, train.py:199) as uint8 -- [N,H,W] when origins is NULL, else stitched into the scene mask [Hs,Ws] at
 *   origins[n] = (y0, x0) with bdn_argmax_stitch's ownership rule (utils/inference.py:187-236).  act_out (NULL: not stored) = the activation.
 * bdn_conv3x3_eval_pair: the second convolution of an encoder level on BOTH dates of B patch pairs at once -- in [2B,H,W,C0] (date 1 first;
 *   C0 a multiple of 64 bf16 / 32 f32 channels) -- on tiles that hold the two dates of the same pixels: f_out [B,H,W,Cout] = relu(x_d2 * x_d1)
 *   (models/bidate_model.py:35-38), pool [2B,H/2,W/2,Cout] = nn.MaxPool2d(2) of both dates (NULL: none).  Neither date's activation is stored.
 * dtype BDN_BF16 or BDN_F32.  Every tensor below 4 GB. */
int bdn_bn_eval_fold_multi(const void* desc, int n_layers, int max_C, float eps, void* stream);
int bdn_conv3x3_eval(int dtype, const void* in0, int C0, const void* in1, int C1, const void* w,
                     const float* ep_scale, const float* ep_shift, void* out, const void* mul, void* pool,
                     int N, int H, int W, int Cout, void* stream);
int bdn_conv3x3_eval_pair(int dtype, const void* in, int C0, const void* w, const float* ep_scale, const float* ep_shift,
                          void* f_out, void* pool, int B, int H, int W, int Cout, void* stream);
/* The two above with the date fusion as an argument (models/bidate_model.py:35-38 generalised: BDN_FUSE_PRODUCT = the calls above, bit for
 * bit; BDN_FUSE_ABSDIFF: `out` / f_out receive |a_d2 - a_d1|).  Same kernels, same instantiations: the mode is a runtime field. */
int bdn_conv3x3_eval_fusion(int dtype, int fusion, const void* in0, int C0, const void* in1, int C1, const void* w,
                            const float* ep_scale, const float* ep_shift, void* out, const void* mul, void* pool,
                            int N, int H, int W, int Cout, void* stream);
int bdn_conv3x3_eval_pair_fusion(int dtype, int fusion, const void* in, int C0, const void* w, const float* ep_scale, const float* ep_shift,
                                 void* f_out, void* pool, int B, int H, int W, int Cout, void* stream);
int bdn_conv3x3_eval_cls(int dtype, const void* in0, int C0, const void* w, const float* ep_scale, const float* ep_shift, void* act_out,
                         const float* cls_w, const float* cls_b, int ncls, float* logits, uint8_t* mask, const int32_t* origins,
                         int Hs, int Ws, int N, int H, int W, int Cout, void* stream);
/* Name of the kernel instantiation an eval-mode entry point runs for a shape (as bdn_conv3x3_variant; "" for an unsupported shape):
 * kind BDN_EVAL_STAGE = bdn_conv3x3_eval (N images, sources C0 | C1), BDN_EVAL_PAIR = bdn_conv3x3_eval_pair (N = B pairs, C1 = 0),
 * BDN_EVAL_CLS = bdn_conv3x3_eval_cls (C1 = 0).  The fused consumers do not change the instantiation.  Thread-local buffer. */
enum { BDN_EVAL_STAGE = 0, BDN_EVAL_PAIR = 1, BDN_EVAL_CLS = 2 };
const char* bdn_conv3x3_eval_variant(int kind, int dtype, int N, int H, int W, int C0, int C1, int Cout);

/* ---- BatchNorm2d + ReLU backward (autograd of models/unet_parts.py:14-15,17-18) ----
 * g = dA * [z*scale+shift > 0]; sums[g][0][c] = sum g, sums[g][1][c] = sum g*xhat (layout [G][2][C]);
 * dgamma/dbeta (accumulated over groups, overwritten) ; dz = scale*(g - s0/M - xhat*s1/M).
 * dA: [N,H,W,ldA] channel slice starting at dA pointer (ldA = channel stride of the dA tensor).
 * ws: workspace of bdn_bn_bwd_workspace_bytes(). */
size_t bdn_bn_bwd_workspace_bytes(int dtype, int N, int H, int W, int C, int imgs_per_group);
int bdn_bn_bwd(int dtype, const void* dA, int ldA, const void* z, const float* bn,
               int imgs_per_group, int N, int H, int W, int C,
               float* ws, float* sums, float* dgamma, float* dbeta, void* dz, void* stream);

/* Second half of bdn_bn_bwd for callers whose dA producer already emitted the per-tile partial sums (fused
 * BatchNorm-backward statistics): partial is [G][rows_per_group][2][C] holding sum_p g and, with raw_moment != 0,
 * sum_p g*z (converted to sum_p g*xhat in double here), with g = dA * [relu(bn(z)) > 0].  Runs the fixed-order
 * reduction (dgamma, dbeta, sums) and the dz pass.  scratch: NULL or bdn_bn_bwd_scratch_bytes(G, C) bytes; with it,
 * more than 512 rows per group are pre-reduced by many blocks (same result, fixed order either way). */
size_t bdn_bn_bwd_scratch_bytes(int G, int C);
int bdn_bn_bwd_apply(int dtype, const void* dA, int ldA, const void* z, const float* bn,
                     int imgs_per_group, int N, int H, int W, int C,
                     const float* partial, int rows_per_group, int raw_moment,
                     float* sums, float* dgamma, float* dbeta, void* dz, void* scratch, void* stream);
/* bf16x3 setting (float32 tensors): the same, with dz stored directly as the split operand of its two consumers -- dz_split
 * [N,H,W,2 C] bf16 = hi(dz) | lo(dz), bdn_split_pack's layout -- instead of float32: no bdn_split_pack pass over dz. */
int bdn_bn_bwd_apply_split(const void* dA, int ldA, const void* z, const float* bn,
                           int imgs_per_group, int N, int H, int W, int C,
                           const float* partial, int rows_per_group, int raw_moment,
                           float* sums, float* dgamma, float* dbeta, void* dz_split, void* scratch, void* stream);
/* The reduction half of bdn_bn_bwd_apply alone: partial rows -> sums [G][2][C], dgamma, dbeta (same argument meaning),
 * for a consumer that applies the backward while it stages dz (bdn_conv3x3_wgrad_bnbwd). */
int bdn_bn_bwd_finalize(const float* bn, int G, int C, const float* partial, int rows_per_group, int raw_moment,
                        float* sums, float* dgamma, float* dbeta, void* scratch, void* stream);
/* ---- BatchNorm2d + ReLU backward on RUNNING statistics: autograd of models/unet_parts.py:14-15,17-18 after model.eval() ----
 * bn is bdn_bn_eval's table {running_mean, invstd, scale, shift}; the statistics are constants, so dz = scale * g under the ReLU mask.
 * dgamma = sum g * xhat and dbeta = sum g (xhat on the running statistics: the same reduction as the training finalize), and the conv
 * bias in front of the BatchNorm gets dbias = scale * dbeta (NULL: not written).  `sums` is left ZEROED: every consumer that forms
 * dz = scale * (g - s0/M - xhat * s1/M) from it (bdn_conv3x3_dgrad_bb, bdn_conv3x3_wgrad_bnbwd, bdn_outc_bn_bwd_apply,
 * bdn_conv3x3_dgrad_first) then forms the frozen dz with unchanged arithmetic.  Arguments otherwise as bdn_bn_bwd_finalize,
 * bdn_bn_bwd_apply (dtype BDN_BF16X3: dz leaves as bdn_bn_bwd_apply_split's [N,H,W,2 C] operand) and bdn_bn_bwd. */
int bdn_bn_bwd_finalize_frozen(const float* bn, int G, int C, const float* partial, int rows_per_group, int raw_moment,
                               float* sums, float* dgamma, float* dbeta, float* dbias, void* scratch, void* stream);
int bdn_bn_bwd_apply_frozen(int dtype, const void* dA, int ldA, const void* z, const float* bn,
                            int imgs_per_group, int N, int H, int W, int C,
                            const float* partial, int rows_per_group, int raw_moment,
                            float* sums, float* dgamma, float* dbeta, float* dbias, void* dz, void* scratch, void* stream);
int bdn_bn_bwd_frozen(int dtype, const void* dA, int ldA, const void* z, const float* bn,
                      int imgs_per_group, int N, int H, int W, int C,
                      float* ws, float* sums, float* dgamma, float* dbeta, float* dbias, void* dz, void* stream);

/* a = relu(z*scale + shift) written out (nn.BatchNorm2d + nn.ReLU, models/unet_parts.py:14-15): z, out [N,H,W,C]; bn [G][4][C].
 * Rounded exactly like the on-load application inside bdn_conv3x3 / bdn_conv3x3_wgrad; bdn_conv3d_wgrad takes plain operands only. */
int bdn_bnrelu(int dtype, const void* z, const float* bn, int imgs_per_group, void* out,
               int N, int H, int W, int C, void* stream);
/* ---- nn.MaxPool2d(2) on relu(bn(z)): models/unet_parts.py:40 (floor mode) ---- */
int bdn_bnrelu_pool(int dtype, const void* z, const float* bn, int imgs_per_group,
                    void* out, int N, int H, int W, int C, void* stream);

/* ---- date fusion torch.relu(x_d2 * x_d1): models/bidate_model.py:35-38 ----
 * z: [2B,H,W,C] raw conv outputs of both dates, bn: [2][4][C]; f: [B,H,W,C]. */
int bdn_fuse_product(int dtype, const void* z, const float* bn, void* f,
                     int B, int H, int W, int C, void* stream);
/* Both of the above in one pass over z (every encoder level but the last needs the skip AND the pooled maps):
 * f [B,H,W,C] = relu(a_d2*a_d1), pool [2B,H/2,W/2,C] = MaxPool2d(2)(a), a = relu(bn(z)), z [2B,H,W,C] date 1 first. */
int bdn_product_pool(int dtype, const void* z, const float* bn, void* f, void* pool,
                     int B, int H, int W, int C, void* stream);

/* bf16x3 setting (float32 z): both outputs stored directly as the [hi | lo] bf16 operands of the convolutions that consume them -- f into
 * channels [0, C) of the decoder stage's two-source operand f_split [B,H,W,f_ld] (lo half f_half channels further), pool as
 * pool_split [2B,H/2,W/2,2C] -- bdn_split_pack's layout, without the float32 tensors and the split pass over them. */
int bdn_product_pool_split(const void* z, const float* bn, void* f_split, int f_ld, int f_half, void* pool_split,
                           int B, int H, int W, int C, void* stream);

/* The three above with the date fusion as an argument (models/bidate_model.py:35-38 generalised; fusion = BDN_FUSE_PRODUCT / BDN_FUSE_ABSDIFF):
 * f = relu(a_d2 * a_d1) or |a_d2 - a_d1| of the rounded activations a = relu(bn(z)); the pooled maps do not depend on it.  Mode 0 launches the
 * kernels of bdn_fuse_product / bdn_product_pool / bdn_product_pool_split themselves; the split form stores the [hi | lo] split of the float32 f. */
int bdn_fuse_dates(int dtype, int fusion, const void* z, const float* bn, void* f,
                   int B, int H, int W, int C, void* stream);
int bdn_fuse_dates_pool(int dtype, int fusion, const void* z, const float* bn, void* f, void* pool,
                        int B, int H, int W, int C, void* stream);
int bdn_fuse_dates_pool_split(int fusion, const void* z, const float* bn, void* f_split, int f_ld, int f_half, void* pool_split,
                              int B, int H, int W, int C, void* stream);

/* ---- nn.Upsample(scale_factor=2, bilinear, align_corners=True) + F.pad: models/unet_parts.py:56-58,68-72 ----
 * src: [B,h,w,C] (plain, or raw z with bn when in_mode = BDN_IN_BNRELU); out: [B,H,W,C] with the
 * 2h x 2w map placed at offset ((H-2h)/2, (W-2w)/2) and zeros elsewhere. */
int bdn_upsample2x(int dtype, const void* src, int in_mode, const float* bn,
                   void* out, int B, int h, int w, int H, int W, int C, void* stream);
/* bf16x3 setting (float32 src): the upsampled map stored as channels [off, off + C) of the decoder stage's split operand
 * out_split [B,H,W,ld] bf16 (lo half `half` channels further). */
int bdn_upsample2x_split(const void* src, int in_mode, const float* bn, void* out_split, int ld, int off, int half,
                         int B, int h, int w, int H, int W, int C, void* stream);
/* Transpose of the above: dU: [B,H,W,ldU] channel slice -> dsrc: [B,h,w,C]. */
int bdn_upsample2x_bwd(int dtype, const void* dU, int ldU, void* dsrc,
                       int B, int h, int w, int H, int W, int C, void* stream);
/* The same with the BatchNorm-backward partial sums of the layer whose relu(bn(z_prev)) had been upsampled (up's input x1 is the
 * previous double_conv's output, models/unet_parts.py:64-66 after :16-18) fused in: bs_partial f32
 * [bdn_upsample2x_bwd_rows(dtype,B,h,w,C)][2][C] = per block sum g, sum g*z_prev with g = dsrc * [scale*z_prev + shift > 0]
 * (z_prev [B,h,w,C], bn_prev [1][4][C]; one statistic group) -> bdn_bn_bwd_apply(raw_moment = 1); dsrc holds g (masked).  rows() is 0 for shapes the
 * tiled kernel does not take (maps below 8x8, C not a multiple of 32 (bf16) / 16 (f32)): use bdn_upsample2x_bwd + bdn_bn_bwd there. */
int bdn_upsample2x_bwd_rows(int dtype, int B, int h, int w, int C);
int bdn_upsample2x_bwd_bs(int dtype, const void* dU, int ldU, void* dsrc, const void* z_prev, const float* bn_prev,
                          float* bs_partial, int B, int h, int w, int H, int W, int C, void* stream);

/* ---- backward of the date fusion and of MaxPool2d into the encoder outputs ----
 * dF: [B,H,W,ldF] slice; z: [2B,H,W,C], bn [2][4][C]; dP: NULL or [2B,H/2,W/2,C] gradient of the
 * pooled map; dA: [2B,H,W,C] = gradient wrt relu(bn(z)) of each date:
 * dA_d1 = dF * a_d2 + unpool(dP_d1), dA_d2 = dF * a_d1 + unpool(dP_d2)  (first maximum wins ties). */
int bdn_enc_skip_bwd(int dtype, const void* dF, int ldF, const void* z, const float* bn,
                     const void* dP, void* dA, float* bs_partial, int B, int H, int W, int C, void* stream);
/* bs_partial: NULL, or f32 [2][bdn_enc_skip_bwd_rows(dtype,B,H,W,C)][2][C] receiving the BatchNorm-backward partial
 * sums of the layer (per block: sum g, sum g*z; date 1 rows then date 2 rows) -> bdn_bn_bwd_apply(raw_moment = 1); dA then holds
 * the MASKED gradient g = dA * [relu(bn(z)) > 0] (see bdn_conv3x3_dgrad_bs). */
int bdn_enc_skip_bwd_rows(int dtype, int B, int H, int W, int C);
/* bdn_enc_skip_bwd with the date fusion as an argument (autograd of models/bidate_model.py:35-38 generalised).  BDN_FUSE_ABSDIFF:
 * dA_d1 = dF * s + unpool(dP_d1), dA_d2 = -(dF * s) + unpool(dP_d2), s = sign(a_d1 - a_d2) from the rounded activations (0 at a tie, both-dead
 * ReLUs included); pooling gradient, masking and bs_partial (same rows, formed on the stored, rounded values) as above. */
int bdn_enc_skip_bwd_fusion(int dtype, int fusion, const void* dF, int ldF, const void* z, const float* bn,
                            const void* dP, void* dA, float* bs_partial, int B, int H, int W, int C, void* stream);

/* ---- outconv: nn.Conv2d(64, n_classes, 1), models/unet_parts.py:86 ----
 * z: [B,H,W,C] raw output of up4's second conv, bn: [1][4][C]; w: [ncls][C] f32, b: [ncls];
 * logits: [B,ncls,H,W] f32 NCHW (the reference's output layout). */
int bdn_outc_fwd(int dtype, const void* z, const float* bn, const float* w, const float* b,
                 float* logits, int B, int H, int W, int C, int ncls, void* stream);
/* dlogits: [B,ncls,H,W] f32 -> dA [B,H,W,C] (wrt relu(bn(z))), dw [ncls][C], db [ncls] (overwritten).
 * ws: bdn_outc_bwd_workspace_bytes() of scratch -- the blocks' partial dw / db, summed in a fixed order (deterministic). */
size_t bdn_outc_bwd_workspace_bytes(int dtype, int B, int H, int W, int C, int ncls);
int bdn_outc_bwd(int dtype, const float* dlogits, const void* z, const float* bn, const float* w,
                 void* dA, float* dw, float* db, float* bs_partial, float* ws, int B, int H, int W, int C, int ncls, void* stream);
/* BatchNorm+ReLU backward of the layer in front of the classifier with the classifier's data gradient recomputed from
 * dlogits (outconv, models/unet_parts.py:83-90, after double_conv's BN+ReLU, :16-18): dz = bn_bwd(round(sum_k dlogits[k] w[k][c]), z)
 * with `sums` from bdn_bn_bwd_finalize.  Call bdn_outc_bwd with dA = NULL (it still leaves the partial sums) and this instead
 * of bdn_bn_bwd_apply: the gradient tensor in between is never written or read.
 * dtype BDN_BF16X3: z float32, dz the split operand [B,H,W,2 C] bf16 = hi | lo of the float32 result (bdn_bn_bwd_apply_split's form). */
int bdn_outc_bn_bwd_apply(int dtype, const float* dlogits, const float* w, const void* z, const float* bn,
                          int imgs_per_group, const float* sums, void* dz, int B, int H, int W, int C, int ncls, void* stream);
/* bs_partial: NULL, or f32 [bdn_outc_bwd_rows(dtype,B,H,W,C)][2][C]: BatchNorm-backward partial sums of the layer that
 * produced z (sum g, sum g*z on the stored dA) -> bdn_bn_bwd_apply(raw_moment = 1, one statistic group). */
int bdn_outc_bwd_rows(int dtype, int B, int H, int W, int C);

/* ---- TverskyLoss.forward, utils/metrics.py:130-171, for [B,H,W] labels (dims == (0,2)) ----
 * labels: uint8 [B,H,W].  ws: bdn_overlap_workspace_bytes(B, ncls, H, W, 0) bytes of f32 scratch (16-byte aligned): the
 * blocks' partial sums are added in a fixed order, no float atomics -- loss and dlogits are the same bits on every run.
 * loss: f32 scalar.  counts: NULL or int32[4] = {TP, FP, FN, correct} of argmax(logits) vs labels
 * (class 1 positive, first maximum wins; train.py:96-106).  dlogits: NULL or [B,ncls,H,W] = d loss / d logits.
 * Labels outside the classes (label >= ncls, e.g. the 255 of a {0, 255} mask; the reference raises on them): such a pixel has no true
 * class.  In every loss entry point (bdn_tversky, bdn_overlap_loss, bdn_focal, bdn_criterion) its probabilities add to FP of every
 * class and to nothing else; its focal term and focal gradient are exactly 0 while it still counts in the size_average denominator; it
 * is never a correct prediction in `counts` (it is an FP when class 1 is predicted); the class weights are never indexed with it. */
size_t bdn_overlap_workspace_bytes(int B, int ncls, int H, int W, int reduce_w);
int bdn_tversky(const float* logits, const uint8_t* labels, float alpha, float beta, float eps,
                float* ws, float* loss, int32_t* counts, float* dlogits,
                int B, int ncls, int H, int W, void* stream);

/* ---- dice_loss / jaccard_loss / TverskyLoss in either label rank, utils/metrics.py:51-171 ----
 * One ratio TP / (TP + alpha FP + beta FN + eps) per reduction cell, averaged:
 *   TverskyLoss(alpha, beta, eps) as is;  jaccard_loss(eps) = (1, 1, eps);  dice_loss(eps) = (0.5, 0.5, eps / 2)
 *   (2I / (2I + FP + FN + eps), utils/metrics.py:80-83).
 * reduce_w = 0: [B,H,W] labels, reference dims == (0,2): one cell per (class, column);
 * reduce_w = 1: [B,1,H,W] labels, dims == (0,2,3): one cell per class.  ws: bdn_overlap_workspace_bytes(.., reduce_w).
 * Other arguments as bdn_tversky. */
int bdn_overlap_loss(const float* logits, const uint8_t* labels, float alpha, float beta, float eps,
                     int reduce_w, float* ws, float* loss, int32_t* counts, float* dlogits,
                     int B, int ncls, int H, int W, void* stream);

/* ---- FocalLoss(gamma, alpha, size_average).forward, utils/metrics.py:8-48 (criterion 'focal', utils/helpers.py:305) ----
 * labels uint8 [B,H,W] (or [B,1,H,W], same memory).  alpha: NULL or f32[ncls] class weights (device).
 * The modulating factor (1-pt)^gamma is a constant for the gradient exactly as in the reference (:35).
 * log pt is formed on the maximum-subtracted logits, (l_t - max) - log sum exp(l - max): loss and gradient do not depend on a common
 * shift of the logits.  A label >= ncls: term and gradient 0, alpha not read (bdn_tversky, "labels outside the classes").
 * ws: bdn_focal_workspace_bytes() bytes.  loss, counts, dlogits as bdn_tversky. */
size_t bdn_focal_workspace_bytes(void);
int bdn_focal(const float* logits, const uint8_t* labels, float gamma, const float* alpha, int size_average,
              void* ws, float* loss, int32_t* counts, float* dlogits,
              int B, int ncls, int H, int W, void* stream);

/* ---- the criterion of a run, utils/helpers.py:303-312 over utils/metrics.py:8-48 (FocalLoss) and :51-171 (dice / jaccard / Tversky) ----
 *   L = w_overlap * Overlap(alpha, beta, eps, reduce_w) + w_focal * Focal(gamma, class_alpha, size_average)
 * with Overlap exactly bdn_overlap_loss's function and Focal exactly bdn_focal's (the modulating factor a constant for the gradient);
 * w_overlap, w_focal >= 0 and not both zero.  One term with weight 1 and the other with weight 0 runs that entry point's own launches
 * (its bits).  Every other case -- the compound losses focal + dice / jaccard / Tversky -- is three launches: a statistics pass that forms
 * softmax once per pixel (overlap partial sums, focal partial sums in double, argmax counts), a fixed-order finish, and a gradient pass
 * that writes w_overlap dO + w_focal dF once; no float atomics, no memset: loss, terms, counts and dlogits are the same bits every run.
 * Every pointer is device memory.  class_alpha: NULL or f32[ncls].  ws: bdn_criterion_workspace_bytes() bytes, 16-byte aligned.
 * terms: NULL or f32[2] = the unweighted overlap and focal values (0 for a term that did not run).  counts, dlogits: NULL or as
 * bdn_tversky; dlogits == NULL launches no gradient pass (validation). */
size_t bdn_criterion_workspace_bytes(int B, int ncls, int H, int W, int reduce_w);
int bdn_criterion(const float* logits, const uint8_t* labels, float w_overlap, float alpha, float beta, float eps, int reduce_w,
                  float w_focal, float gamma, const float* class_alpha, int size_average, void* ws, float* loss, float* terms,
                  int32_t* counts, float* dlogits, int B, int ncls, int H, int W, void* stream);

/* ---- the same criterion over the labelled pixels only: an ignore label (torch's ignore_index; the reference has none) ----
 * A pixel whose label byte equals ignore_label (0..255) is IGNORED; every other pixel is VALID and treated exactly as by bdn_criterion,
 * the "labels outside the classes" rule (bdn_tversky) for a valid label >= ncls included.  With v = 1 at valid pixels and 0 elsewhere:
 *   Overlap: TP = sum p onehot v, FP = sum p (1 - onehot) v, FN = sum (1 - p) onehot v over the same dims, the mean over the same
 *            (class, column) or (class) cells; a cell without a valid pixel has the ratio 0 / (0 + eps) = 0 (no special case).
 *   Focal:   the per-pixel term summed over the valid pixels; size_average divides by the NUMBER OF VALID PIXELS (0 with none); the
 *            modulating factor stays a constant for the gradient.
 *   dlogits: exactly 0.0f for every class at an ignored pixel (written, not skipped), the gradient of the masked loss elsewhere.
 *   counts:  NULL or int32[5] = {TP, FP, FN, correct, valid}, all over the valid pixels.
 * The logits of an ignored pixel reach no output, whatever they hold (+-inf and NaN included): the kernels branch on the label before
 * they use them.  A batch without a valid pixel gives overlap = 1, focal = 0, loss = w_overlap, an all-zero dlogits and counts[4] = 0;
 * it is not an error and nothing checks for it on the host.
 * Always three launches, whatever the weights (one term with weight 1 included): the statistics pass (softmax once per pixel, overlap
 * block partials, focal block partials in double, argmax counts and the valid count), the fixed-order finish (loss, terms, counts,
 * coefficient tables, and the focal gradient scale 1 / valid -- or 1 -- left in the workspace), and the gradient pass, which reads that
 * scale from device memory.  No atomics, no memset, no host read-back: the same bits on every run.  A term with weight 0 contributes
 * nothing to loss and dlogits and is reported as 0 in `terms`.
 * Arguments and their checks as bdn_criterion, plus ignore_label in 0..255.  ws: bdn_criterion_masked_workspace_bytes() bytes,
 * 16-byte aligned.  Data-parallel training: each rank normalises by its own valid count and the ranks' gradients are averaged with
 * equal weight (torch DistributedDataParallel with ignore_index does the same). */
size_t bdn_criterion_masked_workspace_bytes(int B, int ncls, int H, int W, int reduce_w);
int bdn_criterion_masked(const float* logits, const uint8_t* labels, int ignore_label, float w_overlap, float alpha, float beta, float eps,
                         int reduce_w, float w_focal, float gamma, const float* class_alpha, int size_average, void* ws, float* loss,
                         float* terms, int32_t* counts, float* dlogits, int B, int ncls, int H, int W, void* stream);

/* ---- the masked criterion with top-k hard-pixel mining (nnU-Net's TopKLoss / bootstrapped cross-entropy / OHEM; the reference has none) ----
 * bdn_criterion_masked's function with the focal term averaged over the K hardest valid pixels of the batch only.  ignore_label: -1 (no
 * pixel is ignored) or a byte value 0..255.  topk_ppm in 1..1000000 is the kept fraction in parts per million.
 *   Kept count  n_valid = the pixels whose label is not ignore_label (a valid label >= ncls counts, as in the focal mean);
 *               K = max(1, (n_valid * topk_ppm) / 1000000) in 64-bit integers, K = 0 when n_valid = 0; formed on the device.
 *   Ranked      the float32 focal term of utils/metrics.py:8-48 that the statistics pass forms, -(1 - pt)^gamma a[t] log pt (bdn_focal's
 *               expression, unchanged; 0 for a label >= ncls), through its bit pattern u:
 *                   key = u ^ 0x80000000 when the sign bit is clear, ~u otherwise
 *               (monotone: -0 < +0, +inf ranks highest, every bit pattern has a place).  Among equal keys the lower linear pixel index
 *               (b*H + y)*W + x ranks first.  The kept set is the first K pixels of that order: an exact select on the 32-bit keys (three
 *               radix levels of 11 + 11 + 10 bits), not a histogram approximation.
 *   Focal       S / K with size_average (0 when K = 0), else S; S = the kept terms summed in double in a fixed order.
 *   dlogits     at a kept pixel bdn_criterion_masked's focal gradient with the scale 1 / K (1 without size_average); at a valid pixel that
 *               is not kept the focal part is exactly 0 (selected out, not multiplied by 0); exactly 0.0f at an ignored pixel, none of
 *               whose logits is read.  The selection is a constant for the gradient, as torch.topk is under autograd.
 *   Overlap     unchanged: over all valid pixels; its gradient reaches the pixels that are not kept.
 *   terms       NULL or f32[3] = overlap, focal, the K-th largest term (the threshold; 0 when K = 0).
 *   counts      NULL or int32[6] = {TP, FP, FN, correct, valid, K}.
 *   pixel_terms NULL or f32[B*H*W]: the ranked terms (unspecified at ignored pixels).  kept: NULL or uint8[B*H*W] of 0 / 1.
 * w_focal > 0 (top-k ranks the focal term; gamma = 0 is top-k cross-entropy), w_overlap >= 0; class_alpha values must be >= 0 (the
 * caller's contract: they are device memory).  Non-finite logits at a valid pixel give unspecified values, but exactly K pixels are kept.
 * Launches: one 20 KB memset of the level histograms on the stream, the statistics pass (it also stores every pixel's term), three
 * histogram passes and a tie-count pass (each first reduces the level above to its digit and remaining rank), the kept-term sum, the
 * finish and the gradient pass (none with dlogits == NULL).  Integer histogram atomics only -- no float atomics, no host read-back; the
 * caller never clears the workspace: the same bits on every run, whatever the workspace held.
 * ws: bdn_criterion_topk_workspace_bytes() bytes, 16-byte aligned (about 5 bytes per pixel more than bdn_criterion_masked's).
 * Other arguments and checks as bdn_criterion_masked.  Data-parallel: each rank selects its own K from its own batch. */
size_t bdn_criterion_topk_workspace_bytes(int B, int ncls, int H, int W, int reduce_w);
int bdn_criterion_topk(const float* logits, const uint8_t* labels, int ignore_label, float w_overlap, float alpha, float beta, float eps,
                       int reduce_w, float w_focal, float gamma, const float* class_alpha, int size_average, int topk_ppm, void* ws,
                       float* loss, float* terms, int32_t* counts, float* dlogits, float* pixel_terms, uint8_t* kept,
                       int B, int ncls, int H, int W, void* stream);

/* ---- the criterion on soft targets: label smoothing, pixel weights, probability maps (the reference has none) ----
 * bdn_criterion_masked's function with a target q_c >= 0 per class and a weight w >= 0 per pixel in place of one class index; v = [w > 0],
 * p = softmax(logits).  Exactly one of `labels` and `targets` is given:
 *   labels   uint8 [B,H,W]: lo = smoothing / ncls and hi = (1 - smoothing) + lo, float32 operations of one rounding each; q_c = hi at the
 *            label's class and lo elsewhere (smoothing in [0, 1); 0 gives the one-hot target).  A valid label >= ncls has q = 0 for every
 *            class ("labels outside the classes", bdn_tversky: no smoothing mass).  ignore_label: -1 (none) or a byte value, w = 0 there.
 *   targets  f32 [B,ncls,H,W]: q as given; smoothing must be 0 and ignore_label -1.  Negative or non-finite targets at a valid pixel are
 *            the caller's error: nothing looks for them.
 *   weights  NULL (w = 1 at every pixel that is not ignored) or f32 [B,H,W], multiplied into w.
 *   Overlap  TP_c = sum w p_c q_c, FP_c = sum w p_c (1 - q_c), FN_c = sum w (1 - p_c) q_c over the cells of reduce_w;
 *            O = 1 - mean TP / (TP + alpha FP + beta FN + eps); a cell without a valid pixel has the ratio 0 / eps = 0.
 *   Focal    per pixel f = sum_c [q_c > 0] q_c a_c m_c (-log p_c), m_c = max(1 - p_c, 0)^gamma a constant for the gradient (1 at gamma
 *            0), log p_c = (l_c - max) - log sum exp(l - max); a class with q_c == 0 is selected out, 0 * log 0 is never formed.
 *            F = scale * sum w f; scale = 1 / n_valid with size_average (1 when n_valid = 0: the sum is then 0), else 1.  n_valid is the
 *            NUMBER of pixels with w > 0, not the sum of the weights: 0 / 1 weights are ignore_label exactly.
 *   loss     w_overlap O + w_focal F; a term with weight 0 is selected out and reported as 0.  terms: NULL or f32[2] = {O, F}.
 *   counts   NULL or int32[5] = {TP, FP, FN, correct, valid}: argmax(logits) against the pixel's class -- the label, or argmax_c q_c --
 *            over the valid pixels, class 1 positive, the first maximum on both sides.
 *   dlogits  NULL (no gradient pass) or f32 [B,ncls,H,W]: the gradient, exactly 0.0f for every class at a pixel with v = 0 (written).
 * A pixel with v = 0 is skipped by a branch before any of its logits or targets is used: inf and NaN there reach no output.  A batch
 * without a valid pixel gives O = 1, F = 0, zero gradient and zero counts.
 * Always three launches (two without dlogits): statistics (softmax once per pixel; overlap block partials in float32, the focal partial
 * in double, the counters), a single-block fixed-order finish that leaves the coefficient tables and the focal scale in the workspace,
 * and the gradient pass.  No atomics, no memset, no host read-back: the same bits every run, whatever the workspace held.  With labels
 * the passes read what bdn_criterion_masked's read (plus the weight map if there is one); targets are 4 ncls more bytes per pixel.
 * BDN_E_ARG before any launch: not exactly one of labels / targets; smoothing outside [0, 1) or NaN, or != 0 with targets; ignore_label
 * outside -1..255, or != -1 with targets; a negative weight or both zero; negative gamma; ws, loss or logits NULL; ws not 16-byte
 * aligned or a float32 / int32 pointer not 4-byte aligned.  ws: bdn_criterion_soft_workspace_bytes() bytes (0 outside ncls 2..8 or with
 * B*H*W >= 2^31).  Data-parallel: each rank normalises by its own valid count. */
size_t bdn_criterion_soft_workspace_bytes(int B, int ncls, int H, int W, int reduce_w);
int bdn_criterion_soft(const float* logits, const uint8_t* labels, const float* targets, const float* weights, int ignore_label,
                       float smoothing, float w_overlap, float alpha, float beta, float eps, int reduce_w, float w_focal, float gamma,
                       const float* class_alpha, int size_average, void* ws, float* loss, float* terms, int32_t* counts, float* dlogits,
                       int B, int ncls, int H, int W, void* stream);

/* ---- the Lovasz-Softmax term (Berman, Rahman Triki, Blaschko, CVPR 2018; the reference has none) ----
 * The loss that optimises the Jaccard index itself, batch level (the paper's per_image = False): an add-on term of the criterion of a run,
 * utils/helpers.py:303-312, the loss selection it extends.  ignore_label: -1 (no pixel is ignored) or a byte value 0..255.
 *   Valid       the n pixels whose label is not ignore_label.  A valid label >= ncls is foreground of no class.
 *   Errors      p = softmax(logits) per pixel as bdn_criterion forms it; for class c  fg = (label == c), G = sum fg, err = |fg - p_c| in
 *               float32 with the sign bit clear.
 *   Order       per class the valid pixels by err descending, through bdn_criterion_topk's key of the bit pattern u of err:
 *                   key = u ^ 0x80000000 when the sign bit is clear, ~u otherwise
 *               (monotone, +inf on top, every bit pattern -- NaN included -- has a place).  Among equal keys the lower linear pixel index
 *               (b*H + y)*W + x comes first.  A full stable sort (LSD radix, four passes of eight bits, on the complemented key), not an
 *               approximation: the order is a permutation of the valid pixels whatever the logits hold.
 *   Coefficient at 0-based rank r with c_prev foreground pixels at ranks < r:  I = G - c_prev, U = G + r - c_prev,
 *                   g = 1 / U at a foreground pixel, I / (U (U + 1)) elsewhere, 1 when U = 0 (first pixel of a class with G = 0)
 *               -- the increment J_r - J_(r-1) of the paper's lovasz_grad, formed from the integers in float64.
 *   Term        L_c = sum_r err_r g_r in double in a fixed order; term = the mean of L_c over the included classes: those with G > 0
 *               (classes_all = 0, the paper's 'present') or every class (classes_all = 1).  No included class, or n = 0: term 0, gradient 0.
 *   Gradient    the order is a constant.  With m included classes  q_c = (fg ? -g : +g) / m  (0 for a class that is not included) and
 *               dterm / dlogit_j = p_j (q_j - sum_c q_c p_c).  Exactly 0.0f at an ignored pixel, none of whose logits is read.
 *   accumulate  0: *loss = weight * term, dlogits = weight * dterm.  1: *loss += weight * term and dlogits += weight * dterm, every element
 *               read and written once by one thread, the product rounded to float32 before the add, ignored pixels untouched -- how the
 *               term joins a criterion that has already run on the same stream.
 *   term        NULL or f32[1]: the unweighted value.  dlogits: NULL launches no gradient pass.
 *   pixel_errors NULL or f32[ncls][B*H*W]: err (0 at ignored pixels).  ranks: NULL or int32[ncls][B*H*W]: the 0-based rank, -1 at ignored.
 * Two classes are sorted separately: p_0 and p_1 are rounded separately in float32, so the two error arrays differ.
 * Launches, whatever the data: one preparation pass (softmax, keys, the first digit histogram), per radix pass a tile histogram (not
 * the first), a scan and a stable scatter, then the foreground count per tile, its scan, the coefficient pass, the finish and the gradient
 * pass: 17 (16 without dlogits).  Integer histogram atomics in LDS only -- no float atomics, no host read-back, no kernel waits for another
 * block; the caller never clears the workspace: the same bits on every run, whatever the workspace held.
 * ws: bdn_lovasz_workspace_bytes() bytes (0 for an invalid shape), 16-byte aligned: 16 bytes per pixel and class (two key and two payload
 * buffers; the coefficients reuse one) plus 1 KB per class and 4096 pixels.  weight >= 0; ncls in 2..8; B*H*W < 2^31.
 * Data-parallel: each rank sorts its own batch. */
size_t bdn_lovasz_workspace_bytes(int B, int ncls, int H, int W);
int bdn_lovasz_softmax(const float* logits, const uint8_t* labels, int ignore_label, int classes_all, float weight, int accumulate,
                       void* ws, float* loss, float* term, float* dlogits, float* pixel_errors, int32_t* ranks,
                       int B, int ncls, int H, int W, void* stream);

/* ---- OSCD ingest: utils/dataloaders.py:86-111 city_loader, per band ----
 * dst [H][W] f32 (one plane of a [C][H][W] scene) = cv2.resize((src - mean) / std, (W, H)) with cv2's default float
 * INTER_LINEAR sampling (half-pixel centres, border weights (1,0)).  src: [hs][ws] uint16 (src_is_f32 = 0) or f32, on
 * the device.  cv2 is not installed in the build image, so this row's parity is pinned only against the written-out
 * algorithm (oracle/ingest_oracle.py), not against cv2 itself. */
int bdn_ingest_band(int src_is_f32, const void* src, int hs, int ws, float mean, float stdv,
                    float* dst, int H, int W, void* stream);

/* ---- full-scene sliding-window inference: train.py:182-205, utils/inference.py:134-236 ----
 * The scene stays in HBM as band planes scene_d*: [C][H][W] f32.  origins: device int32 [n_tiles][2] = (y0, x0)
 * in the reference's tile order (utils/inference.py:160-184: hs*ws main tiles, lc last-column tiles, lr last-row
 * tiles, corner).  out: [2*n_tiles][p][p][Cpad] packed batch (date-1 tiles first) = the encoder input. */
int bdn_gather_tiles(int dtype, const float* scene_d1, const float* scene_d2, const int32_t* origins,
                     void* out, int n_tiles, int C, int H, int W, int p, int Cpad, void* stream);
/* Rows [r0, r1) of all C band planes of a HOST scene [C][H][W] f32 (pinned for an asynchronous copy) into the resident device planes, as one
 * 2-D copy on `stream` (the host -> device staging of train.py:190-193 / utils/dataloaders.py:86-101, per row band of the scene instead of per batch). */
int bdn_upload_band(float* dst_planes, const float* src_planes_host, int C, int H, int W, int r0, int r1, void* stream);
/* `_, cd_preds = torch.max(preds, 1)` (train.py:199; first maximum wins): logits [n][ncls][H][W] f32 -> uint8 [n][H][W]. */
int bdn_argmax(const float* logits, uint8_t* out, int n, int ncls, int H, int W, void* stream);
/* argmax + _get_bands (utils/inference.py:187-236): class index of every tile pixel written to mask [H][W] uint8 at
 * the tile origin; far-edge tiles own the far-edge bands exactly as the reference's paste order leaves them. */
int bdn_argmax_stitch(const float* logits, const int32_t* origins, uint8_t* mask,
                      int n_tiles, int ncls, int p, int H, int W, void* stream);

/* ---- full-scene change probabilities from blended overlapping tiles: utils/inference.py:134-236 and train.py:182-205, generalized ----
 * Tile plan of an H x W scene at stride s (1 <= s <= p): ys[k] = min(k s, H - p) for k < ny = (H - p) / s + 1 + ((H - p) % s != 0),
 * xs alike; tile g = ky nx + kx (row-major).  Forward images are (tile, symmetry) pairs in tile-major order, n_syms per tile: image
 * i = g n_syms + k shows tile g under the k-th symmetry code.  sym = 4 t + 2 rr + rc as in bdn_sample_patches.
 * bdn_gather_tiles_sym: bdn_gather_tiles with table = device int32 [n_tiles][3] = (y0, x0, sym): tile i holds the p x p window at
 *   (y0, x0) of both dates under sym.  out: [2*n_tiles][p][p][Cpad] (date-1 tiles first).  Rows outside the scene or with sym outside
 *   0..7 give zero tiles (the caller checks the table).
 * bdn_blend_fold: logits [n_img][ncls][p][p] f32 of n_img forward images whose symmetries are table[i][2] (the gather's table) ->
 *   out [n_img][ncls][p][p] f32 = window[a][b] * softmax over classes, mapped back through the inverse symmetry into scene orientation.
 *   window: [p][p] f32, strictly positive.
 * bdn_blend_stitch: the folded images [img0, img0 + n_img) of the plan (H, W, p, stride, n_syms) added into acc [ncls][H][W] and their
 *   window weights into wsum [H][W].  Each pixel adds its covering images in ascending image index into one register: the same bits for
 *   any split of the images into batches, provided the batches' stitches are ordered on the device.  No float atomics.
 * bdn_blend_finalize: acc /= wsum in place (= the class probabilities) and mask [H][W] uint8 = their argmax (first maximum wins,
 *   train.py:199).  2 <= ncls <= 256. */
int bdn_gather_tiles_sym(int dtype, const float* scene_d1, const float* scene_d2, const int32_t* table,
                         void* out, int n_tiles, int C, int H, int W, int p, int Cpad, void* stream);
int bdn_blend_fold(const float* logits, const int32_t* table, const float* window, float* out, int n_img, int ncls, int p, void* stream);
int bdn_blend_stitch(const float* fold, const float* window, float* acc, float* wsum, long long img0, int n_img,
                     int n_syms, int ncls, int H, int W, int p, int stride, void* stream);
int bdn_blend_finalize(float* acc, const float* wsum, uint8_t* mask, int ncls, int H, int W, void* stream);

/* ---- training patch pairs on the device: utils/dataloaders.py:148-165 (onera_siamese_loader) + the DataLoader collate, for a batch ----
 * cities_dev: DEVICE array of n_cities records { const float* images; const uint8_t* labels; int32 H, W; } (24 bytes each, 8-byte
 * aligned): images [2][C][H][W] f32 and labels [H][W] uint8, both contiguous.  city_hw_host: HOST int32 [n_cities][2] = (H, W), the
 * same values as the records.  desc_host: HOST int32 [n][4] = (city, row, col, sym), every one checked here before anything is
 * launched (city in range, sym in 0..7, 0 <= row, row + S <= H, 0 <= col, col + S <= W); desc_dev: the same table in device memory,
 * 16-byte aligned, which the kernel reads.  sym = 4 t + 2 rr + rc: transpose the window if t, then reverse its rows if rr, then its
 * columns if rc (fabric_amd.utils.dataloaders._apply_symmetry).  out_d1, out_d2: [n][C][S][S] f32 (date 1, date 2); out_labels:
 * [n][S][S] uint8.  Bits are moved, never computed: the output equals the host crop bit for bit. */
int bdn_sample_patches(const void* cities_dev, const int32_t* city_hw_host, int n_cities, int C,
                       const int32_t* desc_host, const int32_t* desc_dev, int n, int S,
                       float* out_d1, float* out_d2, uint8_t* out_labels, void* stream);
/* ---- the same cut, augmented on the device: extends utils/dataloaders.py:148-165, whose augmentation ends at the eight symmetries ----
 * Everything bdn_sample_patches takes, checked the same way, plus keys_dev: DEVICE uint64 [n], 8-byte aligned, the sample keys
 * epoch << 32 | dataset index.  Every draw is Philox4x32-10 (csrc/philox_core.hpp) with key (seed & 0xffffffff, seed >> 32) and counter
 * (key_lo, key_hi, slot, stream); u(w) = float(w >> 8) * 2^-24, range(w, n) = (uint64(w) * n) >> 32.  Stages, in this order:
 *   crop      stream 0 slot 0: row' = clamp(row + range(w0, 2J+1) - J, 0, H - S), col' alike from w1 (clamped on the device: in range
 *             for any draw); J >= 0.
 *   symmetry  sym = w2 >> 29 of the same words if flags & 1, else the descriptor's sym.
 *   gain/bias stream 1 slot date * C + c (slot c for both dates unless flags & 2): g = 1 + gain * (2 u(w0) - 1), b = bias * (2 u(w1) - 1),
 *             out = g * x + b, each operation rounded once (no fused multiply-add).  Off when gain == 0 and bias == 0.
 *   noise     stream 2 + date * C + c, slot i * ceil(S / 4) + (j >> 2) for output element (i, j): words (a, b) = (w[2k], w[2k+1]),
 *             k = (j >> 1) & 1; u1 = float((a >> 8) + 1) * 2^-24, u2 = u(b), r = sqrt(-2 ln u1), z = r cos(2 pi u2) for even j,
 *             r sin(2 pi u2) for odd j; out += sigma * z.  Off when sigma == 0.
 *   erase     erased = u(w3 of stream 0 slot 0) < erase_p; stream 0 slot 1: eh = lo + range(w0, hi - lo + 1), ew alike from w1,
 *             top = range(w2, S - eh + 1), left = range(w3, S - ew + 1).  The output rectangle [top, top + eh) x [left, left + ew) of every
 *             image plane of both dates becomes erase_fill and, when erase_label >= 0, that of the label patch becomes that byte
 *             (erase_label = -1: labels are kept).  Off when erase_p == 0; then lo and hi are not read.
 * A stage that is off does no arithmetic: with gain = bias = sigma = 0 floats travel as 32-bit patterns, and with J = 0, flags = 0 and
 * erase_p = 0 as well the outputs are those of bdn_sample_patches.  Labels are moved or overwritten, never computed.
 * drawn_geom (or NULL): DEVICE int32 [n][8] = (row', col', sym, erased, top, left, eh, ew), the rectangle 0 when the erase stage is off;
 * drawn_radio (or NULL): DEVICE float [n][2][C][2] = (g, b), (1, 0) when gain / bias is off. */
int bdn_sample_patches_aug(const void* cities_dev, const int32_t* city_hw_host, int n_cities, int C,
                           const int32_t* desc_host, const int32_t* desc_dev, int n, int S,
                           float* out_d1, float* out_d2, uint8_t* out_labels, const uint64_t* keys_dev,
                           uint64_t seed, int J, int flags, float gain, float bias, float sigma, float erase_p,
                           int lo, int hi, int erase_label, float erase_fill,
                           int32_t* drawn_geom, float* drawn_radio, void* stream);
/* ---- the augmented cut through an affine map with bilinear taps: extends utils/dataloaders.py:148-165 by what no permutation of pixels
 * expresses: rotation by any angle, zoom, and a sub-pixel shift of date 2 against date 1 (misregistration; labels stay in date 1's frame) ----
 * Everything bdn_sample_patches_aug takes up to its two exports, checked the same way, with the same draws for the crop origin (row',
 * col'), the symmetry and the erase rectangle; then the warp policy, an optional override of the records, and their export.
 *   record    float32 [2][6] per sample; per date (a_ii, a_ij, t_i, a_ji, a_jj, t_j).  Drawn from stream 0x57415250 slot 0, with
 *             sgn(w) = 2 u(w) - 1:  theta = sgn(w0) * rotate_rad,  s = exp2f(log2_lo + u(w1) * (log2_hi - log2_lo)),
 *             a_ii = a_jj = cosf(theta) / s,  a_ij = -sinf(theta) / s,  a_ji = sinf(theta) / s;  translation (0, 0) for date 1 and
 *             (misreg * sgn(w2), misreg * sgn(w3)) for date 2.  0 <= rotate_rad <= pi, -3 <= log2_lo <= log2_hi <= 3 (s > 1 magnifies),
 *             0 <= misreg <= 64.  cosf, sinf and exp2f are the device library's: the a's are TOLERANCED (a few float32 ulp of 1 / s against
 *             the float64 formula), which is why the record is exported; the translations are exact.
 *   mapping   EXACT given the record: every operation below is rounded once, nothing is fused.  For output pixel (i, j) let (i', j') be the
 *             window coordinate the symmetry code gives it in bdn_sample_patches, h = (S - 1) / 2, di = i' - h, dj = j' - h:
 *               y = ((a_ii * di) + (a_ij * dj)) + (h + t_i),   x = ((a_ji * di) + (a_jj * dj)) + (h + t_j)     (relative to the window origin)
 *             y0 = floorf(y), fy = y - y0, x0, fx alike; tap rows row' + (int)y0 and + 1, tap columns col' + (int)x0 and + 1, each clamped
 *             into [0, H - 1] / [0, W - 1] (replicate border);  top = ((1 - fx) * v00) + (fx * v01), bot = ((1 - fx) * v10) + (fx * v11),
 *             out = ((1 - fy) * top) + (fy * bot).  Labels: nearest neighbour with date 1's record, rows row' + (int)floorf(y + 0.5), columns
 *             alike, clamped the same way; where the unclamped index lies outside the city the label becomes oob_label (0..255; -1:
 *             the clamped label is kept).  Labels are moved or overwritten, never computed.
 *   then      gain / bias, noise and erase exactly as in bdn_sample_patches_aug, with the same draws, on the gathered tile.
 * An identity record gives fx = fy = 0: a finite input then passes through unchanged bit for bit (-0.0 may arrive as +0.0), a rotation
 * by a multiple of 90 degrees about the centre lands on integers, an integer translation is a shifted crop with replicate clamping.
 * Non-finite inputs are NOT preserved through the interpolation: 0 * inf is NaN, and a NaN spreads to every element that taps it.
 * warp_host / warp_dev: both NULL (the records are drawn) or both given: float [n][2][6] records used INSTEAD of the drawn ones, the host
 * copy checked here (every entry finite, |a| <= 8, |t| <= 2^20), the device copy read by the kernel (the desc_host / desc_dev arrangement).
 * warp_out (or NULL): DEVICE float [n][2][6], the records used.  S <= 2^24. */
int bdn_sample_patches_warp(const void* cities_dev, const int32_t* city_hw_host, int n_cities, int C,
                            const int32_t* desc_host, const int32_t* desc_dev, int n, int S,
                            float* out_d1, float* out_d2, uint8_t* out_labels, const uint64_t* keys_dev,
                            uint64_t seed, int J, int flags, float gain, float bias, float sigma, float erase_p,
                            int lo, int hi, int erase_label, float erase_fill,
                            int32_t* drawn_geom, float* drawn_radio,
                            float rotate_rad, float log2_lo, float log2_hi, float misreg, int oob_label,
                            const float* warp_host, const float* warp_dev, float* warp_out, void* stream);
/* ---- mixing across samples: CutMix boxes (French et al., BMVC 2020) and copy-paste of change objects (Ghiasi et al., CVPR 2021) on
 * the patches the entries above cut.  No reference: utils/dataloaders.py:148-165 transforms one sample at a time.  A mixed sample (the
 * recipient) takes every band of both dates and the label byte of ONE donor sample wherever a mask is set; bits are moved, never computed.
 * bdn_mix_plan: HOST only (no device call, no stream).  keys_host: uint64 [n], 8-byte aligned, the recipients' sample keys.  Draws of
 *   sample k, from stream 0x4D495820 ('MIX ') keyed by (seed, keys_host[k]) as above:
 *     slot 0   mixed iff u(w0) < p (p a float32 in [0, 1]);  donor_index = pool[range(w1, n_pool)], pool_host int32 [n_pool] or NULL
 *              (then pool[i] = i and n_pool is the dataset length);  h = lo + range(w2, hi - lo + 1), w alike from w3; 1 <= lo <= hi <= S.
 *     slot 1   mode 0 (box) only: top = range(w0, S - h + 1), left = range(w1, S - w + 1).  Mode 1 (object): the rectangle is
 *              (0, 0, S, S) and slot 1 is not drawn.
 *   plan_host: int32 [n][8] = (on, donor_index, donor_row, top, left, h, w, 0); donor_row = n + the number of mixed samples before this
 *   one; an unmixed sample has donor_row = -1 and zeros elsewhere.
 * bdn_mix_patches: d1, d2 f32 [rows][C][S][S], labels uint8 [rows][S][S]; rows 0..n-1 are recipients, mixed in place, rows n..rows-1
 *   donors, only read.  plan_host is checked here before the launch (on in 0..1; for a mixed sample n <= donor_row < rows and the
 *   rectangle inside the patch); plan_dev: the same table in device memory, 16-byte aligned, which the kernel reads.  mode 0: the mask is
 *   the rectangle.  mode 1: the mask is (donor labels == paste_label) dilated by a (2 margin + 1) square, margin in 0..16, donor labels
 *   outside the patch unset, confined to the patch; paste_label in 0..255.  The recipient is never read and is written only where the
 *   mask is set.  mask_out (or NULL): uint8 [n][S][S], 1 where the donor was taken and 0 elsewhere, all of an unmixed sample included.
 *   One launch whatever the data; no atomics.  S <= 2^14 (offsets inside a plane are 32 bits; every other offset is size_t).
 * bdn_patch_label_counts: counts_dev int32 [n], counts[k] = the label bytes equal to `value` (0..255) in the S x S window of descriptor k
 *   (city, row, col, sym; sym is ignored); cities_dev, city_hw_host, desc_host, desc_dev as in bdn_sample_patches, checked the same way.
 *   Integer sums, no atomics: the same bits every run. */
int bdn_mix_plan(uint64_t seed, const uint64_t* keys_host, int n, int S, float p, int mode, int lo, int hi,
                 const int32_t* pool_host, int n_pool, int32_t* plan_host);
int bdn_mix_patches(const int32_t* plan_host, const int32_t* plan_dev, int n, int rows, int C, int S, int mode, int paste_label, int margin,
                    float* d1, float* d2, uint8_t* labels, uint8_t* mask_out, void* stream);
int bdn_patch_label_counts(const void* cities_dev, const int32_t* city_hw_host, int n_cities, const int32_t* desc_host,
                           const int32_t* desc_dev, int n, int S, int value, int32_t* counts_dev, void* stream);

/* ---- optim.SGD(lr) step, train.py:55,95: p -= lr * grad_scale * g over a flat f32 buffer ---- */
int bdn_sgd_step(float* params, const float* grads, float lr, float grad_scale, size_t n, void* stream);
/* ---- optim.SGD(momentum, dampening, weight_decay, nesterov) step, train.py:55-56,95 (torch 2.10 single-tensor rule), g = grad_scale * grads:
 * g += weight_decay*p; buf = g on the first step, momentum*buf + (1-dampening)*g after it; g = g + momentum*buf (nesterov) or buf; p -= lr*g.
 * momentum_buf: NULL iff momentum == 0.  All buffers 16-byte aligned f32 of n elements. ---- */
int bdn_sgd_momentum_step(float* params, const float* grads, float* momentum_buf, float lr, float grad_scale, float momentum,
                          float dampening, float weight_decay, int nesterov, int first_step, size_t n, void* stream);
/* ---- optim.Adam / optim.AdamW step, train.py:56,95 (torch 2.10 single-tensor rule), g = grad_scale * grads: weight decay as
 * p *= 1 - lr*wd (decoupled_weight_decay, AdamW) or g += wd*p (Adam); m = m + (1-beta1)*(g-m); v = beta2*v + (1-beta2)*g*g;
 * p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps), bc_i = 1 - beta_i^step computed in double on the host.
 * step: 1-based, the count AFTER this step's increment (no device sync).  The betas are double, as torch's hyperparameters are: 1 - beta2
 * of a float 0.999 is 1.3e-5 away from 1 - 0.999, a hundred float32 ulps. ---- */
int bdn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float lr, float grad_scale,
                  double beta1, double beta2, float eps, float weight_decay, int decoupled_weight_decay, long long step,
                  size_t n, void* stream);
/* ---- the three rules above with parameter groups and frozen tensors, train.py:55-56,95: one launch in which every float4 of the flat
 * buffers takes lr / weight_decay of the group its tensor belongs to, or is skipped (a frozen vector is neither read nor written:
 * parameter, gradient and state keep their bits).  n: a multiple of 4 (every tensor padded to a float4, as FlatLayout does).
 * seg_end, seg_group: DEVICE arrays of n_seg (1..256) entries that tile [0, n/4): seg_end the sorted segment ends in float4 units,
 * seg_group the group of each segment, 0..n_groups-1, or -1 = frozen.  They are read by the kernel only (nothing here waits for the
 * device), so upload them when the groups change, not per step; a vector behind the last end or with an id outside the groups is
 * skipped.  lr, weight_decay: HOST arrays of n_groups (1..8, else BDN_E_ARG) floats, passed on by value in the kernel arguments.
 * Everything else (momentum, dampening, nesterov, betas, eps, the step count) is one per launch and means what it means above; the
 * element formulas are the same device functions, so one group over the whole buffer gives the bits of the plain entry points. ---- */
int bdn_sgd_step_grouped(float* params, const float* grads, const uint32_t* seg_end, const int32_t* seg_group, int n_seg, int n_groups,
                         const float* lr, float grad_scale, size_t n, void* stream);
int bdn_sgd_momentum_step_grouped(float* params, const float* grads, float* momentum_buf, const uint32_t* seg_end,
                                  const int32_t* seg_group, int n_seg, int n_groups, const float* lr, const float* weight_decay,
                                  float grad_scale, float momentum, float dampening, int nesterov, int first_step, size_t n, void* stream);
int bdn_adam_step_grouped(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint32_t* seg_end,
                          const int32_t* seg_group, int n_seg, int n_groups, const float* lr, const float* weight_decay, float grad_scale,
                          double beta1, double beta2, float eps, int decoupled_weight_decay, long long step, size_t n, void* stream);

/* ---- the three grouped rules with one more factor on the gradient, read from DEVICE memory: g = (grad_scale * *dev_scale) * grads.
 * dev_scale (not NULL, 4-byte aligned) is read by the kernel, once per block when the per-group parameters are staged (plain SGD: the
 * host-formed lr * grad_scale is multiplied there), so a clip coefficient that bdn_grad_norm has just written reaches the update
 * without a host round trip and without a scaling pass over the gradients.  Everything else as above; with *dev_scale == 1.0f the
 * bits are those of the plain grouped entry points. ---- */
int bdn_sgd_step_grouped_ex(float* params, const float* grads, const uint32_t* seg_end, const int32_t* seg_group, int n_seg, int n_groups,
                            const float* lr, float grad_scale, const float* dev_scale, size_t n, void* stream);
int bdn_sgd_momentum_step_grouped_ex(float* params, const float* grads, float* momentum_buf, const uint32_t* seg_end,
                                     const int32_t* seg_group, int n_seg, int n_groups, const float* lr, const float* weight_decay,
                                     float grad_scale, const float* dev_scale, float momentum, float dampening, int nesterov,
                                     int first_step, size_t n, void* stream);
int bdn_adam_step_grouped_ex(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint32_t* seg_end,
                             const int32_t* seg_group, int n_seg, int n_groups, const float* lr, const float* weight_decay,
                             float grad_scale, const float* dev_scale, double beta1, double beta2, float eps,
                             int decoupled_weight_decay, long long step, size_t n, void* stream);

/* ---- gradient accumulation: dst = src (add = 0) or dst = dst + src (add = 1, one IEEE float32 add per element) over n floats; both
 * 16-byte aligned, n arbitrary (float4 body, scalar tail).  Called on sub-ranges (dst + a, src + a, b - a) with a, b multiples of 4. ---- */
int bdn_grad_accumulate(float* dst, const float* src, size_t n, int add, void* stream);

/* ---- the global L2 norm of the gradients and torch.nn.utils.clip_grad_norm_'s coefficient, both left on the device:
 *   out[0] = (float)(grad_scale * sqrt(sum g^2)),  out[1] = clamp(max_norm / (out[0] + 1e-6f), max = 1.0f)   (float32, torch's formula, the
 *   quotient formed as torch forms a float over a tensor: (1 / (out[0] + 1e-6f)) * max_norm; a NaN norm gives a NaN coefficient;
 *   max_norm = +inf gives 1: measure only).
 * n: a multiple of 4.  n_seg = 0: every element counts.  n_seg in 1..256: seg_end / seg_group are the DEVICE segment table of the grouped
 * update rules, and a vector of a segment with group id -1 (frozen), or behind the last end, is NOT READ (torch skips parameters
 * without a gradient).  Each float32 is converted to double before it is squared; sums are double.  Two launches, no atomics, no memset:
 * one double per block of 4096 vectors (16384 floats) into `workspace` (bdn_grad_norm_workspace_bytes(n) bytes, 8-byte aligned; the
 * block count depends on n only, reductions run in a fixed order: bit-identical on any device), then one thread adds them in index
 * order.  max_norm negative or NaN: BDN_E_ARG. ---- */
size_t bdn_grad_norm_workspace_bytes(size_t n);
int bdn_grad_norm(const float* grads, const uint32_t* seg_end, const int32_t* seg_group, int n_seg, float grad_scale, float max_norm,
                  void* workspace, float* out, size_t n, void* stream);

/* ---- layer-wise adaptive updates: LAMB (You et al., ICLR 2020) and LARS (You, Gitman, Ginsburg 2017) over the flat f32 buffers.
 * Both read g = (grad_scale * *dev_scale) * grads (dev_scale: DEVICE float, 4-byte aligned, or NULL = 1) and scale each TENSOR's update
 * by a trust ratio formed from two norms of that tensor, taken before any parameter changes.
 * LAMB (state exp_avg, exp_avg_sq; step as in bdn_adam_step; the moments are that entry's statements, so the state carries its bits):
 *   m = m + (1-beta1)*(g-m); v = beta2*v + (1-beta2)*g*g; r = (m / bc1) / (sqrt(v)/sqrt(bc2) + eps), bc_i = 1 - beta_i^step formed in
 *   double on the host; u = r + wd_group*p.  Per tensor t: wn = ||p_t||, un = ||u_t||; ratio = wn/un if wn > 0 and un > 0, else 1;
 *   ratio = min(ratio, max_trust) when max_trust > 0; ratio = 1 when the tensor's adapt flag is 0.  p -= lr_group * ratio * u.
 * LARS (state momentum_buf, NULL iff momentum == 0): per tensor wn = ||p_t||, gn = ||g_t||; local = trust_coef * wn /
 *   (gn + wd_group*wn + lars_eps) if wn > 0 and gn > 0, else 1; the max_trust clamp and the adapt flag as for LAMB;
 *   d = local * (g + wd_group*p); then bdn_sgd_momentum_step's buffer, dampening and Nesterov formulas with d in place of the decayed
 *   gradient (buf = d on the first step, momentum*buf + (1-dampening)*d after it; d + momentum*buf or buf); p -= lr_group * (...).
 * With every ratio 1, LAMB is AdamW and LARS is SGD(momentum, weight_decay) up to the association of the decay term.
 * The per-tensor table: DEVICE arrays of n_tensors (1..256) entries, read by the kernels only (upload them when the groups change, not
 *   per step): ten_end (uint32) the sorted tensor ends in float4 units, tiling [0, n/4) like seg_end; ten_len (uint32) the real element
 *   count of each tensor (the last vector of a tensor is masked by it: a pad element never enters a norm, whatever it holds); ten_group
 *   (int32) 0..n_groups-1, or -1 = frozen (neither read nor written: parameter, gradient and state keep their bits); ten_adapt (int32)
 *   0 or 1.  A vector behind the last end or with a group id outside the groups is skipped.
 * lr, weight_decay: HOST arrays of n_groups (1..8) floats.  n: a multiple of 4.  All flat buffers 16-byte aligned.
 * workspace: DEVICE, 8-byte aligned, bdn_layerwise_workspace_bytes(n, n_tensors) bytes; never read before it is written.
 * trust_out: DEVICE float32 [n_tensors][3] = {wn, un or gn, the applied ratio}, {0, 0, 0} for a frozen tensor; the apply pass reads the
 *   ratio from it.
 * Three launches, always: partial sums (one pair of doubles per intersection of a 1024-vector chunk with a tensor; a chunk inside one
 *   tensor is summed by its whole block, a chunk that holds several tensors gives them to its four waves in turn), a finish with one wave per tensor,
 *   the apply pass.  No atomics, no memset, no host read-back; every float32 is converted to double before it is squared, sums are
 *   double and run in an order fixed by (n, table): the same bits on every run and any device, from any workspace contents.  LAMB's first
 *   pass writes the new moments and the apply pass recomputes u from them and the still-old parameter through the same device function:
 *   no n-sized scratch.
 * BDN_E_ARG: null pointers, misalignment, n % 4, n_tensors or n_groups out of range, betas outside [0, 1), a negative eps, trust_coef,
 *   lars_eps or max_trust (0: no clamp), Nesterov with dampening or without momentum, momentum_buf given iff momentum != 0, step < 1. ---- */
size_t bdn_layerwise_workspace_bytes(size_t n, int n_tensors);
int bdn_lamb_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint32_t* ten_end, const uint32_t* ten_len,
                  const int32_t* ten_group, const int32_t* ten_adapt, int n_tensors, int n_groups, const float* lr,
                  const float* weight_decay, float grad_scale, const float* dev_scale, double beta1, double beta2, float eps,
                  float max_trust, long long step, void* workspace, float* trust_out, size_t n, void* stream);
int bdn_lars_step(float* params, const float* grads, float* momentum_buf, const uint32_t* ten_end, const uint32_t* ten_len,
                  const int32_t* ten_group, const int32_t* ten_adapt, int n_tensors, int n_groups, const float* lr,
                  const float* weight_decay, float grad_scale, const float* dev_scale, float momentum, float dampening, int nesterov,
                  int first_step, float trust_coef, float lars_eps, float max_trust, void* workspace, float* trust_out, size_t n,
                  void* stream);

/* ---- sharpness-aware minimisation over the flat f32 buffers: SAM (Foret et al., ICLR 2021) and ASAM (Kwon et al., ICML 2021).
 * bdn_sam_perturb moves the parameters to w + e, the point whose gradient a SAM update applies at w; bdn_sam_restore moves them back.
 *   t_i = |w_i| when adaptive = 1 (ASAM), else 1;  norm = sqrt(sum (t_i * g_i)^2) over the real elements of every non-frozen tensor;
 *   out[0] = (float)norm, out[1] = rho / (out[0] + eps) in float32;  saved_i = w_i, then w_i += ((out[1] * t_i) * t_i) * g_i: float32
 *   products in that order and one float32 add, none contracted; a product that is exactly 0 leaves w_i's bits alone.
 * The per-tensor table is bdn_lamb_step's without the adapt flags: DEVICE arrays of n_tensors (1..256) entries, ten_end (uint32, sorted
 *   ends in float4 units tiling [0, n/4)), ten_len (uint32, the real element count: a pad element behind it inside the tensor's last
 *   float4 never enters the norm and keeps its bits, whatever it holds), ten_group (int32, -1 = frozen, anything >= 0 trainable).  A
 *   frozen tensor, and a vector behind the last end, is neither read nor written in params, grads or saved.
 * out: DEVICE float32 [2].  workspace: DEVICE, 8-byte aligned, bdn_sam_workspace_bytes(n, n_tensors) bytes (one double per 4096
 *   vectors today, whatever n_tensors), never read before it is written.  n: a multiple of 4; params, saved, grads 16-byte aligned.
 * Three launches, always: one double per block of 4096 vectors, one thread adds them in index order and writes out, the apply pass.
 *   Every float32 is converted to double before it is multiplied, the sums are double and run in an order fixed by (n, table): no
 *   atomics, no memset, no host read-back, the same bits on every run and any device, from any workspace contents.  A zero gradient
 *   gives out[0] = 0 and leaves params as they are (eps > 0: without a NaN).  A non-finite gradient is no special case: out is
 *   non-finite then, and so are the parameters until the restore.
 * bdn_sam_restore: ONE launch, params = saved bit for bit on exactly the float4s bdn_sam_perturb wrote under the same table: a copy,
 *   never a subtraction of the perturbation (w + e - e is not w in float32).
 * BDN_E_ARG, before any launch: null pointers, misalignment, params == saved, n % 4, n_tensors outside 1..256, rho <= 0 or NaN,
 *   eps < 0 or NaN, adaptive other than 0 / 1. ---- */
size_t bdn_sam_workspace_bytes(size_t n, int n_tensors);
int bdn_sam_perturb(float* params, float* saved, const float* grads, const uint32_t* ten_end, const uint32_t* ten_len,
                    const int32_t* ten_group, int n_tensors, float rho, int adaptive, float eps, void* workspace, float* out, size_t n,
                    void* stream);
int bdn_sam_restore(float* params, const float* saved, const uint32_t* ten_end, const int32_t* ten_group, int n_tensors, size_t n,
                    void* stream);

/* ---- averaged weights (torch.optim.swa_utils.AveragedModel's EMA / SWA) over the flat f32 buffers of the fused step.
 * bdn_ema_update: copy = 1: avg = params bit for bit (AveragedModel's first update); copy = 0: avg = lerp(avg, params, weight) by torch's
 *   element formula in float32, weight < 0.5: avg + weight * (p - avg), otherwise p - (p - avg) * (1 - weight) -- so weight 0 keeps avg's
 *   bits and weight 1 gives p's (for finite values other than -0).  EMA: weight = 1 - decay; SWA: weight = 1 / (n_averaged + 1).  weight
 *   outside [0, 1] or NaN, or copy other than 0 / 1: BDN_E_ARG.
 * bdn_swap_segments: exchanges a and b in place (bits are moved, not computed); a == b: BDN_E_ARG.
 * Both: n a multiple of 4, buffers 16-byte aligned.  n_seg = 0: every vector counts.  n_seg in 1..256: seg_end / seg_group are the DEVICE
 *   segment table of the grouped update rules above; a vector of a segment with group id -1 (frozen) or an id outside 0..7, or behind the
 *   last end, is neither read nor written in either buffer, every other group id counts alike.  One launch of the grouped rules' kernel
 *   (the same LDS-staged lookup, one float4 per lane, every load of a pass issued before the first store, no atomics: bit-reproducible).
 * bdn_ema_update_multi: the same rule (weight, copy) over n_tensors (0..65535) small tensors in ONE launch.  desc_dev: DEVICE array of
 *   n_tensors records { float* avg; const float* src; int32 len; int32 pad; } (24 bytes each, 8-byte aligned); the pointers need 4-byte
 *   alignment only (a float4 body where both are 16-byte aligned, one element per lane otherwise and for the len % 4 tail).  max_len:
 *   the largest len, sizes the grid only (every tensor is grid-strided to its own len; len <= 0 is skipped).
 * Every pointer is device memory; nothing waits for the device; all work is enqueued on `stream`. ---- */
int bdn_ema_update(float* avg, const float* params, const uint32_t* seg_end, const int32_t* seg_group, int n_seg, float weight, int copy,
                   size_t n, void* stream);
int bdn_ema_update_multi(const void* desc_dev, int n_tensors, int max_len, float weight, int copy, void* stream);
int bdn_swap_segments(float* a, float* b, const uint32_t* seg_end, const int32_t* seg_group, int n_seg, size_t n, void* stream);

/* ---- threshold-free validation: the score histogram, the precision / recall curve and a thresholded scene mask.  The reference judges
 * a model at the argmax only -- train.py:96-106 and train.py:151-158 (argmax + sklearn's prfs per batch), train.py:199 (the scene mask) --
 * which for two classes is a probability threshold of 0.5.
 * bdn_score_hist (replaces train.py:96-106 / train.py:151-158): x [n_img][ncls][HW] f32 (a logits batch [B,ncls,H,W], or a scene
 *   probability map [ncls,H,W] with n_img = 1; HW is 64-bit: a 10 000^2 scene works), labels [n_img][HW] uint8.  The score of a pixel is
 *   s = P(pos_class): x_is_logits = 1: formed exactly as bdn_blend_fold forms it (m = max_c l_c, e_c = expf(l_c - m), sum in class order,
 *   e_pos / sum); x_is_logits = 0: x[pos_class] as it is.  bin = n_bins - 1 if s >= 1, (int)(s * n_bins) if s > 0, 0 otherwise (NaN lands
 *   there); n_bins is a power of two in 2..4096, so the product is exact and bin >= i <=> s >= (float)i / n_bins.  A pixel whose label
 *   equals ignore_label (0..255; -1 = none) is skipped before any of its logits is used (inf / NaN there reaches no output); a pixel is
 *   positive iff label == pos_class, every other valid label (values >= ncls included) is negative.  hist: uint64 [2][n_bins], negatives
 *   first; the kernel ADDS into it -- zero it once per pass, then accumulate batches without a host sync.  scores_out (NULL: not stored):
 *   f32 [n_img][HW], every pixel's score and exactly 0.0f at an ignored pixel (written, not skipped).  Integer atomics (LDS and global)
 *   carry the counts: integer sums do not depend on arrival order, so hist is the same bits on every run.  At most 2^40 pixels per call.
 * bdn_score_curve (replaces the prfs of train.py:103-106 / train.py:155-158): one launch, one block, fixed order, double precision.
 *   For threshold index i in 0..n_bins-1, t_i = i / n_bins (predict positive iff bin >= i): TP_i = sum_{b>=i} hist[1][b],
 *   FP_i = sum_{b>=i} hist[0][b] (exact 64-bit suffix sums), n_pos = TP_0, n_neg = FP_0, P_i = TP_i / (TP_i + FP_i), R_i = TP_i / n_pos,
 *   F_i = 2 TP_i / (2 TP_i + FP_i + n_pos - TP_i): each one correctly rounded double division of integers, 0 where the denominator is 0.
 *   AP = sum_i (R_i - R_{i+1}) P_i with R_{n_bins} = 0 (sklearn's average_precision_score on the bin-quantised scores).  The best
 *   threshold is the first maximum of F_i in ascending i.  summary: double[8] = {F_best, t_best, i_best, P_best, R_best, AP, n_pos,
 *   n_neg}; curve_out (NULL: not stored): double [4][n_bins] = {TP, FP, P, R}.  An all-zero histogram gives an all-zero summary.
 * bdn_threshold_mask (replaces train.py:199 where a threshold is wanted): mask[i] = proba[pos_class][i] >= threshold as uint8 0 / 1 for a
 *   [ncls][HW] f32 map; threshold outside [0, 1] or NaN: BDN_E_ARG. ---- */
int bdn_score_hist(const float* x, int x_is_logits, const uint8_t* labels, int ignore_label, int pos_class, int n_img, int ncls,
                   long long HW, int n_bins, unsigned long long* hist, float* scores_out, void* stream);
int bdn_score_curve(const unsigned long long* hist, int n_bins, double* curve_out, double* summary, void* stream);
int bdn_threshold_mask(const float* proba, int pos_class, float threshold, uint8_t* mask, int ncls, long long HW, void* stream);

/* ---- connected components of a scene mask: label, compact, filter by area, per-object statistics.  They replace the host-side
 * scipy.ndimage.label + np.bincount after a device-to-host copy of the scene mask that train.py:199 produces (the reference stops at the
 * pixel mask; dropping speckle and counting objects are the steps a change-detection product takes next).  All rasters are [H][W]
 * row-major, 1 <= H, W and H * W <= 2^31 - 2; connectivity is 4 or 8; a null required pointer, a misaligned pointer or a value outside
 * its range is BDN_E_ARG before any launch.  Integer arithmetic only: integer sums do not depend on arrival order and a component's root
 * is its smallest linear index y * W + x whatever the schedule, so every output is the same bits on every run.  The number of launches
 * depends on H and W only; nothing is read back; no loop waits for another thread and every chain walk is capped (counts[2]).
 * bdn_cc_workspace_bytes: the workspace of bdn_cc_label and bdn_cc_compact (16-byte aligned; 0 for a shape outside the limits).  The
 *   kernels initialise every word they read: a workspace born 0xFF gives the outputs of a zeroed one.  bdn_cc_tile: the tile edge (64).
 * bdn_cc_label: a pixel is foreground iff src[i] == fg_value (uint8) and, with exclude non-NULL, exclude[i] != exclude_value (the ignore
 *   label of a truth raster applied to a predicted mask).  labels int32 [H][W]: 0 on background, 1 + r elsewhere, r the smallest linear
 *   index of the pixel's component (canonical: comparable without relabelling).  area int32 [H][W] (NULL: not computed): the component's
 *   pixel count at its root pixel r, 0 everywhere else (written, not skipped).  counts int32[4] = {n_components, n_foreground, status, 0};
 *   status is non-zero only if an iteration cap was hit (the result is then unspecified).  Three launches (tiles in LDS, seams, flatten).
 * bdn_cc_compact: compact int32 [H][W] (not aliasing labels): 0 on background, elsewhere the 1-based rank of the pixel's root among all
 *   roots in ascending index -- scipy.ndimage.label's numbering.  counts (NULL allowed): counts[0] = the number of roots, the other
 *   words stay.  Four launches: block sums, one block scanning them, ranks at the roots, ranks spread; no block waits for another.
 * bdn_cc_filter: out_mask[i] (uint8) = 1 iff labels[i] != 0 and area[labels[i] - 1] >= min_area, else 0; min_area <= 1 keeps every
 *   foreground pixel (area may then be NULL).  src_mask is not read (labels carry the foreground test) and out_mask may alias it.
 * bdn_cc_stats: table int32 [n_max][8] = {area, ymin, xmin, ymax, xmax, overlap, 0, 0} of compact label k in row k - 1; overlap = the
 *   component's pixels with other[i] == other_value (other uint8, NULL: 0); a pixel with other[i] == other_exclude_value (-1: none) adds
 *   to no column.  Rows of labels that do not occur are {0, H, W, -1, -1, 0, 0, 0}; a label above n_max (1..2^28 - 1) is skipped.  The
 *   kernel initialises the table itself, then integer atomicAdd / atomicMin / atomicMax.
 * Every pointer is device memory; nothing waits for the device; all work is enqueued on `stream`. ---- */
size_t bdn_cc_workspace_bytes(int H, int W);
int bdn_cc_tile(void);
int bdn_cc_label(const uint8_t* src, int fg_value, const uint8_t* exclude, int exclude_value, int connectivity, int H, int W,
                 int32_t* labels, int32_t* area, int32_t* counts, void* workspace, void* stream);
int bdn_cc_compact(const int32_t* labels, int H, int W, int32_t* compact, int32_t* counts, void* workspace, void* stream);
int bdn_cc_filter(const uint8_t* src_mask, const int32_t* labels, const int32_t* area, int min_area, uint8_t* out_mask, int H, int W,
                  void* stream);
int bdn_cc_stats(const int32_t* compact, int n_max, const uint8_t* other, int other_value, int other_exclude_value, int H, int W,
                 int32_t* table, void* stream);

/* ---- exact squared Euclidean distance transform, the boundary loss and the boundary scores built on it.  They replace a device-to-host
 * copy and scipy.ndimage.distance_transform_edt.  Rasters are [N][H][W] row-major uint8; 1 <= N, 1 <= H, W <= 32767 and N*H*W < 2^31, so
 * every squared distance fits an int32.  Integer arithmetic only (the signed distance takes one correctly rounded square root of an integer: the float64 root rounded to float32);
 * a fixed number of launches for a shape; no float atomics, no host read-back, no kernel waits for another block; the caller never
 * clears a workspace: the same bits on every run, whatever the workspace held.  A null required pointer, a misaligned one, a value
 * outside its range or a shape outside the limits is BDN_E_ARG before anything touches a device.
 * bdn_edt: the N images are independent.  A pixel is valid unless valid_src is given and its byte there equals invalid_value; it is a site
 *   if it is valid and its byte in src compares to site_value as site_equal says (1: ==, 0: !=).
 *       out_d2[n][y][x] = min(limit, min over the sites (y', x') of image n of (y - y')^2 + (x - x')^2)
 *   limit in 1..2^31-1; an image without a site gives limit everywhere, a site 0.  Two launches: per column the distance to the nearest
 *   site of the column (one thread per column, a down and an up sweep), then per row the lower envelope of the parabolas
 *   (x - x')^2 + g(x')^2 (Meijster, Roerdink, Hesselink 2000), one lane per row over the transposed column result: O(W) per row for every
 *   input.  Rows up to 128 wide keep their stack in LDS, wider ones in the workspace.  ws: bdn_edt_workspace_bytes() bytes (0 for a shape
 *   outside the limits), 16-byte aligned: 2 bytes per pixel, 6 for W > 128.
 * bdn_boundary_loss: the boundary term of Kervadec et al. (MIDL 2019) on float32 NCHW logits and uint8 labels, an add-on pass with the
 *   calling shape of bdn_lovasz_softmax.
 *   Valid       the n pixels of the batch whose label is not ignore_label (-1: none is ignored).
 *   Included    classes 1..ncls-1 (classes_all = 0, the paper's choice for the binary case) or every class (classes_all = 1).
 *   Distance    per image and included class c, on the device each call: fg = valid and label == c, bg = valid and label != c (a valid
 *               label >= ncls is foreground of no class);  phi_c = +sqrtf(d2 to the nearest fg pixel) at a bg pixel,
 *               -(sqrtf(d2 to the nearest bg pixel) - 1) at an fg pixel, 0 at an ignored pixel, and 0 over an image without an fg or
 *               without a bg pixel of the class (no contour) -- the paper's one_hot2dist with the ignored pixels out of both site sets.
 *               max_dist > 0 clamps phi to [-max_dist, max_dist]; 0: no clamp.
 *   Term        p = softmax(logits) as bdn_criterion forms it; term = (1/n) sum over valid pixels and included classes of p_c phi_c, in
 *               double in a fixed order.  n = 0: term 0, gradient 0.  The term can be negative.
 *   Gradient    phi is a constant; phi'_c = phi_c for an included class, 0 otherwise; dterm / dlogit_j = p_j (phi'_j - sum_c phi'_c p_c) / n.
 *               Exactly 0.0f at an ignored pixel, none of whose logits is read.
 *   accumulate, loss, term, dlogits = NULL: exactly as in bdn_lovasz_softmax.  phi_out: NULL or f32[ncls][B*H*W], 0 for a class that is
 *               not included.
 *   Five launches (four without dlogits): the two of the transform over 2 x included classes x B images, phi and the blocks' partial
 *   sums, the finish, the gradient.  ws: bdn_boundary_workspace_bytes() bytes (0 for an invalid shape; sized for classes_all = 1),
 *   16-byte aligned.  weight >= 0; max_dist >= 0; ncls in 2..8; 2*ncls*B*H*W < 2^31.  Data-parallel: each rank uses its own n.
 * bdn_signed_distance: phi of one class cls (0..255) of [N][H][W] labels, as defined above, without logits: three launches.
 * bdn_boundary_mask: out[i] (uint8) = 1 iff pixel i is valid, src[i] == fg_value and one of its 4-neighbours inside the image is valid
 *   and not fg_value, else 0 (valid as in bdn_edt): valid & fg & ~binary_erosion(fg | ~valid, cross, border_value = 1).  The image edge
 *   and the invalid region make no contour.  One [H][W] raster; out must not alias src.
 * bdn_boundary_score: bnd uint8 [2][H][W] = the boundary sets of the prediction and of the truth, d2 int32 [2][H][W] = bdn_edt of bnd with
 *   site_value 1 and limit 2^31-1.  out int64[6] = {n_pred, n_true, pred_hit, true_hit, hd2_pred_to_true, hd2_true_to_pred}: the set
 *   sizes, the boundary pixels whose d2 to the other set is <= tol2, and the largest d2 of a set's pixels to the other set (-1 if either
 *   set is empty).  Integer block sums, one 64-bit atomicAdd per block and count, integer atomicMax; out is cleared by the call.
 * Every pointer is device memory; nothing waits for the device; all work is enqueued on `stream`. ---- */
size_t bdn_edt_workspace_bytes(int N, int H, int W);
int bdn_edt(const uint8_t* src, int site_value, int site_equal, const uint8_t* valid_src, int invalid_value, int limit, int32_t* out_d2,
            void* ws, int N, int H, int W, void* stream);
size_t bdn_boundary_workspace_bytes(int B, int ncls, int H, int W);
int bdn_boundary_loss(const float* logits, const uint8_t* labels, int ignore_label, int classes_all, float max_dist, float weight,
                      int accumulate, void* ws, float* loss, float* term, float* dlogits, float* phi_out, int B, int ncls, int H, int W,
                      void* stream);
size_t bdn_signed_distance_workspace_bytes(int N, int H, int W);
int bdn_signed_distance(const uint8_t* labels, int cls, int ignore_label, float max_dist, void* ws, float* phi, int N, int H, int W,
                        void* stream);
int bdn_boundary_mask(const uint8_t* src, int fg_value, const uint8_t* valid_src, int invalid_value, uint8_t* out, int H, int W,
                      void* stream);
int bdn_boundary_score(const uint8_t* bnd, const int32_t* d2, long long tol2, long long* out, int H, int W, void* stream);

/* ---- cleaning a scene mask: binary reconstruction on bdn_cc_label's labels (hysteresis thresholding, hole filling, border clearing) and
 * disc morphology as a threshold on bdn_edt's squared distances.  Each replaces a host-side scipy.ndimage call after a device-to-host copy
 * of the mask of train.py:199 (the reference stops at the pixel mask).  Rasters are [H][W] row-major; 1 <= H, W and H * W <= 2^31 - 2 (the
 * limits of bdn_cc_label).  Integers only but for the two comparisons of bdn_threshold_pair; a fixed number of launches; nothing is read
 * back; no loop waits for another thread; every store of a flag stores the same 1, so every output is the same bits on every run.  A null
 * required pointer, a misaligned one, a value outside its range or a shape outside the limits is BDN_E_ARG before anything touches a
 * device.  Four pixels per thread where W (n, HW) % 4 == 0 and the pointers are aligned (int32 16, uint8 4 bytes), one otherwise.
 * bdn_cc_mark (replaces the seed test of scipy.ndimage.binary_propagation / the border test of binary_fill_holes): labels int32 [H][W] as
 *   bdn_cc_label writes them (0 or 1 + root index).  mark int32 [H][W] (not aliasing labels) is written everywhere by the call: 0, then 1
 *   at index r if the component rooted at r has a pixel with seed[i] == seed_value (seed uint8 [H][W], NULL: no seed) or, with border != 0,
 *   a pixel in row 0, row H - 1, column 0 or column W - 1.  Two launches (clear, mark); what mark held before does not matter.
 * bdn_cc_select (replaces the propagation itself): with sel(i) = labels[i] != 0 and (mark[labels[i] - 1] != 0) == keep_marked and
 *   min_area <= area[labels[i] - 1] <= max_area,  out[i] (uint8) = (base && base[i] == 1) || sel(i).  mark NULL: no flag test; area NULL
 *   (bdn_cc_label's areas otherwise): the bounds must be 1 and 2^31 - 1; base NULL: sel alone.  out may alias base.  One launch.
 * bdn_d2_mask (replaces scipy.ndimage.binary_dilation / binary_erosion with a disc): out[i] (uint8) = greater ? d2[i] > r2 : d2[i] <= r2 for
 *   n int32 squared distances (bdn_edt with limit r2 + 1 suffices); r2 >= 0, 1 <= n < 2^31.  One launch.
 * bdn_threshold_pair (replaces two passes of train.py:199's thresholding): mask_low[i] = proba[pos_class][i] >= low and mask_high[i] =
 *   proba[pos_class][i] >= high (uint8 0 / 1, two different rasters) in one pass over a [ncls][HW] f32 map; a NaN probability gives 0 in
 *   both.  low / high outside [0, 1], NaN or low > high: BDN_E_ARG.  2 <= ncls <= 256, 1 <= HW <= 2^31 - 2.  One launch.
 * bdn_mask_not (the background raster that scipy.ndimage.binary_fill_holes labels): out[i] (uint8) = src[i] != 1, 1 <= n < 2^31, out not
 *   aliasing src.  One launch.
 * Every pointer is device memory; nothing waits for the device; all work is enqueued on `stream`. ---- */
int bdn_cc_mark(const int32_t* labels, const uint8_t* seed, int seed_value, int border, int32_t* mark, int H, int W, void* stream);
int bdn_cc_select(const int32_t* labels, const int32_t* mark, int keep_marked, const int32_t* area, int min_area, int max_area,
                  const uint8_t* base, uint8_t* out, int H, int W, void* stream);
int bdn_d2_mask(const int32_t* d2, int r2, int greater, uint8_t* out, long long n, void* stream);
int bdn_threshold_pair(const float* proba, int pos_class, float low, float high, uint8_t* mask_low, uint8_t* mask_high, int ncls,
                       long long HW, void* stream);
int bdn_mask_not(const uint8_t* src, uint8_t* out, long long n, void* stream);

/* ---- co-registration of the two dates of a scene: the shift between them is estimated by normalised cross-correlation over integer
 * shifts, per cell of a grid and for the whole scene, refined to a fraction of a pixel, and date 2 is resampled through the shift field.
 * No reference: the reference assumes co-registered pairs.  Scenes are float32 [C][H][W] planes (what city_stack_device leaves in HBM, per
 * date); 1 <= C <= 65535, 1 <= H, W <= 32767.  Cells: a grid (ny, nx), 1..64 each, ny <= H, nx <= W; cell (i, j) owns rows
 * [floor(i H / ny), floor((i + 1) H / ny)) and the columns alike.  Sign convention: d2(y + dy, x + dx) ~ d1(y, x).  A fixed number of launches
 * whatever the data, no atomics, no host read-back, no kernel waits for another block; the caller never clears a workspace: the same bits
 * on every run, whatever the workspace held.  A null required pointer, a misaligned one, a value outside its range or a shape outside the
 * limits is BDN_E_ARG before anything touches a device.
 * bdn_shift_corr: bands: DEVICE int32 [n_b], 1 <= n_b <= 64, indices into C (an index outside [0, C) reads nothing: its entries are 0).
 *   R: the search radius, 1..16.  exclude (or NULL): uint8 [H][W]; exclude_value 0..255.
 *       table[b][i][j][dy + R][dx + R][0..5] = {n, sum a, sum b, sum a^2, sum b^2, sum a b}     (float64, dy-major, dy, dx in [-R, R])
 *   over the pixels (y, x) of cell (i, j) with a = d1[bands[b]][y][x], b = d2[bands[b]][y + dy][x + dx], for which (y + dy, x + dx) lies
 *   inside the scene (in whichever cell), neither exclude[y][x] nor exclude[y + dy][x + dx] equals exclude_value, and a and b are both
 *   finite: a NaN or infinite nodata pixel leaves the sums.  Every product is formed in double from the float32 values, so every term is
 *   exact; every sum is a chain of double additions in a fixed order, one rounding per term: an entry lies within
 *   (n - 1) 2^-53 sum |term| of the exact sum, and n is exact.  Two launches: blocks of 256 threads stage a 32 x 32 date-1 tile and the
 *   date-2 tile with its halo of R in LDS, each thread keeps the sums of up to five shifts in registers while the block walks its tiles;
 *   then the partials are added in index order.  ws: bdn_shift_corr_workspace_bytes() bytes (0 for arguments outside the limits), 16-byte
 *   aligned: P partial tables, P = max(1, min(1024 / (ny nx), 256 MiB / the table's bytes)) -- it does not grow with H W (13 bands,
 *   R = 8: 176 MiB for 1 x 1 and for 8 x 8 cells, for any scene).  The size query is host-only.
 * bdn_shift_peak: table as above (n_b, R, ny, nx the same).  The score of a shift, per cell and once more for the whole scene (whose table is
 *   the sum of the cells' tables in (i, j) order, per band and entry), is the mean over the bands of
 *       NCC = (n Sab - Sa Sb) / sqrt((n Saa - Sa Sa) (n Sbb - Sb Sb))
 *   over the bands with n >= 2 and both variances > 0, added in band order and divided by their number; a shift with no such band scores -2.
 *   Float64, one rounding per operation, in exactly the order written (each variance and the covariance a difference of two rounded
 *   products; the two variances multiplied, then the root, then the quotient): numpy float64 reproduces the score from the same table.
 *   Peak: the first maximum in raster order; each axis refined by delta = (0.5 (c- - c+)) / ((c- - 2 c0) + c+), clamped to [-0.5, 0.5];
 *   delta = 0 when the peak sits on the window border, a neighbour is undefined (-2) or the denominator is not < 0.
 *   report: float64 [ny nx + 1][4] = {dy, dx, ncc, ok}, the last row the whole scene; ok = 0 when every shift is undefined: the shift is
 *   then (0, 0) and ncc -2.  field: float32 [ny][nx][2] = (dy, dx) of the cell; a cell with ok = 0 or ncc < min_ncc takes the whole-scene
 *   shift, or (0, 0) if that is not ok either.  One launch of ny nx + 1 blocks; a cell that falls back forms the whole-scene peak itself.
 * bdn_shift_apply: out[c][y][x] = bilinear(src[c], y + s_y(y, x), x + s_x(y, x)) with a replicate border; out != src.  Float32, every
 *   operation rounded once, nothing fused, in this order.  The field between cell centres, per axis (rows; columns alike):
 *       cy_i = 0.5f (r0_i + r1_i - 1);  i0 = the last i with cy_i <= y, clamped to [0, ny - 2];  i1 = i0 + 1;
 *       t_y = clamp((y - cy_i0) / (cy_i1 - cy_i0), 0, 1);  a grid of one along the axis: i0 = i1 = 0, t_y = 0
 *       s = ((1 - t_y) * (((1 - t_x) * f[i0][j0]) + (t_x * f[i0][j1]))) + (t_y * (((1 - t_x) * f[i1][j0]) + (t_x * f[i1][j1])))     for s_y and s_x
 *   The taps and the blend are bdn_sample_patches_warp's ("mapping" above): yy = y + s_y, y0 = floorf(yy), fy = yy - y0, xx, x0, fx alike;
 *   tap rows (int)y0 and + 1, tap columns (int)x0 and + 1, each clamped into the scene (y0, x0 saturate at +-2^30 first);
 *       top = ((1 - fx) * v00) + (fx * v01),  bot = ((1 - fx) * v10) + (fx * v11),  out = ((1 - fy) * top) + (fy * bot)
 *   So a zero field returns finite inputs bit for bit (-0.0 may arrive as +0.0), an integer shift moves bits with a replicated edge, and
 *   numpy float32 reproduces the output exactly.  Non-finite inputs spread to every element that taps them.  oob (or NULL): uint8 [H][W],
 *   1 where an unclamped tap of non-zero weight lies outside the scene (the second tap of an axis has weight 0 when its fraction is 0).
 *   field: DEVICE float32 [ny][nx][2], any finite values.  One launch.
 * Every pointer is device memory; nothing waits for the device; all work is enqueued on `stream`. ---- */
size_t bdn_shift_corr_workspace_bytes(int n_b, int H, int W, int R, int ny, int nx);
int bdn_shift_corr(const float* d1, const float* d2, const int32_t* bands, int n_b, const uint8_t* exclude, int exclude_value,
                   int R, int ny, int nx, double* table, void* ws, int C, int H, int W, void* stream);
int bdn_shift_peak(const double* table, int n_b, int R, int ny, int nx, double min_ncc, double* report, float* field, void* stream);
int bdn_shift_apply(const float* src, const float* field, int ny, int nx, float* out, uint8_t* oob, int C, int H, int W, void* stream);

/* ---- radiometric matching of the two dates of a scene: order statistics per band at many probabilities at once, the piecewise-linear
 * transfer between two knot tables (quantile transfer: the knots of date 2 onto the knots of date 1), and the reference's stretch_8bit
 * (utils/dataloaders.py:38-48) arithmetic.  Scenes are float32 [C][H][W] planes; 1 <= C <= 65535, 1 <= H, W <= 32767.  A fixed number of
 * launches whatever the data, integer atomics only (histogram counts from LDS and global adds: a sum of ones has no order), no float
 * atomics, no host read-back, no kernel waits for another block; the caller never clears a workspace: the same bits on every run, whatever
 * the workspace held.  A null required pointer, a misaligned one, a value outside its range or a shape outside the limits is BDN_E_ARG
 * before anything touches a device.
 * bdn_band_quantiles: bands: DEVICE int32 [n_b], 1 <= n_b <= 64, indices into C (an index outside [0, C) reads nothing: its count is 0).
 *   The valid pixels of a band: finite; not at exclude[y][x] == exclude_value when exclude (uint8 [H][W], or NULL) is given; > 0 when
 *   positive_only = 1 (stretch_8bit's rule).  count[b] (int64) = n, their number.  probs: DEVICE float64 [n_q], 1 <= n_q <= 1024, each in
 *   [0, 1].  For probability p:   h = p * (n - 1)  (one double multiplication),  lo = floor(h),  hi = min(lo + 1, n - 1),  t = h - lo;
 *       order[b][q][0..1] = {v_(lo), v_(hi)}   (float32) the exact order statistics, 0-based, in the total order of the bit patterns' keys
 *                                             (-0.0 below +0.0)
 *       value[b][q] = a + ((b - a) * t)        (float64) a = v_(lo), b = v_(hi); one rounding per operation, nothing fused
 *   With n = 0, or for a p outside [0, 1] (NaN included), value and both order entries are NaN.  Method: a radix select over the monotone
 *   key of a float32 in three levels of 11 + 11 + 10 bits for all 2 n_q ranks of a band together: a histogram of the top digit, the top
 *   digits the ranks fall in each get a slot, a histogram of the second digit per slot, a slot per wanted 22-bit prefix, a histogram of the
 *   last digit per slot.  Seven launches (a memset, three histogram passes over the scene, three selects) per group of bands; the bands
 *   are taken in groups of G = max(1, min(n_b, 128 MiB / band bytes)), band bytes = 16 KiB + n_q (24 KiB + 32 B).
 *   ws: bdn_band_quantiles_workspace_bytes() = G * band bytes (0 for arguments outside the limits), 16-byte aligned: at most 128 MiB, a
 *   function of n_b and n_q only -- it does not grow with H W (13 bands: 0.8 MiB at n_q = 2, 78 MiB at n_q = 256).  The size query is host-only.
 * bdn_transfer_apply: out[c] = f_b(src[c]) for the bands named (bands: DEVICE int32 [n_b], 1 <= n_b <= 64; the first row that names a band
 *   counts), a copy for the others when out != src; out == src is allowed (pointwise).  s_knots, t_knots: DEVICE float32 [n_b][K], each row
 *   nondecreasing, 2 <= K <= 1024.  For a finite x, float32, one rounding per operation, nothing fused:
 *       s_0 <= x < s_{K-1}:   k = the last index with s_k <= x  (so s_{k+1} > s_k);   seg_k(x) = t_k + ((x - s_k) * ((t_{k+1} - t_k) / (s_{k+1} - s_k)))
 *       x < s_0:              BDN_EXTRAPOLATE_OFFSET: off_0(x);      BDN_EXTRAPOLATE_SLOPE: seg_0(x) if s_1 > s_0, else off_0(x)
 *       x >= s_{K-1}:         BDN_EXTRAPOLATE_OFFSET: off_{K-1}(x);  BDN_EXTRAPOLATE_SLOPE: seg_{K-2}(x) if s_{K-1} > s_{K-2}, else off_{K-1}(x)
 *       off_e(x) = x + (t_e - s_e), and x itself where t_e - s_e == 0;   seg_k(x) = x itself where s_k == t_k and s_{k+1} == t_{k+1}
 *   so a table with t == s returns the source bit for bit.  NaN and infinite pixels pass through with their bits.  A band with a NaN knot
 *   (what a band without valid pixels in either date gets) or with exact[b] != 0 (exact: DEVICE uint8 [n_b], or NULL) passes through whole.
 *   The knot tables of the block's band sit in LDS.  One launch.
 * bdn_stretch_u8: out[c][y][x] (uint8) = trunc(clamp((x - cd[c][0]) * (255.0 / (cd[c][1] - cd[c][0])), 0, 255)) in float64, one rounding per
 *   operation; src: float32 (src_is_u16 = 0) or uint16 (1) [C][H][W]; cd: DEVICE float64 [C][2] = {c, d}.  A NaN (a NaN pixel, a NaN c or d,
 *   or x == c when d == c) gives 0; with d == c every x > c gives 255 and every x <= c gives 0.  One launch.
 * Every pointer is device memory; nothing waits for the device; all work is enqueued on `stream`. ---- */
#define BDN_EXTRAPOLATE_OFFSET 0
#define BDN_EXTRAPOLATE_SLOPE 1
size_t bdn_band_quantiles_workspace_bytes(int n_b, int n_q, int H, int W);
int bdn_band_quantiles(const float* scene, const int32_t* bands, int n_b, const uint8_t* exclude, int exclude_value, int positive_only,
                       const double* probs, int n_q, double* value, float* order, long long* count, void* ws, int C, int H, int W,
                       void* stream);
int bdn_transfer_apply(const float* src, float* out, const int32_t* bands, int n_b, const float* s_knots, const float* t_knots, int K,
                       int extrapolate, const uint8_t* exact, int C, int H, int W, void* stream);
int bdn_stretch_u8(const void* src, int src_is_u16, const double* cd, uint8_t* out, int C, int H, int W, void* stream);

/* ---- IR-MAD, the iteratively reweighted multivariate alteration detection (Nielsen 2007; Canty and Nielsen 2008) between the two dates of
 * a scene: a canonical correlation analysis of date 1 against date 2 in which every pixel is weighted by its probability of no change,
 * iterated to a fixed point.  It gives a per-pixel chi-square change statistic with its no-change probability, invariant to any affine
 * radiometric difference between the dates, and from it an invariant-pixel mask that needs no labels.  Scenes are float32 [C][H][W] planes
 * per date; 1 <= C <= 65535, 1 <= H, W <= 32767.  bands: DEVICE int32 [n_b], 1 <= n_b <= 32; exclude: NULL or uint8 [H][W] with
 * exclude_value (a byte).  A fixed number of launches whatever the data, no float atomics, no host read-back, no kernel waits for another
 * block; the caller never clears a workspace or an output: the same bits on every run, whatever those buffers held.  A null required
 * pointer, a misaligned one, a value outside its range or a shape outside the limits is BDN_E_ARG before anything touches a device.
 * Valid pixels: all 2 n_b selected values finite and exclude[y][x] != exclude_value.  A band index outside [0, C) makes every pixel
 * invalid (nothing is read).  D = 2 n_b; the vector of a pixel is (x, y) = (date 1's n_b values, date 2's n_b values).
 * bdn_mad_centre: centre[D] (float64) = the unweighted mean of the valid pixels per selected band and date (0 without a valid pixel),
 *   n_valid (int64) = their number.  Summed in double in a fixed order: block partials, then an index-order finish.  Two launches.
 * bdn_mad_moments: with z = (x - centre_x, y - centre_y) formed in double and w = weight[y][x] (float32 [H][W]; a weight that is not in
 *   [0, FLT_MAX] counts as 0; NULL: 1), over the valid pixels
 *       moments[0] = S0 = sum w;   moments[1 + k] = S1[k] = sum w z_k;
 *       moments[1 + D + k D - k (k - 1) / 2 + (l - k)] = S2[k][l] = sum w z_k z_l,  k <= l      (1 + D + D (D + 1) / 2 doubles)
 *   A term is fl(w z_k) z_l, added by one fused multiply-add; every sum is a chain of double additions in an order fixed by (n_b, H, W):
 *   an entry lies within n 2^-53 sum |term| of the exact sum of its rounded terms, n = the valid pixels.  Block partials go to ws, then an
 *   index-order reduction.  ws: bdn_mad_workspace_bytes(n_b, H, W) = min(ceil(H W / 64), 768) * 128 * T (T + 1) / 2 bytes,
 *   T = ceil((D + 1) / 4): bounded whatever the scene size (13 bands: at most 2.6 MiB; 32 bands: 14.3 MiB), 0 for arguments outside the
 *   limits; the size query is host-only; 16-byte aligned.  bdn_mad_centre takes the same ws.  state: NULL, or the state block of the run:
 *   with state[CONVERGED] != 0 the call writes nothing.  Two launches.
 * bdn_mad_solve: one block, float64.  mean_z = S1 / S0, cov = S2 / S0 - mean_z mean_z^T, cut into Sxx, Sxy, Syy; Cholesky Sxx = Lx Lx^T,
 *   Syy = Ly Ly^T; K = Lx^-1 Sxy Ly^-T; K = U diag(rho) V^T by one-sided Jacobi; a_i = Lx^-T u_i, b_i = Ly^-T v_i: the variates a_i^T x and
 *   b_i^T y have unit weighted variance and correlation rho_i >= 0.  Ordered by rho descending; rho clamped to at most 1; the sign of
 *   (a_i, b_i) such that sum_k (Sxx a_i)[k] / sqrt(Sxx[k][k]) >= 0; var_i = max(2 (1 - rho_i), min_var); delta = max_i |rho_i - rho_i of the
 *   previous solve|, +inf with first = 1.  A singular value of exactly 0 leaves a_i = 0.  The solve fails (ok = 0) when S0 <= 0, when
 *   n_valid < D + 1, or when a Cholesky pivot is <= 1e-12 times its original diagonal entry (a rank-deficient date): rho, var, a, b and
 *   delta are then NaN.  state: float64 [BDN_MAD_STATE_DOUBLES(n_b)]:
 *       [0] iter  [1] ok  [2] converged  [3] skip  [4] delta  [5] S0  [6] n_valid  [7 ..] rho[n_b], var[n_b], mean[D], centre[D],
 *       a[n_b][n_b] (a[i][k]: coefficient k of variate i), b[n_b][n_b];     mean = centre + mean_z
 *   Flags: with first = 1 the state's previous content is ignored (iter = 1).  Otherwise, with converged != 0 on entry the solve sets
 *   skip = 1 and does nothing else.  A solve that works sets iter += 1, skip = 0, converged = (delta < tol), and converged = 1, ok = 0 when
 *   it fails.  tol >= 0 (0 never stops), min_var > 0.  One launch.
 * bdn_mad_chi2: with state[SKIP] != 0 the call writes nothing.  Per valid pixel, in double:  M_i = a_i^T (x - mean_x) - b_i^T (y - mean_y),
 *   chi2 = sum_i M_i^2 / var_i,  nochange = Q(n_b / 2, chi2 / 2), the chi-square tail with n_b degrees of freedom by its finite closed form,
 *   t = chi2 / 2, h = e^(-t/2):   even n_b = 2m: h sum_{k<m} (h t^k / k!);   odd n_b = 2m + 1: erfc(sqrt t) + h sum_{k=1..m} (h t^(k-1/2) / Gamma(k + 1/2)),
 *   the terms built by recurrence from h (every term is below 2^16, nothing overflows), clamped to at most 1.  Outputs, each rounded once to
 *   float32: chi2[H][W]; proba[2][H][W] = {nochange, 1 - nochange} (the layout bdn_score_hist and bdn_threshold_mask take); variates
 *   (NULL or [n_b][H][W]) = M_i.  An invalid pixel gets chi2 = 0, proba = {1, 0}, variates 0.  With ok = 0 every pixel gets NaN in all
 *   outputs.  Plane 0 of proba is the next iteration's weight.  One launch.
 * bdn_mad_mask: mask[y][x] (uint8) = 1 where proba[0][y][x] < threshold, 0 elsewhere (a NaN gives 0), excluded_out (a byte) where the pixel
 *   is invalid; threshold in [0, 1].  One launch.
 * Iteration without a host read: centre once, then `iters` times (moments with the state, solve, chi2); the first moments call takes
 *   state = NULL and weight = NULL, the first solve first = 1, later moments calls weight = plane 0 of proba.  Only the single-block solve
 *   writes the flags, so no launch reads a flag that the same launch writes: the chi2 of the converged iteration still runs, and every
 *   launch after it changes no byte anywhere.
 * Every pointer is device memory; nothing waits for the device; all work is enqueued on `stream`. ---- */
#define BDN_MAD_STATE_ITER 0
#define BDN_MAD_STATE_OK 1
#define BDN_MAD_STATE_CONVERGED 2
#define BDN_MAD_STATE_SKIP 3
#define BDN_MAD_STATE_DELTA 4
#define BDN_MAD_STATE_S0 5
#define BDN_MAD_STATE_NVALID 6
#define BDN_MAD_STATE_RHO 7
#define BDN_MAD_STATE_DOUBLES(n_b) (7 + 6 * (n_b) + 2 * (n_b) * (n_b))
#define BDN_MAD_MOMENT_DOUBLES(n_b) (1 + 2 * (n_b) + (n_b) * (2 * (n_b) + 1))
size_t bdn_mad_workspace_bytes(int n_b, int H, int W);
int bdn_mad_centre(const float* d1, const float* d2, const int32_t* bands, int n_b, const uint8_t* exclude, int exclude_value,
                   double* centre, long long* n_valid, void* ws, int C, int H, int W, void* stream);
int bdn_mad_moments(const float* d1, const float* d2, const int32_t* bands, int n_b, const uint8_t* exclude, int exclude_value,
                    const float* weight, const double* centre, const double* state, double* moments, void* ws, int C, int H, int W,
                    void* stream);
int bdn_mad_solve(const double* moments, const double* centre, const long long* n_valid, int n_b, int first, double tol, double min_var,
                  double* state, void* stream);
int bdn_mad_chi2(const float* d1, const float* d2, const int32_t* bands, int n_b, const uint8_t* exclude, int exclude_value,
                 const double* state, float* chi2, float* proba, float* variates, int C, int H, int W, void* stream);
int bdn_mad_mask(const float* proba, const float* d1, const float* d2, const int32_t* bands, int n_b, const uint8_t* exclude,
                 int exclude_value, float threshold, int excluded_out, uint8_t* mask, int C, int H, int W, void* stream);

/* ---- thresholds without labels: the histogram of a float raster, four selection rules on it, and a mask at a threshold that lives on the
 * device.  The reference has one operating point, the argmax of train.py:199; a change statistic without labels (IR-MAD's chi2 above, a
 * scene's change probability from a city without ground truth) gets its threshold from the histogram of the statistic itself.  A null
 * required pointer, a misaligned pointer or a value outside its range is BDN_E_ARG before any launch; the outputs are the same bits on
 * every run.
 * bdn_raster_hist: raster float32 [HW] (HW is 64-bit, 1..2^40); exclude: NULL or uint8 [HW] with exclude_value (a byte); edges: float32
 *   [n_bins + 1], non-decreasing, 2 <= n_bins <= 4096; hist: uint64 [n_bins + 3], the kernel ADDS into it -- zero it once, then accumulate
 *   rasters or tiles, as bdn_score_hist does.  A pixel with exclude == exclude_value or a value that is not finite is skipped and counted
 *   in hist[n_bins + 2].  v < edges[0] is counted in hist[n_bins] (below), v > edges[n_bins] in hist[n_bins + 1] (above); every other v in
 *   bin max{i < n_bins : edges[i] <= v}, i.e. np.searchsorted(edges[:n_bins], v, side='right') - 1: a value equal to the last edge lands in
 *   the last bin, -0.0 == 0.0.  The bin comes from comparisons with the edges alone (a bisection of the table staged in LDS), no float
 *   arithmetic takes part: the counts are exact whatever the spacing.  The bisection's index stays in [0, n_bins - 1] for any table, sorted
 *   or not.  LDS and global integer atomics carry the counts.  Four pixels per thread where HW % 4 == 0 and raster is 16-byte, exclude
 *   4-byte aligned, one otherwise.  One launch.
 * bdn_hist_threshold: one launch of one block, float64.  c = hist[0 .. n_bins) (below, above and skipped take no part), N = sum c;
 *   coord: float64 [n_bins], non-decreasing: the coordinate of each bin the criteria are computed in (the bin centres, or their sqrt or
 *   log); every criterion uses y_i = coord[i] - M, M = (sum c_i coord_i) / N.  A split t in 1..n_bins-1 puts the bins < t in class 0 and the
 *   bins >= t in class 1; its threshold is edges[t], so that the mask v >= edges[t] has exactly sum c[t:] + above ones.  Counts and their
 *   prefix sums are 64-bit integers.  Floating-point sums over the bins have a fixed order: thread k of 256 adds the bins
 *   [k per, (k + 1) per), per = ceil(n_bins / 256), ascending from 0; the 256 partials are added in thread order from 0; a prefix sum
 *   continues the sum of the earlier threads' partials with the owner's bins.  No product is contracted into a fused multiply-add.
 *   methods: a mask of BDN_THR_*.  Ties go to the first (lowest) t.
 *     OTSU: the first t that maximises n0 n1 (m0 - m1)^2 over the splits with n0, n1 > 0 (class 1's sums are totals minus prefixes).
 *     KITTLER: the first t that minimises J = 1 + (P0 ln v0 + P1 ln v1) - 2 (P0 ln P0 + P1 ln P1), P_k = n_k / N, v_k the class variance
 *       sum c y^2 / n_k - m_k^2, over the splits with both v_k > 0 (Kittler and Illingworth 1986; ln v = 2 ln s).
 *     ROSIN: p = the first maximum bin, e = the last occupied bin; needs e >= p + 2; the first i in (p, e) that maximises
 *       (c[e] - c[p]) (i - p) - (e - p) (c[i] - c[p]), the distance from the chord (Rosin 2001), in signed 64-bit integers: bit-exact.
 *       N >= 2^49 gives OK = 0.  Right tails only.
 *     EM: two Gaussians fitted to the histogram (Bruzzone and Prieto 2000), started from Kittler's split (Otsu's if Kittler has none) with
 *       that split's class weights, means and variances; variances are floored at (the smallest positive coord[i+1] - coord[i])^2 / 12.
 *       Step j evaluates the log-likelihood L_j and the responsibilities under the current parameters; it stops before updating them when
 *       j > 1 and |L_j - L_{j-1}| <= em_tol |L_j|, otherwise updates, up to em_iters steps (1..1000; em_tol finite, >= 0; 0 stops only where L repeats bit for bit).  t = the first bin
 *       above the last bin with y <= m0, up to the last bin with y <= m1, at which ln w1 + ln N(y_t; m1, v1) >= ln w0 + ln N(y_t; m0, v0);
 *       OK = 0 without such a bin, with m1 <= m0, or when a class weight reaches 0.
 *   table: float64 [4][BDN_THR_COLS], row = OTSU, KITTLER, ROSIN, EM; thr: float32 [4] = edges[BIN].  Columns: OK; BIN = t; VALUE =
 *   edges[t]; CRIT (the criterion at t; EM: LOGLIK); N0, N1 = sum c[:t], sum c[t:]; MEAN0, MEAN1, SD0, SD1: of the two classes of the split,
 *   each summed for itself (EM: the fitted parameters); W1 = N1 / N (EM: the fitted weight); ITERS, LOGLIK (EM; 0 otherwise); N; BELOW;
 *   ABOVE.  A method that was not requested or has nothing to split (fewer than two occupied bins, N = 0, no valid split) leaves a row of
 *   zeros and thr = NaN: every call writes all of table and thr.
 * bdn_raster_mask: mask[i] (uint8) = raster[i] >= *thr (below = 1: raster[i] < *thr) for a finite raster[i], 0 for a non-finite one,
 *   excluded_out (a byte) where exclude[i] == exclude_value.  thr: ONE float32 in device memory (an entry of bdn_hist_threshold's thr): no
 *   host read between selecting a threshold and applying it.  A NaN threshold gives 0 at every pixel that is not excluded.  Four pixels
 *   per thread where HW % 4 == 0 and raster is 16-byte, exclude and mask 4-byte aligned, one otherwise.  One launch.
 * Every pointer is device memory; nothing waits for the device; all work is enqueued on `stream`. ---- */
#define BDN_THR_OTSU 1
#define BDN_THR_KITTLER 2
#define BDN_THR_ROSIN 4
#define BDN_THR_EM 8
#define BDN_THR_COL_OK 0
#define BDN_THR_COL_BIN 1
#define BDN_THR_COL_VALUE 2
#define BDN_THR_COL_CRIT 3
#define BDN_THR_COL_N0 4
#define BDN_THR_COL_N1 5
#define BDN_THR_COL_MEAN0 6
#define BDN_THR_COL_MEAN1 7
#define BDN_THR_COL_SD0 8
#define BDN_THR_COL_SD1 9
#define BDN_THR_COL_W1 10
#define BDN_THR_COL_ITERS 11
#define BDN_THR_COL_LOGLIK 12
#define BDN_THR_COL_N 13
#define BDN_THR_COL_BELOW 14
#define BDN_THR_COL_ABOVE 15
#define BDN_THR_COLS 16
int bdn_raster_hist(const float* raster, const uint8_t* exclude, int exclude_value, const float* edges, int n_bins,
                    unsigned long long* hist, long long HW, void* stream);
int bdn_hist_threshold(const unsigned long long* hist, const double* coord, const float* edges, int n_bins, int methods, int em_iters,
                       double em_tol, double* table, float* thr, void* stream);
int bdn_raster_mask(const float* raster, const uint8_t* exclude, int exclude_value, const float* thr, int below, int excluded_out,
                    uint8_t* mask, long long HW, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BIDATE_HIP_H */
