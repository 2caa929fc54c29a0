// 3x3 / stride 1 / pad 1 convolution as an NHWC implicit GEMM on MFMA (gfx950).
// Replaces nn.Conv2d(ci, co, 3, padding=1) forward and its data gradient
// (reference models/unet_parts.py:13,16 and autograd thereof).
//
// GEMM view: M = N*H*W output pixels, N = Cout, K = 9*Cin.
// One 256-thread block (4 waves) owns a TI x TH x TW spatial tile (128 or 256 output pixels) x BN output
// channels; each wave a 64 x 64 (or 64 x 32) sub-tile of v_mfma_f32_32x32x16_bf16 / 32x32x2_f32.
//   A operand (activations): per channel chunk the (TH+2)x(TW+2) halo patch is staged ONCE into LDS
//     (BatchNorm+ReLU of the producer applied on the way in, next chunk prefetched through registers into
//     the second LDS buffer); the nine taps read it at shifted pixel offsets, so activations cross
//     HBM/L2 -> LDS once instead of nine times.  Pixel stride and row pitch are padded so every
//     ds_read_b128 lane group hits disjoint banks.
//   B operand (filters): never touches LDS.  The filters are tiny (<= 9.4 MB), shared by every block and
//     L2/MALL resident, so they are packed once per step in MFMA *fragment order* (one contiguous 1 KB
//     record per 32 output channels x tap x k-group) and each wave streams its fragments straight from
//     L2 into registers, one tap ahead of the MFMAs.  This removes the per-tap filter staging, its LDS
//     writes, half of all LDS fragment reads and eight of the nine barriers per chunk (LDS bandwidth was
//     the co-limiter of the LDS-staged version: 96 % busy at 50 % MFMA).
// Epilogue: + bias, per-tile sum / sum^2 for the following BatchNorm, transpose through LDS, 16-byte
// coalesced NHWC stores.  Block ids are remapped so the N-tiles of one M-tile share an XCD's L2.
// Template flags on the same main loop: D3 (3x3x3: three depth sources of one reduction), BB (data gradient with the layer's BatchNorm
// backward formed while the operand is staged), EV (round 6, eval mode: the epilogue applies the folded running-statistics affine + ReLU and
// stores the activation; optional date product / 2x2 max-pool / 1x1 classifier + argmax + stitching from the tile in LDS; date-paired
// tiles), X3 (round 6, bf16x3: hi and lo patches of a chunk in LDS, the terms of the split product into one accumulator) and XF (X3 on a
// float32 source: BatchNorm+ReLU and the hi / lo split inside the staging).
// Round 7: two block-uniform fast paths of the training launches, bit-identical to the general code they skip (bdn_conv3x3_force_general turns
// them off; tests/test_gpu_conv_interior.py compares): a tile whose whole halo lies inside the image stages its patch without validity
// tests, fallback addresses, zero fill or exec-mask branches (single-chunk and BB kernels, which stage once), and a full tile copies out
// without bounds tests.  The same staging path inside the multi-chunk main loop and paired accumulator stores were measured and not kept
// (profiles/conv_interior_ab.txt).
#include "common.hpp"
#include <type_traits>

// Compile-time switches of the round-7 prologue / epilogue trims, so that each can be built out and A/B'ed on its own
// (tools/build_lib_variant.sh --only conv3x3 name "-DBDN_CONV_INTERIOR=0"); profiles/conv_interior_ab.txt has the measurements.
#ifndef BDN_CONV_INTERIOR
#define BDN_CONV_INTERIOR 1          // interior fast path of the training launches that stage once (single-chunk and BB kernels)
#endif
#ifndef BDN_CONV_FULLCOPY
#define BDN_CONV_FULLCOPY 1          // full tiles: copy-out without bounds tests
#endif

struct ConvArgs {
    const void* in0; const void* in1; int C0, C1;
    int ld0, ld1;                // pixel strides of in0 / in1 in elements (= C0 / C1 unless the source is a channel window of a wider tensor)
    // 3x3x3 mode (template flag D3; BASELINE configs[3], the multi-date stack): the N images are the D depth slices of N/Dz samples,
    // stored consecutively ([samples, Dz, H, W, C]); the reduction walks THREE sources of C0 channels each -- the slice below
    // (in0 = in1 - H*W*C), the slice itself (in1), the slice above (in2 = in1 + H*W*C) -- and a source whose slice falls outside
    // its sample's depth range is zero (block-uniform mask: a tile never spans two slices in this mode).  Dz = 0: 2-D convolution.
    const void* in2; int Dz;
    const float* in_bn;          // [G][4][C0] or null
    int imgs_per_group;
    const void* w;               // fragment-ordered filter image (common.hpp: wfrag_index)
    int w_kgroups;               // records per (cout block, tap) row of that image; 0 = (C0 + C1) / KCH.  BDN_BF16X2 walks the first two thirds of a bf16x3 row
    const float* bias;           // [Cout] or null
    void* out;                   // [N,H,W,Cout]
    float* stats_partial;        // [n_mtiles][2][Cout] or null
    int N, H, W, Cout;
    int tiles_y, tiles_x, n_ntiles;
    // data-gradient launches only: the output is dA of the layer whose raw output is bs_z and whose BatchNorm table
    // is bs_bn; the epilogue then also emits that layer's BatchNorm-backward partial sums (stats_partial, same
    // [n_mtiles][2][Cout] layout):  sum_p g  and  sum_p g*z  with  g = dA * [scale*z + shift > 0], and what it stores is g (masked)
    const void* bs_z; const float* bs_bn;
    // data-gradient launches with the BatchNorm+ReLU backward of THIS layer applied while the input is staged (template flag BB; round 4,
    // three-constant form round 5): in0 = g, the MASKED gradient g = dA * [scale z + shift > 0] exactly as every fused producer stores it
    // (dgrad_bs epilogue below, bdn_enc_skip_bwd, bdn_upsample2x_bwd_bs), bb_z = the layer's raw output z [N,H,W,C0], bb_bn its table,
    // bb_sums [G][2][C0] from bdn_bn_bwd_finalize; the staged operand is dz = a g + b z + c with the per-channel constants
    //   a = scale,  b = -scale invstd s1/M,  c = -scale s0/M - b mean      ( = scale (g - s0/M - xhat s1/M), bdn_bn_bwd_apply's value up to
    // rounding) -- two FMAs per element, no compare, three constants -- and the blocks of column tile 0 also store their tile's dz to bb_dz
    const void* bb_z; const float* bb_bn; const float* bb_sums; void* bb_dz; float bb_invM;
    // eval-mode launches (template flag EV; round 6, bdn_conv3x3_eval / bdn_conv3x3_eval_cls): nothing depends on batch statistics, so the
    // epilogue applies the FOLLOWING BatchNorm (running statistics, folded with the conv bias by bdn_bn_eval_fold_multi) and the ReLU once,
    //   a = relu(acc * ep_scale[c] + ep_shift[c]),
    // and stores the ACTIVATION: every consumer stages plain bytes, there are no statistics partials and no finalize launches.  Optional:
    //   ep_mul   [N,H,W,Cout]      the other date's activation of the same layer: what is stored to `out` is a * mul (relu(x_d2 * x_d1),
    //                              models/bidate_model.py:35-38; both factors are >= 0) and a itself is not stored at all;
    //   ep_pool  [N,H/2,W/2,Cout]  nn.MaxPool2d(2) of a (models/unet_parts.py:40; floor mode), from the tile in LDS;
    //   cls_*    the 1x1 classifier (models/unet_parts.py:88-89) on a tile that holds all Cout = 64 channels: logits [N,ncls,H,W] f32 and / or
    //            the class index (first maximum wins, train.py:199) as a [N,H,W] map or stitched into a scene mask (utils/inference.py:187-236).
    //   pair_stride > 0 (bdn_conv3x3_eval_pair; two-image tile configurations only): the two images of a tile are n and n + pair_stride -- the
    //            two DATES of one patch pair (N = 2 pair_stride) -- instead of two consecutive ones.  The block then holds both dates'
    //            activations of its pixels in LDS: `out` [pair_stride,H,W,Cout] receives their product, ep_pool [N,H/2,W/2,Cout] both pooled
    //            maps, and neither date's activation reaches HBM.
    //   ep_fuse  how two dates' rounded activations meet in `out`, with ep_mul and in paired launches: BDN_FUSE_PRODUCT a * mul as above,
    //            BDN_FUSE_ABSDIFF |a_d2 - a_d1| (one float32 subtraction, rounded once; FC-Siam-diff).  A runtime, block-uniform field: the
    //            instantiations are the same.
    const float* ep_scale; const float* ep_shift; const void* ep_mul; void* ep_pool; int pair_stride; int ep_fuse;
    const float* cls_w; const float* cls_b; int cls_n; float* cls_logits; unsigned char* cls_mask; const int* cls_origins; int cls_H, cls_W;
    // bf16x3 launches on a FLOAT32 source (template flag XF; round 6, bdn_conv3x3_x3src): in0 = the float32 tensor [N,H,W,C0] itself (ld0 = C0), in_bn
    // its producer's BatchNorm table or null.  The staging applies relu(z * scale + shift) and splits the value into bf16 hi + lo on its way into the
    // two LDS patches -- bdn_split_pack's arithmetic, element for element -- so no split pass runs in front of the convolution.  x3_split
    // (optional, [N,H,W,2 C0] bf16 = hi | lo): the blocks of column tile 0 also store their tile's own pixels of the split operand there,
    // for the layer's weight-gradient GEMM (what bdn_split_pack would have written).
    void* x3_split;
    // bdn_conv3x3_force_general (tests): every block takes the general path -- no interior staging, no full-tile copy-out
    int force_general;
};

template <typename T> struct Mma;
template <> struct Mma<bf16s> {
    __device__ __forceinline__ static void run(const uint4& a, const uint4& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    // 16 bytes per lane-half = 4 k-values per half -> four 32x32x2 steps (k order is a permutation
    // shared by A and B, which leaves the sum unchanged)
    __device__ __forceinline__ static void run(const uint4& a, const uint4& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
    }
};

// TO: element type of the OUTPUT tensor (and of bs_z).  TO = T except in the bf16x3 setting, whose operands are bf16 hi/lo
// splits of float32 tensors and whose outputs are float32.
template <typename T, int CKB, int TH, int TW, int TI, int BN, int WM, int WN, bool BF = true, typename TO = T, int X3 = 0>
struct ConvCfg {
    using TL = Tile<TH, TW, TI>;
    static constexpr int ES = sizeof(T);
    static constexpr int OES = sizeof(TO);
    static constexpr int EPU = 16 / ES;
    static constexpr int CK = CKB / ES;
    static constexpr int UPP = CKB / 16;
    static constexpr int BM = TL::BM;
    static constexpr int PSTR = CKB + 16;              // LDS pixel stride: odd number of 16-byte slots
    // LDS row pitch: a 16-lane ds_read_b128 group spans two (TW=16) or four (TW=8) patch rows; the row
    // pitch is padded so that those rows land on disjoint bank slots (pitch/16 = 0 resp. 8 mod 16).
    static constexpr int ROWSLOTS = TL::PW * (PSTR / 16);
    static constexpr int RPAD = (((TW == 16 ? 0 : 8) - ROWSLOTS % 16 + 16) % 16) * 16;
    static constexpr int ROWP = TL::PW * PSTR + RPAD;
    static constexpr int MI = BM / (WM * 32), NJ = BN / (WN * 32);
    static constexpr int KG = CKB / 32;                // k-groups (32 bytes of channels) per chunk
    static constexpr int NPU0 = (TL::NPIX * UPP + 255) / 256;
    // rows backed by LDS: the patch itself, rounded up so that EVERY thread's unit slots (NPU0 * 256 of them, the
    // tail beyond the patch is padding) have an address -- staging then needs no per-unit bounds branch
    static constexpr int ROWS_ALLOC = ((NPU0 * 256 / UPP) + TL::PW - 1) / TL::PW;
    static constexpr int PATCH_ROWS = (BF && ROWS_ALLOC > TI * TL::PH) ? ROWS_ALLOC : TI * TL::PH;   // BF: branch-free staging
    static constexpr int PATCH_BYTES = PATCH_ROWS * ROWP;
    // double-buffer when two blocks still fit a CU; the single-chunk kernels (BF == false) never fill a second buffer, and without
    // it their 8x16 instantiation fits three blocks per CU instead of two
    // X3 (bf16x3 with the split product fused into one reduction): TWO patches per chunk -- the hi and the lo part of the operand -- single-buffered
    static constexpr int PBUF = X3 ? 1 : ((BF && 2 * PATCH_BYTES <= 64 * 1024) ? 2 : 1);
    static constexpr int OSTR = BN * OES + 16;
    static constexpr int NPU = (TL::NPIX * UPP + 255) / 256;
    static constexpr int MAIN_BYTES = (X3 ? 2 : PBUF) * PATCH_BYTES;
    static constexpr int EPI_BYTES = BM * OSTR + 4 * BN * 2 * 4;
    static constexpr int SMEM = MAIN_BYTES > EPI_BYTES ? MAIN_BYTES : EPI_BYTES;
    static_assert(WM * WN == 4, "4 waves");
    static_assert(BM % (WM * 32) == 0 && BN % (WN * 32) == 0, "wave tiling");
    static_assert(NJ <= 2 && (KG == 1 || KG == 2 || KG == 4), "filter fragment registers are named scalars");
    __device__ __forceinline__ static int slot_off(int s) {       // LDS byte offset of a slot's (r=0,c=0) tap
        int ti, py, px; TL::slot_to_nyx(s, ti, py, px);
        return (ti * TL::PH + py) * ROWP + px * PSTR;
    }
};

// ONE: the whole reduction fits one channel chunk (Cin == CK: the 64-channel layers at full resolution).  Those
// blocks are prologue/epilogue bound (144 MFMAs per wave), so the variant drops the next-chunk prefetch state and
// is compiled for three blocks per CU instead of two.
template <typename T, int CKB, int TH, int TW, int TI, int BN, int WM, int WN, bool ONE = false, typename TO = T, bool D3 = false, bool BB = false, bool EV = false, int X3 = 0, bool XF = false>
// blocks per CU the kernel is compiled for: three where the register budget of 168 holds without spilling
// (single-chunk variant, 64-wide column tiles on 8-row spatial tiles), two otherwise
// the multi-chunk 64-wide instantiation on 8 x 16 tiles needs 171 registers: at three blocks per CU (168) it spilled three of them;
// two blocks per CU measure the same (d1a fwd 74.6 -> 73.8 us, step 6.16 ms either way) without scratch
__global__ __launch_bounds__(256, (!BB && sizeof(TO) == sizeof(T) && ((ONE && BN == 64) || (BN == 64 && TH == 8))) ? ((!ONE && BN == 64 && TH == 8) ? 2 : 3) : 2) void conv3x3_kernel(ConvArgs a) {
    using CF = ConvCfg<T, CKB, TH, TW, TI, BN, WM, WN, !ONE, TO, X3>;
    using TL = typename CF::TL;
    constexpr int MI = CF::MI, NJ = CF::NJ, KG = CF::KG, PSTR = CF::PSTR, ROWP = CF::ROWP;
    constexpr int EPU = CF::EPU, UPP = CF::UPP, NPU = CF::NPU, CK = CF::CK, PBUF = CF::PBUF;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int half = lane >> 5, l31 = lane & 31;

    const int logical = xcd_remap(blockIdx.x, gridDim.x);
    const int ntile = logical % a.n_ntiles, mtile = logical / a.n_ntiles;   // block-uniform scalar divisions (shifts for power-of-two grids measured no faster)
    const int tx = mtile % a.tiles_x, ty = (mtile / a.tiles_x) % a.tiles_y, ib = mtile / (a.tiles_x * a.tiles_y);
    const bool paired = EV && TI == 2 && a.pair_stride > 0;                   // block-uniform (eval-mode date-paired tiles)
    const int istr = paired ? a.pair_stride : 1;                              // image stride between the tile's images
    const int n0 = paired ? ib : ib * TI, y0 = ty * TH, x0 = tx * TW, col0 = ntile * BN;
    const int Cin = D3 ? 3 * a.C0 : a.C0 + a.C1;
    const int grp = n0 / a.imgs_per_group;
    // 3x3x3 mode: which of the three depth sources exist for this tile's slice (bit s: slice d + s - 1 lies inside the sample)
    const int dslice = D3 ? n0 % a.Dz : 0;
    const unsigned dmask = D3 ? ((dslice > 0 ? 1u : 0u) | 2u | (dslice + 1 < a.Dz ? 4u : 0u)) : 7u;
    static_assert(!D3 || TI == 1, "a 3x3x3 tile belongs to one depth slice");

    // eval-mode kernels (above all the full-resolution 64-channel layers: instruction-issue bound, 14.8 instructions per MFMA of which
    // three quarters are prologue and epilogue): tiles whose halo lies inside the image stage their patches without bounds tests / zero fill
    // training launches (round 7): the same block-uniform fast path.  At 128x128 36 of 64 16x16 tiles and 84 of 128 8x16 tiles are interior;
    // their staging carries no validity test, fallback address, zero fill or exec-mask branch per unit.  Border tiles run the general code.
    // Not for 3x3x3 launches (depth masks) and the fused split product (its own staging macros).
    constexpr bool INTR = EV || (BDN_CONV_INTERIOR && !D3 && X3 == 0 && (ONE || BB));
    const bool fast = a.force_general == 0;                                   // block-uniform (bdn_conv3x3_force_general)
    const bool interior = INTR && fast && y0 >= 1 && x0 >= 1 && y0 + TH + 1 <= a.H && x0 + TW + 1 <= a.W && n0 + (TI - 1) * istr < a.N;
    // ---- activation patch: every thread owns NPU 16-byte units whose pixel / LDS offsets never change
    int p_pix[NPU];                                      // global pixel index of each unit (-1 = zero padding)
    {
        // unit i of a thread is patch pixel tid/UPP + i*(256/UPP): walk (ti, yy, xx) incrementally instead of
        // dividing per unit (the divisions were a quarter of the prologue of the single-chunk layers)
        constexpr int STEP = 256 / UPP, DX = STEP % TL::PW, DY = STEP / TL::PW;
        static_assert(256 % UPP == 0, "incremental patch walk");
        constexpr int YWRAPS = (DY + 1) / TL::PH + 1;        // upper bound on row wraps per step
        const int pix0 = tid / UPP;
        int xx = pix0 % TL::PW, t0 = pix0 / TL::PW, yy = t0 % TL::PH, ti = t0 / TL::PH;
        if (interior) {                                      // (block-uniform) every patch pixel lies inside the image: no per-unit tests
#pragma unroll
            for (int i = 0; i < NPU; i++) {
                p_pix[i] = ti < TI ? ((n0 + ti * istr) * a.H + y0 + yy - 1) * a.W + x0 + xx - 1 : 0;      // ti == TI: the tail units behind the patch
                xx += DX; yy += DY;
                if (xx >= TL::PW) { xx -= TL::PW; yy += 1; }
#pragma unroll
                for (int k = 0; k < YWRAPS; k++) if (yy >= TL::PH) { yy -= TL::PH; ti += 1; }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NPU; i++) {
                const int n = n0 + ti * istr, y = y0 + yy - 1, x = x0 + xx - 1;
                const bool ok = ti < TI && n < a.N && (unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W;
                p_pix[i] = ok ? (n * a.H + y) * a.W + x : -1;
                xx += DX; yy += DY;
                if (xx >= TL::PW) { xx -= TL::PW; yy += 1; }
#pragma unroll
                for (int k = 0; k < YWRAPS; k++) if (yy >= TL::PH) { yy -= TL::PH; ti += 1; }
            }
        }
    }
    const int p_sub = (tid % UPP) * EPU;                 // channel offset of this thread's units (256 % UPP == 0)
    const unsigned p_subb = (unsigned)p_sub * CF::ES;
    // padding units load SOME valid pixel (zeroed at the store): pixel 0 of the tensor in 2-D; in 3x3x3 mode the sources are
    // shifted by a slice (pixel 0 of the lower one lies in front of the tensor), so the tile's own origin pixel
    const int p_fall = D3 ? (n0 * a.H + y0) * a.W + x0 : 0;
    constexpr bool BRANCHFREE = !ONE;
    static_assert(!BB || (sizeof(T) == 2 && sizeof(TO) == 2 && !D3 && TI == 1), "BatchNorm backward on load: bf16 2-D launches, one image per tile");
    static_assert(!EV || (!BB && !D3 && sizeof(T) == sizeof(TO)), "eval-mode epilogue: plain 2-D launches");
    static_assert(X3 == 0 || ((X3 == 2 || X3 == 3) && sizeof(T) == 2 && sizeof(TO) == 4 && (CKB == 128 || CKB == 32) && !ONE && !D3 && !BB && !EV), "fused split product: bf16 operands, float32 outputs");
    static_assert(!XF || CKB == 128, "float32-source staging: 64-channel chunks");
    static_assert(!XF || X3 != 0, "float32-source staging belongs to the fused split product");
    uint4 preg[NPU];
    uint4 pregz[BB ? NPU : 1];                           // BB: the z units of the same pixels
#define LOAD_PATCH(c0_)                                                                                  \
    {                                                                                                   \
        const T* src_; int cs_, Cs_;                                                                    \
        if (D3) {                                          /* source s = depth tap; a missing slice reads the centre one (masked at the store) */ \
            const int s_ = (c0_) / a.C0; cs_ = (c0_) - s_ * a.C0; Cs_ = a.ld0;                          \
            const bool dv_ = (dmask >> s_) & 1u;                                                        \
            src_ = reinterpret_cast<const T*>(!dv_ || s_ == 1 ? a.in1 : (s_ == 0 ? a.in0 : a.in2));     \
        } else if ((c0_) < a.C0) { src_ = reinterpret_cast<const T*>(a.in0); Cs_ = a.ld0; cs_ = (c0_); } \
        else { src_ = reinterpret_cast<const T*>(a.in1); Cs_ = a.ld1; cs_ = (c0_) - a.C0; }             \
        /* one block-uniform base + a 32-bit byte offset per unit (the entry points keep every tensor below 4 GB): the loads take \
           the scalar-base addressing form, no 64-bit vector arithmetic, no branches.  Padding units read SOME valid pixel and \
           are zeroed at the store */                                                                   \
        const unsigned char* sb_ = reinterpret_cast<const unsigned char*>(src_ + cs_);                  \
        const unsigned cb_ = (unsigned)Cs_ * CF::ES;                                                    \
        if (interior) {                                    /* block-uniform: every unit's pixel is inside the image */ \
            _Pragma("unroll") for (int i = 0; i < NPU; i++)                                              \
                preg[i] = *reinterpret_cast<const uint4*>(sb_ + ((unsigned)p_pix[i] * cb_ + p_subb));   \
        } else {                                                                                        \
            _Pragma("unroll") for (int i = 0; i < NPU; i++)                                              \
                preg[i] = *reinterpret_cast<const uint4*>(sb_ + ((unsigned)(p_pix[i] >= 0 ? p_pix[i] : p_fall) * cb_ + p_subb)); \
        }                                                                                               \
        if constexpr (BB) {                                                                             \
            const unsigned char* zb_ = reinterpret_cast<const unsigned char*>(reinterpret_cast<const T*>(a.bb_z) + (c0_)); \
            const unsigned zc_ = (unsigned)a.C0 * CF::ES;                                               \
            if (interior) {                                                                             \
                _Pragma("unroll") for (int i = 0; i < NPU; i++)                                          \
                    pregz[i] = *reinterpret_cast<const uint4*>(zb_ + ((unsigned)p_pix[i] * zc_ + p_subb)); \
            } else {                                                                                    \
                _Pragma("unroll") for (int i = 0; i < NPU; i++)                                          \
                    pregz[i] = *reinterpret_cast<const uint4*>(zb_ + ((unsigned)(p_pix[i] >= 0 ? p_pix[i] : 0) * zc_ + p_subb)); \
            }                                                                                           \
        }                                                                                               \
    }
#define STORE_PATCH(c0_, buf_)                                                                           \
    {                                                                                                   \
        unsigned char* pb_ = smem + (buf_) * CF::PATCH_BYTES;                                           \
        const int bs_ = D3 ? (c0_) / a.C0 : 0;             /* depth source of this chunk */               \
        const int bc_ = D3 ? (c0_) - bs_ * a.C0 : (c0_);   /* channel inside its source */                \
        const bool dvs_ = !D3 || ((dmask >> bs_) & 1u);                                                 \
        const bool bn_ = !EV && a.in_bn != nullptr && (D3 || (c0_) < a.C0);   /* eval-mode launches stage plain activations */ \
        float sc_[EPU], sh_[EPU];                          /* all units of a thread share one channel group */ \
        if (bn_) {                                                                                      \
            const float* ps_ = bn_row(a.in_bn, grp, 2, a.C0) + bc_ + p_sub;                             \
            const float* ph_ = bn_row(a.in_bn, grp, 3, a.C0) + bc_ + p_sub;                             \
            _Pragma("unroll") for (int e = 0; e < EPU; e++) { sc_[e] = ps_[e]; sh_[e] = ph_[e]; }        \
        }                                                                                               \
        float bk_[BB ? 3 : 1][EPU];                        /* BB: a, b, c of this thread's channels (see ConvArgs) */ \
        if constexpr (BB) {                                                                             \
            {                                                                                           \
                const float* rm_ = bn_row(a.bb_bn, grp, 0, a.C0) + bc_ + p_sub;                         \
                const float* ri_ = bn_row(a.bb_bn, grp, 1, a.C0) + bc_ + p_sub;                         \
                const float* rs_ = bn_row(a.bb_bn, grp, 2, a.C0) + bc_ + p_sub;                         \
                const float* s0_ = a.bb_sums + ((size_t)grp * 2 + 0) * a.C0 + bc_ + p_sub;              \
                const float* s1_ = a.bb_sums + ((size_t)grp * 2 + 1) * a.C0 + bc_ + p_sub;              \
                _Pragma("unroll") for (int e = 0; e < EPU; e++) {                                        \
                    const float sc1_ = rs_[e];                                                          \
                    bk_[0][e] = sc1_;                                                                   \
                    bk_[1][e] = -(sc1_ * ri_[e]) * (s1_[e] * a.bb_invM);                                \
                    bk_[2][e] = fmaf(-bk_[1][e], rm_[e], -(sc1_ * (s0_[e] * a.bb_invM)));               \
                }                                                                                       \
            }                                                                                           \
            _Pragma("unroll") for (int i = 0; i < NPU; i++) {                                            \
                float fz_[EPU], fg_[EPU], o_[EPU];                                                      \
                Unit<T>::unpack(pregz[i], fz_);                                                         \
                Unit<T>::unpack(preg[i], fg_);                                                          \
                _Pragma("unroll") for (int e = 0; e < EPU; e++)                                          \
                    o_[e] = fmaf(fg_[e], bk_[0][e], fmaf(fz_[e], bk_[1][e], bk_[2][e]));                 \
                preg[i] = Unit<T>::pack(o_);                                                            \
                /* the tile's own pixels: the weight-gradient GEMM reads them.  (interior tiles: every patch pixel exists, the tail units behind the patch do not) */ \
                if (a.bb_dz != nullptr && ntile == 0 && (interior ? tid + i * 256 < TL::NPIX * UPP : p_pix[i] >= 0)) { \
                    const int u_ = tid + i * 256, pix_ = u_ / UPP, xx_ = pix_ % TL::PW, yy_ = (pix_ / TL::PW) % TL::PH;   \
                    if (xx_ >= 1 && xx_ <= TW && yy_ >= 1 && yy_ <= TH)                                  \
                        *reinterpret_cast<uint4*>(reinterpret_cast<unsigned char*>(a.bb_dz) + ((unsigned)p_pix[i] * ((unsigned)a.C0 * CF::ES) + (unsigned)(bc_) * CF::ES + p_subb)) = preg[i]; \
                }                                                                                       \
            }                                                                                           \
        }                                                                                               \
        if (!EV && interior) {                             /* block-uniform: halo inside the image -- no compare, select or exec branch per unit */ \
            _Pragma("unroll") for (int i = 0; i < NPU; i++) {                                            \
                const int u_ = tid + i * 256;                                                           \
                const int pix_ = u_ / UPP, xx_ = pix_ % TL::PW, t_ = pix_ / TL::PW;                      \
                if (BRANCHFREE || (i + 1) * 256 <= TL::NPIX * UPP || u_ < TL::NPIX * UPP)               \
                    *reinterpret_cast<uint4*>(pb_ + t_ * ROWP + xx_ * PSTR + (u_ % UPP) * 16) = bn_ ? bnrelu_unit<T>(preg[i], sc_, sh_) : preg[i]; \
            }                                                                                           \
        } else                                                                                          \
        _Pragma("unroll") for (int i = 0; i < NPU; i++) {                                                \
            const int u_ = tid + i * 256;                  /* LDS offset recomputed: cheaper than 11 live registers */ \
            const int pix_ = u_ / UPP, xx_ = pix_ % TL::PW, t_ = pix_ / TL::PW;                          \
            if (BRANCHFREE && EV && interior) {            /* eval mode, halo inside the image: plain bytes, nothing to select */ \
                *reinterpret_cast<uint4*>(pb_ + t_ * ROWP + xx_ * PSTR + (u_ % UPP) * 16) = preg[i];     \
            } else if (BRANCHFREE) {                       /* multi-chunk kernels: the staging is scheduled into the MFMAs */ \
                uint4 v_ = bn_ ? bnrelu_unit<T>(preg[i], sc_, sh_) : preg[i];                           \
                const bool ok_ = p_pix[i] >= 0 && dvs_;                                                 \
                v_.x = ok_ ? v_.x : 0u; v_.y = ok_ ? v_.y : 0u; v_.z = ok_ ? v_.z : 0u; v_.w = ok_ ? v_.w : 0u; \
                *reinterpret_cast<uint4*>(pb_ + t_ * ROWP + xx_ * PSTR + (u_ % UPP) * 16) = v_;          \
            } else if (u_ < TL::NPIX * UPP) {              /* single-chunk kernels stage once, in the prologue */ \
                uint4 v_ = make_uint4(0, 0, 0, 0);                                                      \
                if (p_pix[i] >= 0 && dvs_) v_ = bn_ ? bnrelu_unit<T>(preg[i], sc_, sh_) : preg[i];      \
                *reinterpret_cast<uint4*>(pb_ + t_ * ROWP + xx_ * PSTR + (u_ % UPP) * 16) = v_;          \
            }                                                                                           \
        }                                                                                               \
    }

    // the first patch is requested before anything else is computed: the rest of the prologue (LDS offsets, accumulator
    // clear, filter addressing) runs in the shadow of its HBM latency
    // X3: the operand is the [hi | lo] split of a float32 tensor (bdn_split_pack: [pixel][2 C0], hi at channel c, lo at C0 + c); a chunk
    // stages BOTH parts of its 64 channels, into two patches
    uint4 pregl[X3 ? NPU : 1];
#define X3_LOAD(c0_)                                                                                     \
    {                                                                                                   \
        if constexpr (XF) {                                /* float32 source: a unit's eight channels are two 16-byte loads */ \
            const unsigned char* sb_ = reinterpret_cast<const unsigned char*>(reinterpret_cast<const float*>(a.in0) + (c0_)); \
            const unsigned cb_ = (unsigned)a.ld0 * 4u;                                                  \
            _Pragma("unroll") for (int i = 0; i < NPU; i++) {                                            \
                const unsigned o_ = (unsigned)(p_pix[i] >= 0 ? p_pix[i] : 0) * cb_ + p_subb * 2u;       \
                preg[i] = *reinterpret_cast<const uint4*>(sb_ + o_);                                    \
                pregl[i] = *reinterpret_cast<const uint4*>(sb_ + o_ + 16u);                             \
            }                                                                                           \
        } else {                                                                                        \
        const unsigned char* sb_ = reinterpret_cast<const unsigned char*>(reinterpret_cast<const T*>(a.in0) + (c0_)); \
        const unsigned cb_ = (unsigned)a.ld0 * CF::ES, lo_ = (unsigned)a.C0 * CF::ES;                   \
        _Pragma("unroll") for (int i = 0; i < NPU; i++) {                                                \
            const unsigned o_ = (unsigned)(p_pix[i] >= 0 ? p_pix[i] : 0) * cb_ + p_subb;                \
            preg[i] = *reinterpret_cast<const uint4*>(sb_ + o_);                                        \
            pregl[i] = *reinterpret_cast<const uint4*>(sb_ + o_ + lo_);                                 \
        }                                                                                               \
        }                                                                                               \
    }
    // XF: unit i_ of the prefetched chunk c0_ in place, float32 z (preg = channels 0..3, pregl = 4..7) -> bf16 hi (preg) and lo (pregl) units --
    // bdn_split_pack's arithmetic: v = relu(z * scale + shift), hi = bf16(v), lo = bf16(v - hi).  Run for one unit every other k-step in the
    // middle of the PREVIOUS chunk's MFMAs (the loads have landed by then), so the ~50 VALU instructions per unit issue between
    // MFMAs instead of in front of a barrier; the scale / shift rows come from the table the prologue left in LDS.
#define X3_CONVERT(i_, c0_)                                                                              \
    {                                                                                                   \
        float f_[8], r_[8], g_[8];                                                                      \
        Unit<float>::unpack(preg[i_], f_); Unit<float>::unpack(pregl[i_], f_ + 4);                      \
        if (a.in_bn != nullptr) {                          /* block-uniform */                            \
            const float* t_ = reinterpret_cast<const float*>(smem + 2 * CF::PATCH_BYTES) + (c0_) + p_sub; \
            float xsc_[8], xsh_[8];                                                                     \
            Unit<float>::unpack(*reinterpret_cast<const uint4*>(t_), xsc_); Unit<float>::unpack(*reinterpret_cast<const uint4*>(t_ + 4), xsc_ + 4); \
            Unit<float>::unpack(*reinterpret_cast<const uint4*>(t_ + a.C0), xsh_); Unit<float>::unpack(*reinterpret_cast<const uint4*>(t_ + a.C0 + 4), xsh_ + 4); \
            _Pragma("unroll") for (int e = 0; e < 8; e++) f_[e] = fmaxf(fmaf(f_[e], xsc_[e], xsh_[e]), 0.f); \
        }                                                                                               \
        const uint4 h_ = Unit<bf16s>::pack(f_);                                                         \
        Unit<bf16s>::unpack(h_, g_);                                                                    \
        _Pragma("unroll") for (int e = 0; e < 8; e++) r_[e] = f_[e] - g_[e];                             \
        const uint4 l_ = Unit<bf16s>::pack(r_);                                                         \
        preg[i_] = h_; pregl[i_] = l_;                                                                  \
        if (a.x3_split != nullptr && ntile == 0 && p_pix[i_] >= 0) {      /* the tile's own pixels, once: the weight-gradient GEMM's operand */ \
            const int u_ = tid + (i_) * 256, pix_ = u_ / UPP, xx_ = pix_ % TL::PW, yy_ = (pix_ / TL::PW) % TL::PH; \
            if (xx_ >= 1 && xx_ <= TW && yy_ >= 1 && yy_ <= TH) {                                        \
                unsigned char* so_ = reinterpret_cast<unsigned char*>(a.x3_split) + ((size_t)(unsigned)p_pix[i_] * (unsigned)(4 * a.C0) + (unsigned)(2 * (c0_)) + p_subb); \
                *reinterpret_cast<uint4*>(so_) = h_;                                                    \
                *reinterpret_cast<uint4*>(so_ + 2 * a.C0) = l_;                                         \
            }                                                                                           \
        }                                                                                               \
    }
#define X3_STORE()                                                                                       \
    {                                                                                                   \
        _Pragma("unroll") for (int i = 0; i < NPU; i++) {                                                \
            const int u_ = tid + i * 256, pix_ = u_ / UPP, xx_ = pix_ % TL::PW, t_ = pix_ / TL::PW;      \
            const bool ok_ = p_pix[i] >= 0;                                                             \
            uint4 h_ = preg[i], l_ = pregl[i];                                                          \
            h_.x = ok_ ? h_.x : 0u; h_.y = ok_ ? h_.y : 0u; h_.z = ok_ ? h_.z : 0u; h_.w = ok_ ? h_.w : 0u; \
            l_.x = ok_ ? l_.x : 0u; l_.y = ok_ ? l_.y : 0u; l_.z = ok_ ? l_.z : 0u; l_.w = ok_ ? l_.w : 0u; \
            const int lo_ = t_ * ROWP + xx_ * PSTR + (u_ % UPP) * 16;                                   \
            *reinterpret_cast<uint4*>(smem + lo_) = h_;                                                 \
            *reinterpret_cast<uint4*>(smem + CF::PATCH_BYTES + lo_) = l_;                               \
        }                                                                                               \
    }
    if constexpr (X3 != 0) X3_LOAD(0)
    else if (EV && ONE && interior) {
        const unsigned char* sb_ = reinterpret_cast<const unsigned char*>(a.in0);
        const unsigned cb_ = (unsigned)a.ld0 * CF::ES;
#pragma unroll
        for (int i = 0; i < NPU; i++) preg[i] = *reinterpret_cast<const uint4*>(sb_ + ((unsigned)p_pix[i] * cb_ + p_subb));
    } else LOAD_PATCH(0)

    int a_off[MI];                                       // per-lane LDS offsets of the A rows (pixel slots)
#pragma unroll
    for (int mi = 0; mi < MI; mi++) a_off[mi] = CF::slot_off((wm * MI + mi) * 32 + l31) + half * 16;

    f32x16 acc[MI][NJ];
#pragma unroll
    for (int mi = 0; mi < MI; mi++)
#pragma unroll
        for (int nj = 0; nj < NJ; nj++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[mi][nj][r] = 0.f;

    // ---- filter fragments: per wave NJ x KG records of 1 KB (64 lanes x 16 B), streamed one tap ahead from
    // the fragment-ordered image.  Named scalars on purpose (register arrays that meet a scheduling fence were
    // kept in scratch).  Record index: ((cout/32 * 9 + tap) * Cin/KCH + c/KCH); see wfrag_index in common.hpp.
    constexpr int KCH = 32 / CF::ES;                     // channels per k-group
    const int kgroups = a.w_kgroups ? a.w_kgroups : Cin / KCH;   // records per (cout block, tap)
    // wave-uniform base (scalar registers) + the lane's 16-byte slot as a 32-bit offset: the loads take the
    // SGPR-base addressing form and need no per-load 64-bit vector address arithmetic
    const int wn_u = __builtin_amdgcn_readfirstlane(wn);
    const unsigned char* wb0 = reinterpret_cast<const unsigned char*>(a.w)
        + ((size_t)((col0 >> 5) + wn_u * NJ) * 9 * kgroups) * 1024;
    const unsigned char* wb1 = wb0 + (size_t)9 * kgroups * 1024;     // second cout block of this wave (NJ == 2)
    const unsigned lane16 = lane * 16;
    // Ring of three register sets r0/r1/r2, one per STEP (= half a tap when a chunk has four k-groups, a whole
    // tap otherwise).  Step s computes from ring[s % 3] while the loads of step s+2 land in ring[(s+2) % 3];
    // a chunk has 9 or 18 steps (multiples of 3), so every index is a compile-time constant, nothing is
    // ever copied, and the prefetch distance is one full tap (two for the short chunks).
    constexpr int SPT = (KG == 4) ? 2 : 1;               // steps per tap
    constexpr int KPS = KG / SPT;                        // k-groups per step (1 or 2)
    constexpr int NST = 9 * SPT;                         // steps per chunk
    static_assert(KPS <= 2 && NST % 3 == 0, "ring layout");
    uint4 r0_00, r0_01, r0_10, r0_11, r1_00, r1_01, r1_10, r1_11, r2_00, r2_01, r2_10, r2_11;   // [nj][kps]
    r0_00 = r0_01 = r0_10 = r0_11 = r1_00 = r1_01 = r1_10 = r1_11 = r2_00 = r2_01 = r2_10 = r2_11 = make_uint4(0, 0, 0, 0);
#define LDB(p_, k_) (*reinterpret_cast<const uint4*>((p_) + (k_) * 1024 + lane16))
    // load the fragments of step st_ (tap st_/SPT, k-groups (st_%SPT)*KPS ...) of the chunk whose record offset is rec_
#define LOAD_R(R, st_, rec_)                                                                             \
    {                                                                                                   \
        const size_t o_ = ((size_t)((st_) / SPT) * kgroups + (rec_) + ((st_) % SPT) * KPS) * 1024;       \
        R##_00 = LDB(wb0 + o_, 0); if (KPS > 1) R##_01 = LDB(wb0 + o_, 1);                              \
        if (NJ > 1) { R##_10 = LDB(wb1 + o_, 0); if (KPS > 1) R##_11 = LDB(wb1 + o_, 1); }              \
    }
    // A fragments are double-buffered in registers (sets ae / ao, by parity of the k-group index q inside the
    // chunk): the ds_reads of k-group q+1 are issued, and pinned, ahead of the MFMAs of k-group q, so their LDS
    // latency hides behind 4-8 MFMAs instead of stalling the wave before every pair of MFMAs.
    uint4 ae0, ae1, ae2, ae3, ao0, ao1, ao2, ao3;
    ae0 = ae1 = ae2 = ae3 = ao0 = ao1 = ao2 = ao3 = make_uint4(0, 0, 0, 0);
    static_assert(MI <= 4, "A fragment registers are named scalars");
#define A_OFF(q_) ((((q_) / KG) / 3) * ROWP + (((q_) / KG) % 3) * PSTR + ((q_) % KG) * 32)
#define LDSA(mi_, q_) (*reinterpret_cast<const uint4*>(pcur + a_off[mi_] + A_OFF(q_)))
#define A_LOAD(S, q_)                                                                                    \
    {                                                                                                   \
        S##0 = LDSA(0, q_);                                                                             \
        if (MI > 1) S##1 = LDSA(MI > 1 ? 1 : 0, q_);                                                    \
        if (MI > 2) { S##2 = LDSA(MI > 2 ? 2 : 0, q_); S##3 = LDSA(MI > 2 ? 3 : 0, q_); }               \
    }
#define A_MMA(S, b0_, b1_)                                                                               \
    {                                                                                                   \
        Mma<T>::run(S##0, b0_, acc[0][0]); if (NJ > 1) Mma<T>::run(S##0, b1_, acc[0][NJ - 1]);          \
        if (MI > 1) { Mma<T>::run(S##1, b0_, acc[MI > 1 ? 1 : 0][0]); if (NJ > 1) Mma<T>::run(S##1, b1_, acc[MI > 1 ? 1 : 0][NJ - 1]); } \
        if (MI > 2) {                                                                                   \
            Mma<T>::run(S##2, b0_, acc[MI > 2 ? 2 : 0][0]); if (NJ > 1) Mma<T>::run(S##2, b1_, acc[MI > 2 ? 2 : 0][NJ - 1]); \
            Mma<T>::run(S##3, b0_, acc[MI > 2 ? 3 : 0][0]); if (NJ > 1) Mma<T>::run(S##3, b1_, acc[MI > 2 ? 3 : 0][NJ - 1]); \
        }                                                                                               \
    }
    // k-group q of the chunk: prefetch q+1 into the other set (except after the last one), then the MFMAs of q
#define KGSTEP(q_, b0_, b1_)                                                                             \
    {                                                                                                   \
        if constexpr ((((q_)) & 1) == 0) {                                                              \
            if constexpr ((q_) + 1 < 9 * KG) { A_LOAD(ao, (q_) + 1) }                                    \
            __builtin_amdgcn_sched_barrier(0);                                                          \
            A_MMA(ae, b0_, b1_)                                                                         \
        } else {                                                                                        \
            if constexpr ((q_) + 1 < 9 * KG) { A_LOAD(ae, (q_) + 1) }                                    \
            __builtin_amdgcn_sched_barrier(0);                                                          \
            A_MMA(ao, b0_, b1_)                                                                         \
        }                                                                                               \
    }
#define STEP(st_, RC, RN)                                                                                \
    {                                                                                                   \
        if ((st_) + 2 < NST) { LOAD_R(RN, (st_) + 2, rec0) }                                            \
        else if (more) { LOAD_R(RN, (st_) + 2 - NST, rec0 + KG) }                                       \
        if ((st_) == SPT && more) { LOAD_PATCH(c0 + CK) }                                               \
        __builtin_amdgcn_sched_barrier(0);                                                              \
        KGSTEP((st_) * KPS, RC##_00, RC##_10)                                                           \
        if constexpr (KPS > 1) KGSTEP((st_) * KPS + 1, RC##_01, RC##_11)                                \
        if (PBUF == 2 && (st_) == 6 * SPT && more) { STORE_PATCH(c0 + CK, (chunk + 1) & 1) }            \
    }
#define STEP3(s_) STEP((s_), r0, r2) STEP((s_) + 1, r1, r0) STEP((s_) + 2, r2, r1)

    if constexpr (X3 != 0) {
        // ---- bf16x3 with the split product fused into ONE reduction (round 6).  The operand's hi and lo parts of a chunk sit in two LDS
        // patches; a k-step (tap, k-group) loads the w_hi fragment (and for three terms the w_lo fragment) ONCE and issues
        //     acc += a_hi w_hi;  acc += a_lo w_hi;  [acc += a_hi w_lo]
        // per pixel fragment: 2 (3) MFMAs per LDS fragment read and 2 MI (3 MI) MFMAs per filter fragment streamed through the L1, where the
        // K = [hi | lo | hi] walk of rounds 3-5 had 1 and MI -- the vector-memory fragment is the expensive feed instruction
        // (profiles/r5_feed_power.txt) -- and the hi patch is staged once instead of twice.  Filter image: bdn_pack_weights(BDN_BF16X3)
        // rows [w_hi | w_hi | w_lo] of 3 C0 channels per tap: w_hi from the first third, w_lo from the last.
        constexpr int NSTEP = 9 * KG;
        static_assert(NSTEP % 3 == 0, "ring of three filter sets");
        if constexpr (XF) {
            if (a.in_bn != nullptr) {                                    // scale | shift rows of this block's statistic group, behind the two patches
                float* tab = reinterpret_cast<float*>(smem + 2 * CF::PATCH_BYTES);
                const float* ps = bn_row(a.in_bn, grp, 2, a.C0);         // rows 2 and 3 are consecutive: [scale(C0) | shift(C0)]
                for (int i = tid * 4; i < 2 * a.C0; i += 1024) *reinterpret_cast<uint4*>(tab + i) = *reinterpret_cast<const uint4*>(ps + i);
                __syncthreads();
            }
#pragma unroll
            for (int i = 0; i < NPU; i++) X3_CONVERT(i, 0)               // the first chunk: nothing to hide behind yet
        }
        const unsigned lo_rec = 2u * (unsigned)(a.C0 / KCH);             // record offset of w_lo inside a (cout block, tap) row
        int chunk = 0;
        for (int c0 = 0; c0 < a.C0; c0 += CK, chunk++) {
            const bool more = c0 + CK < a.C0;
            X3_STORE()
            __syncthreads();
            if (more) X3_LOAD(c0 + CK)                                   // in flight under this chunk's MFMAs
            const unsigned rec0 = (unsigned)chunk * KG;
            uint4 bh[3][NJ], bl[X3 == 3 ? 3 : 1][NJ], ah[2][MI], al[2][MI];
#define X3_LDB(set_, st_)                                                                                \
            {                                                                                           \
                const size_t o_ = ((size_t)((st_) / KG) * kgroups + rec0 + ((st_) % KG)) * 1024;        \
                bh[set_][0] = LDB(wb0 + o_, 0); if (NJ > 1) bh[set_][NJ - 1] = LDB(wb1 + o_, 0);        \
                if (X3 == 3) { bl[(X3 == 3) ? (set_) : 0][0] = LDB(wb0 + o_, lo_rec); if (NJ > 1) bl[(X3 == 3) ? (set_) : 0][NJ - 1] = LDB(wb1 + o_, lo_rec); } \
            }
#define X3_LDA(set_, st_)                                                                                \
            {                                                                                           \
                const int ao_ = (((st_) / KG) / 3) * ROWP + (((st_) / KG) % 3) * PSTR + ((st_) % KG) * 32; \
                _Pragma("unroll") for (int mi = 0; mi < MI; mi++) {                                      \
                    ah[set_][mi] = *reinterpret_cast<const uint4*>(smem + a_off[mi] + ao_);             \
                    al[set_][mi] = *reinterpret_cast<const uint4*>(smem + CF::PATCH_BYTES + a_off[mi] + ao_); \
                }                                                                                       \
            }
            X3_LDB(0, 0)
            X3_LDB(1, 1)
            X3_LDA(0, 0)
#pragma unroll
            for (int s_ = 0; s_ < NSTEP; s_++) {
                if (s_ + 2 < NSTEP) X3_LDB((s_ + 2) % 3, s_ + 2)
                if (s_ + 1 < NSTEP) X3_LDA((s_ + 1) & 1, s_ + 1)
                if constexpr (XF) {                                      // the next chunk's units, one every other k-step from step CV0 on
                    constexpr int CV0 = 12;
                    static_assert(CV0 + 2 * (NPU - 1) < NSTEP, "conversion steps inside the chunk");
                    if (more && s_ >= CV0 && ((s_ - CV0) & 1) == 0 && (s_ - CV0) / 2 < NPU) X3_CONVERT((s_ - CV0) / 2 < NPU ? (s_ - CV0) / 2 : 0, c0 + CK)
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int mi = 0; mi < MI; mi++)
#pragma unroll
                    for (int nj = 0; nj < NJ; nj++) {
                        Mma<T>::run(ah[s_ & 1][mi], bh[s_ % 3][nj], acc[mi][nj]);
                        Mma<T>::run(al[s_ & 1][mi], bh[s_ % 3][nj], acc[mi][nj]);
                        if (X3 == 3) Mma<T>::run(ah[s_ & 1][mi], bl[(X3 == 3) ? (s_ % 3) : 0][nj], acc[mi][nj]);
                    }
            }
#undef X3_LDB
#undef X3_LDA
            __syncthreads();                                             // everyone done reading before the next chunk's patches land
        }
    } else {
    // prologue: first patch -> LDS buffer 0, steps 0 and 1 -> ring slots 0 and 1
    LOAD_R(r0, 0, 0)
    LOAD_R(r1, 1, 0)
    if (EV && ONE && interior) {
#pragma unroll
        for (int i = 0; i < NPU; i++) {
            const int u_ = tid + i * 256, pix_ = u_ / UPP, xx_ = pix_ % TL::PW, t_ = pix_ / TL::PW;
            if ((i + 1) * 256 <= TL::NPIX * UPP || u_ < TL::NPIX * UPP)
                *reinterpret_cast<uint4*>(smem + t_ * ROWP + xx_ * PSTR + (u_ % UPP) * 16) = preg[i];
        }
    } else STORE_PATCH(0, 0)
    __syncthreads();

    int chunk = 0;
    // (eval-mode single-chunk kernels: the trip count is spelled as a constant, so the accumulator clear folds into the first MFMAs' C operand)
    for (int c0 = 0; (EV && ONE) ? c0 < CK : c0 < Cin; c0 += CK, chunk++) {
        const unsigned char* pcur = smem + (PBUF == 2 ? (chunk & 1) : 0) * CF::PATCH_BYTES;
        const bool more = ONE ? false : (c0 + CK < Cin);
        const int rec0 = chunk * KG;                     // record offset of this chunk inside a (cout block, tap) row
        A_LOAD(ae, 0)
        STEP3(0) STEP3(3) STEP3(6)
        if constexpr (SPT == 2) { STEP3(9) STEP3(12) STEP3(15) }
        if (PBUF == 1 && more) {                         // single patch buffer: everyone done reading, then refill
            __syncthreads();
            STORE_PATCH(c0 + CK, 0)
        }
        __syncthreads();
    }
    }
#undef X3_LOAD
#undef X3_STORE
#undef X3_CONVERT
#undef LDB
#undef LOAD_R
#undef STEP
#undef STEP3
#undef KGSTEP
#undef A_MMA
#undef A_LOAD
#undef LDSA
#undef A_OFF
#undef LOAD_PATCH
#undef STORE_PATCH

    // ------------------------------------------------------------------ eval-mode epilogue (EV launches; see ConvArgs)
    if constexpr (EV) {
        unsigned char* otile = smem;
        constexpr int UPR = BN * CF::OES / 16, OEPU = 16 / CF::OES, NIT = CF::BM * UPR / 256;
        static_assert(256 % UPR == 0 && UPR <= 64 && (CF::BM * UPR) % 256 == 0, "a thread keeps one channel unit through the copy-out loop");
        constexpr bool PRE = NIT <= 8;
        constexpr int NPRE = PRE ? NIT : 1;
        const unsigned orow = (unsigned)a.Cout * CF::OES;
        unsigned char* outp = reinterpret_cast<unsigned char*>(a.out) + (size_t)col0 * CF::OES;
        const unsigned char* mulp = reinterpret_cast<const unsigned char*>(a.ep_mul) + (size_t)col0 * CF::OES;
        const bool has_mul = a.ep_mul != nullptr, has_out = a.out != nullptr;       // block-uniform
        const bool absdiff = a.ep_fuse == BDN_FUSE_ABSDIFF;                         // block-uniform (ep_mul and paired launches)
        const bool full = (n0 + (TI - 1) * istr < a.N) && (y0 + TH <= a.H) && (x0 + TW <= a.W);          // block-uniform
#define OUT_OFS(i_, dst_)                                   /* byte offset of copy-out unit i_ in the output tensor, ~0 = outside the image */ \
        {                                                                                               \
            const int u_ = tid + (i_) * 256, slot_ = u_ / UPR, sub_ = u_ % UPR;                         \
            int ti_, py_, px_; TL::slot_to_nyx(slot_, ti_, py_, px_);                                   \
            const int n_ = n0 + ti_ * istr, y_ = y0 + py_, x_ = x0 + px_;                                      \
            dst_ = (full || (n_ < a.N && y_ < a.H && x_ < a.W)) ? (unsigned)((n_ * a.H + y_) * a.W + x_) * orow + (unsigned)sub_ * 16u : 0xffffffffu; \
        }
        unsigned oofs[NPRE];
        uint4 mq[NPRE];
        if (PRE && !paired && a.cls_w == nullptr) {
            if (full) {                                      // (block-uniform: the same offsets without the per-unit bounds tests)
#pragma unroll
                for (int i = 0; i < NPRE; i++) {
                    const int u_ = tid + i * 256, slot_ = u_ / UPR, sub_ = u_ % UPR;
                    int ti_, py_, px_; TL::slot_to_nyx(slot_, ti_, py_, px_);
                    oofs[i] = (unsigned)(((n0 + ti_ * istr) * a.H + y0 + py_) * a.W + x0 + px_) * orow + (unsigned)sub_ * 16u;
                }
            } else {
#pragma unroll
                for (int i = 0; i < NPRE; i++) OUT_OFS(i, oofs[i])
            }
            if (has_mul) {                                   // the other date's units: requested a whole accumulator pass ahead of their use
#pragma unroll
                for (int i = 0; i < NPRE; i++) mq[i] = *reinterpret_cast<const uint4*>(mulp + (oofs[i] != 0xffffffffu ? oofs[i] : 0u));
            }
        }
        // accumulators -> activation -> LDS (rounded to the storage type: what every consumer of the tensor sees)
#pragma unroll
        for (int nj = 0; nj < NJ; nj++) {
            const int col = (wn * NJ + nj) * 32 + l31;
            unsigned char* ob_ = otile + (wm * MI * 32 + 4 * half) * CF::OSTR + col * CF::OES;
            const float esc = a.ep_scale[col0 + col], esh = a.ep_shift[col0 + col];
#pragma unroll
            for (int mi = 0; mi < MI; mi++) {
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int srel_ = mi * 32 + (r & 3) + 8 * (r >> 2);
                    *reinterpret_cast<TO*>(ob_ + srel_ * CF::OSTR) = from_f<TO>(fmaxf(fmaf(acc[mi][nj][r], esc, esh), 0.f));
                }
            }
        }
        __syncthreads();
        if (a.cls_w != nullptr) {
            // 1x1 classifier on the tile (Cout == BN == 64: the UPR lanes of a pixel hold all its channels).  Same association as
            // outc_fwd_kernel<T, 2, UPR>: eight (four) channels per lane in ascending order, then the DPP row sums -- the logits are
            // bit-identical to bdn_outc_fwd on the stored activation.
            if constexpr (BN == 64 && (UPR == 8 || UPR == 16)) {
                const int bsub = (tid % UPR) * OEPU;
                float wk[2][OEPU], bk[2];
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    const int kk = k < a.cls_n ? k : 0;
                    const float bv = a.cls_b[kk];
                    bk[k] = k < a.cls_n ? bv : 0.f;
#pragma unroll
                    for (int i = 0; i < OEPU; i++) { const float wv = a.cls_w[kk * 64 + bsub + i]; wk[k][i] = k < a.cls_n ? wv : 0.f; }
                }
                const int hw = a.H * a.W;
#pragma unroll 2
                for (int i = 0; i < NIT; i++) {
                    const int u_ = tid + i * 256, slot_ = u_ / UPR;
                    int ti_, py_, px_; TL::slot_to_nyx(slot_, ti_, py_, px_);
                    const int n_ = n0 + ti_ * istr, y_ = y0 + py_, x_ = x0 + px_;
                    const bool in_ = n_ < a.N && y_ < a.H && x_ < a.W;
                    const uint4 v = *reinterpret_cast<const uint4*>(otile + slot_ * CF::OSTR + (u_ % UPR) * 16);
                    float f[OEPU], l0 = 0.f, l1 = 0.f;
                    Unit<TO>::unpack(v, f);
#pragma unroll
                    for (int e = 0; e < OEPU; e++) { l0 = fmaf(f[e], wk[0][e], l0); l1 = fmaf(f[e], wk[1][e], l1); }
                    l0 = first_lane_sum<UPR == 16 ? 16 : 8>(l0); l1 = first_lane_sum<UPR == 16 ? 16 : 8>(l1);
                    if (in_ && has_out) *reinterpret_cast<uint4*>(outp + ((unsigned)((n_ * a.H + y_) * a.W + x_) * orow + (unsigned)(u_ % UPR) * 16u)) = v;
                    if (in_ && (tid % UPR) == 0) {
                        l0 += bk[0]; l1 += bk[1];
                        const int q_ = y_ * a.W + x_;
                        if (a.cls_logits) {
                            a.cls_logits[((size_t)n_ * a.cls_n) * hw + q_] = l0;
                            if (a.cls_n > 1) a.cls_logits[((size_t)n_ * a.cls_n + 1) * hw + q_] = l1;
                        }
                        if (a.cls_mask) {
                            const unsigned char arg = (a.cls_n > 1 && l1 > l0) ? 1 : 0;           // first maximum wins ties (train.py:199)
                            if (!a.cls_origins) a.cls_mask[(size_t)n_ * hw + q_] = arg;
                            else {
                                // the stitching rule of argmax_stitch_kernel (scene.hip): a pixel of a far-edge band is written only by a tile anchored on it
                                const int ty0 = a.cls_origins[2 * n_], tx0 = a.cls_origins[2 * n_ + 1];
                                const int sy = ty0 + y_, sx = tx0 + x_;
                                const bool tyb = ty0 == a.cls_H - a.H, txb = tx0 == a.cls_W - a.W;
                                const bool pyb = sy >= a.cls_H - a.H, pxb = sx >= a.cls_W - a.W;
                                if (tyb == pyb && txb == pxb) a.cls_mask[(size_t)sy * a.cls_W + sx] = arg;
                            }
                        }
                    }
                }
            }
            return;
        }
        if (paired) {
            // date-paired tile: slots [0, TH*TW) hold date 1, [TH*TW, 2 TH*TW) date 2 of the same pixels -- the skip relu(x_d2 * x_d1) is formed
            // from LDS (both factors rounded activations, as fuse_product_kernel forms it) and is the only full-resolution tensor stored
            constexpr int HALF = TH * TW, NF = (HALF * UPR + 255) / 256;
            auto product = [&](auto full_c) {                 // full tiles (block-uniform) carry no per-unit bounds tests
                constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
                for (int i = 0; i < NF; i++) {
                    const int u_ = tid + i * 256, slot_ = u_ / UPR, sub_ = u_ % UPR;
                    const int py_ = slot_ / TW, px_ = slot_ % TW, y_ = y0 + py_, x_ = x0 + px_;
                    if ((HALF * UPR) % 256 == 0 || u_ < HALF * UPR) {
                        if (FULL || (y_ < a.H && x_ < a.W)) {
                            float fa[OEPU], fb[OEPU];
                            Unit<TO>::unpack(*reinterpret_cast<const uint4*>(otile + slot_ * CF::OSTR + sub_ * 16), fa);
                            Unit<TO>::unpack(*reinterpret_cast<const uint4*>(otile + (slot_ + HALF) * CF::OSTR + sub_ * 16), fb);
#pragma unroll
                            for (int e = 0; e < OEPU; e++) fa[e] = absdiff ? fabsf(fb[e] - fa[e]) : fa[e] * fb[e];
                            *reinterpret_cast<uint4*>(outp + ((unsigned)((n0 * a.H + y_) * a.W + x_) * orow + (unsigned)sub_ * 16u)) = Unit<TO>::pack(fa);
                        }
                    }
                }
            };
            if (full) product(std::true_type{}); else product(std::false_type{});
        } else
        {
        // copy-out: 16-byte NHWC units; with ep_mul what leaves is the date product (both factors rounded activations, as fuse_product_kernel forms it)
#define COPY_UNIT(i_, o_, mexpr_)                                                                        \
        if ((o_) != 0xffffffffu) {                                                                      \
            const int u_ = tid + (i_) * 256;                                                            \
            uint4 v = *reinterpret_cast<const uint4*>(otile + (u_ / UPR) * CF::OSTR + (u_ % UPR) * 16); \
            if (has_mul) {                                                                              \
                float fa[OEPU], fb[OEPU];                                                               \
                Unit<TO>::unpack(v, fa); Unit<TO>::unpack(mexpr_, fb);                                  \
                _Pragma("unroll") for (int e = 0; e < OEPU; e++) fa[e] = absdiff ? fabsf(fb[e] - fa[e]) : fa[e] * fb[e]; \
                v = Unit<TO>::pack(fa);                                                                 \
            }                                                                                           \
            *reinterpret_cast<uint4*>(outp + (o_)) = v;                                                 \
        }
        if (has_out) {
            if constexpr (PRE) {
#pragma unroll
                for (int i = 0; i < NPRE; i++) COPY_UNIT(i, oofs[i], mq[i])
            } else {
#pragma unroll 1
                for (int i = 0; i < NIT; i++) {
                    unsigned o; OUT_OFS(i, o)
                    COPY_UNIT(i, o, *reinterpret_cast<const uint4*>(mulp + o))
                }
            }
        }
#undef COPY_UNIT
#undef OUT_OFS
        }
        if (a.ep_pool != nullptr) {
            // MaxPool2d(2) of the tile's own activation (still in LDS, untouched by the product above): tiles start on even rows / columns,
            // so every 2x2 window lies inside one tile; floor mode drops the window of a trailing odd row / column
            constexpr int PHT = TH / 2, PWT = TW / 2, NPP = TI * PHT * PWT * UPR;
            const int Ho = a.H / 2, Wo = a.W / 2;
            unsigned char* poolp = reinterpret_cast<unsigned char*>(a.ep_pool) + (size_t)col0 * CF::OES;
            auto pooling = [&](auto full_c) {
                constexpr bool FULL = decltype(full_c)::value;
#pragma unroll
                for (int i = 0; i < (NPP + 255) / 256; i++) {
                    const int u_ = tid + i * 256, pp_ = u_ / UPR, sub_ = u_ % UPR;
                    const int ti_ = pp_ / (PHT * PWT), r_ = pp_ % (PHT * PWT), py_ = r_ / PWT, px_ = r_ % PWT;
                    const int n_ = n0 + ti_ * istr, yo_ = y0 / 2 + py_, xo_ = x0 / 2 + px_;
                    if (NPP % 256 == 0 || u_ < NPP) {
                        if (FULL || (n_ < a.N && yo_ < Ho && xo_ < Wo)) {
                            const unsigned char* w00 = otile + ((ti_ * TH + 2 * py_) * TW + 2 * px_) * CF::OSTR + sub_ * 16;
                            const uint4 m = unit_max_nonneg<TO>(unit_max_nonneg<TO>(*reinterpret_cast<const uint4*>(w00), *reinterpret_cast<const uint4*>(w00 + CF::OSTR)),
                                                                unit_max_nonneg<TO>(*reinterpret_cast<const uint4*>(w00 + TW * CF::OSTR),
                                                                                    *reinterpret_cast<const uint4*>(w00 + (TW + 1) * CF::OSTR)));
                            *reinterpret_cast<uint4*>(poolp + ((unsigned)((n_ * Ho + yo_) * Wo + xo_) * orow + (unsigned)sub_ * 16u)) = m;
                        }
                    }
                }
            };
            if (full) pooling(std::true_type{}); else pooling(std::false_type{});
        }
        return;
    }
    // ------------------------------------------------------------------ epilogue (LDS reused)
    unsigned char* otile = smem;
    float* red = reinterpret_cast<float*>(smem + CF::BM * CF::OSTR);
    const bool do_stats = a.stats_partial != nullptr && a.bs_z == nullptr;
    const bool full_tile = (n0 + TI <= a.N) && (y0 + TH <= a.H) && (x0 + TW <= a.W);   // block-uniform
    constexpr int UPR = BN * CF::OES / 16;                   // 16-byte units per output pixel row
    constexpr int OEPU = 16 / CF::OES;                       // output elements per 16-byte unit
    constexpr int NIT = CF::BM * UPR / 256;                  // copy-out units per thread
    static_assert(256 % UPR == 0 && UPR <= 64 && (CF::BM * UPR) % 256 == 0, "a thread keeps one channel unit through the copy-out loop");
    unsigned char* outp = reinterpret_cast<unsigned char*>(a.out) + (size_t)col0 * CF::OES;        // block-uniform bases + 32-bit byte offsets
    const bool bs = !D3 && a.bs_z != nullptr;                // block-uniform
    const unsigned char* bsz = reinterpret_cast<const unsigned char*>(a.bs_z) + (size_t)col0 * CF::OES;
    // PRE: the copy-out offsets and (data-gradient launches with BatchNorm-backward statistics) the z units are produced
    // BEFORE the accumulator pass; only where that costs at most 40 registers (16-bit outputs)
    constexpr bool PRE = NIT <= 8 && !D3;
    constexpr int NPRE = PRE ? NIT : 1;
    const unsigned orow = (unsigned)a.Cout * CF::OES;
    const int bsub = (tid % UPR) * OEPU;                     // this thread's channels inside the block's column tile
    float bs0[OEPU], bs1[OEPU], bsc[OEPU], bsh[OEPU];
#pragma unroll
    for (int i = 0; i < OEPU; i++) { bs0[i] = 0.f; bs1[i] = 0.f; bsc[i] = 0.f; bsh[i] = 0.f; }
#define OUT_OFS(i_, dst_)                                   /* byte offset of copy-out unit i_ in the output tensor, ~0 = outside the image */ \
    {                                                                                                   \
        const int u_ = tid + (i_) * 256, slot_ = u_ / UPR, sub_ = u_ % UPR;                             \
        int ti_, py_, px_; TL::slot_to_nyx(slot_, ti_, py_, px_);                                       \
        const int n_ = n0 + ti_, y_ = y0 + py_, x_ = x0 + px_;                                          \
        dst_ = (n_ < a.N && y_ < a.H && x_ < a.W) ? (unsigned)((n_ * a.H + y_) * a.W + x_) * orow + (unsigned)sub_ * 16u : 0xffffffffu; \
    }
    unsigned oofs[NPRE];
    uint4 zq[NPRE];
    // full tiles (block-uniform; every tile of the flagship launches): the copy-out offsets carry no bounds tests, the units no "outside" branch
    const bool full_copy = BDN_CONV_FULLCOPY && PRE && full_tile && fast;
    if (PRE) {
        if (full_copy) {
#pragma unroll
            for (int i = 0; i < NPRE; i++) {
                const int u_ = tid + i * 256, slot_ = u_ / UPR, sub_ = u_ % UPR;
                int ti_, py_, px_; TL::slot_to_nyx(slot_, ti_, py_, px_);
                oofs[i] = (unsigned)(((n0 + ti_) * a.H + y0 + py_) * a.W + x0 + px_) * orow + (unsigned)sub_ * 16u;
            }
        } else {
#pragma unroll
            for (int i = 0; i < NPRE; i++) OUT_OFS(i, oofs[i])
        }
    }
    if (bs) {
        // the z units are requested HERE, a whole accumulator pass ahead of their use: inside the copy-out loop every one of them
        // was a dependent HBM round trip behind the store before it (eight per block)
        if (PRE && full_copy) {
#pragma unroll
            for (int i = 0; i < NPRE; i++) zq[i] = *reinterpret_cast<const uint4*>(bsz + oofs[i]);
        } else if (PRE) {
#pragma unroll
            for (int i = 0; i < NPRE; i++) zq[i] = *reinterpret_cast<const uint4*>(bsz + (oofs[i] != 0xffffffffu ? oofs[i] : 0u));
        }
        const float* ps = bn_row(a.bs_bn, grp, 2, a.Cout) + col0 + bsub;
        const float* ph = bn_row(a.bs_bn, grp, 3, a.Cout) + col0 + bsub;
#pragma unroll
        for (int i = 0; i < OEPU; i++) { bsc[i] = ps[i]; bsh[i] = ph[i]; }
    }
    // Three block-uniform variants of the accumulator -> LDS pass, so the common cases carry no dead work:
    //   plain (data gradient: no bias, no statistics), full tile with statistics, ragged tile with statistics.
    // LDS addresses are one per-lane base + compile-time offsets (folded into the ds_write immediates).
#define EPI_PASS(STATS_, RAGGED_)                                                                         \
    _Pragma("unroll") for (int nj = 0; nj < NJ; nj++) {                                                   \
        const int col = (wn * NJ + nj) * 32 + l31;                                                       \
        unsigned char* ob_ = otile + (wm * MI * 32 + 4 * half) * CF::OSTR + col * CF::OES;               \
        const float bias = (STATS_) && a.bias ? a.bias[col0 + col] : 0.f;                                \
        float s = 0.f, q = 0.f;                                                                          \
        _Pragma("unroll") for (int mi = 0; mi < MI; mi++) {                                               \
            _Pragma("unroll") for (int r = 0; r < 16; r++) {                                              \
                constexpr int dummy_ = 0; (void)dummy_;                                                  \
                const int srel_ = mi * 32 + (r & 3) + 8 * (r >> 2);            /* slot - (wm*MI*32 + 4*half) */ \
                float v = acc[mi][nj][r];                                                                \
                if (STATS_) {                                                                            \
                    v += bias;                                                                           \
                    bool valid = true;                                                                   \
                    if (RAGGED_) {                                                                       \
                        int ti, py, px; TL::slot_to_nyx((wm * MI) * 32 + 4 * half + srel_, ti, py, px);  \
                        valid = (n0 + ti < a.N) && (y0 + py < a.H) && (x0 + px < a.W);                   \
                    }                                                                                    \
                    if (valid) { s += v; q = fmaf(v, v, q); }                                            \
                }                                                                                        \
                *reinterpret_cast<TO*>(ob_ + srel_ * CF::OSTR) = from_f<TO>(v);                          \
            }                                                                                            \
        }                                                                                                \
        if (STATS_) {                                                                                    \
            s += __shfl_xor(s, 32); q += __shfl_xor(q, 32);                                              \
            if (half == 0) { red[(wm * BN + col) * 2] = s; red[(wm * BN + col) * 2 + 1] = q; }           \
        }                                                                                                \
    }
    if (!do_stats && a.bias == nullptr) { EPI_PASS(false, false) }
    else if (full_tile) { EPI_PASS(true, false) }
    else { EPI_PASS(true, true) }
#undef EPI_PASS
    __syncthreads();
    if (do_stats && tid < BN) {
        float s = 0.f, q = 0.f;
#pragma unroll
        for (int m = 0; m < WM; m++) { s += red[(m * BN + tid) * 2]; q += red[(m * BN + tid) * 2 + 1]; }
        a.stats_partial[((size_t)mtile * 2 + 0) * a.Cout + col0 + tid] = s;
        a.stats_partial[((size_t)mtile * 2 + 1) * a.Cout + col0 + tid] = q;
    }
    // copy-out: the tile leaves LDS in 16-byte NHWC units; the offsets were computed (and, for data-gradient launches with the
    // BatchNorm-backward statistics, the z units requested) before the accumulator pass
#define COPY_UNIT(i_, o_, zexpr_) if ((o_) != 0xffffffffu) COPY_BODY(i_, o_, zexpr_)
#define COPY_BODY(i_, o_, zexpr_)                                                                        \
    {                                                                                                   \
        const int u_ = tid + (i_) * 256;                                                                \
        uint4 v = *reinterpret_cast<const uint4*>(otile + (u_ / UPR) * CF::OSTR + (u_ % UPR) * 16);     \
        if (bs) {                                            /* the stored (rounded) gradient is what BatchNorm backward sees; it leaves */ \
            float fg[OEPU], fz[OEPU];                        /* MASKED: g = dA * [scale z + shift > 0] -- every consumer applies the same */ \
            Unit<TO>::unpack(v, fg);                         /* mask again (idempotent), the on-load BatchNorm backward (BB) relies on it  */ \
            Unit<TO>::unpack(zexpr_, fz);                                                               \
            _Pragma("unroll") for (int e = 0; e < OEPU; e++) {                                           \
                const float g = fmaf(fz[e], bsc[e], bsh[e]) > 0.f ? fg[e] : 0.f;                        \
                bs0[e] += g; bs1[e] = fmaf(g, fz[e], bs1[e]);                                           \
                fg[e] = g;                                                                              \
            }                                                                                           \
            v = Unit<TO>::pack(fg);                          /* exact: the values are already rounded */ \
        }                                                                                               \
        *reinterpret_cast<uint4*>(outp + (o_)) = v;                                                     \
    }
    if constexpr (PRE) {
        if (full_copy) {
#pragma unroll
            for (int i = 0; i < NPRE; i++) COPY_BODY(i, oofs[i], zq[i])
        } else {
#pragma unroll
            for (int i = 0; i < NPRE; i++) COPY_UNIT(i, oofs[i], zq[i])
        }
    } else {
#pragma unroll 1
        for (int i = 0; i < NIT; i++) {
            unsigned o; OUT_OFS(i, o)
            COPY_UNIT(i, o, *reinterpret_cast<const uint4*>(bsz + o))
        }
    }
#undef COPY_UNIT
#undef COPY_BODY
#undef OUT_OFS
    if (bs) {
        // lanes tid, tid+UPR, ... of a wave hold the same channels: butterfly over those lane bits, then the four
        // waves meet in LDS (fixed order -> deterministic)
#pragma unroll
        for (int i = 0; i < OEPU; i++) {
#pragma unroll
            for (int m = UPR; m < 64; m <<= 1) { bs0[i] += __shfl_xor(bs0[i], m); bs1[i] += __shfl_xor(bs1[i], m); }
        }
        if (lane < UPR) {
#pragma unroll
            for (int i = 0; i < OEPU; i++) {
                red[((wave * BN) + lane * OEPU + i) * 2] = bs0[i];
                red[((wave * BN) + lane * OEPU + i) * 2 + 1] = bs1[i];
            }
        }
        __syncthreads();
        if (tid < BN) {
            float t0 = 0.f, t1 = 0.f;
#pragma unroll
            for (int wv = 0; wv < 4; wv++) { t0 += red[(wv * BN + tid) * 2]; t1 += red[(wv * BN + tid) * 2 + 1]; }
            a.stats_partial[((size_t)mtile * 2 + 0) * a.Cout + col0 + tid] = t0;
            a.stats_partial[((size_t)mtile * 2 + 1) * a.Cout + col0 + tid] = t1;
        }
    }
}

// bdn_conv3x3_variant: the dispatcher below runs as usual but, instead of launching, the chosen instantiation writes
// its name here (one source of truth for profilers that have to match rocprofv3 kernel names)
static thread_local bool g_conv_query = false;
static thread_local char g_conv_variant[160];
// bdn_conv3x3_force_general: every launch of this thread takes the general path (tests compare the two paths bit for bit)
static thread_local int g_conv_force_general = 0;
extern "C" int bdn_conv3x3_force_general(int on) { const int was = g_conv_force_general; g_conv_force_general = on ? 1 : 0; return was; }

template <typename T, int CKB, int TH, int TW, int TI, int BN, int WM, int WN, bool ONE = false, typename TO = T, bool D3 = false, bool BB = false, bool EV = false, int X3 = 0, bool XF = false>
static int launch_conv(const ConvArgs& a, int n_mtiles, hipStream_t st) {
    using CF = ConvCfg<T, CKB, TH, TW, TI, BN, WM, WN, !ONE, TO, X3>;
    if (g_conv_query) {
        // the full template spelling, so that a profiler can match rocprofv3's kernel names exactly ("bf16" = unsigned short)
        snprintf(g_conv_variant, sizeof(g_conv_variant), "conv3x3_kernel<%s,%d,%d,%d,%d,%d,%d,%d,%s,%s,%s,%s,%s,%d,%s>",
                 sizeof(T) == 2 ? "bf16" : "float", CKB, TH, TW, TI, BN, WM, WN, ONE ? "true" : "false",
                 sizeof(TO) == 2 ? "bf16" : "float", D3 ? "true" : "false", BB ? "true" : "false", EV ? "true" : "false", X3, XF ? "true" : "false");
        return BDN_OK;
    }
    auto kern = conv3x3_kernel<T, CKB, TH, TW, TI, BN, WM, WN, ONE, TO, D3, BB, EV, X3, XF>;
    // XF: the BatchNorm scale | shift rows of the operand's channels sit behind the two patches (<= 4 KB: C0 <= 512, checked by the entry point)
    constexpr int XF_TAB_MAX = XF ? 4096 : 0;
    constexpr int SMEM_MAX = (CF::MAIN_BYTES + XF_TAB_MAX > CF::SMEM) ? CF::MAIN_BYTES + XF_TAB_MAX : CF::SMEM;
    BDN_SET_SMEM_ONCE(kern, SMEM_MAX, "conv3x3");
    const int xf_tab = XF ? 2 * a.C0 * 4 : 0;
    const int smem_bytes = (CF::MAIN_BYTES + xf_tab > CF::SMEM) ? CF::MAIN_BYTES + xf_tab : CF::SMEM;
    ConvArgs b = a;
    b.n_ntiles = a.Cout / BN;
    b.force_general = g_conv_force_general;
    hipLaunchKernelGGL(kern, dim3(n_mtiles * b.n_ntiles), dim3(256), smem_bytes, st, b);
    BDN_CHECK_LAUNCH("conv3x3");
    return BDN_OK;
}

// Tile choice (shared with bdn_conv3x3_num_mtiles so the caller can size the statistics buffer):
//   8x8x2 images   for maps up to 8x8;
//   16x16 (BM=256) for 64-wide outputs on larger maps: one filter slice feeds twice the pixels;
//   8x16  (BM=128) otherwise.  BN = 128 when Cout allows it and the grid still has >= 512 blocks.
struct ConvPlan { TileGeom g; int BN; };
static ConvPlan conv_plan(int N, int H, int W, int Cout, int imgs_per_group) {
    ConvPlan p;
    TileGeom& g = p.g;
    const bool narrow = (Cout % 128 != 0);
    if (W <= 8 && H <= 8 && imgs_per_group % 2 == 0) { g.TI = 2; g.TH = 8; g.TW = 8; }
    else if (narrow && H >= 12 && W >= 12) { g.TI = 1; g.TH = 16; g.TW = 16; }
    else { g.TI = 1; g.TH = 8; g.TW = 16; }
    g.tiles_y = (H + g.TH - 1) / g.TH;
    g.tiles_x = (W + g.TW - 1) / g.TW;
    g.n_mtiles = ((N + g.TI - 1) / g.TI) * g.tiles_y * g.tiles_x;
    p.BN = (!narrow && (long)g.n_mtiles * (Cout / 128) >= 512) ? 128 : 64;
    if (g.TH == 16) p.BN = narrow ? 64 : 128;
    return p;
}

template <typename T, int CKB, bool EV = false>
static int dispatch_conv(const ConvArgs& a, const ConvPlan& p, hipStream_t st) {
    const TileGeom& g = p.g;
    const bool one = (a.C0 + a.C1) * (int)sizeof(T) == CKB;
    // 64-wide outputs on 16x16 tiles: the single-chunk kernels (three blocks per CU share one L1) take the 2x2 wave
    // layout, whose waves stream half the filter bytes each (e1b: +9..12 %); with several chunks the 4x1 layout wins
    if (g.TH == 16 && one) return launch_conv<T, CKB, 16, 16, 1, 64, 2, 2, true, T, false, false, EV>(a, g.n_mtiles, st);
    if (g.TH == 16) return launch_conv<T, CKB, 16, 16, 1, 64, 4, 1, false, T, false, false, EV>(a, g.n_mtiles, st);
    if (g.TI == 1) {
        // 128-wide column tiles: 1x4 waves (each 128 pixels x 32 channels) stream half the filter bytes of the 2x2 layout
        // through the L1 and need half the ring registers; the A fragments are read from LDS by all four (+1.5 % overall)
        if (p.BN == 128 && one) return launch_conv<T, CKB, 8, 16, 1, 128, 1, 4, true, T, false, false, EV>(a, g.n_mtiles, st);
        if (p.BN == 128) return launch_conv<T, CKB, 8, 16, 1, 128, 1, 4, false, T, false, false, EV>(a, g.n_mtiles, st);
        return launch_conv<T, CKB, 8, 16, 1, 64, 2, 2, false, T, false, false, EV>(a, g.n_mtiles, st);
    }
    if (p.BN == 128) return launch_conv<T, CKB, 8, 8, 2, 128, 2, 2, false, T, false, false, EV>(a, g.n_mtiles, st);
    return launch_conv<T, CKB, 8, 8, 2, 64, 2, 2, false, T, false, false, EV>(a, g.n_mtiles, st);
}

// BatchNorm backward on load (bdn_conv3x3_dgrad_bb): the single-chunk shapes only (dz of a 64-channel layer) -- there the staging runs once,
// in the prologue.  Inside the main loop of the two-chunk kernels the second operand (24 registers) and the three constants (24) do not fit:
// 8x16x128 1x4 256 registers + 24 B of scratch, 16x16x64 4x1 256 + 308 B; the former was measured on e2b anyway (round 5): +0.5 % step time.
static int dispatch_conv_bb(const ConvArgs& a, const ConvPlan& p, hipStream_t st) {
    const TileGeom& g = p.g;
    if (g.TI != 1) BDN_FAIL(BDN_E_SHAPE, "conv3x3_dgrad_bb: maps of 8x8 and below are not supported");
    if (g.TH == 16) return launch_conv<bf16s, 128, 16, 16, 1, 64, 2, 2, true, bf16s, false, true>(a, g.n_mtiles, st);
    if (p.BN == 128) return launch_conv<bf16s, 128, 8, 16, 1, 128, 1, 4, true, bf16s, false, true>(a, g.n_mtiles, st);
    return launch_conv<bf16s, 128, 8, 16, 1, 64, 2, 2, false, bf16s, false, true>(a, g.n_mtiles, st);
}

// bf16x3 with the split product fused into one reduction (operands of at least 64 channels): two patches per chunk in LDS, so no 16x16 tiles
static ConvPlan conv_plan_x3f(int N, int H, int W, int Cout, int imgs_per_group) {
    ConvPlan p;
    p.g = pick_tile(N, H, W, imgs_per_group);          // the weight gradient's tiles (common.hpp)
    p.BN = (p.g.TI == 1 && Cout % 128 == 0 && (long)p.g.n_mtiles * (Cout / 128) >= 512) ? 128 : 64;
    return p;
}

template <int X3, bool XF = false, int CKB = 128>
static int dispatch_conv_x3f(const ConvArgs& a, const ConvPlan& p, hipStream_t st) {
    const TileGeom& g = p.g;
    if (g.TI == 1 && p.BN == 128) return launch_conv<bf16s, CKB, 8, 16, 1, 128, 1, 4, false, float, false, false, false, X3, XF>(a, g.n_mtiles, st);
    if (g.TI == 1) return launch_conv<bf16s, CKB, 8, 16, 1, 64, 2, 2, false, float, false, false, false, X3, XF>(a, g.n_mtiles, st);
    return launch_conv<bf16s, CKB, 8, 8, 2, 64, 2, 2, false, float, false, false, false, X3, XF>(a, g.n_mtiles, st);
}

// tiles of a launch by operand type: the bf16x3 kernels with the fused split product have their own tile plan
extern "C" int bdn_conv3x3_num_mtiles_ex(int dtype, int N, int H, int W, int C0, int Cout, int imgs_per_group) {
    if (N <= 0 || H <= 0 || W <= 0 || Cout <= 0 || imgs_per_group <= 0) return 0;
    if ((dtype == BDN_BF16X3 || dtype == BDN_BF16X2) && C0 % 16 == 0) return conv_plan_x3f(N, H, W, Cout, imgs_per_group).g.n_mtiles;
    return conv_plan(N, H, W, Cout, imgs_per_group).g.n_mtiles;
}

extern "C" int bdn_conv3x3_num_mtiles(int N, int H, int W, int Cout, int imgs_per_group) {
    if (N <= 0 || H <= 0 || W <= 0 || Cout <= 0 || imgs_per_group <= 0) return 0;
    return conv_plan(N, H, W, Cout, imgs_per_group).g.n_mtiles;
}

static int conv3x3_impl(int dtype, const void* in0, int C0, const void* in1, int C1,
                        int in_mode, const float* in_bn, int imgs_per_group,
                        const void* w, const float* bias, void* out, float* stats_partial,
                        const void* bs_z, const float* bs_bn,
                        int N, int H, int W, int Cout, void* stream,
                        const void* bb_z = nullptr, const float* bb_bn = nullptr, const float* bb_sums = nullptr, void* bb_dz = nullptr) {
    if (!in0 || !w || !out) BDN_FAIL(BDN_E_ARG, "conv3x3: null pointer");
    if (N <= 0 || H <= 0 || W <= 0 || imgs_per_group <= 0 || N % imgs_per_group)
        BDN_FAIL(BDN_E_SHAPE, "conv3x3: bad N=%d H=%d W=%d imgs_per_group=%d", N, H, W, imgs_per_group);
    if (Cout <= 0 || Cout % 64) BDN_FAIL(BDN_E_SHAPE, "conv3x3: Cout=%d must be a multiple of 64", Cout);
    if (in1 == nullptr) C1 = 0;
    if (C1 < 0 || (in1 && C1 == 0)) BDN_FAIL(BDN_E_SHAPE, "conv3x3: bad C1=%d", C1);
    if (in_mode == BDN_IN_BNRELU && !in_bn) BDN_FAIL(BDN_E_ARG, "conv3x3: BNRELU input needs in_bn");
    if (in_mode != BDN_IN_BNRELU && in_mode != BDN_IN_PLAIN) BDN_FAIL(BDN_E_ARG, "conv3x3: bad in_mode %d", in_mode);
    if (in_mode == BDN_IN_BNRELU && in1) BDN_FAIL(BDN_E_ARG, "conv3x3: two-source input must be plain");
    ConvArgs a;
    a.in0 = in0; a.in1 = in1; a.C0 = C0; a.C1 = C1; a.ld0 = C0; a.ld1 = C1;
    a.w_kgroups = 0;
    if (dtype == BDN_BF16X3 || dtype == BDN_BF16X2) {
        // in0 is the split operand of bdn_split_pack: [N,H,W,2*C0] bf16 = hi(C0) | lo(C0), staged as two patches per chunk against the
        // packed filter image [w_hi | w_hi | w_lo]: a_hi*w_hi + a_lo*w_hi + a_hi*w_lo accumulate in the same f32 MFMA tile.
        // BDN_BF16X2: the first two terms -- a_hi*w_hi + a_lo*w_hi
        if (in1 || in_mode != BDN_IN_PLAIN) BDN_FAIL(BDN_E_ARG, "conv3x3(bf16x3): one split-packed, plain operand (bdn_split_pack does cat / BatchNorm+ReLU)");
        if (C0 % 16) BDN_FAIL(BDN_E_SHAPE, "conv3x3(bf16x3): C0=%d must be a multiple of 16", C0);
        a.in1 = nullptr; a.C0 = C0; a.C1 = 0; a.ld0 = 2 * C0; a.ld1 = 0; a.w_kgroups = 3 * C0 / 16;
    }
    {   // the kernels address every tensor as one uniform base + a 32-bit byte offset
        const size_t npix = (size_t)N * H * W, es = dtype == BDN_F32 ? 4 : 2, oes = dtype == BDN_BF16 ? 2 : 4;      // (bf16x3 / bf16x2: bf16 operands, float32 outputs)
        const size_t widest = (size_t)(a.ld0 > a.ld1 ? a.ld0 : a.ld1);
        if (npix * widest * es >= ((size_t)1 << 32) || npix * (size_t)Cout * oes >= ((size_t)1 << 32))
            BDN_FAIL(BDN_E_SHAPE, "conv3x3: a tensor of N*H*W=%zu pixels reaches 4 GB; split the batch", npix);
    }
    a.in_bn = in_mode == BDN_IN_BNRELU ? in_bn : nullptr;
    a.imgs_per_group = imgs_per_group; a.w = w; a.bias = bias; a.out = out; a.stats_partial = stats_partial;
    a.bs_z = bs_z; a.bs_bn = bs_bn; a.in2 = nullptr; a.Dz = 0;
    a.bb_z = bb_z; a.bb_bn = bb_bn; a.bb_sums = bb_sums; a.bb_dz = bb_dz; a.bb_invM = 1.f / (float)((size_t)imgs_per_group * H * W);
    a.N = N; a.H = H; a.W = W; a.Cout = Cout;
    a.ep_scale = a.ep_shift = nullptr; a.ep_mul = nullptr; a.ep_pool = nullptr; a.pair_stride = 0; a.ep_fuse = BDN_FUSE_PRODUCT;
    a.cls_w = a.cls_b = nullptr; a.cls_n = 0; a.cls_logits = nullptr; a.cls_mask = nullptr; a.cls_origins = nullptr; a.cls_H = a.cls_W = 0; a.x3_split = nullptr;
    const bool x3f = (dtype == BDN_BF16X3 || dtype == BDN_BF16X2);       // (C0 % 16 == 0 was checked above: 64-channel chunks where C0 allows, else 16)
    const ConvPlan g = x3f ? conv_plan_x3f(N, H, W, Cout, imgs_per_group) : conv_plan(N, H, W, Cout, imgs_per_group);
    a.tiles_y = g.g.tiles_y; a.tiles_x = g.g.tiles_x; a.n_ntiles = 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (x3f && C0 % 64 == 0) return dtype == BDN_BF16X3 ? dispatch_conv_x3f<3>(a, g, st) : dispatch_conv_x3f<2>(a, g, st);
    if (x3f) return dtype == BDN_BF16X3 ? dispatch_conv_x3f<3, false, 32>(a, g, st) : dispatch_conv_x3f<2, false, 32>(a, g, st);
    if (bb_z) {
        if (dtype != BDN_BF16 || C0 != 64 || in1 || in_mode != BDN_IN_PLAIN)
            BDN_FAIL(BDN_E_SHAPE, "conv3x3_dgrad_bb: bf16, one plain source of C0 = 64 channels (got %d)", C0);
        return dispatch_conv_bb(a, g, st);
    }
    if (dtype == BDN_BF16) {
        // channel chunk: 64 channels (128 B) when both sources allow it, else 16 channels (32 B)
        if (C0 % 64 == 0 && C1 % 64 == 0) return dispatch_conv<bf16s, 128>(a, g, st);
        if (C0 % 16 == 0 && C1 % 16 == 0) return dispatch_conv<bf16s, 32>(a, g, st);
        BDN_FAIL(BDN_E_SHAPE, "conv3x3(bf16): C0=%d C1=%d must be multiples of 16", C0, C1);
    } else if (dtype == BDN_F32) {
        if (C0 % 32 == 0 && C1 % 32 == 0) return dispatch_conv<float, 128>(a, g, st);
        if (C0 % 16 == 0 && C1 % 16 == 0) return dispatch_conv<float, 64>(a, g, st);
        BDN_FAIL(BDN_E_SHAPE, "conv3x3(f32): C0=%d C1=%d must be multiples of 16", C0, C1);
    }
    BDN_FAIL(BDN_E_ARG, "conv3x3: bad dtype %d", dtype);
}

extern "C" int bdn_conv3x3(int dtype, const void* in0, int C0, const void* in1, int C1,
                           int in_mode, const float* in_bn, int imgs_per_group,
                           const void* w, const float* bias, void* out, float* stats_partial,
                           int N, int H, int W, int Cout, void* stream) {
    return conv3x3_impl(dtype, in0, C0, in1, C1, in_mode, in_bn, imgs_per_group, w, bias, out, stats_partial,
                        nullptr, nullptr, N, H, W, Cout, stream);
}

extern "C" const char* bdn_conv3x3_variant(int dtype, int N, int H, int W, int C0, int C1, int Cout, int imgs_per_group) {
    g_conv_variant[0] = 0;
    g_conv_query = true;
    void* dummy = reinterpret_cast<void*>(16);             // never dereferenced: nothing is launched in query mode
    const int rc = conv3x3_impl(dtype, dummy, C0, C1 ? dummy : nullptr, C1, BDN_IN_PLAIN, nullptr, imgs_per_group, dummy, nullptr, dummy,
                                nullptr, nullptr, nullptr, N, H, W, Cout, nullptr);
    g_conv_query = false;
    return rc == BDN_OK ? g_conv_variant : "";
}

// bf16x3 / bf16x2 convolution on a FLOAT32 operand (round 6): what bdn_split_pack(in, BNRELU / PLAIN) + bdn_conv3x3(BDN_BF16X3) compute, in one
// launch -- the staging applies relu(z * scale + shift) and the bf16 hi / lo split on the way into LDS (models/unet_parts.py:14-16: BatchNorm ->
// ReLU -> Conv2d).  in [N,H,W,C0] float32, C0 a multiple of 64 and <= 512; w the bdn_pack_weights(BDN_BF16X3) image; out float32.
// split_out: NULL, or [N,H,W,2 C0] bf16 that receives exactly bdn_split_pack's output (the layer's weight-gradient GEMM reads it).
extern "C" int bdn_conv3x3_x3src(int dtype, const float* in, int C0, int in_mode, const float* in_bn, int imgs_per_group,
                                 const void* w, const float* bias, float* out, float* stats_partial, void* split_out,
                                 int N, int H, int W, int Cout, void* stream) {
    if (!in || !w || !out) BDN_FAIL(BDN_E_ARG, "conv3x3_x3src: null pointer");
    if (dtype != BDN_BF16X3 && dtype != BDN_BF16X2) BDN_FAIL(BDN_E_ARG, "conv3x3_x3src: bad dtype %d (bf16x3 / bf16x2)", dtype);
    if (N <= 0 || H <= 0 || W <= 0 || imgs_per_group <= 0 || N % imgs_per_group)
        BDN_FAIL(BDN_E_SHAPE, "conv3x3_x3src: bad N=%d H=%d W=%d imgs_per_group=%d", N, H, W, imgs_per_group);
    if (Cout <= 0 || Cout % 64) BDN_FAIL(BDN_E_SHAPE, "conv3x3_x3src: Cout=%d must be a multiple of 64", Cout);
    if (C0 <= 0 || C0 % 64 || C0 > 512) BDN_FAIL(BDN_E_SHAPE, "conv3x3_x3src: C0=%d must be a multiple of 64, at most 512", C0);
    if (in_mode != BDN_IN_BNRELU && in_mode != BDN_IN_PLAIN) BDN_FAIL(BDN_E_ARG, "conv3x3_x3src: bad in_mode %d", in_mode);
    if (in_mode == BDN_IN_BNRELU && !in_bn) BDN_FAIL(BDN_E_ARG, "conv3x3_x3src: BNRELU input needs in_bn");
    const size_t npix = (size_t)N * H * W;
    if (npix * (size_t)C0 * 4 >= ((size_t)1 << 32) || npix * (size_t)Cout * 4 >= ((size_t)1 << 32))
        BDN_FAIL(BDN_E_SHAPE, "conv3x3_x3src: a tensor of N*H*W=%zu pixels reaches 4 GB; split the batch", npix);
    ConvArgs a;
    a.in0 = in; a.in1 = nullptr; a.C0 = C0; a.C1 = 0; a.ld0 = C0; a.ld1 = 0; a.in2 = nullptr; a.Dz = 0;
    a.w_kgroups = 3 * C0 / 16;
    a.in_bn = in_mode == BDN_IN_BNRELU ? in_bn : nullptr;
    a.imgs_per_group = imgs_per_group; a.w = w; a.bias = bias; a.out = out; a.stats_partial = stats_partial;
    a.bs_z = nullptr; a.bs_bn = nullptr; a.bb_z = nullptr; a.bb_bn = nullptr; a.bb_sums = nullptr; a.bb_dz = nullptr; a.bb_invM = 0.f;
    a.N = N; a.H = H; a.W = W; a.Cout = Cout;
    a.ep_scale = a.ep_shift = nullptr; a.ep_mul = nullptr; a.ep_pool = nullptr; a.pair_stride = 0; a.ep_fuse = BDN_FUSE_PRODUCT;
    a.cls_w = a.cls_b = nullptr; a.cls_n = 0; a.cls_logits = nullptr; a.cls_mask = nullptr; a.cls_origins = nullptr; a.cls_H = a.cls_W = 0;
    a.x3_split = split_out;
    const ConvPlan g = conv_plan_x3f(N, H, W, Cout, imgs_per_group);
    a.tiles_y = g.g.tiles_y; a.tiles_x = g.g.tiles_x; a.n_ntiles = 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype == BDN_BF16X3 ? dispatch_conv_x3f<3, true>(a, g, st) : dispatch_conv_x3f<2, true>(a, g, st);
}

extern "C" const char* bdn_conv3x3_x3src_variant(int dtype, int N, int H, int W, int C0, int Cout, int imgs_per_group) {
    g_conv_variant[0] = 0;
    g_conv_query = true;
    const float* dummy = reinterpret_cast<const float*>(16);      // never dereferenced: nothing is launched in query mode
    const int rc = bdn_conv3x3_x3src(dtype, dummy, C0, BDN_IN_PLAIN, nullptr, imgs_per_group, dummy, nullptr, const_cast<float*>(dummy), nullptr, nullptr,
                                     N, H, W, Cout, nullptr);
    g_conv_query = false;
    return rc == BDN_OK ? g_conv_variant : "";
}

extern "C" int bdn_conv3x3_dgrad_bs(int dtype, const void* dz, int C0, const void* w_dgrad, void* dA,
                                    const void* z_prev, const float* bn_prev, int imgs_per_group, float* bs_partial,
                                    int N, int H, int W, int Cout, void* stream) {
    if (!z_prev || !bn_prev || !bs_partial) BDN_FAIL(BDN_E_ARG, "conv3x3_dgrad_bs: null pointer");
    return conv3x3_impl(dtype, dz, C0, nullptr, 0, BDN_IN_PLAIN, nullptr, imgs_per_group, w_dgrad, nullptr, dA, bs_partial,
                        z_prev, bn_prev, N, H, W, Cout, stream);
}

// Data gradient of layer L with L's BatchNorm+ReLU backward applied while dz is staged (bdn_bn_bwd_apply never runs, dz is written once
// as a by-product for the weight-gradient GEMM): dA = the MASKED gradient g [N,H,W,C0] (ldA == C0) as stored by bdn_conv3x3_dgrad_bs /
// bdn_enc_skip_bwd / bdn_upsample2x_bwd_bs, z / bn / sums of layer L (sums from bdn_bn_bwd_finalize).
// z_prev / bn_prev / bs_partial: as bdn_conv3x3_dgrad_bs (all three NULL: no fused statistics of the producing layer).
extern "C" int bdn_conv3x3_dgrad_bb(int dtype, const void* dA, int C0, const void* z, const float* bn, const float* sums, int imgs_per_group,
                                    const void* w_dgrad, void* dA_prev, const void* z_prev, const float* bn_prev, float* bs_partial,
                                    void* dz_out, int N, int H, int W, int Cout, void* stream) {
    if (!z || !bn || !sums) BDN_FAIL(BDN_E_ARG, "conv3x3_dgrad_bb: null pointer");
    if ((z_prev != nullptr) != (bn_prev != nullptr) || (z_prev != nullptr) != (bs_partial != nullptr))
        BDN_FAIL(BDN_E_ARG, "conv3x3_dgrad_bb: z_prev, bn_prev and bs_partial come together");
    if (H <= 8 && W <= 8) BDN_FAIL(BDN_E_SHAPE, "conv3x3_dgrad_bb: maps of 8x8 and below are not supported");
    return conv3x3_impl(dtype, dA, C0, nullptr, 0, BDN_IN_PLAIN, nullptr, imgs_per_group, w_dgrad, nullptr, dA_prev, bs_partial,
                        z_prev, bn_prev, N, H, W, Cout, stream, z, bn, sums, dz_out);
}

extern "C" const char* bdn_conv3x3_dgrad_bb_variant(int N, int H, int W, int Cout, int imgs_per_group) {
    g_conv_variant[0] = 0;
    g_conv_query = true;
    void* dummy = reinterpret_cast<void*>(16);             // never dereferenced: nothing is launched in query mode
    const int rc = conv3x3_impl(BDN_BF16, dummy, 64, nullptr, 0, BDN_IN_PLAIN, nullptr, imgs_per_group, dummy, nullptr, dummy, nullptr, nullptr, nullptr,
                                N, H, W, Cout, nullptr, dummy, reinterpret_cast<const float*>(dummy), reinterpret_cast<const float*>(dummy), nullptr);
    g_conv_query = false;
    return rc == BDN_OK ? g_conv_variant : "";
}

// Eval-mode convolution stage (models/unet_parts.py:13-18 with the BatchNorm in eval mode): conv3x3 -> BatchNorm (running statistics, folded
// with the conv bias into ep_scale / ep_shift by bdn_bn_eval_fold_multi) -> ReLU in ONE launch that stores the activation.  Optional fused
// consumers: the date product (mul), MaxPool2d(2) (pool), the 1x1 classifier + argmax (+ scene stitching).  See ConvArgs.
static int conv3x3_eval_impl(int dtype, const void* in0, int C0, const void* in1, int C1, const void* w, const float* ep_scale, const float* ep_shift,
                             void* out, const void* mul, int fusion, void* pool, const float* cls_w, const float* cls_b, int ncls, float* logits,
                             unsigned char* mask, const int* origins, int Hs, int Ws, int N, int H, int W, int Cout, void* stream) {
    if (!in0 || !w || !ep_scale || !ep_shift) BDN_FAIL(BDN_E_ARG, "conv3x3_eval: null pointer");
    if (N <= 0 || H <= 0 || W <= 0) BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval: bad N=%d H=%d W=%d", N, H, W);
    if (Cout <= 0 || Cout % 64) BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval: Cout=%d must be a multiple of 64", Cout);
    if (in1 == nullptr) C1 = 0;
    if (C1 < 0 || (in1 && C1 == 0)) BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval: bad C1=%d", C1);
    if (dtype != BDN_BF16 && dtype != BDN_F32) BDN_FAIL(BDN_E_ARG, "conv3x3_eval: bad dtype %d (bf16 / f32)", dtype);
    if (fusion != BDN_FUSE_PRODUCT && fusion != BDN_FUSE_ABSDIFF) BDN_FAIL(BDN_E_ARG, "conv3x3_eval: bad fusion mode %d", fusion);
    if (pool && (H < 2 || W < 2)) BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval: pooling needs H, W >= 2");
    if (cls_w) {
        if (!cls_b || (!logits && !mask)) BDN_FAIL(BDN_E_ARG, "conv3x3_eval_cls: null pointer");
        if (Cout != 64 || ncls < 1 || ncls > 2) BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval_cls: Cout=%d must be 64 and ncls=%d 1 or 2 (bdn_outc_fwd covers the rest)", Cout, ncls);
        if (mul || pool) BDN_FAIL(BDN_E_ARG, "conv3x3_eval_cls: no product / pooling on the classifier stage");
        if (origins && (!mask || Hs < H || Ws < W)) BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval_cls: stitching needs a mask of at least one tile");
    } else if (!out) BDN_FAIL(BDN_E_ARG, "conv3x3_eval: null pointer");
    const size_t es = dtype == BDN_F32 ? 4 : 2, npix = (size_t)N * H * W, widest = (size_t)(C0 > C1 ? C0 : C1);
    if (npix * widest * es >= ((size_t)1 << 32) || npix * (size_t)Cout * es >= ((size_t)1 << 32))
        BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval: a tensor of N*H*W=%zu pixels reaches 4 GB; split the batch", npix);
    ConvArgs a;
    a.in0 = in0; a.in1 = in1; a.C0 = C0; a.C1 = C1; a.ld0 = C0; a.ld1 = C1; a.in2 = nullptr; a.Dz = 0;
    a.in_bn = nullptr; a.imgs_per_group = N; a.w = w; a.w_kgroups = 0; a.bias = nullptr; a.out = out; a.stats_partial = nullptr;
    a.bs_z = nullptr; a.bs_bn = nullptr; a.bb_z = nullptr; a.bb_bn = nullptr; a.bb_sums = nullptr; a.bb_dz = nullptr; a.bb_invM = 0.f;
    a.N = N; a.H = H; a.W = W; a.Cout = Cout;
    a.ep_scale = ep_scale; a.ep_shift = ep_shift; a.ep_mul = mul; a.ep_pool = pool; a.pair_stride = 0; a.ep_fuse = fusion;
    a.cls_w = cls_w; a.cls_b = cls_b; a.cls_n = ncls; a.cls_logits = logits; a.cls_mask = mask; a.cls_origins = origins; a.cls_H = Hs; a.cls_W = Ws; a.x3_split = nullptr;
    // no statistic groups in eval mode: two images of a small map may always share a tile
    const ConvPlan g = conv_plan(N, H, W, Cout, N % 2 == 0 ? 2 : 1);
    a.tiles_y = g.g.tiles_y; a.tiles_x = g.g.tiles_x; a.n_ntiles = 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == BDN_BF16) {
        if (C0 % 64 == 0 && C1 % 64 == 0) return dispatch_conv<bf16s, 128, true>(a, g, st);
        if (C0 % 16 == 0 && C1 % 16 == 0) return dispatch_conv<bf16s, 32, true>(a, g, st);
        BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval(bf16): C0=%d C1=%d must be multiples of 16", C0, C1);
    }
    if (C0 % 32 == 0 && C1 % 32 == 0) return dispatch_conv<float, 128, true>(a, g, st);
    if (C0 % 16 == 0 && C1 % 16 == 0) return dispatch_conv<float, 64, true>(a, g, st);
    BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval(f32): C0=%d C1=%d must be multiples of 16", C0, C1);
}

extern "C" int bdn_conv3x3_eval(int dtype, const void* in0, int C0, const void* in1, int C1, const void* w,
                                const float* ep_scale, const float* ep_shift, void* out, const void* mul, void* pool,
                                int N, int H, int W, int Cout, void* stream) {
    return conv3x3_eval_impl(dtype, in0, C0, in1, C1, w, ep_scale, ep_shift, out, mul, BDN_FUSE_PRODUCT, pool, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0,
                             N, H, W, Cout, stream);
}

extern "C" int bdn_conv3x3_eval_fusion(int dtype, int fusion, const void* in0, int C0, const void* in1, int C1, const void* w,
                                       const float* ep_scale, const float* ep_shift, void* out, const void* mul, void* pool,
                                       int N, int H, int W, int Cout, void* stream) {
    return conv3x3_eval_impl(dtype, in0, C0, in1, C1, w, ep_scale, ep_shift, out, mul, fusion, pool, nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0, 0,
                             N, H, W, Cout, stream);
}

// Date-paired eval stage: the second convolution of an encoder level on BOTH dates of B patch pairs (in [2B,H,W,C0], date 1 first) with tiles
// of two images n and n + B.  f_out [B,H,W,Cout] = relu(a_d2 * a_d1) (models/bidate_model.py:35-38), pool [2B,H/2,W/2,Cout] = MaxPool2d(2) of
// both dates (NULL at the last level); the activations themselves are never stored.
static ConvPlan conv_plan_pair(int B, int H, int W, int Cout) {
    ConvPlan p;
    TileGeom& g = p.g;
    const bool narrow = (Cout % 128 != 0);
    g.TI = 2; g.TH = 8;
    g.TW = (!(W <= 8 && H <= 8) && narrow) ? 16 : 8;
    g.tiles_y = (H + g.TH - 1) / g.TH;
    g.tiles_x = (W + g.TW - 1) / g.TW;
    g.n_mtiles = B * g.tiles_y * g.tiles_x;
    p.BN = (!narrow && (long)g.n_mtiles * (Cout / 128) >= 512) ? 128 : 64;
    return p;
}

template <typename T>
static int dispatch_conv_pair(const ConvArgs& a, const ConvPlan& p, hipStream_t st) {
    const TileGeom& g = p.g;
    const bool one = a.C0 * (int)sizeof(T) == 128;
    if (g.TW == 16 && one) return launch_conv<T, 128, 8, 16, 2, 64, 2, 2, true, T, false, false, true>(a, g.n_mtiles, st);
    if (g.TW == 16) return launch_conv<T, 128, 8, 16, 2, 64, 4, 1, false, T, false, false, true>(a, g.n_mtiles, st);
    if (p.BN == 128 && (a.H > 8 || a.W > 8)) return launch_conv<T, 128, 8, 8, 2, 128, 1, 4, false, T, false, false, true>(a, g.n_mtiles, st);
    if (p.BN == 128) return launch_conv<T, 128, 8, 8, 2, 128, 2, 2, false, T, false, false, true>(a, g.n_mtiles, st);
    return launch_conv<T, 128, 8, 8, 2, 64, 2, 2, false, T, false, false, true>(a, g.n_mtiles, st);
}

static int conv3x3_eval_pair_impl(int dtype, int fusion, const void* in, int C0, const void* w, const float* ep_scale, const float* ep_shift,
                                  void* f_out, void* pool, int B, int H, int W, int Cout, void* stream) {
    if (!in || !w || !ep_scale || !ep_shift || !f_out) BDN_FAIL(BDN_E_ARG, "conv3x3_eval_pair: null pointer");
    if (B <= 0 || H <= 0 || W <= 0) BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval_pair: bad B=%d H=%d W=%d", B, H, W);
    if (Cout <= 0 || Cout % 64) BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval_pair: Cout=%d must be a multiple of 64", Cout);
    if (dtype != BDN_BF16 && dtype != BDN_F32) BDN_FAIL(BDN_E_ARG, "conv3x3_eval_pair: bad dtype %d (bf16 / f32)", dtype);
    if (fusion != BDN_FUSE_PRODUCT && fusion != BDN_FUSE_ABSDIFF) BDN_FAIL(BDN_E_ARG, "conv3x3_eval_pair: bad fusion mode %d", fusion);
    const int es = dtype == BDN_F32 ? 4 : 2;
    if (C0 <= 0 || (C0 * es) % 128) BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval_pair: C0=%d must be a multiple of %d", C0, 128 / es);
    if (pool && (H < 2 || W < 2)) BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval_pair: pooling needs H, W >= 2");
    const size_t npix = (size_t)2 * B * H * W;
    if (npix * (size_t)C0 * es >= ((size_t)1 << 32) || npix * (size_t)Cout * es >= ((size_t)1 << 32))
        BDN_FAIL(BDN_E_SHAPE, "conv3x3_eval_pair: a tensor of N*H*W=%zu pixels reaches 4 GB; split the batch", npix);
    ConvArgs a;
    a.in0 = in; a.in1 = nullptr; a.C0 = C0; a.C1 = 0; a.ld0 = C0; a.ld1 = 0; a.in2 = nullptr; a.Dz = 0;
    a.in_bn = nullptr; a.imgs_per_group = B; a.w = w; a.w_kgroups = 0; a.bias = nullptr; a.out = f_out; a.stats_partial = nullptr;
    a.bs_z = nullptr; a.bs_bn = nullptr; a.bb_z = nullptr; a.bb_bn = nullptr; a.bb_sums = nullptr; a.bb_dz = nullptr; a.bb_invM = 0.f;
    a.N = 2 * B; a.H = H; a.W = W; a.Cout = Cout;
    a.ep_scale = ep_scale; a.ep_shift = ep_shift; a.ep_mul = nullptr; a.ep_pool = pool; a.pair_stride = B; a.ep_fuse = fusion;
    a.cls_w = a.cls_b = nullptr; a.cls_n = 0; a.cls_logits = nullptr; a.cls_mask = nullptr; a.cls_origins = nullptr; a.cls_H = a.cls_W = 0; a.x3_split = nullptr;
    const ConvPlan g = conv_plan_pair(B, H, W, Cout);
    a.tiles_y = g.g.tiles_y; a.tiles_x = g.g.tiles_x; a.n_ntiles = 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    return dtype == BDN_BF16 ? dispatch_conv_pair<bf16s>(a, g, st) : dispatch_conv_pair<float>(a, g, st);
}

extern "C" int bdn_conv3x3_eval_pair(int dtype, const void* in, int C0, const void* w, const float* ep_scale, const float* ep_shift,
                                     void* f_out, void* pool, int B, int H, int W, int Cout, void* stream) {
    return conv3x3_eval_pair_impl(dtype, BDN_FUSE_PRODUCT, in, C0, w, ep_scale, ep_shift, f_out, pool, B, H, W, Cout, stream);
}

extern "C" int bdn_conv3x3_eval_pair_fusion(int dtype, int fusion, const void* in, int C0, const void* w, const float* ep_scale, const float* ep_shift,
                                            void* f_out, void* pool, int B, int H, int W, int Cout, void* stream) {
    return conv3x3_eval_pair_impl(dtype, fusion, in, C0, w, ep_scale, ep_shift, f_out, pool, B, H, W, Cout, stream);
}

extern "C" int bdn_conv3x3_eval_cls(int dtype, const void* in0, int C0, const void* w, const float* ep_scale, const float* ep_shift, void* act_out,
                                    const float* cls_w, const float* cls_b, int ncls, float* logits, uint8_t* mask, const int32_t* origins,
                                    int Hs, int Ws, int N, int H, int W, int Cout, void* stream) {
    if (!cls_w) BDN_FAIL(BDN_E_ARG, "conv3x3_eval_cls: null pointer");
    return conv3x3_eval_impl(dtype, in0, C0, nullptr, 0, w, ep_scale, ep_shift, act_out, nullptr, BDN_FUSE_PRODUCT, nullptr, cls_w, cls_b, ncls, logits, mask, origins,
                             Hs, Ws, N, H, W, Cout, stream);
}

// which instantiation an eval-mode entry point runs (kind BDN_EVAL_STAGE / _PAIR / _CLS): the entry point itself in query mode.  The fused
// consumers (mul, pool, logits / mask / stitching) are runtime arguments of the same instantiation and do not change the answer.
extern "C" const char* bdn_conv3x3_eval_variant(int kind, int dtype, int N, int H, int W, int C0, int C1, int Cout) {
    g_conv_variant[0] = 0;
    g_conv_query = true;
    void* dummy = reinterpret_cast<void*>(16);             // never dereferenced: nothing is launched in query mode
    const float* fd = reinterpret_cast<const float*>(dummy);
    int rc = BDN_E_ARG;
    if (kind == BDN_EVAL_STAGE)
        rc = bdn_conv3x3_eval(dtype, dummy, C0, C1 ? dummy : nullptr, C1, dummy, fd, fd, dummy, nullptr, nullptr, N, H, W, Cout, nullptr);
    else if (kind == BDN_EVAL_PAIR && C1 == 0)
        rc = bdn_conv3x3_eval_pair(dtype, dummy, C0, dummy, fd, fd, dummy, nullptr, N, H, W, Cout, nullptr);
    else if (kind == BDN_EVAL_CLS && C1 == 0)
        rc = bdn_conv3x3_eval_cls(dtype, dummy, C0, dummy, fd, fd, nullptr, fd, fd, 2, reinterpret_cast<float*>(dummy), nullptr, nullptr,
                                  0, 0, N, H, W, Cout, nullptr);
    g_conv_query = false;
    return rc == BDN_OK ? g_conv_variant : "";
}

// ---------------------------------------------------------------------------------------------------------------------
// 3x3x3 convolution, stride 1, zero padding 1 in depth / height / width -- the building block of BASELINE configs[3], the
// multi-date 3-D U-Net (5 dates x 13 bands x 128 x 128).  The reference tree has NO source for that model (UNetLSTM/ is an
// empty sub-module): parity is unpinned, the oracle is torch.nn.functional.conv3d (tests/test_gpu_conv3d.py).
// Implicit GEMM with K = 27 Cin on the 2-D kernel: the D slices of a sample are consecutive NHWC images, a 3x3x3 window is
// three 3x3 windows on the slices d-1, d, d+1, i.e. three SOURCES of one longer reduction (the two-source K loop of the
// never-materialised torch.cat, generalised), and a slice outside the sample is a block-uniform zero mask.  No depth padding is
// ever materialised, nothing is im2col'ed, the filter image is the 2-D fragment order with 3 Cin channels per tap.
static ConvPlan conv3d_plan(int NS, int H, int W, int Cout) {
    ConvPlan p;
    TileGeom& g = p.g;
    g.TI = 1; g.TH = 8; g.TW = 16;
    g.tiles_y = (H + 7) / 8; g.tiles_x = (W + 15) / 16;
    g.n_mtiles = NS * g.tiles_y * g.tiles_x;
    p.BN = (Cout % 128 == 0 && (long)g.n_mtiles * (Cout / 128) >= 512) ? 128 : 64;
    return p;
}

extern "C" int bdn_conv3d_num_mtiles(int N, int D, int H, int W) {
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
    return conv3d_plan(N * D, H, W, 64).g.n_mtiles;
}

template <typename T, int CKB, typename TO = T>
static int dispatch_conv3d(const ConvArgs& a, const ConvPlan& p, hipStream_t st) {
    if (p.BN == 128) return launch_conv<T, CKB, 8, 16, 1, 128, 1, 4, false, TO, true>(a, p.g.n_mtiles, st);
    return launch_conv<T, CKB, 8, 16, 1, 64, 2, 2, false, TO, true>(a, p.g.n_mtiles, st);
}

// in: [N,D,H,W,C]; w: bdn_pack_weights image of the OIHW view [Cout][3 C][3][3] whose input channel kd*C + c is tap kd of channel c
// (wf: [Cout][9][3 C]); out: [N,D,H,W,Cout]; stats_partial: NULL or [bdn_conv3d_num_mtiles][2][Cout]; imgs_per_group counts SAMPLES.
extern "C" int bdn_conv3d(int dtype, const void* in, int C, int in_mode, const float* in_bn, int imgs_per_group,
                          const void* w, const float* bias, void* out, float* stats_partial,
                          int N, int D, int H, int W, int Cout, void* stream) {
    if (!in || !w || !out) BDN_FAIL(BDN_E_ARG, "conv3d: null pointer");
    if (N <= 0 || D <= 0 || H <= 0 || W <= 0 || imgs_per_group <= 0 || N % imgs_per_group)
        BDN_FAIL(BDN_E_SHAPE, "conv3d: bad N=%d D=%d H=%d W=%d imgs_per_group=%d", N, D, H, W, imgs_per_group);
    if (Cout <= 0 || Cout % 64 || C <= 0 || C % 16) BDN_FAIL(BDN_E_SHAPE, "conv3d: Cout=%d must be a multiple of 64, C=%d of 16", Cout, C);
    if (in_mode != BDN_IN_PLAIN && in_mode != BDN_IN_BNRELU) BDN_FAIL(BDN_E_ARG, "conv3d: bad in_mode %d", in_mode);
    if (in_mode == BDN_IN_BNRELU && !in_bn) BDN_FAIL(BDN_E_ARG, "conv3d: BNRELU input needs in_bn");
    if (dtype != BDN_BF16 && dtype != BDN_F32 && dtype != BDN_BF16X3) BDN_FAIL(BDN_E_ARG, "conv3d: bad dtype %d (bf16 / f32 / bf16x3)", dtype);
    // bf16x3: `in` is the bf16 operand [N,D,H,W,C] with C = 3 x the logical width, channels [hi | lo | hi] of the float32 tensor (bdn_split_pack
    // + a repeat of its hi half), `w` the plain bf16 image of the view whose channels are [w_hi | w_hi | w_lo] per depth tap; out is float32
    if (dtype == BDN_BF16X3 && in_mode != BDN_IN_PLAIN) BDN_FAIL(BDN_E_ARG, "conv3d(bf16x3): plain operand (the split applies BatchNorm+ReLU)");
    const size_t es = dtype == BDN_F32 ? 4 : 2, oes = dtype == BDN_BF16 ? 2 : 4, slice = (size_t)H * W * C * es;
    if ((size_t)N * D * slice >= ((size_t)1 << 32) || (size_t)N * D * H * W * Cout * oes >= ((size_t)1 << 32))
        BDN_FAIL(BDN_E_SHAPE, "conv3d: a tensor reaches 4 GB (32-bit byte offsets inside the kernel); split the batch");
    ConvArgs a;
    a.in1 = in; a.in0 = static_cast<const unsigned char*>(in) - slice; a.in2 = static_cast<const unsigned char*>(in) + slice;
    a.C0 = C; a.C1 = C; a.ld0 = C; a.ld1 = C; a.Dz = D; a.w_kgroups = 0;
    a.in_bn = in_mode == BDN_IN_BNRELU ? in_bn : nullptr;
    a.imgs_per_group = imgs_per_group * D;
    a.w = w; a.bias = bias; a.out = out; a.stats_partial = stats_partial; a.bs_z = nullptr; a.bs_bn = nullptr;
    a.N = N * D; a.H = H; a.W = W; a.Cout = Cout;
    a.bb_z = nullptr; a.bb_bn = nullptr; a.bb_sums = nullptr; a.bb_dz = nullptr; a.bb_invM = 0.f;
    a.ep_scale = a.ep_shift = nullptr; a.ep_mul = nullptr; a.ep_pool = nullptr; a.pair_stride = 0; a.ep_fuse = BDN_FUSE_PRODUCT;
    a.cls_w = a.cls_b = nullptr; a.cls_n = 0; a.cls_logits = nullptr; a.cls_mask = nullptr; a.cls_origins = nullptr; a.cls_H = a.cls_W = 0; a.x3_split = nullptr;
    const ConvPlan p = conv3d_plan(N * D, H, W, Cout);
    a.tiles_y = p.g.tiles_y; a.tiles_x = p.g.tiles_x; a.n_ntiles = 0;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    if (dtype == BDN_BF16X3) return C % 64 == 0 ? dispatch_conv3d<bf16s, 128, float>(a, p, st) : dispatch_conv3d<bf16s, 32, float>(a, p, st);
    if (dtype == BDN_BF16) return C % 64 == 0 ? dispatch_conv3d<bf16s, 128>(a, p, st) : dispatch_conv3d<bf16s, 32>(a, p, st);
    return C % 32 == 0 ? dispatch_conv3d<float, 128>(a, p, st) : dispatch_conv3d<float, 64>(a, p, st);
}
