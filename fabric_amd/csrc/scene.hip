// libbidate_hip: full-scene sliding-window inference helpers.
// The two dates of a scene stay resident in HBM as band planes; tiles are gathered straight into the packed
// NHWC batch and predictions are written straight into the scene mask -- no host-side patch stack.
#include "common.hpp"
#include "patch_core.hpp"
#include "philox_core.hpp"
#include <climits>
#include <cmath>
#include <cstring>
#include <type_traits>

// ============================================================ band upload
// One row band of ALL band planes of a host scene in ONE copy: [C] planes of H x W float32, rows [r0, r1) of each -- a 2-D copy of C "rows" of
// (r1 - r0) * W * 4 bytes at pitch H * W * 4 (what train.py:190-193 does per batch with .to(device), here per band of the resident scene).
// The round-5 feeder issued one copy per plane (26 per band for both dates); boxes whose DMA engines pay more per copy sustained 37 of 57 GB/s.
extern "C" int bdn_upload_band(float* dst_planes, const float* src_planes_host, int C, int H, int W, int r0, int r1, void* stream) {
    if (!dst_planes || !src_planes_host) BDN_FAIL(BDN_E_ARG, "upload_band: null pointer");
    if (C <= 0 || H <= 0 || W <= 0 || r0 < 0 || r1 <= r0 || r1 > H) BDN_FAIL(BDN_E_SHAPE, "upload_band: bad C=%d H=%d W=%d rows [%d, %d)", C, H, W, r0, r1);
    const size_t pitch = (size_t)H * W * sizeof(float), off = (size_t)r0 * W, width = (size_t)(r1 - r0) * W * sizeof(float);
    const hipError_t e = hipMemcpy2DAsync(dst_planes + off, pitch, src_planes_host + off, pitch, width, (size_t)C, hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e != hipSuccess) BDN_FAIL(BDN_E_HIP, "upload_band: hipMemcpy2DAsync: %s", hipGetErrorString(e));
    return BDN_OK;
}

// ============================================================ gather_tiles
// reference: utils/inference.py:134-184 (_get_patches) + :61-66 (NHWC->NCHW transpose) + train.py:190-193
// (batch slice, host->device).  scene_d*: [C][H][W] f32 band planes.  origins: int32 [n][2] = (y0, x0).
// out: [2n][p][p][Cpad] T, date-1 tiles first (the layout bdn_pack_input produces).
// One thread per (tile pixel, 16-byte unit): plane reads are coalesced along x, every store is 16 bytes.
template <typename T>
__global__ void gather_tiles_kernel(const float* __restrict__ s1, const float* __restrict__ s2,
                                    const int* __restrict__ origins, T* __restrict__ out,
                                    int n, int C, int H, int W, int p, int Cpad) {
    constexpr int EPU = ET<T>::EPU;
    const int upp = Cpad / EPU;
    const size_t total = (size_t)2 * n * p * p * upp;
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    // unit index is the SLOW coordinate inside a tile row so that a wave reads 64 consecutive x of one plane set
    const int x = i % p; size_t t = i / p;
    const int u = t % upp; t /= upp;
    const int y = t % p; const int tile = t / p;
    const int date = tile >= n, tt = tile - date * n;
    const int y0 = origins[2 * tt], x0 = origins[2 * tt + 1];
    const size_t hw = (size_t)H * W;
    const float* src = (date ? s2 : s1) + (size_t)(y0 + y) * W + (x0 + x);
    float f[EPU];
#pragma unroll
    for (int e = 0; e < EPU; e++) {
        const int c = u * EPU + e;
        f[e] = c < C ? src[(size_t)c * hw] : 0.f;
    }
    T* dst = out + (((size_t)tile * p + y) * p + x) * Cpad + u * EPU;
    *reinterpret_cast<uint4*>(dst) = Unit<T>::pack(f);
}

extern "C" int bdn_gather_tiles(int dtype, const float* scene_d1, const float* scene_d2, const int32_t* origins,
                                void* out, int n_tiles, int C, int H, int W, int p, int Cpad, void* stream) {
    if (!scene_d1 || !scene_d2 || !origins || !out) BDN_FAIL(BDN_E_ARG, "gather_tiles: null pointer");
    if (n_tiles <= 0 || C <= 0 || p <= 0 || H < p || W < p || Cpad < C || Cpad % 16)
        BDN_FAIL(BDN_E_SHAPE, "gather_tiles: need H,W >= p, Cpad a multiple of 16 and >= C");
    hipStream_t st = (hipStream_t)stream;
    if (dtype == BDN_BF16) {
        const size_t total = (size_t)2 * n_tiles * p * p * (Cpad / 8);
        hipLaunchKernelGGL(gather_tiles_kernel<bf16s>, dim3(grid_for(total)), dim3(256), 0, st,
                           scene_d1, scene_d2, origins, (bf16s*)out, n_tiles, C, H, W, p, Cpad);
    } else if (dtype == BDN_F32) {
        const size_t total = (size_t)2 * n_tiles * p * p * (Cpad / 4);
        hipLaunchKernelGGL(gather_tiles_kernel<float>, dim3(grid_for(total)), dim3(256), 0, st,
                           scene_d1, scene_d2, origins, (float*)out, n_tiles, C, H, W, p, Cpad);
    } else BDN_FAIL(BDN_E_ARG, "gather_tiles: bad dtype");
    BDN_CHECK_LAUNCH("gather_tiles");
    return BDN_OK;
}

// ============================================================ ingest: per-band normalisation + resize to the label grid
// reference utils/dataloaders.py:86-111 (city_loader): band = (band.astype(float32) - mean) / std; band = cv2.resize(band,
// (W, H)) (default INTER_LINEAR).  Sentinel-2 bands come at 10 / 20 / 60 m, the label raster at 10 m, so most bands
// are upsampled 2x or 6x into their plane of the [C][H][W] scene that the tile gather reads.
// cv2's float INTER_LINEAR (OpenCV imgproc/resize.cpp): fx = (dx + 0.5) * (src_w / dst_w) - 0.5, sx = floor(fx),
// fx -= sx, clamped to [0, src_w - 1] with weight (1, 0) at either border; rows alike; horizontal pass first.
template <typename S>
__global__ void ingest_band_kernel(const S* __restrict__ src, int hs, int ws, float mean, float stdv,
                                   float* __restrict__ dst, int H, int W, double scale_y, double scale_x) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    float fy = (float)((y + 0.5) * scale_y - 0.5), fx = (float)((x + 0.5) * scale_x - 0.5);
    int sy = (int)floorf(fy), sx = (int)floorf(fx);
    fy -= (float)sy; fx -= (float)sx;
    if (sy < 0) { sy = 0; fy = 0.f; }
    if (sy >= hs - 1) { sy = hs - 1; fy = 0.f; }
    if (sx < 0) { sx = 0; fx = 0.f; }
    if (sx >= ws - 1) { sx = ws - 1; fx = 0.f; }
    const int sy1 = min(sy + 1, hs - 1), sx1 = min(sx + 1, ws - 1);
    const float a00 = ((float)src[(size_t)sy * ws + sx] - mean) / stdv, a01 = ((float)src[(size_t)sy * ws + sx1] - mean) / stdv;
    const float a10 = ((float)src[(size_t)sy1 * ws + sx] - mean) / stdv, a11 = ((float)src[(size_t)sy1 * ws + sx1] - mean) / stdv;
    const float r0 = a00 * (1.f - fx) + a01 * fx, r1 = a10 * (1.f - fx) + a11 * fx;      // horizontal pass, then vertical
    dst[(size_t)y * W + x] = r0 * (1.f - fy) + r1 * fy;
}

extern "C" int bdn_ingest_band(int src_is_f32, const void* src, int hs, int ws, float mean, float stdv,
                               float* dst, int H, int W, void* stream) {
    if (!src || !dst) BDN_FAIL(BDN_E_ARG, "ingest_band: null pointer");
    if (hs <= 0 || ws <= 0 || H <= 0 || W <= 0 || !(stdv != 0.f)) BDN_FAIL(BDN_E_SHAPE, "ingest_band: bad shape or zero std");
    const dim3 grid((W + 255) / 256, H);
    const double sy = (double)hs / H, sx = (double)ws / W;
    if (src_is_f32) hipLaunchKernelGGL(ingest_band_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src, hs, ws, mean, stdv, dst, H, W, sy, sx);
    else hipLaunchKernelGGL(ingest_band_kernel<unsigned short>, grid, dim3(256), 0, (hipStream_t)stream, (const unsigned short*)src, hs, ws, mean, stdv, dst, H, W, sy, sx);
    BDN_CHECK_LAUNCH("ingest_band");
    return BDN_OK;
}

// ============================================================ argmax (+ stitch)
// reference: `_, cd_preds = torch.max(preds, 1)` train.py:199 (first maximum wins ties), then
// utils/inference.py:187-236 (_get_bands): main tiles, then last-column tiles, then last-row tiles, then the
// corner are pasted in that order, later pastes overwriting earlier ones.  Equivalent order-free rule used here:
// a pixel belongs to the far-edge band(s) it lies in (y >= H-p, x >= W-p) and only a tile anchored on exactly
// those bands writes it, so tiles of one launch never race with different values.
__global__ void argmax_stitch_kernel(const float* __restrict__ logits, const int* __restrict__ origins,
                                     unsigned char* __restrict__ out, int n, int ncls, int p, int H, int W, size_t pp) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;      // pp: pixels per image (p * p for tiles; H * W for the plain argmax of [n,ncls,H,W])
    if (i >= (size_t)n * pp) return;
    const int tile = i / pp; const int rem = i % pp;
    const float* l = logits + (size_t)tile * ncls * pp + rem;
    float best = l[0]; int arg = 0;
    for (int c = 1; c < ncls; c++) {
        const float v = l[(size_t)c * pp];
        if (v > best) { best = v; arg = c; }
    }
    if (!origins) { out[i] = (unsigned char)arg; return; }
    const int y0 = origins[2 * tile], x0 = origins[2 * tile + 1];
    const int y = y0 + rem / p, x = x0 + rem % p;
    const bool ty = y0 == H - p, tx = x0 == W - p;
    const bool py = y >= H - p, px = x >= W - p;
    if (ty == py && tx == px) out[(size_t)y * W + x] = (unsigned char)arg;
}

extern "C" int bdn_argmax(const float* logits, uint8_t* out, int n, int ncls, int H, int W, void* stream) {
    if (!logits || !out) BDN_FAIL(BDN_E_ARG, "argmax: null pointer");
    if (n <= 0 || ncls <= 0 || ncls > 256 || H <= 0 || W <= 0) BDN_FAIL(BDN_E_SHAPE, "argmax: bad shape (<= 256 classes)");
    hipLaunchKernelGGL(argmax_stitch_kernel, dim3(grid_for((size_t)n * H * W)), dim3(256), 0, (hipStream_t)stream,
                       logits, (const int*)nullptr, out, n, ncls, H, H, W, (size_t)H * W);
    BDN_CHECK_LAUNCH("argmax");
    return BDN_OK;
}

extern "C" int bdn_argmax_stitch(const float* logits, const int32_t* origins, uint8_t* mask,
                                 int n_tiles, int ncls, int p, int H, int W, void* stream) {
    if (!logits || !origins || !mask) BDN_FAIL(BDN_E_ARG, "argmax_stitch: null pointer");
    if (n_tiles <= 0 || ncls <= 0 || ncls > 256 || p <= 0 || H < p || W < p) BDN_FAIL(BDN_E_SHAPE, "argmax_stitch: bad shape");
    hipLaunchKernelGGL(argmax_stitch_kernel, dim3(grid_for((size_t)n_tiles * p * p)), dim3(256), 0, (hipStream_t)stream,
                       logits, origins, mask, n_tiles, ncls, p, H, W, (size_t)p * p);
    BDN_CHECK_LAUNCH("argmax_stitch");
    return BDN_OK;
}

// ============================================================ sample_patches: training patch pairs cut from HBM-resident cities
// reference: utils/dataloaders.py:148-165 (onera_siamese_loader: crop + rot90 + two flips, per item) and the DataLoader's
// default_collate, for a whole batch.  One descriptor (city, row, col, sym) per sample; sym = 4 t + 2 rr + rc is the dihedral
// element of fabric_amd.utils.dataloaders._apply_symmetry: transpose if t, then reverse the rows if rr, then the columns if rc.
// With W the S x S window at (row, col):  out[i][j] = t ? W[cj][ri] : W[ri][cj],  ri = rr ? S-1-i : i,  cj = rc ? S-1-j : j.
// Pure data movement: floats travel as 32-bit patterns (NaN payloads, -0.0 and inf arrive unchanged), there is no arithmetic.
// A block copies one 64 x 64 output tile of one plane.  Lane x walks an output row, so every store is one contiguous row segment per
// wave.  Without transpose the load is also one row segment (descending under rc).  With transpose the tile is first loaded along
// source rows into LDS and then read down an LDS column: a row pitch of 65 dwords puts the 64 lanes of a column read (and of a row
// write) on distinct banks of their 32-lane groups.  Source rows start at arbitrary columns and S need not be a multiple of 4, so
// the accesses are dwords (bytes for labels): 64 lanes x 4 B = 256 B per wave instruction, 16 independent loads per thread in flight.
// SampleCity, SP_TILE, SP_WAVES, SP_ROWS: patch_core.hpp (shared with mix.hip).
template <bool LABELS>
__global__ __launch_bounds__(SP_TILE * SP_WAVES) void sample_patches_kernel(const SampleCity* __restrict__ cities, const int4* __restrict__ desc,
                                                                            int C, int S, int tiles, uint32_t* __restrict__ o1,
                                                                            uint32_t* __restrict__ o2, uint8_t* __restrict__ ol) {
    using T = typename std::conditional<LABELS, uint8_t, uint32_t>::type;
    __shared__ uint32_t lds[SP_TILE][SP_TILE + 1];
    const int planes = LABELS ? 1 : 2 * C;
    int b = blockIdx.x;
    const int tt = b % (tiles * tiles); b /= tiles * tiles;
    const int p = b % planes, s = b / planes;
    const int4 d = desc[s];                                  // (city, row, col, sym), validated on the host
    const SampleCity ct = cities[d.x];
    const int t = d.w >> 2, rr = (d.w >> 1) & 1, rc = d.w & 1;
    const int i0 = (tt / tiles) * SP_TILE, j0 = (tt % tiles) * SP_TILE;
    const int ni = min(SP_TILE, S - i0), nj = min(SP_TILE, S - j0);
    const size_t W = (size_t)ct.W, SS = (size_t)S * S;
    const T* src;
    T* dst;
    if (LABELS) {
        src = reinterpret_cast<const T*>(ct.labels);
        dst = reinterpret_cast<T*>(ol + s * SS);
    } else {
        const int date = p >= C, c = p - date * C;
        src = reinterpret_cast<const T*>(ct.images) + (size_t)p * ct.H * W;      // images [2][C][H][W]: plane p = date * C + c
        dst = reinterpret_cast<T*>((date ? o2 : o1) + ((size_t)s * C + c) * SS);
    }
    src += (size_t)d.y * W + d.z;                            // window origin
    const int x = threadIdx.x, y = threadIdx.y;
    T v[SP_ROWS];
    if (!t) {
        const int j = j0 + x, cj = rc ? S - 1 - j : j;
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) {
            const int i = i0 + y + k * SP_WAVES, ri = rr ? S - 1 - i : i;
            if (x < nj && i < i0 + ni) v[k] = src[(size_t)ri * W + cj];
        }
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) {
            const int i = i0 + y + k * SP_WAVES;
            if (x < nj && i < i0 + ni) dst[(size_t)i * S + j] = v[k];
        }
        return;
    }
    // transposed: output rows i take source columns ri, output columns j take source rows cj.  The source block is rows
    // [a0, a0 + nj) x columns [b0, b0 + ni) of the window; lds[a - a0][b - b0] holds W[a][b].
    const int a0 = rc ? S - j0 - nj : j0, b0 = rr ? S - i0 - ni : i0;
#pragma unroll
    for (int k = 0; k < SP_ROWS; k++) {
        const int a = y + k * SP_WAVES;
        if (x < ni && a < nj) v[k] = src[(size_t)(a0 + a) * W + b0 + x];
    }
#pragma unroll
    for (int k = 0; k < SP_ROWS; k++) {
        const int a = y + k * SP_WAVES;
        if (x < ni && a < nj) lds[a][x] = (uint32_t)v[k];
    }
    __syncthreads();
    const int jj = x, aa = rc ? nj - 1 - jj : jj;            // a - a0 of output column j0 + jj
#pragma unroll
    for (int k = 0; k < SP_ROWS; k++) {
        const int ii = y + k * SP_WAVES, bb = rr ? ni - 1 - ii : ii;
        if (jj < nj && ii < ni) dst[(size_t)(i0 + ii) * S + j0 + jj] = (T)lds[aa][bb];
    }
}

// The argument checks of bdn_sample_patches and bdn_sample_patches_aug (`who` names the entry in the message); *img_blocks: the image grid.
static int sample_patches_check(const char* who, const void* cities_dev, const int32_t* city_hw_host, int n_cities, int C,
                                const int32_t* desc_host, const int32_t* desc_dev, int n, int S,
                                const float* out_d1, const float* out_d2, const uint8_t* out_labels, long long* img_blocks) {
    if (!cities_dev || !city_hw_host || !desc_host || !desc_dev || !out_d1 || !out_d2 || !out_labels)
        BDN_FAIL(BDN_E_ARG, "%s: null pointer", who);
    if ((uintptr_t)desc_dev % 16 || (uintptr_t)cities_dev % 8) BDN_FAIL(BDN_E_ARG, "%s: desc_dev must be 16-byte and cities_dev 8-byte aligned", who);
    if (n <= 0 || S <= 0 || C <= 0 || n_cities <= 0)
        BDN_FAIL(BDN_E_SHAPE, "%s: need n, S, C, n_cities > 0 (got n=%d S=%d C=%d n_cities=%d)", who, n, S, C, n_cities);
    const int rd = patch_desc_check(who, city_hw_host, n_cities, desc_host, n, S);
    if (rd != BDN_OK) return rd;
    const long long tiles = (S + SP_TILE - 1) / SP_TILE;
    *img_blocks = (long long)n * 2 * C * tiles * tiles;
    if (*img_blocks > INT_MAX) BDN_FAIL(BDN_E_SHAPE, "%s: %lld blocks exceed the grid", who, *img_blocks);
    return BDN_OK;
}

extern "C" int bdn_sample_patches(const void* cities_dev, const int32_t* city_hw_host, int n_cities, int C,
                                  const int32_t* desc_host, const int32_t* desc_dev, int n, int S,
                                  float* out_d1, float* out_d2, uint8_t* out_labels, void* stream) {
    long long img_blocks = 0;
    const int rc = sample_patches_check("sample_patches", cities_dev, city_hw_host, n_cities, C, desc_host, desc_dev, n, S,
                                        out_d1, out_d2, out_labels, &img_blocks);
    if (rc != BDN_OK) return rc;
    const long long tiles = (S + SP_TILE - 1) / SP_TILE;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(SP_TILE, SP_WAVES);
    hipLaunchKernelGGL(sample_patches_kernel<false>, dim3((unsigned)img_blocks), block, 0, st, (const SampleCity*)cities_dev,
                       (const int4*)desc_dev, C, S, (int)tiles, (uint32_t*)out_d1, (uint32_t*)out_d2, out_labels);
    BDN_CHECK_LAUNCH("sample_patches");
    hipLaunchKernelGGL(sample_patches_kernel<true>, dim3((unsigned)(n * tiles * tiles)), block, 0, st, (const SampleCity*)cities_dev,
                       (const int4*)desc_dev, C, S, (int)tiles, (uint32_t*)out_d1, (uint32_t*)out_d2, out_labels);
    BDN_CHECK_LAUNCH("sample_patches (labels)");
    return BDN_OK;
}

// ============================================================ sample_patches_aug: the same cut, augmented on the way through the registers
// No reference: the reference's loader stops at the eight symmetries (utils/dataloaders.py:148-165).  Every draw of a sample comes from
// Philox4x32-10 (philox_core.hpp) keyed by (seed, sample key = epoch << 32 | dataset index), so a sample looks the same in any batch, on
// any rank and after a resume.  Stages, in order: crop at the jittered and clamped origin, symmetry, per-date per-band gain / bias,
// Gaussian noise, erase.  sample_patches_kernel's structure is kept: one 64 x 64 output tile of one plane per block, lane x walks an
// output row, dword (byte) accesses, the 64 x 65 LDS tile for the transposing symmetries, labels in a second launch; both paths end with
// the tile in registers in OUTPUT coordinates (row i0 + y + 4 k, column j0 + x), where the value stages run before the store.  What is
// loaded and stored does not change.
//   geometry, gain / bias: the sample key, the descriptor and the policy are block-uniform, so these Philox calls run on the scalar
//     unit, once per wave, never per element.
//   noise: one Philox call serves the four output columns 4 q .. 4 q + 3 of one row.  The four lanes of a quad share q; lane m of the quad
//     makes the calls of the rows k = 4 kk + m (4 of the thread's 16) and both Box-Muller pairs of each, and the quad exchanges the
//     4 x 4 values by DPP quad broadcasts (full-rate moves, no LDS, no barrier).  Every lane of the block takes part, also one whose
//     element lies outside a ragged tile: its quad may need its call.
// A disabled stage is compiled out (RADIO, NOISE) or skipped on a block-uniform branch (erase): with every value stage off the tile
// travels as 32-bit patterns, as in sample_patches_kernel.  Labels are never arithmetic.
struct AugPolicy {
    uint64_t seed;
    int J, flags, lo, hi, erase_label;
    float gain, bias, sigma, erase_p;
    uint32_t fill_bits;
};
constexpr int AUG_SYMMETRY = 1, AUG_PER_DATE = 2;

// One rounding per operation: the products and sums below must not be contracted into fused multiply-adds, or numpy float32 could not
// reproduce the bits.  (__fmul_rn / __fadd_rn are plain `*` and `+` in this toolchain's headers and inherit the caller's contraction.)
__device__ __forceinline__ float aug_fmul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float aug_fadd(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float aug_u(uint32_t w) { return (float)philox_u24(w) * 0x1p-24f; }      // exact: 24 bits, a power of two

template <int L> __device__ __forceinline__ float quad_bcast(float v) {          // the value of lane L of this lane's quad
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), L * 0x55, 0xf, 0xf, false));
}
template <int L> __device__ __forceinline__ float quad_pick(const float (&z)[4], int m) {      // z[m] of lane L of the quad
    const float a = quad_bcast<L>(z[0]), b = quad_bcast<L>(z[1]), c = quad_bcast<L>(z[2]), d = quad_bcast<L>(z[3]);
    const float lo = (m & 1) ? b : a, hi = (m & 1) ? d : c;
    return (m & 2) ? hi : lo;
}

// The value stages of one tile, shared by sample_patches_aug_kernel and sample_patches_warp_kernel: gain / bias, noise, erase, in this
// order, on v[k] = out[i0 + y + 4 k][j0 + x] (x = threadIdx.x, y = threadIdx.y).  p = date * C + c is the plane, s the sample; `first`
// marks the one thread of a plane that exports (g, b).
template <bool LABELS, bool RADIO, bool NOISE, typename T>
__device__ __forceinline__ void aug_value_stages(T (&v)[SP_ROWS], const AugPolicy& pol, uint64_t key, const PhiloxGeom& g, bool erased,
                                                 int C, int S, int planes, int s, int p, int date, int c, int i0, int j0, bool first,
                                                 float* __restrict__ drawn_radio) {
    const int x = threadIdx.x, y = threadIdx.y;
    const int j = j0 + x;
    if (!LABELS && RADIO) {                                   // stream 1: g, b of this plane, block-uniform
        const Philox4 w = philox_draw(pol.seed, key, PHILOX_RADIOMETRY, (uint32_t)(((pol.flags & AUG_PER_DATE) ? date * C : 0) + c));
        const float ta = aug_fadd(aug_fmul(2.f, aug_u(w.w[0])), -1.f), tb = aug_fadd(aug_fmul(2.f, aug_u(w.w[1])), -1.f);
        const float gg = aug_fadd(1.f, aug_fmul(pol.gain, ta)), bb = aug_fmul(pol.bias, tb);
        if (drawn_radio && first) { drawn_radio[2 * ((size_t)s * planes + p)] = gg; drawn_radio[2 * ((size_t)s * planes + p) + 1] = bb; }
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) v[k] = (T)__float_as_uint(aug_fadd(aug_fmul(gg, __uint_as_float((uint32_t)v[k])), bb));
    } else if (!LABELS) {
        if (drawn_radio && first) { drawn_radio[2 * ((size_t)s * planes + p)] = 1.f; drawn_radio[2 * ((size_t)s * planes + p) + 1] = 0.f; }
    }
    if (!LABELS && NOISE) {                                   // stream 2 + p, slot i * ceil(S / 4) + (j >> 2): every lane, no bounds test
        const int m = x & 3;
        const uint32_t q = (uint32_t)j >> 2, G = (uint32_t)(S + 3) >> 2;
#pragma unroll
        for (int kk = 0; kk < SP_ROWS / 4; kk++) {
            const uint32_t i = (uint32_t)(i0 + y + (4 * kk + m) * SP_WAVES);
            const Philox4 w = philox_draw(pol.seed, key, PHILOX_NOISE + (uint32_t)p, i * G + q);
            float z[4];
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const float u1 = (float)(philox_u24(w.w[2 * h]) + 1u) * 0x1p-24f, u2 = aug_u(w.w[2 * h + 1]);      // (0, 1] and [0, 1)
                const float r = sqrtf(-2.f * logf(u1));
                float sn, cs;
                sincospif(2.f * u2, &sn, &cs);               // sin, cos of 2 pi u2: the argument 2 u2 is exact
                z[2 * h] = aug_fmul(r, cs);
                z[2 * h + 1] = aug_fmul(r, sn);
            }
            const float z0 = quad_pick<0>(z, m), z1 = quad_pick<1>(z, m), z2 = quad_pick<2>(z, m), z3 = quad_pick<3>(z, m);
            v[4 * kk + 0] = (T)__float_as_uint(aug_fadd(__uint_as_float((uint32_t)v[4 * kk + 0]), aug_fmul(pol.sigma, z0)));
            v[4 * kk + 1] = (T)__float_as_uint(aug_fadd(__uint_as_float((uint32_t)v[4 * kk + 1]), aug_fmul(pol.sigma, z1)));
            v[4 * kk + 2] = (T)__float_as_uint(aug_fadd(__uint_as_float((uint32_t)v[4 * kk + 2]), aug_fmul(pol.sigma, z2)));
            v[4 * kk + 3] = (T)__float_as_uint(aug_fadd(__uint_as_float((uint32_t)v[4 * kk + 3]), aug_fmul(pol.sigma, z3)));
        }
    }
    if (erased && (!LABELS || pol.erase_label >= 0)) {        // block-uniform: the rectangle [top, top + eh) x [left, left + ew) of the output
        const T fill = LABELS ? (T)pol.erase_label : (T)pol.fill_bits;
        const bool in_cols = j >= g.left && j < g.left + g.ew;
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) {
            const int i = i0 + y + k * SP_WAVES;
            if (in_cols && i >= g.top && i < g.top + g.eh) v[k] = fill;
        }
    }
}

template <bool LABELS, bool RADIO, bool NOISE>
__global__ __launch_bounds__(SP_TILE * SP_WAVES) void sample_patches_aug_kernel(const SampleCity* __restrict__ cities, const int4* __restrict__ desc,
                                                                                const uint64_t* __restrict__ keys, const AugPolicy pol,
                                                                                int C, int S, int tiles, uint32_t* __restrict__ o1,
                                                                                uint32_t* __restrict__ o2, uint8_t* __restrict__ ol,
                                                                                int32_t* __restrict__ drawn_geom, float* __restrict__ drawn_radio) {
    using T = typename std::conditional<LABELS, uint8_t, uint32_t>::type;
    __shared__ uint32_t lds[SP_TILE][SP_TILE + 1];
    const int planes = LABELS ? 1 : 2 * C;
    int b = blockIdx.x;
    const int tt = b % (tiles * tiles); b /= tiles * tiles;
    const int p = b % planes, s = b / planes;
    const int4 d = desc[s];                                  // (city, row, col, sym), validated on the host
    const SampleCity ct = cities[d.x];
    const uint64_t key = keys[s];
    const bool erase_on = pol.erase_p > 0.f;
    const PhiloxGeom g = philox_geometry(pol.seed, key, d.y, d.z, d.w, ct.H, ct.W, S, pol.J, (pol.flags & AUG_SYMMETRY) != 0, erase_on,
                                         pol.lo, pol.hi);    // row, col clamped into the city here: in range for any draw
    const bool erased = erase_on && (float)g.erase_u24 * 0x1p-24f < pol.erase_p;
    const int t = g.sym >> 2, rr = (g.sym >> 1) & 1, rc = g.sym & 1;
    const int i0 = (tt / tiles) * SP_TILE, j0 = (tt % tiles) * SP_TILE;
    const int ni = min(SP_TILE, S - i0), nj = min(SP_TILE, S - j0);
    const size_t W = (size_t)ct.W, SS = (size_t)S * S;
    const int date = p >= C, c = p - date * C;
    const bool first = tt == 0 && threadIdx.x == 0 && threadIdx.y == 0;
    const T* src;
    T* dst;
    if (LABELS) {
        src = reinterpret_cast<const T*>(ct.labels);
        dst = reinterpret_cast<T*>(ol + s * SS);
    } else {
        src = reinterpret_cast<const T*>(ct.images) + (size_t)p * ct.H * W;      // images [2][C][H][W]: plane p = date * C + c
        dst = reinterpret_cast<T*>((date ? o2 : o1) + ((size_t)s * C + c) * SS);
        if (drawn_geom && first && p == 0) {
            int32_t* e = drawn_geom + 8 * (size_t)s;
            e[0] = g.row; e[1] = g.col; e[2] = g.sym; e[3] = erased; e[4] = g.top; e[5] = g.left; e[6] = g.eh; e[7] = g.ew;
        }
    }
    src += (size_t)g.row * W + g.col;                        // window origin
    const int x = threadIdx.x, y = threadIdx.y;
    const int j = j0 + x;
    T v[SP_ROWS];
#pragma unroll
    for (int k = 0; k < SP_ROWS; k++) v[k] = 0;
    if (!t) {
        const int cj = rc ? S - 1 - j : j;
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) {
            const int i = i0 + y + k * SP_WAVES, ri = rr ? S - 1 - i : i;
            if (x < nj && i < i0 + ni) v[k] = src[(size_t)ri * W + cj];
        }
    } else {
        // transposed: output rows i take source columns ri, output columns j take source rows cj.  The source block is rows
        // [a0, a0 + nj) x columns [b0, b0 + ni) of the window; lds[a - a0][b - b0] holds W[a][b].
        const int a0 = rc ? S - j0 - nj : j0, b0 = rr ? S - i0 - ni : i0;
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) {
            const int a = y + k * SP_WAVES;
            if (x < ni && a < nj) v[k] = src[(size_t)(a0 + a) * W + b0 + x];
        }
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) {
            const int a = y + k * SP_WAVES;
            if (x < ni && a < nj) lds[a][x] = (uint32_t)v[k];
        }
        __syncthreads();
        const int aa = rc ? nj - 1 - x : x;                  // a - a0 of output column j0 + x
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++) {
            const int ii = y + k * SP_WAVES, bb = rr ? ni - 1 - ii : ii;
            if (x < nj && ii < ni) v[k] = (T)lds[aa][bb];
        }
    }
    // ---- the tile is in registers in output coordinates: v[k] = out[i0 + y + 4 k][j0 + x]
    aug_value_stages<LABELS, RADIO, NOISE>(v, pol, key, g, erased, C, S, planes, s, p, date, c, i0, j0, first, drawn_radio);
#pragma unroll
    for (int k = 0; k < SP_ROWS; k++) {
        const int i = i0 + y + k * SP_WAVES;
        if (x < nj && i < i0 + ni) dst[(size_t)i * S + j] = v[k];
    }
}

// The policy checks of bdn_sample_patches_aug and bdn_sample_patches_warp (`who` names the entry in the message); fills *pol.
static int aug_policy_check(const char* who, const uint64_t* keys_dev, uint64_t seed, int J, int flags, float gain, float bias, float sigma,
                            float erase_p, int lo, int hi, int erase_label, float erase_fill, const int32_t* drawn_geom,
                            const float* drawn_radio, int C, int S, AugPolicy* pol) {
    if (!keys_dev) BDN_FAIL(BDN_E_ARG, "%s: null pointer", who);
    if ((uintptr_t)keys_dev % 8) BDN_FAIL(BDN_E_ARG, "%s: keys_dev must be 8-byte aligned", who);
    if ((uintptr_t)drawn_geom % 4 || (uintptr_t)drawn_radio % 4) BDN_FAIL(BDN_E_ARG, "%s: drawn_geom and drawn_radio must be 4-byte aligned", who);
    if (J < 0 || J > (1 << 24)) BDN_FAIL(BDN_E_ARG, "%s: jitter J=%d outside [0, 2^24]", who, J);
    if (flags & ~(AUG_SYMMETRY | AUG_PER_DATE)) BDN_FAIL(BDN_E_ARG, "%s: unknown flags %#x", who, flags);
    if (!std::isfinite(gain) || !std::isfinite(bias) || !std::isfinite(erase_fill))
        BDN_FAIL(BDN_E_ARG, "%s: gain, bias and erase_fill must be finite (got %g, %g, %g)", who, gain, bias, erase_fill);
    if (!(sigma >= 0.f) || !std::isfinite(sigma)) BDN_FAIL(BDN_E_ARG, "%s: need a finite sigma >= 0 (got %g)", who, sigma);
    if (!(erase_p >= 0.f && erase_p <= 1.f)) BDN_FAIL(BDN_E_ARG, "%s: erase_p %g outside [0, 1]", who, erase_p);
    if (erase_p > 0.f && !(1 <= lo && lo <= hi && hi <= S))
        BDN_FAIL(BDN_E_ARG, "%s: erase size needs 1 <= lo <= hi <= S (got lo=%d hi=%d S=%d)", who, lo, hi, S);
    if (erase_label < -1 || erase_label > 255) BDN_FAIL(BDN_E_ARG, "%s: erase_label %d outside -1..255", who, erase_label);
    if (sigma > 0.f && S > 65536) BDN_FAIL(BDN_E_SHAPE, "%s: noise slots are 32 bits: S=%d above 65536", who, S);
    if (sigma > 0.f && 2LL * C + PHILOX_NOISE > UINT32_MAX) BDN_FAIL(BDN_E_SHAPE, "%s: too many planes", who);
    pol->seed = seed; pol->J = J; pol->flags = flags; pol->lo = lo; pol->hi = hi; pol->erase_label = erase_label;
    pol->gain = gain; pol->bias = bias; pol->sigma = sigma; pol->erase_p = erase_p;
    memcpy(&pol->fill_bits, &erase_fill, 4);
    return BDN_OK;
}

extern "C" int bdn_sample_patches_aug(const void* cities_dev, const int32_t* city_hw_host, int n_cities, int C,
                                      const int32_t* desc_host, const int32_t* desc_dev, int n, int S,
                                      float* out_d1, float* out_d2, uint8_t* out_labels, const uint64_t* keys_dev,
                                      uint64_t seed, int J, int flags, float gain, float bias, float sigma, float erase_p,
                                      int lo, int hi, int erase_label, float erase_fill,
                                      int32_t* drawn_geom, float* drawn_radio, void* stream) {
    long long img_blocks = 0;
    const int rc = sample_patches_check("sample_patches_aug", cities_dev, city_hw_host, n_cities, C, desc_host, desc_dev, n, S,
                                        out_d1, out_d2, out_labels, &img_blocks);
    if (rc != BDN_OK) return rc;
    AugPolicy pol;
    const int rp = aug_policy_check("sample_patches_aug", keys_dev, seed, J, flags, gain, bias, sigma, erase_p, lo, hi, erase_label, erase_fill,
                                    drawn_geom, drawn_radio, C, S, &pol);
    if (rp != BDN_OK) return rp;
    const int tiles = (S + SP_TILE - 1) / SP_TILE;
    const bool radio = gain != 0.f || bias != 0.f, noise = sigma > 0.f;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(SP_TILE, SP_WAVES), grid((unsigned)img_blocks);
#define AUG_LAUNCH(R, N) hipLaunchKernelGGL((sample_patches_aug_kernel<false, R, N>), grid, block, 0, st, (const SampleCity*)cities_dev, \
        (const int4*)desc_dev, keys_dev, pol, C, S, tiles, (uint32_t*)out_d1, (uint32_t*)out_d2, out_labels, drawn_geom, drawn_radio)
    if (radio && noise) AUG_LAUNCH(true, true);
    else if (radio) AUG_LAUNCH(true, false);
    else if (noise) AUG_LAUNCH(false, true);
    else AUG_LAUNCH(false, false);
#undef AUG_LAUNCH
    BDN_CHECK_LAUNCH("sample_patches_aug");
    hipLaunchKernelGGL((sample_patches_aug_kernel<true, false, false>), dim3((unsigned)(n * tiles * tiles)), block, 0, st,
                       (const SampleCity*)cities_dev, (const int4*)desc_dev, keys_dev, pol, C, S, tiles, (uint32_t*)out_d1,
                       (uint32_t*)out_d2, out_labels, drawn_geom, drawn_radio);
    BDN_CHECK_LAUNCH("sample_patches_aug (labels)");
    return BDN_OK;
}

// ============================================================ sample_patches_warp: the augmented cut through an affine map with bilinear taps
// Extends utils/dataloaders.py:148-165, as bdn_sample_patches_aug does: rotation by any angle, zoom, and a sub-pixel shift of date 2
// against date 1 (misregistration; the labels stay in date 1's frame).  None of these is a permutation of pixels, so the tile is
// gathered: four dword loads and one bilinear blend per image element, one byte load (nearest neighbour) per label.
//   record    float32 [2][6] per sample, per date (a_ii, a_ij, t_i, a_ji, a_jj, t_j).  Drawn from stream PHILOX_WARP slot 0 (w0 the angle, w1
//             the zoom, w2 / w3 date 2's shift) or given by the caller (warp_dev).  The key, the policy and the record are block-uniform:
//             the Philox call, cosf, sinf, exp2f and the two divisions run once per wave, never per element.  cosf / sinf / exp2f are not
//             reproducible bit for bit outside this toolchain, so the record is exported (warp_out) and compared under a tolerance.
//   mapping   EXACT given the record, one rounding per operation and no fused multiply-add: with (i', j') the window coordinate that the
//             symmetry gives output pixel (i, j), h = (S - 1) / 2, di = i' - h, dj = j' - h (exact),
//               y = ((a_ii di) + (a_ij dj)) + (h + t_i),   x = ((a_ji di) + (a_jj dj)) + (h + t_j)          relative to the window origin;
//             y0 = floor(y), fy = y - y0, taps at rows row + y0, + 1 and columns col + x0, + 1, each clamped into the city (replicate);
//             top = ((1 - fx) v00) + (fx v01), bot alike, out = ((1 - fy) top) + (fy bot).  Labels: floor(y + 0.5), floor(x + 0.5) of date
//             1's record, clamped the same way; where the unclamped index is outside the city the label becomes oob_label (if >= 0).
//   An identity record gives fx = fy = 0 and out = (1 v00) + (0 v01) ...: a finite input passes unchanged bit for bit, except that -0.0
//   may arrive as +0.0.  Non-finite inputs are NOT preserved through the interpolation (0 * inf is NaN; a NaN spreads to the elements
//   that tap it).  Labels are moved or overwritten, never computed.
// The structure is sample_patches_aug_kernel's: one 64 x 64 output tile of one plane per block, lane x walks an output row, the tile ends in
// registers in output coordinates and the value stages (aug_value_stages: one copy) run before the store; labels in a second launch.
// Plain global loads: the footprint of a rotated tile is at most about 92 x 92 source pixels of one plane, which the vector cache holds.
// 160 registers, three waves per SIMD (a cap at 128 spills).  The kernel is bound by instruction issue, not by the taps: an identity record
// (coalesced taps) costs what a rotation costs, and staging the footprint in LDS was measured SLOWER, so it is not built.
struct WarpPolicy { float rotate_rad, log2_lo, log2_hi, misreg; int oob_label; };
struct WarpRec { float a_ii, a_ij, t_i, a_ji, a_jj, t_j; };
constexpr float WARP_MAX_A = 8.f, WARP_MAX_T = 1048576.f, WARP_MAX_MISREG = 64.f, WARP_MAX_LOG2 = 3.f;
constexpr int WARP_MAX_S = 1 << 24;

__device__ __forceinline__ float aug_fdiv(float a, float b) {
#pragma clang fp contract(off)
    return a / b;
}
__device__ __forceinline__ float aug_sgn(uint32_t w) { return aug_fadd(aug_fmul(2.f, aug_u(w)), -1.f); }      // 2 u(w) - 1 in [-1, 1)

// both dates' records of sample s: the caller's (warp_dev) or the draw of (seed, key)
__device__ __forceinline__ void warp_records(const AugPolicy& pol, const WarpPolicy& wp, uint64_t key, const float* __restrict__ warp_dev,
                                             int s, WarpRec (&r)[2]) {
    if (warp_dev) {
        const float* e = warp_dev + 12 * (size_t)s;
#pragma unroll
        for (int d = 0; d < 2; d++) r[d] = WarpRec{e[6 * d], e[6 * d + 1], e[6 * d + 2], e[6 * d + 3], e[6 * d + 4], e[6 * d + 5]};
        return;
    }
    const Philox4 w = philox_draw(pol.seed, key, PHILOX_WARP, 0);
    const float theta = aug_fmul(aug_sgn(w.w[0]), wp.rotate_rad);
    const float zoom = exp2f(aug_fadd(wp.log2_lo, aug_fmul(aug_u(w.w[1]), aug_fadd(wp.log2_hi, -wp.log2_lo))));
    const float cs = aug_fdiv(cosf(theta), zoom), sn = aug_fdiv(sinf(theta), zoom);
    r[0] = WarpRec{cs, -sn, 0.f, sn, cs, 0.f};
    r[1] = WarpRec{cs, -sn, aug_fmul(wp.misreg, aug_sgn(w.w[2])), sn, cs, aug_fmul(wp.misreg, aug_sgn(w.w[3]))};
}

__device__ __forceinline__ int warp_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

template <bool LABELS, bool RADIO, bool NOISE>
__global__ __launch_bounds__(SP_TILE * SP_WAVES) void sample_patches_warp_kernel(const SampleCity* __restrict__ cities, const int4* __restrict__ desc,
                                                                                 const uint64_t* __restrict__ keys, const AugPolicy pol,
                                                                                 const WarpPolicy wp, const float* __restrict__ warp_dev,
                                                                                 int C, int S, int tiles, uint32_t* __restrict__ o1,
                                                                                 uint32_t* __restrict__ o2, uint8_t* __restrict__ ol,
                                                                                 int32_t* __restrict__ drawn_geom, float* __restrict__ drawn_radio,
                                                                                 float* __restrict__ warp_out) {
    using T = typename std::conditional<LABELS, uint8_t, uint32_t>::type;
    const int planes = LABELS ? 1 : 2 * C;
    int b = blockIdx.x;
    const int tt = b % (tiles * tiles); b /= tiles * tiles;
    const int p = b % planes, s = b / planes;
    const int4 d = desc[s];                                  // (city, row, col, sym), validated on the host
    const SampleCity ct = cities[d.x];
    const uint64_t key = keys[s];
    const bool erase_on = pol.erase_p > 0.f;
    const PhiloxGeom g = philox_geometry(pol.seed, key, d.y, d.z, d.w, ct.H, ct.W, S, pol.J, (pol.flags & AUG_SYMMETRY) != 0, erase_on,
                                         pol.lo, pol.hi);    // row, col clamped into the city here: in range for any draw
    const bool erased = erase_on && (float)g.erase_u24 * 0x1p-24f < pol.erase_p;
    const int t = g.sym >> 2, rr = (g.sym >> 1) & 1, rc = g.sym & 1;
    const int i0 = (tt / tiles) * SP_TILE, j0 = (tt % tiles) * SP_TILE;
    const int ni = min(SP_TILE, S - i0), nj = min(SP_TILE, S - j0);
    const ptrdiff_t W = (ptrdiff_t)ct.W;
    const size_t SS = (size_t)S * S;
    const int date = p >= C, c = p - date * C;
    const bool first = tt == 0 && threadIdx.x == 0 && threadIdx.y == 0;
    WarpRec recs[2];
    warp_records(pol, wp, key, warp_dev, s, recs);
    const T* src;
    T* dst;
    if (LABELS) {
        src = reinterpret_cast<const T*>(ct.labels);
        dst = reinterpret_cast<T*>(ol + s * SS);
    } else {
        src = reinterpret_cast<const T*>(ct.images) + (size_t)p * ct.H * W;      // images [2][C][H][W]: plane p = date * C + c
        dst = reinterpret_cast<T*>((date ? o2 : o1) + ((size_t)s * C + c) * SS);
        if (first && p == 0) {
            if (drawn_geom) {
                int32_t* e = drawn_geom + 8 * (size_t)s;
                e[0] = g.row; e[1] = g.col; e[2] = g.sym; e[3] = erased; e[4] = g.top; e[5] = g.left; e[6] = g.eh; e[7] = g.ew;
            }
            if (warp_out) {
                float* e = warp_out + 12 * (size_t)s;
#pragma unroll
                for (int k = 0; k < 2; k++) {
                    e[6 * k] = recs[k].a_ii; e[6 * k + 1] = recs[k].a_ij; e[6 * k + 2] = recs[k].t_i;
                    e[6 * k + 3] = recs[k].a_ji; e[6 * k + 4] = recs[k].a_jj; e[6 * k + 5] = recs[k].t_j;
                }
            }
        }
    }
    src += (ptrdiff_t)g.row * W + g.col;                     // window origin: taps are addressed relative to it, inside the bounds below
    const WarpRec r = recs[LABELS ? 0 : date];               // labels follow date 1
    // the city in window-relative coordinates: every tap row lies in [rlo, rhi], every tap column in [clo, chi], whatever the record
    const int rlo = -g.row, rhi = ct.H - 1 - g.row, clo = -g.col, chi = ct.W - 1 - g.col;
    const float h = (float)(S - 1) * 0.5f;                   // exact: S - 1 < 2^24
    const float oy = aug_fadd(h, r.t_i), ox = aug_fadd(h, r.t_j);
    const int x = threadIdx.x, y = threadIdx.y;
    const int j = j0 + x;
    // window-relative source coordinate of output pixel (i, j): (i', j') = t ? (cj, ri) : (ri, cj), then the affine map
    auto coord = [&](int i, int jj, float& yy, float& xx) {
        const float fri = aug_fadd((float)(rr ? S - 1 - i : i), -h), fcj = aug_fadd((float)(rc ? S - 1 - jj : jj), -h);      // exact
        const float di = t ? fcj : fri, dj = t ? fri : fcj;
        yy = aug_fadd(aug_fadd(aug_fmul(r.a_ii, di), aug_fmul(r.a_ij, dj)), oy);
        xx = aug_fadd(aug_fadd(aug_fmul(r.a_ji, di), aug_fmul(r.a_jj, dj)), ox);
    };
    const int jc = min(j, j0 + nj - 1);                       // a lane outside a ragged tile repeats the tile's last column / row: no bounds test
    T v[SP_ROWS];
#pragma unroll
    for (int k = 0; k < SP_ROWS; k++) {
        float yy, xx;
        coord(min(i0 + y + k * SP_WAVES, i0 + ni - 1), jc, yy, xx);
        if (LABELS) {
            const int iy = (int)floorf(aug_fadd(yy, 0.5f)), ix = (int)floorf(aug_fadd(xx, 0.5f));
            const bool inside = iy >= rlo && iy <= rhi && ix >= clo && ix <= chi;
            const T lab = src[(ptrdiff_t)warp_clamp(iy, rlo, rhi) * W + warp_clamp(ix, clo, chi)];
            v[k] = (!inside && wp.oob_label >= 0) ? (T)wp.oob_label : lab;
        } else {
            const float y0 = floorf(yy), x0 = floorf(xx);
            const float fy = aug_fadd(yy, -y0), fx = aug_fadd(xx, -x0);
            const int iy = (int)y0, ix = (int)x0;
            const int ya = warp_clamp(iy, rlo, rhi), yb = warp_clamp(iy + 1, rlo, rhi);
            const int ca = warp_clamp(ix, clo, chi), cb = warp_clamp(ix + 1, clo, chi);
            const ptrdiff_t ra = (ptrdiff_t)ya * W, rb = (ptrdiff_t)yb * W;
            const float v00 = __uint_as_float((uint32_t)src[ra + ca]), v01 = __uint_as_float((uint32_t)src[ra + cb]);
            const float v10 = __uint_as_float((uint32_t)src[rb + ca]), v11 = __uint_as_float((uint32_t)src[rb + cb]);
            const float gx = aug_fadd(1.f, -fx), gy = aug_fadd(1.f, -fy);
            const float top = aug_fadd(aug_fmul(gx, v00), aug_fmul(fx, v01)), bot = aug_fadd(aug_fmul(gx, v10), aug_fmul(fx, v11));
            v[k] = (T)__float_as_uint(aug_fadd(aug_fmul(gy, top), aug_fmul(fy, bot)));
        }
    }
    // ---- the tile is in registers in output coordinates: v[k] = out[i0 + y + 4 k][j0 + x]
    aug_value_stages<LABELS, RADIO, NOISE>(v, pol, key, g, erased, C, S, planes, s, p, date, c, i0, j0, first, drawn_radio);
#pragma unroll
    for (int k = 0; k < SP_ROWS; k++) {
        const int i = i0 + y + k * SP_WAVES;
        if (x < nj && i < i0 + ni) dst[(size_t)i * S + j] = v[k];
    }
}

extern "C" int bdn_sample_patches_warp(const void* cities_dev, const int32_t* city_hw_host, int n_cities, int C,
                                       const int32_t* desc_host, const int32_t* desc_dev, int n, int S,
                                       float* out_d1, float* out_d2, uint8_t* out_labels, const uint64_t* keys_dev,
                                       uint64_t seed, int J, int flags, float gain, float bias, float sigma, float erase_p,
                                       int lo, int hi, int erase_label, float erase_fill,
                                       int32_t* drawn_geom, float* drawn_radio,
                                       float rotate_rad, float log2_lo, float log2_hi, float misreg, int oob_label,
                                       const float* warp_host, const float* warp_dev, float* warp_out, void* stream) {
    static const char* who = "sample_patches_warp";
    long long img_blocks = 0;
    const int rc = sample_patches_check(who, cities_dev, city_hw_host, n_cities, C, desc_host, desc_dev, n, S, out_d1, out_d2, out_labels,
                                        &img_blocks);
    if (rc != BDN_OK) return rc;
    AugPolicy pol;
    const int rp = aug_policy_check(who, keys_dev, seed, J, flags, gain, bias, sigma, erase_p, lo, hi, erase_label, erase_fill, drawn_geom,
                                    drawn_radio, C, S, &pol);
    if (rp != BDN_OK) return rp;
    if (S > WARP_MAX_S) BDN_FAIL(BDN_E_SHAPE, "%s: S=%d above 2^24 (window coordinates are float32)", who, S);
    if (!(rotate_rad >= 0.f && rotate_rad <= (float)M_PI)) BDN_FAIL(BDN_E_ARG, "%s: rotate_rad %g outside [0, pi]", who, rotate_rad);
    if (!(log2_lo >= -WARP_MAX_LOG2 && log2_lo <= log2_hi && log2_hi <= WARP_MAX_LOG2))
        BDN_FAIL(BDN_E_ARG, "%s: scale needs -3 <= log2_lo <= log2_hi <= 3, a zoom in [1/8, 8] (got %g, %g)", who, log2_lo, log2_hi);
    if (!(misreg >= 0.f && misreg <= WARP_MAX_MISREG)) BDN_FAIL(BDN_E_ARG, "%s: misreg %g outside [0, 64]", who, misreg);
    if (oob_label < -1 || oob_label > 255) BDN_FAIL(BDN_E_ARG, "%s: oob_label %d outside -1..255", who, oob_label);
    if (!warp_host != !warp_dev) BDN_FAIL(BDN_E_ARG, "%s: warp_host and warp_dev go together (both null: the records are drawn)", who);
    if ((uintptr_t)warp_dev % 4 || (uintptr_t)warp_out % 4) BDN_FAIL(BDN_E_ARG, "%s: warp_dev and warp_out must be 4-byte aligned", who);
    // With |a| <= 8, |t| <= 2^20 and |di|, |dj| < S / 2 <= 2^23, |y| and |x| stay below 8 S + 2^20 + S < 2^28: every float -> int
    // conversion of the kernel is in range (drawn records: |a| <= 8 (1 + a few ulp), |t| <= 64).  No address depends on that bound: every
    // tap is clamped into the city in integers, so the kernel reads inside the planes for ANY record.
    for (size_t k = 0; warp_host && k < 12 * (size_t)n; k++) {
        const float e = warp_host[k], bound = (k % 3 == 2) ? WARP_MAX_T : WARP_MAX_A;
        if (!std::isfinite(e)) BDN_FAIL(BDN_E_ARG, "%s: warp record %zu: entry %zu is not finite", who, k / 12, k % 12);
        if (!(std::fabs(e) <= bound))
            BDN_FAIL(BDN_E_ARG, "%s: warp record %zu: entry %zu = %g outside [-%g, %g]", who, k / 12, k % 12, e, bound, bound);
    }
    WarpPolicy wp{rotate_rad, log2_lo, log2_hi, misreg, oob_label};
    const int tiles = (S + SP_TILE - 1) / SP_TILE;
    const bool radio = gain != 0.f || bias != 0.f, noise = sigma > 0.f;
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(SP_TILE, SP_WAVES), grid((unsigned)img_blocks);
#define WARP_LAUNCH(R, N) hipLaunchKernelGGL((sample_patches_warp_kernel<false, R, N>), grid, block, 0, st, (const SampleCity*)cities_dev, \
        (const int4*)desc_dev, keys_dev, pol, wp, warp_dev, C, S, tiles, (uint32_t*)out_d1, (uint32_t*)out_d2, out_labels, drawn_geom, \
        drawn_radio, warp_out)
    if (radio && noise) WARP_LAUNCH(true, true);
    else if (radio) WARP_LAUNCH(true, false);
    else if (noise) WARP_LAUNCH(false, true);
    else WARP_LAUNCH(false, false);
#undef WARP_LAUNCH
    BDN_CHECK_LAUNCH("sample_patches_warp");
    hipLaunchKernelGGL((sample_patches_warp_kernel<true, false, false>), dim3((unsigned)(n * tiles * tiles)), block, 0, st,
                       (const SampleCity*)cities_dev, (const int4*)desc_dev, keys_dev, pol, wp, warp_dev, C, S, tiles, (uint32_t*)out_d1,
                       (uint32_t*)out_d2, out_labels, drawn_geom, drawn_radio, warp_out);
    BDN_CHECK_LAUNCH("sample_patches_warp (labels)");
    return BDN_OK;
}
