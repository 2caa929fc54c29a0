// libbidate_hip: full-scene sliding-window inference helpers.
// The two dates of a scene stay resident in HBM as band planes; tiles are gathered straight into the packed
// NHWC batch and predictions are written straight into the scene mask -- no host-side patch stack.
#include "common.hpp"
#include <climits>
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
struct SampleCity { const float* images; const uint8_t* labels; int32_t H, W; };       // bdn_sample_patches' city record, 24 bytes

constexpr int SP_TILE = 64, SP_WAVES = 4, SP_ROWS = SP_TILE / SP_WAVES;

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

extern "C" int bdn_sample_patches(const void* cities_dev, const int32_t* city_hw_host, int n_cities, int C,
                                  const int32_t* desc_host, const int32_t* desc_dev, int n, int S,
                                  float* out_d1, float* out_d2, uint8_t* out_labels, void* stream) {
    if (!cities_dev || !city_hw_host || !desc_host || !desc_dev || !out_d1 || !out_d2 || !out_labels)
        BDN_FAIL(BDN_E_ARG, "sample_patches: null pointer");
    if ((uintptr_t)desc_dev % 16 || (uintptr_t)cities_dev % 8) BDN_FAIL(BDN_E_ARG, "sample_patches: desc_dev must be 16-byte and cities_dev 8-byte aligned");
    if (n <= 0 || S <= 0 || C <= 0 || n_cities <= 0)
        BDN_FAIL(BDN_E_SHAPE, "sample_patches: need n, S, C, n_cities > 0 (got n=%d S=%d C=%d n_cities=%d)", n, S, C, n_cities);
    for (int k = 0; k < n_cities; k++)
        if (city_hw_host[2 * k] <= 0 || city_hw_host[2 * k + 1] <= 0)
            BDN_FAIL(BDN_E_SHAPE, "sample_patches: city %d has shape %d x %d", k, city_hw_host[2 * k], city_hw_host[2 * k + 1]);
    for (int k = 0; k < n; k++) {                            // every address the kernel forms comes from a descriptor checked here
        const int32_t* e = desc_host + 4 * (size_t)k;
        const int city = e[0], row = e[1], col = e[2], sym = e[3];
        if (city < 0 || city >= n_cities) BDN_FAIL(BDN_E_ARG, "sample_patches: descriptor %d: city %d outside [0, %d)", k, city, n_cities);
        if (sym < 0 || sym > 7) BDN_FAIL(BDN_E_ARG, "sample_patches: descriptor %d: sym %d outside [0, 8)", k, sym);
        const long long H = city_hw_host[2 * city], W = city_hw_host[2 * city + 1];
        if (row < 0 || (long long)row + S > H)
            BDN_FAIL(BDN_E_ARG, "sample_patches: descriptor %d: row %d + S %d outside H %lld of city %d", k, row, S, H, city);
        if (col < 0 || (long long)col + S > W)
            BDN_FAIL(BDN_E_ARG, "sample_patches: descriptor %d: col %d + S %d outside W %lld of city %d", k, col, S, W, city);
    }
    const long long tiles = (S + SP_TILE - 1) / SP_TILE, img_blocks = (long long)n * 2 * C * tiles * tiles;
    if (img_blocks > INT_MAX) BDN_FAIL(BDN_E_SHAPE, "sample_patches: %lld blocks exceed the grid", img_blocks);
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
