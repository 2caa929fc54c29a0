// libbidate_hip: mixing ACROSS the samples of a device-cut batch (include/bidate_hip.h: bdn_mix_plan, bdn_mix_patches) and the per-window
// label counts that pick the donors (bdn_patch_label_counts).
// No reference: the reference's loader transforms one sample at a time (utils/dataloaders.py:148-165).  CutMix for segmentation (French
// et al., BMVC 2020) replaces a rectangle of the recipient by the same rectangle of a donor; copy-paste (Ghiasi et al., CVPR 2021)
// replaces the pixels of the donor's objects, here its changed regions, on BOTH dates and in the labels at once, so the seam is not change.
#include "common.hpp"
#include "patch_core.hpp"
#include "philox_core.hpp"
#include <climits>

constexpr int MIX_BOX = 0, MIX_OBJECT = 1;
constexpr int MIX_MAX_MARGIN = 16, MIX_SPAN = SP_TILE + 2 * MIX_MAX_MARGIN;      // the label tile with its halo: at most 96 x 96 bytes
constexpr int MIX_GROUPS = 4;                // blocks per (sample, tile): group g takes the planes g, g + 4, ... of the 2 C + 1 (labels last)
constexpr int MIX_MAX_S = 1 << 14;           // a plane of S x S floats stays below 2^32 bytes: offsets inside a plane are 32 bits

// ============================================================ mix_plan: the draws of a batch, on the host
extern "C" int bdn_mix_plan(uint64_t seed, const uint64_t* keys_host, int n, int S, float p, int mode, int lo, int hi,
                            const int32_t* pool_host, int n_pool, int32_t* plan_host) {
    if (!keys_host || !plan_host) BDN_FAIL(BDN_E_ARG, "mix_plan: null pointer");
    if ((uintptr_t)keys_host % 8 || (uintptr_t)plan_host % 4 || (uintptr_t)pool_host % 4)
        BDN_FAIL(BDN_E_ARG, "mix_plan: keys_host must be 8-byte, plan_host and pool_host 4-byte aligned");
    if (n <= 0 || S <= 0) BDN_FAIL(BDN_E_SHAPE, "mix_plan: need n, S > 0 (got n=%d S=%d)", n, S);
    if (!(p >= 0.f && p <= 1.f)) BDN_FAIL(BDN_E_ARG, "mix_plan: p %g outside [0, 1]", p);
    if (mode != MIX_BOX && mode != MIX_OBJECT) BDN_FAIL(BDN_E_ARG, "mix_plan: unknown mode %d (0: box, 1: object)", mode);
    if (!(1 <= lo && lo <= hi && hi <= S)) BDN_FAIL(BDN_E_ARG, "mix_plan: box size needs 1 <= lo <= hi <= S (got lo=%d hi=%d S=%d)", lo, hi, S);
    if (n_pool < 1) BDN_FAIL(BDN_E_ARG, "mix_plan: n_pool %d: the donor pool is empty", n_pool);
    int mixed = 0;
    for (int k = 0; k < n; k++) {
        int32_t* e = plan_host + 8 * (size_t)k;
        const PhiloxMix m = philox_mix(seed, keys_host[k], S, p, mode == MIX_BOX, lo, hi, (uint32_t)n_pool);
        e[0] = m.on;
        e[1] = m.on ? (pool_host ? pool_host[m.pick] : m.pick) : 0;
        e[2] = m.on ? n + mixed : -1;
        e[3] = m.top; e[4] = m.left; e[5] = m.h; e[6] = m.w; e[7] = 0;
        mixed += m.on;
    }
    return BDN_OK;
}

// ============================================================ mix_patches: the donor's pixels into the recipient wherever the mask is set
// sample_patches_kernel's tiling: a block works on one 64 x 64 output tile of one sample, thread (x, y) on column j0 + x of the rows
// i0 + y + 4 k, k = 0..15, so every store is one contiguous row segment per wave; dwords for the images, bytes for the labels (a row of S
// floats is not 16-byte aligned for general S).  The mask of the tile is formed ONCE per block, as 16 bits per thread, and then serves all
// of the block's planes: MIX_GROUPS blocks share the 2 C image planes and the label plane of a tile, so that a batch in which few samples
// are mixed still fills the device.  An unmixed sample's blocks return after reading their plan row, and so do the blocks of a tile whose
// mask is empty (most object tiles: change pixels are a few percent).
//   box     the rectangle of the plan row; no memory for the mask.
//   object  the donor's label tile with a halo of `margin` pixels is staged in LDS as (label == paste_label) bytes, zero outside the patch
//           (at most 96 x 96 of them); the (2 margin + 1) square dilation is separable: a maximum along rows into a second LDS array,
//           then along columns into the registers.
// The recipient is never read and is written only where the mask is set; donor rows are only read.  Recipient rows (< n) and donor rows
// (>= n) are disjoint and a recipient element is written by one thread of one block, so no two blocks race.  No atomics.
// Every load and every store of a plane sits under its own lane mask.  The compiler places the wait for a loaded value inside the masked
// region of the store that uses it, and must then repeat it before every later store (a wave that skipped the region has not waited),
// which also waits for the store before: sixteen stores in series.  One wait for all the loads, outside any region, lets the stores
// stream.  s_waitcnt vmcnt(0) with expcnt and lgkmcnt left alone: vmcnt in bits 3:0 and 15:14, expcnt 6:4, lgkmcnt 11:8.
#define MIX_LOADS_DONE() __builtin_amdgcn_s_waitcnt(0x0F70)

template <bool OBJECT>
__global__ __launch_bounds__(SP_TILE * SP_WAVES) void mix_patches_kernel(const int4* __restrict__ plan, int C, int S, int tiles, int paste_label,
                                                                         int margin, uint32_t* d1, uint32_t* d2, uint8_t* labels,
                                                                         uint8_t* __restrict__ mask_out) {
    constexpr int SPAN = OBJECT ? MIX_SPAN : 1;
    __shared__ uint8_t eq[SPAN][SPAN + 4];                   // (donor label == paste_label) of rows i0 - margin .., columns j0 - margin ..
    __shared__ uint8_t rowmax[SPAN][OBJECT ? SP_TILE : 1];   // its maximum over the columns x .. x + 2 margin
    const int s = blockIdx.x / (tiles * tiles), tt = blockIdx.x % (tiles * tiles), g = blockIdx.y;
    const int4 pa = plan[2 * s], pb = plan[2 * s + 1];       // (on, donor_index, donor_row, top), (left, h, w, 0): validated on the host
    const int i0 = (tt / tiles) * SP_TILE, j0 = (tt % tiles) * SP_TILE;
    const int ni = min(SP_TILE, S - i0), nj = min(SP_TILE, S - j0);
    const int x = threadIdx.x, y = threadIdx.y, j = j0 + x;
    const size_t SS = (size_t)S * S;
    const bool owns_mask = mask_out && g == (2 * C) % MIX_GROUPS;      // the group of the label plane also writes mask_out
    uint32_t valid = 0;                                      // bit k: element (i0 + y + 4 k, j) lies in the patch
#pragma unroll
    for (int k = 0; k < SP_ROWS; k++) valid |= (uint32_t)(x < nj && y + k * SP_WAVES < ni) << k;
    uint32_t bits = 0;                                       // bit k: the donor replaces element (i0 + y + 4 k, j)
    if (pa.x) {
        if (!OBJECT) {
            const int top = pa.w, left = pb.x, h = pb.y, w = pb.z;
            const bool in_cols = j >= left && j < left + w;
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++) {
                const int i = i0 + y + k * SP_WAVES;
                bits |= (uint32_t)(in_cols && i >= top && i < top + h) << k;
            }
        } else {
            const uint8_t* dl = labels + (size_t)pa.z * SS;
            const int span = SP_TILE + 2 * margin, tid = y * SP_TILE + x;
#pragma unroll 4
            for (int e = tid; e < span * span; e += SP_TILE * SP_WAVES) {      // no branch around the load: four of them are in flight
                const int r = e / span, c = e - r * span, gi = i0 - margin + r, gj = j0 - margin + c;
                const bool inside = gi >= 0 && gi < S && gj >= 0 && gj < S;
                const uint8_t lab = dl[(size_t)min(max(gi, 0), S - 1) * S + min(max(gj, 0), S - 1)];      // clamped into the patch
                eq[r][c] = inside & (lab == paste_label);
            }
            __syncthreads();
            for (int e = tid; e < span * SP_TILE; e += SP_TILE * SP_WAVES) {
                const int r = e / SP_TILE, c = e % SP_TILE;
                uint8_t v = 0;
                for (int d = 0; d <= 2 * margin; d++) v |= eq[r][c + d];
                rowmax[r][c] = v;
            }
            __syncthreads();
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++) {
                uint8_t v = 0;
                for (int d = 0; d <= 2 * margin; d++) v |= rowmax[y + k * SP_WAVES + d][x];
                bits |= (uint32_t)v << k;
            }
        }
        bits &= valid;
    }
    if (owns_mask) {
        uint8_t* mo = mask_out + (size_t)s * SS;
#pragma unroll
        for (int k = 0; k < SP_ROWS; k++)
            if (valid >> k & 1) mo[(size_t)(i0 + y + k * SP_WAVES) * S + j] = bits >> k & 1;
    }
    if (!__syncthreads_or(bits != 0)) return;                // unmixed, or nothing of this tile is taken: block-uniform
    const size_t donor = (size_t)pa.z;
    // An element's offset inside its plane fits 32 bits (S <= MIX_MAX_S, checked on the host) and is formed once; a plane's base is a
    // 64-bit scalar.  Each access is then base + a register of its own, so the 16 loads of a plane are in flight together.
    uint32_t off[SP_ROWS];
#pragma unroll
    for (int k = 0; k < SP_ROWS; k++) off[k] = (uint32_t)(i0 + y + k * SP_WAVES) * (uint32_t)S + (uint32_t)j;
    for (int u = g; u <= 2 * C; u += MIX_GROUPS) {           // plane u of the 2 C + 1: date 1's, then date 2's image planes, then the labels
        if (u < 2 * C) {
            const int date = u >= C, c = u - date * C;
            uint32_t* base = date ? d2 : d1;
            const uint32_t* src = base + (donor * C + c) * SS;
            uint32_t* dst = base + ((size_t)s * C + c) * SS;
            uint32_t v[SP_ROWS];
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++)
                if (bits >> k & 1) v[k] = src[off[k]];
            MIX_LOADS_DONE();
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++)
                if (bits >> k & 1) dst[off[k]] = v[k];
        } else {
            const uint8_t* src = labels + donor * SS;
            uint8_t* dst = labels + (size_t)s * SS;
            uint32_t v[SP_ROWS];                             // a register per byte: packed bytes would chain the loads through their register
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++)
                if (bits >> k & 1) v[k] = src[off[k]];
            MIX_LOADS_DONE();
#pragma unroll
            for (int k = 0; k < SP_ROWS; k++)
                if (bits >> k & 1) dst[off[k]] = (uint8_t)v[k];
        }
    }
}

extern "C" int bdn_mix_patches(const int32_t* plan_host, const int32_t* plan_dev, int n, int rows, int C, int S, int mode, int paste_label,
                               int margin, float* d1, float* d2, uint8_t* labels, uint8_t* mask_out, void* stream) {
    if (!plan_host || !plan_dev || !d1 || !d2 || !labels) BDN_FAIL(BDN_E_ARG, "mix_patches: null pointer");
    if ((uintptr_t)plan_host % 4 || (uintptr_t)plan_dev % 16 || (uintptr_t)d1 % 4 || (uintptr_t)d2 % 4)
        BDN_FAIL(BDN_E_ARG, "mix_patches: plan_dev must be 16-byte, plan_host, d1 and d2 4-byte aligned");
    if (n <= 0 || rows < n || C <= 0 || S <= 0)
        BDN_FAIL(BDN_E_SHAPE, "mix_patches: need n, C, S > 0 and rows >= n (got n=%d rows=%d C=%d S=%d)", n, rows, C, S);
    if (S > MIX_MAX_S) BDN_FAIL(BDN_E_SHAPE, "mix_patches: S=%d above 2^14 (offsets inside a plane are 32 bits)", S);
    if (mode != MIX_BOX && mode != MIX_OBJECT) BDN_FAIL(BDN_E_ARG, "mix_patches: unknown mode %d (0: box, 1: object)", mode);
    if (paste_label < 0 || paste_label > 255) BDN_FAIL(BDN_E_ARG, "mix_patches: paste_label %d outside 0..255", paste_label);
    if (margin < 0 || margin > MIX_MAX_MARGIN) BDN_FAIL(BDN_E_ARG, "mix_patches: margin %d outside 0..%d", margin, MIX_MAX_MARGIN);
    for (int k = 0; k < n; k++) {                            // every address the kernel forms comes from a plan row checked here
        const int32_t* e = plan_host + 8 * (size_t)k;
        const int on = e[0], donor_row = e[2], top = e[3], left = e[4], h = e[5], w = e[6];
        if (on != 0 && on != 1) BDN_FAIL(BDN_E_ARG, "mix_patches: plan row %d: on = %d is neither 0 nor 1", k, on);
        if (!on) continue;
        if (donor_row < n || donor_row >= rows) BDN_FAIL(BDN_E_ARG, "mix_patches: plan row %d: donor_row %d outside [%d, %d)", k, donor_row, n, rows);
        if (top < 0 || h < 1 || (long long)top + h > S || left < 0 || w < 1 || (long long)left + w > S)
            BDN_FAIL(BDN_E_ARG, "mix_patches: plan row %d: rectangle (top=%d left=%d h=%d w=%d) outside the %d x %d patch", k, top, left, h, w, S, S);
    }
    const long long tiles = (S + SP_TILE - 1) / SP_TILE, blocks = (long long)n * tiles * tiles;
    if (blocks > INT_MAX) BDN_FAIL(BDN_E_SHAPE, "mix_patches: %lld blocks exceed the grid", blocks);
    const dim3 grid((unsigned)blocks, MIX_GROUPS), block(SP_TILE, SP_WAVES);
    hipStream_t st = (hipStream_t)stream;
    if (mode == MIX_OBJECT)
        hipLaunchKernelGGL(mix_patches_kernel<true>, grid, block, 0, st, (const int4*)plan_dev, C, S, (int)tiles, paste_label, margin,
                           (uint32_t*)d1, (uint32_t*)d2, labels, mask_out);
    else
        hipLaunchKernelGGL(mix_patches_kernel<false>, grid, block, 0, st, (const int4*)plan_dev, C, S, (int)tiles, paste_label, margin,
                           (uint32_t*)d1, (uint32_t*)d2, labels, mask_out);
    BDN_CHECK_LAUNCH("mix_patches");
    return BDN_OK;
}

// ============================================================ patch_label_counts: how many label bytes of each window equal `value`
// One block per descriptor: every thread counts its share of the window (lane x walks a row), the waves sum by shuffles, the block
// through LDS.  Integer sums in a fixed order: the same bits every run.
__global__ __launch_bounds__(SP_TILE * SP_WAVES) void patch_label_counts_kernel(const SampleCity* __restrict__ cities, const int4* __restrict__ desc,
                                                                                int S, int value, int32_t* __restrict__ counts) {
    __shared__ int part[SP_WAVES];
    const int4 d = desc[blockIdx.x];                         // (city, row, col, sym), validated on the host
    const SampleCity ct = cities[d.x];
    const size_t W = (size_t)ct.W;
    const uint8_t* src = ct.labels + (size_t)d.y * W + d.z;
    int cnt = 0;
    for (int i = threadIdx.y; i < S; i += SP_WAVES)
        for (int j = threadIdx.x; j < S; j += SP_TILE) cnt += src[(size_t)i * W + j] == value;
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if (threadIdx.x == 0) part[threadIdx.y] = cnt;
    __syncthreads();
    if (threadIdx.x == 0 && threadIdx.y == 0) counts[blockIdx.x] = part[0] + part[1] + part[2] + part[3];
}

extern "C" int bdn_patch_label_counts(const void* cities_dev, const int32_t* city_hw_host, int n_cities, const int32_t* desc_host,
                                      const int32_t* desc_dev, int n, int S, int value, int32_t* counts_dev, void* stream) {
    static const char* who = "patch_label_counts";
    if (!cities_dev || !city_hw_host || !desc_host || !desc_dev || !counts_dev) BDN_FAIL(BDN_E_ARG, "%s: null pointer", who);
    if ((uintptr_t)desc_dev % 16 || (uintptr_t)cities_dev % 8 || (uintptr_t)counts_dev % 4)
        BDN_FAIL(BDN_E_ARG, "%s: desc_dev must be 16-byte, cities_dev 8-byte and counts_dev 4-byte aligned", who);
    if (n <= 0 || S <= 0 || n_cities <= 0) BDN_FAIL(BDN_E_SHAPE, "%s: need n, S, n_cities > 0 (got n=%d S=%d n_cities=%d)", who, n, S, n_cities);
    if (S > 46340) BDN_FAIL(BDN_E_SHAPE, "%s: S=%d: a count above 2^31 - 1 does not fit int32", who, S);
    if (value < 0 || value > 255) BDN_FAIL(BDN_E_ARG, "%s: value %d outside 0..255", who, value);
    const int rd = patch_desc_check(who, city_hw_host, n_cities, desc_host, n, S);
    if (rd != BDN_OK) return rd;
    hipLaunchKernelGGL(patch_label_counts_kernel, dim3((unsigned)n), dim3(SP_TILE, SP_WAVES), 0, (hipStream_t)stream,
                       (const SampleCity*)cities_dev, (const int4*)desc_dev, S, value, counts_dev);
    BDN_CHECK_LAUNCH(who);
    return BDN_OK;
}
