// libbidate_hip: full-scene change probabilities from blended overlapping tiles.
// Generalizes the reference's sliding-window scan (utils/inference.py:134-236, train.py:182-205: non-overlapping tiles, hard argmax,
// far-edge tiles pasted over the aligned ones) to tiles at any stride, a weighted blend of softmax probabilities and test-time
// averaging over the symmetries of the square.  Tile plan (fabric_amd.utils.inference.blend_tile_origins): ys[k] = min(k s, H - p)
// for k < ny, xs alike; tile g = ky nx + kx; forward image (g, k) = tile g under the k-th symmetry code, images in tile-major order.
// Every sum runs in a fixed order and there are no float atomics: the result is the same bits on every run, for one scan lane or two
// and for any split of the images into batches.
#include "common.hpp"
#include <climits>

constexpr int BL_TILE = 32, BL_ROWS = 8, BL_PER = BL_TILE / BL_ROWS;     // a block: one 32 x 32 pixel tile, 32 x 8 threads, 4 rows each
constexpr int BL_CLS = 8;                                                  // classes per LDS pass of the fold

// A window under symmetry sym = 4 t + 2 rr + rc (fabric_amd.utils.dataloaders._apply_symmetry; bdn_sample_patches' encoding):
//   out[i][j] = t ? W[cj][ri] : W[ri][cj],  ri = rr ? p-1-i : i,  cj = rc ? p-1-j : j.
// The output block rows [i0, i0 + ni) x columns [j0, j0 + nj) reads the source block rows [sa0, sa0 + na) x columns [sb0, sb0 + nb);
// src_of gives the source coordinates inside that block of output (ii, jj).
struct SymBlock {
    int t, rr, rc, ni, nj, na, nb, sa0, sb0;
    __device__ SymBlock(int sym, int p, int i0, int j0, int ni_, int nj_) : t(sym >> 2 & 1), rr(sym >> 1 & 1), rc(sym & 1), ni(ni_), nj(nj_) {
        na = t ? nj : ni; nb = t ? ni : nj;
        const int ra = rr ? p - i0 - ni : i0, cb = rc ? p - j0 - nj : j0;       // the rows / columns the output rows / columns come from
        sa0 = t ? cb : ra; sb0 = t ? ra : cb;
    }
    __device__ void src_of(int ii, int jj, int& a, int& b) const {
        const int ri = rr ? ni - 1 - ii : ii, cj = rc ? nj - 1 - jj : jj;
        a = t ? cj : ri; b = t ? ri : cj;
    }
};

// ============================================================ gather_tiles_sym
// reference: utils/inference.py:134-184 (_get_patches) + train.py:190-193, generalized: tile i of the batch is the p x p window at
// table[i] = (y0, x0, sym) of both dates under symmetry sym.  out: [2n][p][p][Cpad] T, date-1 tiles first (bdn_gather_tiles' layout).
// A block copies one 32 x 32 output tile of one 16-byte channel unit of one tile image.  The source block is loaded along its rows (one
// 128-byte row segment per plane and half-wave) into LDS, one [32][33] float plane per channel of the unit; the output is read back
// along output rows -- down an LDS column under the transposing symmetries, where the row pitch of 33 dwords keeps the 32 lanes of a
// half-wave on distinct banks -- and stored as 16-byte units.  Bits are moved (bf16: rounded exactly as bdn_gather_tiles rounds them).
template <typename T>
__global__ __launch_bounds__(BL_TILE * BL_ROWS) void gather_tiles_sym_kernel(const float* __restrict__ s1, const float* __restrict__ s2,
                                                                              const int* __restrict__ table, T* __restrict__ out,
                                                                              int n, int C, int H, int W, int p, int Cpad, int tb) {
    constexpr int EPU = ET<T>::EPU;
    __shared__ float lds[EPU][BL_TILE][BL_TILE + 1];
    const int upp = Cpad / EPU;
    int b = blockIdx.x;
    const int u = b % upp; b /= upp;
    const int tt = b % (tb * tb), img = b / (tb * tb);
    const int date = img >= n, ti = img - date * n;
    const int y0 = table[3 * ti], x0 = table[3 * ti + 1], sym = table[3 * ti + 2];
    const bool ok = sym >= 0 && sym < 8 && y0 >= 0 && x0 >= 0 && y0 <= H - p && x0 <= W - p;     // the host checks the table; a bad row reads nothing
    const int i0 = (tt / tb) * BL_TILE, j0 = (tt % tb) * BL_TILE;
    const SymBlock sb(sym, p, i0, j0, min(BL_TILE, p - i0), min(BL_TILE, p - j0));
    const size_t hw = (size_t)H * W;
    const float* src = (date ? s2 : s1) + (ok ? (size_t)(y0 + sb.sa0) * W + x0 + sb.sb0 : 0);
    const int x = threadIdx.x, y = threadIdx.y;
#pragma unroll
    for (int k = 0; k < BL_PER; k++) {
        const int a = y + k * BL_ROWS;
        if (x < sb.nb && a < sb.na) {
#pragma unroll
            for (int e = 0; e < EPU; e++) {
                const int c = u * EPU + e;
                lds[e][a][x] = ok && c < C ? src[(size_t)c * hw + (size_t)a * W + x] : 0.f;
            }
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BL_PER; k++) {
        const int ii = y + k * BL_ROWS, jj = x;
        if (ii < sb.ni && jj < sb.nj) {
            int a, bb;
            sb.src_of(ii, jj, a, bb);
            float f[EPU];
#pragma unroll
            for (int e = 0; e < EPU; e++) f[e] = lds[e][a][bb];
            T* dst = out + (((size_t)img * p + i0 + ii) * p + j0 + jj) * Cpad + u * EPU;
            *reinterpret_cast<uint4*>(dst) = Unit<T>::pack(f);
        }
    }
}

extern "C" int bdn_gather_tiles_sym(int dtype, const float* scene_d1, const float* scene_d2, const int32_t* table,
                                    void* out, int n_tiles, int C, int H, int W, int p, int Cpad, void* stream) {
    if (!scene_d1 || !scene_d2 || !table || !out) BDN_FAIL(BDN_E_ARG, "gather_tiles_sym: null pointer");
    if (n_tiles <= 0 || C <= 0 || p <= 0 || H < p || W < p || Cpad < C || Cpad % 16)
        BDN_FAIL(BDN_E_SHAPE, "gather_tiles_sym: need H,W >= p, Cpad a multiple of 16 and >= C");
    const int tb = (p + BL_TILE - 1) / BL_TILE;
    const int epu = dtype == BDN_BF16 ? 8 : 4;
    const long long blocks = 2LL * n_tiles * tb * tb * (Cpad / epu);
    if (blocks > INT_MAX) BDN_FAIL(BDN_E_SHAPE, "gather_tiles_sym: %lld blocks exceed the grid", blocks);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(BL_TILE, BL_ROWS);
    if (dtype == BDN_BF16)
        hipLaunchKernelGGL(gather_tiles_sym_kernel<bf16s>, dim3((unsigned)blocks), block, 0, st,
                           scene_d1, scene_d2, table, (bf16s*)out, n_tiles, C, H, W, p, Cpad, tb);
    else if (dtype == BDN_F32)
        hipLaunchKernelGGL(gather_tiles_sym_kernel<float>, dim3((unsigned)blocks), block, 0, st,
                           scene_d1, scene_d2, table, (float*)out, n_tiles, C, H, W, p, Cpad, tb);
    else BDN_FAIL(BDN_E_ARG, "gather_tiles_sym: bad dtype");
    BDN_CHECK_LAUNCH("gather_tiles_sym");
    return BDN_OK;
}

// ============================================================ blend_fold
// reference: train.py:199 (torch.max(preds, 1) over the logits), replaced by the weighted class probabilities of every forward image,
// mapped back into scene orientation: out[i][c][a][b] = window[a][b] * softmax(logits[i])[c] at the pixel of image i that shows scene
// pixel (a, b) of its window, i.e. the image under the inverse of its symmetry table[i][2].  softmax: m = max_c l_c, e_c = exp(l_c - m),
// s = sum_c e_c in class order, e_c / s.  Same block shape and LDS treatment as the gather (with the roles of source and output swapped):
// probabilities are formed along the logits' rows, written to LDS, read back along scene rows; BL_CLS classes per LDS pass.
__global__ __launch_bounds__(BL_TILE * BL_ROWS) void blend_fold_kernel(const float* __restrict__ logits, const int* __restrict__ table,
                                                                        const float* __restrict__ window, float* __restrict__ out,
                                                                        int ncls, int p, int tb) {
    __shared__ float lds[BL_CLS][BL_TILE][BL_TILE + 1];
    const int tt = blockIdx.x % (tb * tb), img = blockIdx.x / (tb * tb);
    const int sym = table[3 * img + 2] & 7;
    const int inv = sym & 4 ? 4 | (sym & 1) << 1 | (sym >> 1 & 1) : sym;     // (t, rr, rc) -> (t, rc, rr) when t: the others are involutions
    const int a0 = (tt / tb) * BL_TILE, b0 = (tt % tb) * BL_TILE;
    // scene orientation = the image under the inverse symmetry: scene pixel (a0 + aa, b0 + bb) is pixel (a, b) of the logits block that
    // SymBlock(inv) maps to output (aa, bb)
    const SymBlock sb(inv, p, a0, b0, min(BL_TILE, p - a0), min(BL_TILE, p - b0));
    const size_t pp = (size_t)p * p;
    const float* L = logits + (size_t)img * ncls * pp + (size_t)sb.sa0 * p + sb.sb0;
    float* O = out + (size_t)img * ncls * pp + (size_t)a0 * p + b0;
    const float* wv = window + (size_t)a0 * p + b0;
    const int x = threadIdx.x, y = threadIdx.y;
    for (int c0 = 0; c0 < ncls; c0 += BL_CLS) {
        const int nc = min(BL_CLS, ncls - c0);
        if (c0) __syncthreads();                             // the previous pass's LDS reads are done
#pragma unroll
        for (int k = 0; k < BL_PER; k++) {
            const int a = y + k * BL_ROWS;
            if (x < sb.nb && a < sb.na) {
                const float* l = L + (size_t)a * p + x;
                float m = l[0];
                for (int c = 1; c < ncls; c++) m = fmaxf(m, l[c * pp]);
                float s = 0.f;
                for (int c = 0; c < ncls; c++) s += expf(l[c * pp] - m);
                for (int c = 0; c < nc; c++) lds[c][a][x] = expf(l[(c0 + c) * pp] - m) / s;
            }
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < BL_PER; k++) {
            const int ii = y + k * BL_ROWS, jj = x;
            if (ii < sb.ni && jj < sb.nj) {
                int a, bb;
                sb.src_of(ii, jj, a, bb);
                const float w = wv[(size_t)ii * p + jj];
                for (int c = 0; c < nc; c++) O[(c0 + c) * pp + (size_t)ii * p + jj] = w * lds[c][a][bb];
            }
        }
    }
}

extern "C" int bdn_blend_fold(const float* logits, const int32_t* table, const float* window, float* out,
                              int n_img, int ncls, int p, void* stream) {
    if (!logits || !table || !window || !out) BDN_FAIL(BDN_E_ARG, "blend_fold: null pointer");
    if (n_img <= 0 || ncls < 2 || p <= 0) BDN_FAIL(BDN_E_SHAPE, "blend_fold: need n_img > 0, ncls >= 2, p > 0");
    const int tb = (p + BL_TILE - 1) / BL_TILE;
    const long long blocks = (long long)n_img * tb * tb;
    if (blocks > INT_MAX) BDN_FAIL(BDN_E_SHAPE, "blend_fold: %lld blocks exceed the grid", blocks);
    hipLaunchKernelGGL(blend_fold_kernel, dim3((unsigned)blocks), dim3(BL_TILE, BL_ROWS), 0, (hipStream_t)stream,
                       logits, table, window, out, ncls, p, tb);
    BDN_CHECK_LAUNCH("blend_fold");
    return BDN_OK;
}

// ============================================================ blend_stitch
// reference: utils/inference.py:187-236 (_get_bands), generalized: instead of the last paste winning, every forward image that covers a
// scene pixel adds its folded values (bdn_blend_fold) to acc [ncls][H][W] and its window weight to wsum [H][W].  One thread per pixel
// of the rows the batch touches; it finds the covering tiles arithmetically from the tile plan and visits this batch's images of them in
// ascending global image index, adding to a register loaded once and stored once.  The sequence of additions of every pixel is therefore
// the global image order whatever the batch boundaries -- provided the batches' stitches run in order (the caller's events).
struct BlendPlan { int H, W, p, s, ny, nx, S; long long img0, img1; };

static inline int blend_count(int n, int p, int s) { return (n - p) / s + 1 + ((n - p) % s != 0); }

template <typename F>
__device__ __forceinline__ void for_each_cover(const BlendPlan& P, int y, int x, F&& f) {
    const int ky0 = y - P.p + 1 > 0 ? (y - P.p + P.s) / P.s : 0, kx0 = x - P.p + 1 > 0 ? (x - P.p + P.s) / P.s : 0;
    for (int ky = ky0; ky < P.ny; ky++) {                    // every tile row from ky0 on reaches down to y; stop at the first that starts below it
        const int ty = min(ky * P.s, P.H - P.p);
        if (ty > y) return;
        for (int kx = kx0; kx < P.nx; kx++) {
            const int tx = min(kx * P.s, P.W - P.p);
            if (tx > x) break;
            const long long g = (long long)ky * P.nx + kx;
            for (int k = 0; k < P.S; k++) {
                const long long i = g * P.S + k;
                if (i >= P.img1) return;                     // images ascend with (ky, kx, k): nothing later is in this batch
                if (i >= P.img0) f(i - P.img0, (size_t)(y - ty) * P.p + (x - tx));
            }
        }
    }
}

__global__ void blend_stitch_kernel(const float* __restrict__ fold, const float* __restrict__ window, float* __restrict__ acc,
                                    float* __restrict__ wsum, BlendPlan P, int ncls, int r0, int c0, int cols, int col_blocks) {
    const int x = c0 + (blockIdx.x % col_blocks) * blockDim.x + threadIdx.x, y = r0 + blockIdx.x / col_blocks;
    if (x >= c0 + cols) return;
    const size_t pix = (size_t)y * P.W + x, HW = (size_t)P.H * P.W, pp = (size_t)P.p * P.p;
    bool any = false;
    float ws = 0.f;
    for_each_cover(P, y, x, [&](long long, size_t o) {
        if (!any) { ws = wsum[pix]; any = true; }
        ws += window[o];
    });
    if (!any) return;                                        // no image of this batch covers the pixel
    wsum[pix] = ws;
    for (int c = 0; c < ncls; c++) {
        float v = acc[c * HW + pix];
        for_each_cover(P, y, x, [&](long long i, size_t o) { v += fold[((size_t)i * ncls + c) * pp + o]; });
        acc[c * HW + pix] = v;
    }
}

extern "C" int bdn_blend_stitch(const float* fold, const float* window, float* acc, float* wsum, long long img0, int n_img,
                                int n_syms, int ncls, int H, int W, int p, int stride, void* stream) {
    if (!fold || !window || !acc || !wsum) BDN_FAIL(BDN_E_ARG, "blend_stitch: null pointer");
    if (n_img <= 0 || img0 < 0 || n_syms < 1 || n_syms > 8 || ncls < 2 || p <= 0 || H < p || W < p || stride < 1 || stride > p)
        BDN_FAIL(BDN_E_SHAPE, "blend_stitch: bad shape (n_img=%d img0=%lld syms=%d ncls=%d %dx%d p=%d stride=%d)", n_img, img0, n_syms, ncls, H, W, p, stride);
    BlendPlan P{H, W, p, stride, blend_count(H, p, stride), blend_count(W, p, stride), n_syms, img0, img0 + n_img};
    const long long g0 = img0 / n_syms, g1 = (P.img1 - 1) / n_syms;          // first and last tile of the batch
    if (g1 >= (long long)P.ny * P.nx) BDN_FAIL(BDN_E_SHAPE, "blend_stitch: images [%lld, %lld) beyond the tile plan", img0, P.img1);
    const int ky0 = (int)(g0 / P.nx), ky1 = (int)(g1 / P.nx);
    const int r0 = min(ky0 * stride, H - p), r1 = min(ky1 * stride, H - p) + p;
    int c0 = 0, c1 = W;
    if (ky0 == ky1) { c0 = min((int)(g0 % P.nx) * stride, W - p); c1 = min((int)(g1 % P.nx) * stride, W - p) + p; }
    const int col_blocks = (c1 - c0 + 255) / 256;
    const long long blocks = (long long)(r1 - r0) * col_blocks;
    if (blocks > INT_MAX) BDN_FAIL(BDN_E_SHAPE, "blend_stitch: %lld blocks exceed the grid", blocks);
    hipLaunchKernelGGL(blend_stitch_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                       fold, window, acc, wsum, P, ncls, r0, c0, c1 - c0, col_blocks);
    BDN_CHECK_LAUNCH("blend_stitch");
    return BDN_OK;
}

// ============================================================ blend_finalize
// proba = acc / wsum in place, mask = its argmax over classes (first maximum wins, as torch.max(preds, 1) in train.py:199).
__global__ void blend_finalize_kernel(float* __restrict__ acc, const float* __restrict__ wsum, uint8_t* __restrict__ mask, int ncls, size_t HW) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= HW) return;
    const float ws = wsum[i];
    float best = 0.f;
    int arg = 0;
    for (int c = 0; c < ncls; c++) {
        const float v = acc[c * HW + i] / ws;
        acc[c * HW + i] = v;
        if (c == 0 || v > best) { best = v; arg = c; }
    }
    mask[i] = (uint8_t)arg;
}

extern "C" int bdn_blend_finalize(float* acc, const float* wsum, uint8_t* mask, int ncls, int H, int W, void* stream) {
    if (!acc || !wsum || !mask) BDN_FAIL(BDN_E_ARG, "blend_finalize: null pointer");
    if (ncls < 2 || ncls > 256 || H <= 0 || W <= 0) BDN_FAIL(BDN_E_SHAPE, "blend_finalize: bad shape (2 <= ncls <= 256)");
    const size_t HW = (size_t)H * W;
    hipLaunchKernelGGL(blend_finalize_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, acc, wsum, mask, ncls, HW);
    BDN_CHECK_LAUNCH("blend_finalize");
    return BDN_OK;
}
