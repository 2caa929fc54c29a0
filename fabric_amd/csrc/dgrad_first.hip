// Data gradient of the FIRST convolution (inc.conv.conv.0: C_pad = 16 -> 64, 3x3, pad 1; reference models/unet_parts.py:13 inside
// models/bidate_model.py:22-30): the gradient on the two input images, for attribution and input perturbation through autograd.
//
// dx[n][y][x][ci] = sum_{co,ky,kx} dz[n][y+1-ky][x+1-kx][co] * w[co][ci][ky][kx] over the 2B images of the shared encoder (date 1 first,
// bdn_pack_input's order).  The output has 16 columns (ci), of which C_real are real: one v_mfma_f32_16x16x32_bf16 covers all of them
// (N = 16), M = 16 output pixels of a tile row, K = 32 of the 64 dz channels; a tile row is 9 taps x 2 chunks = 18 MFMAs per term.
//
// dz is formed while the dz halo is staged into LDS, from dA and z with bdn_bn_bwd_apply's expression (the staging of
// wgrad_first_kernel / wgrad_first_x3_kernel):  dz = scale * (g - s0/M - xhat * s1/M),  g = dA where scale z + shift > 0.
// With a running-statistics table (bdn_bn_eval) and the zeroed `sums` bdn_bn_bwd_finalize_frozen leaves this is the frozen
// BatchNorm backward dz = scale * g.  z == NULL: dA is dz itself.
//   bf16 storage: dz rounded to bf16 (as the fused weight gradient rounds it), filter rounded to bf16, one MFMA per product.
//   float32 storage: dz and the filter split into bf16 hi + lo, three terms (hi hi, lo hi, hi lo) into one accumulator.
// The filter's B fragments are built once per block from the float32 OIHW master weight and stay in registers; blocks walk
// 8 x 16 output tiles grid-stride.  The epilogue writes float32 NCHW straight into the two date tensors; padded channels and
// pixels outside a ragged map are never written.
#include "common.hpp"

typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

constexpr int DF_TH = 8, DF_TW = 16;                              // output tile; one wave per two tile rows
constexpr int DF_PH = DF_TH + 2, DF_PW = DF_TW + 2, DF_NPIX = DF_PH * DF_PW;
constexpr int DF_PSTR = 144;                                      // dz pixel stride in LDS: 64 bf16 + 16 B (conflict-free b128 reads)
constexpr int DF_PATCH = DF_NPIX * DF_PSTR;                       // 25 920 B per term

struct DgFirstArgs {
    const void* dA; int ldA; const void* z; const float* bn; const float* sums;
    const float* w;                                               // [64][Cin_real][3][3] float32
    float* dx1; float* dx2;                                       // [B][Cin_real][H][W] float32
    int B, H, W, Cin_real, imgs_per_group;
    int tiles_y, tiles_x, n_tiles;
    float invM;
};

template <typename T, int TERMS>
__global__ __launch_bounds__(256) void dgrad_first_kernel(DgFirstArgs a) {
    constexpr int C = 64, EPU = ET<T>::EPU, UPP = C / EPU;        // elements per staged unit, units per patch pixel
    constexpr int NU = (DF_NPIX * UPP + 255) / 256;               // units per thread
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* ph = smem;
    unsigned char* pl = smem + DF_PATCH;                          // TERMS == 3 only

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int cu = (tid % UPP) * EPU;                             // the thread's channels in every unit it stages (256 % UPP == 0)
    const int kq = lane >> 4, m = lane & 15;

    // B fragments: lane holds B[k = 8 kq + j][n = m] = w[co = 32 kc + 8 kq + j][ci = m][tap]
    uint4 wh[18], wl[18];
#pragma unroll
    for (int t = 0; t < 9; t++)
#pragma unroll
        for (int kc = 0; kc < 2; kc++) {
            float f[8], h[8], r[8];
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const int co = 32 * kc + 8 * kq + j;
                f[j] = m < a.Cin_real ? a.w[((size_t)co * a.Cin_real + m) * 9 + t] : 0.f;
            }
            wh[t * 2 + kc] = Unit<bf16s>::pack(f);
            Unit<bf16s>::unpack(wh[t * 2 + kc], h);
#pragma unroll
            for (int j = 0; j < 8; j++) r[j] = f[j] - h[j];
            wl[t * 2 + kc] = Unit<bf16s>::pack(r);
        }

    float mean[EPU], inv[EPU], sc[EPU], sh[EPU], k0[EPU], k1[EPU];
    int grp_cur = -1;
    const int N = 2 * a.B;
    (void)N;

    for (int q = blockIdx.x; q < a.n_tiles; q += gridDim.x) {
        const int tx = q % a.tiles_x, ty = (q / a.tiles_x) % a.tiles_y, n = q / (a.tiles_x * a.tiles_y);
        const int y0 = ty * DF_TH, x0 = tx * DF_TW;
        if (a.z) {
            const int g = n / a.imgs_per_group;
            if (g != grp_cur) {
                grp_cur = g;
#pragma unroll
                for (int e = 0; e < EPU; e++) {
                    mean[e] = bn_row(a.bn, g, 0, C)[cu + e]; inv[e] = bn_row(a.bn, g, 1, C)[cu + e];
                    sc[e] = bn_row(a.bn, g, 2, C)[cu + e]; sh[e] = bn_row(a.bn, g, 3, C)[cu + e];
                    k0[e] = a.sums[((size_t)g * 2 + 0) * C + cu + e] * a.invM;
                    k1[e] = a.sums[((size_t)g * 2 + 1) * C + cu + e] * a.invM;
                }
            }
        }
        __syncthreads();                                          // the previous tile's fragment reads are done
#pragma unroll
        for (int i = 0; i < NU; i++) {
            const int u = tid + i * 256;
            if (u >= DF_NPIX * UPP) break;
            const int pp = u / UPP, py = pp / DF_PW, px = pp % DF_PW;
            const int y = y0 + py - 1, x = x0 + px - 1;
            float o[EPU];
#pragma unroll
            for (int e = 0; e < EPU; e++) o[e] = 0.f;
            if ((unsigned)y < (unsigned)a.H && (unsigned)x < (unsigned)a.W) {
                const size_t pix = ((size_t)n * a.H + y) * a.W + x;
                float fg[EPU];
                Unit<T>::unpack(*reinterpret_cast<const uint4*>(static_cast<const T*>(a.dA) + pix * a.ldA + cu), fg);
                if (a.z) {
                    float fz[EPU];
                    Unit<T>::unpack(*reinterpret_cast<const uint4*>(static_cast<const T*>(a.z) + pix * C + cu), fz);
#pragma unroll
                    for (int e = 0; e < EPU; e++) {
                        const float gm = fmaf(fz[e], sc[e], sh[e]) > 0.f ? fg[e] : 0.f;
                        const float xhat = (fz[e] - mean[e]) * inv[e];
                        o[e] = sc[e] * (gm - k0[e] - xhat * k1[e]);
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < EPU; e++) o[e] = fg[e];
                }
            }
            unsigned char* dst = ph + pp * DF_PSTR + cu * 2;
            if constexpr (EPU == 8) {                             // bf16 storage: dz is already bf16-exact (rounded on form)
                *reinterpret_cast<uint4*>(dst) = Unit<bf16s>::pack(o);
            } else {
#pragma unroll
                for (int e = 0; e < EPU; e++) asm volatile("" : "+v"(o[e]));   // the float32 dz, pinned: lo is its residual
                const uint32_t h0 = f2bf2(o[0], o[1]), h1 = f2bf2(o[2], o[3]);
                *reinterpret_cast<uint2*>(dst) = make_uint2(h0, h1);
                if (TERMS == 3) {
                    const float r0 = o[0] - bf2f(h0 & 0xffffu), r1 = o[1] - bf2f(h0 >> 16);
                    const float r2 = o[2] - bf2f(h1 & 0xffffu), r3 = o[3] - bf2f(h1 >> 16);
                    *reinterpret_cast<uint2*>(pl + pp * DF_PSTR + cu * 2) = make_uint2(f2bf2(r0, r1), f2bf2(r2, r3));
                }
            }
        }
        __syncthreads();

        f32x4 acc[2];
#pragma unroll
        for (int rr = 0; rr < 2; rr++) acc[rr] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const int ky = t / 3, kx = t % 3;
#pragma unroll
            for (int rr = 0; rr < 2; rr++) {
                const int py = 2 * wave + rr + 2 - ky, px = m + 2 - kx;
                const unsigned off = (py * DF_PW + px) * DF_PSTR + kq * 16;
#pragma unroll
                for (int kc = 0; kc < 2; kc++) {
                    const uint4 ah = *reinterpret_cast<const uint4*>(ph + off + kc * 64);
                    acc[rr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah),
                                                                      __builtin_bit_cast(bf16x8, wh[t * 2 + kc]), acc[rr], 0, 0, 0);
                    if constexpr (TERMS == 3) {
                        const uint4 al = *reinterpret_cast<const uint4*>(pl + off + kc * 64);
                        acc[rr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, al),
                                                                          __builtin_bit_cast(bf16x8, wh[t * 2 + kc]), acc[rr], 0, 0, 0);
                        acc[rr] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, ah),
                                                                          __builtin_bit_cast(bf16x8, wl[t * 2 + kc]), acc[rr], 0, 0, 0);
                    }
                }
            }
        }

        // C tile: column m = ci, rows 4 kq + reg = pixels of the tile row
        const int b = n < a.B ? n : n - a.B;
        float* out = (n < a.B ? a.dx1 : a.dx2) + ((size_t)b * a.Cin_real + m) * a.H * a.W;
#pragma unroll
        for (int rr = 0; rr < 2; rr++) {
            const int y = y0 + 2 * wave + rr;
            if (m < a.Cin_real && y < a.H) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const int x = x0 + 4 * kq + r;
                    if (x < a.W) out[(size_t)y * a.W + x] = acc[rr][r];
                }
            }
        }
    }
}

}  // namespace

extern "C" int bdn_conv3x3_dgrad_first(int dtype, const void* dA, int ldA, const void* z, const float* bn, const float* sums,
                                       int imgs_per_group, const float* w_oihw, int Cin_real,
                                       float* dx1, float* dx2, int B, int H, int W, void* stream) {
    if (!dA || !w_oihw || !dx1 || !dx2) BDN_FAIL(BDN_E_ARG, "conv3x3_dgrad_first: null pointer");
    if (z && (!bn || !sums)) BDN_FAIL(BDN_E_ARG, "conv3x3_dgrad_first: null pointer (bn / sums with z)");
    if (dtype != BDN_BF16 && dtype != BDN_F32) BDN_FAIL(BDN_E_ARG, "conv3x3_dgrad_first: bad dtype %d", dtype);
    const int epu = dtype == BDN_BF16 ? 8 : 4;
    if (B <= 0 || H <= 0 || W <= 0 || Cin_real <= 0 || Cin_real > 16 || ldA < 64 || ldA % epu)
        BDN_FAIL(BDN_E_SHAPE, "conv3x3_dgrad_first: bad shape (B=%d H=%d W=%d Cin_real=%d ldA=%d)", B, H, W, Cin_real, ldA);
    if (z && (imgs_per_group <= 0 || (2 * B) % imgs_per_group))
        BDN_FAIL(BDN_E_SHAPE, "conv3x3_dgrad_first: imgs_per_group=%d must divide 2B=%d", imgs_per_group, 2 * B);
    DgFirstArgs a;
    a.dA = dA; a.ldA = ldA; a.z = z; a.bn = bn; a.sums = sums; a.w = w_oihw; a.dx1 = dx1; a.dx2 = dx2;
    a.B = B; a.H = H; a.W = W; a.Cin_real = Cin_real; a.imgs_per_group = z ? imgs_per_group : 1;
    a.tiles_y = (H + DF_TH - 1) / DF_TH; a.tiles_x = (W + DF_TW - 1) / DF_TW;
    const long long nt = 2LL * B * a.tiles_y * a.tiles_x;
    if (nt >= (1LL << 31)) BDN_FAIL(BDN_E_SHAPE, "conv3x3_dgrad_first: too many tiles");
    a.n_tiles = (int)nt;
    a.invM = z ? 1.f / (float)((size_t)imgs_per_group * H * W) : 0.f;
    hipStream_t st = (hipStream_t)stream;
    const unsigned grid = (unsigned)(a.n_tiles < 2048 ? a.n_tiles : 2048);   // 256 CUs x 8 blocks, grid-stride over the tiles
    if (dtype == BDN_BF16) {
        hipLaunchKernelGGL((dgrad_first_kernel<bf16s, 1>), dim3(grid), dim3(256), DF_PATCH, st, a);
    } else {
        auto kern = dgrad_first_kernel<float, 3>;
        BDN_SET_SMEM_ONCE(kern, 2 * DF_PATCH, "conv3x3_dgrad_first");
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 2 * DF_PATCH, st, a);
    }
    BDN_CHECK_LAUNCH("conv3x3_dgrad_first");
    return BDN_OK;
}
