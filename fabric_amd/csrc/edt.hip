// Exact squared Euclidean distance transform on uint8 rasters (bdn_edt), the boundary loss of Kervadec et al. (MIDL 2019) built on it
// (bdn_boundary_loss, bdn_signed_distance) and the boundary sets and scores of boundary F1 / Hausdorff (bdn_boundary_mask,
// bdn_boundary_score).  include/bidate_hip.h states the semantics; edt_core.hpp holds the arithmetic (checked on the host by
// tools/edt_host_check.cpp).  Integers only up to the one square root of the signed distance.
//
// bdn_edt, two launches whatever the data (R = N * H rows in all):
//   columns   one thread per (image, column): a down sweep and an up sweep over y, the loads of src coalesced across x; g (16 bits) goes to
//             the workspace transposed, gT[x][R], so that the row pass reads it coalesced across rows.  The price: the lanes of a wave store
//             g 2 bytes each at a stride of 2 R bytes, and the up sweep reads and rewrites the same scattered places
//   rows      one lane per row, a wave per block: the lower envelope of the row's parabolas (edt_core.hpp), O(W) per row for every
//             input.  W <= 128: the row's g and the stack live in LDS (48 KiB per block, [k][lane]: conflict-free); wider rows keep the
//             g stack in gT itself and the (s, t) stack in the workspace, [k][R]
// ws: [gT u16 W*R][st u32 W*R, only for W > 128], each part padded to 16 bytes.  Every word read has been written by the same call.
// The loss runs the same two kernels over 2 x (included classes) x B virtual images (grid.y = the job: class and polarity), then
//   phi       per pixel the signed distances, softmax, p . phi in double, a tree per block; valid pixels per block
//   finish    the blocks' partials in a fixed order, n, term, loss, 1 / n
//   grad      dlogit_j = weight p_j (phi_j - sum_c phi_c p_c) / n, written or added once per element (none with dlogits == NULL)
#include "common.hpp"
#include "edt_core.hpp"
#include <limits.h>

static inline size_t edt_up16(size_t v) { return (v + 15) / 16 * 16; }

// the sites of job j of a launch: plain (one job, the caller's test) or pairs (class sv0 + j / 2; even j: the class, odd j: the others)
struct EdtJobs { int nj, sv0, site_equal, pairs; };
__device__ __forceinline__ void edt_job(const EdtJobs& J, int j, int& sv, int& eq) {
    if (J.pairs) { sv = J.sv0 + (j >> 1); eq = !(j & 1); } else { sv = J.sv0; eq = J.site_equal; }
}

// ---------------------------------------------------------------- pass 1: columns
__global__ __launch_bounds__(256) void edt_col_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ valid, int invalid_value,
                                                      EdtJobs J, uint16_t* __restrict__ gT, int N, int H, int W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)N * W) return;
    const int n = (int)(i / W), x = (int)(i - (long long)n * W), j = blockIdx.y;
    int sv, eq; edt_job(J, j, sv, eq);
    const size_t R = (size_t)N * H;
    const uint8_t* s = src + (size_t)n * H * W + x;
    const uint8_t* v = valid ? valid + (size_t)n * H * W + x : nullptr;
    uint16_t* g = gT + ((size_t)j * W + x) * R + (size_t)n * H;
    unsigned d = EDT_INF;
#pragma unroll 8
    for (int y = 0; y < H; y++) {
        const size_t o = (size_t)y * W;
        d = edt_col_step(d, edt_is_site(s[o], sv, eq, v != nullptr, v ? v[o] : 0, invalid_value));
        g[y] = (uint16_t)d;
    }
    d = EDT_INF;
#pragma unroll 8
    for (int y = H - 1; y >= 0; y--) {
        const unsigned down = g[y];
        d = edt_col_step(d, down == 0);
        g[y] = (uint16_t)edt_col_min(down, d);
    }
}

// ---------------------------------------------------------------- pass 2: rows
static_assert(EDT_LANES == 64, "one wave of rows per block");
struct EdtOutRow { int32_t* p; __device__ __forceinline__ int32_t& operator()(int k) const { return p[k]; } };

template <bool LDS>
__global__ __launch_bounds__(64) void edt_row_kernel(uint16_t* __restrict__ gT, uint32_t* __restrict__ stG, int32_t* __restrict__ out,
                                                     int limit, long long rows, long long R, int W) {
    const long long r = (long long)blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;                                 // (no barrier below: a lane touches its own column of the LDS arrays only)
    const long long j = r / R, rr = r - j * R;
    uint16_t* g = gT + (size_t)j * W * R + rr;             // element k of this row: g[k * R]
    EdtOutRow o{out + (size_t)r * W};
    if constexpr (LDS) {
        __shared__ uint16_t lgs[EDT_LDS_W * 64];
        __shared__ uint32_t lst[EDT_LDS_W * 64];
        const int lane = threadIdx.x;
#pragma unroll 8
        for (int k = 0; k < W; k++) lgs[k * 64 + lane] = g[(size_t)k * R];
        edt_row_pass(EdtLaned<uint16_t>{lgs + lane}, EdtLaned<uint32_t>{lst + lane}, o, W, limit);
    } else {
        edt_row_pass(EdtStrided<uint16_t>{g, (size_t)R}, EdtStrided<uint32_t>{stG + (size_t)j * W * R + rr, (size_t)R}, o, W, limit);
    }
}

struct EdtPlan { size_t o_g, o_st, total; };
static EdtPlan edt_plan(size_t images, int H, int W) {
    EdtPlan p;
    const size_t px = images * H * W;
    p.o_g = 0;
    p.o_st = edt_up16(sizeof(uint16_t) * px);
    p.total = p.o_st + (W > EDT_LDS_W ? edt_up16(sizeof(uint32_t) * px) : 0);
    return p;
}

// the two launches over J.nj * N images; out: int32 [J.nj][N][H][W]
static int edt_run(const uint8_t* src, const uint8_t* valid, int invalid_value, EdtJobs J, int limit, int32_t* out, void* ws,
                   int N, int H, int W, hipStream_t st) {
    const EdtPlan p = edt_plan((size_t)J.nj * N, H, W);
    uint16_t* gT = (uint16_t*)((char*)ws + p.o_g);
    uint32_t* stG = (uint32_t*)((char*)ws + p.o_st);
    hipLaunchKernelGGL(edt_col_kernel, dim3(grid_for((size_t)N * W), J.nj), dim3(256), 0, st, src, valid, invalid_value, J, gT, N, H, W);
    BDN_CHECK_LAUNCH("edt_col");
    const long long R = (long long)N * H, rows = R * J.nj;
    const dim3 grid((unsigned)((rows + 63) / 64));
    if (W <= EDT_LDS_W) hipLaunchKernelGGL(edt_row_kernel<true>, grid, dim3(64), 0, st, gT, stG, out, limit, rows, R, W);
    else hipLaunchKernelGGL(edt_row_kernel<false>, grid, dim3(64), 0, st, gT, stG, out, limit, rows, R, W);
    BDN_CHECK_LAUNCH("edt_row");
    return BDN_OK;
}

static bool edt_shape_ok(long long images, int H, int W) {
    return images > 0 && H > 0 && W > 0 && H <= EDT_MAX_DIM && W <= EDT_MAX_DIM && (unsigned long long)images * H * W < (1ull << 31);
}

extern "C" size_t bdn_edt_workspace_bytes(int N, int H, int W) {
    if (!edt_shape_ok(N, H, W)) return 0;
    return edt_plan((size_t)N, H, W).total;
}

extern "C" int bdn_edt(const uint8_t* src, int site_value, int site_equal, const uint8_t* valid_src, int invalid_value, int limit,
                       int32_t* out_d2, void* ws, int N, int H, int W, void* stream) {
    if (!src || !out_d2 || !ws) BDN_FAIL(BDN_E_ARG, "edt: null pointer");
    if (site_value < 0 || site_value > 255 || (site_equal != 0 && site_equal != 1))
        BDN_FAIL(BDN_E_ARG, "edt: site_value=%d must be a byte value (0..255) and site_equal=%d 0 or 1", site_value, site_equal);
    if (valid_src && (invalid_value < 0 || invalid_value > 255)) BDN_FAIL(BDN_E_ARG, "edt: invalid_value=%d must be a byte value (0..255)", invalid_value);
    if (limit < 1) BDN_FAIL(BDN_E_ARG, "edt: limit=%d must lie in 1..2^31-1", limit);
    if (!edt_shape_ok(N, H, W)) BDN_FAIL(BDN_E_ARG, "edt: bad shape %d x %d x %d (1 <= N, 1 <= H, W <= 32767, N*H*W < 2^31)", N, H, W);
    if (((uintptr_t)ws & 15) || ((uintptr_t)out_d2 & 3)) BDN_FAIL(BDN_E_ARG, "edt: ws must be 16-byte aligned and out_d2 4-byte aligned");
    return edt_run(src, valid_src, invalid_value, EdtJobs{1, site_value, site_equal, 0}, limit, out_d2, ws, N, H, W, (hipStream_t)stream);
}

// ---------------------------------------------------------------- the boundary loss
// phi of class c at a pixel: + the distance to the nearest pixel of the class at a valid pixel outside it, -(the distance to the nearest
// valid pixel outside it - 1) inside, 0 at an ignored pixel and wherever the image holds no such site (INT_MAX: the transform's
// "no site").  The root is the float64 square root of the integer rounded to float32: the correctly rounded float32 root, whatever the
// compiler's float32 sqrt options are (the fast float32 root of the hardware is off by one unit in the last place on some integers).
__device__ __forceinline__ float bnd_sqrt(int d2) { return (float)sqrt((double)d2); }
__device__ __forceinline__ float bnd_phi(bool valid, bool fg, int d2_fg, int d2_bg, float max_dist) {
    float phi = 0.f;
    if (valid) {
        if (fg) { if (d2_bg != INT_MAX) phi = -(bnd_sqrt(d2_bg) - 1.f); }
        else if (d2_fg != INT_MAX) phi = bnd_sqrt(d2_fg);
    }
    if (max_dist > 0.f) phi = fminf(fmaxf(phi, -max_dist), max_dist);
    return phi;
}

// classes c0 .. c1-1 are included; d2: int32 [(c - c0) * 2 + {0: to the class, 1: to the others}][npix]; phi_ws: f32 [c1 - c0][npix];
// phi_out (NULL or f32 [c1][npix]): 0 for the classes below c0.  logits == NULL: the distances only.
__global__ __launch_bounds__(256) void bnd_phi_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels, int ignore,
                                                      const int32_t* __restrict__ d2, float max_dist, float* __restrict__ phi_ws,
                                                      float* __restrict__ phi_out, double* __restrict__ part, int32_t* __restrict__ pval,
                                                      int npix, int ncls, int c0, int c1, FastDiv dhw) {
    __shared__ double dred[256];
    __shared__ int s_valid;
    const int tid = threadIdx.x;
    const long long e = (long long)blockIdx.x * 256 + tid;
    if (tid == 0) s_valid = 0;
    __syncthreads();
    double acc = 0.0;
    if (e < npix) {
        const int t = labels[e];
        const bool valid = t != ignore;
        float phi[OUTC_MAXCLS];
#pragma unroll
        for (int k = 0; k < OUTC_MAXCLS; k++) {
            const int c = c0 + k;
            phi[k] = 0.f;
            if (c < c1) {
                const size_t o = (size_t)(2 * k) * npix + (size_t)e;
                phi[k] = bnd_phi(valid, t == c, d2[o], d2[o + npix], max_dist);
                if (phi_ws) phi_ws[(size_t)k * npix + (size_t)e] = phi[k];
            }
        }
        if (phi_out) {
            for (int c = 0; c < c0; c++) phi_out[(size_t)c * npix + (size_t)e] = 0.f;
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (c0 + k < c1) phi_out[(size_t)(c0 + k) * npix + (size_t)e] = phi[k];
        }
        if (logits && valid) {                             // an ignored pixel: none of its logits is read
            const size_t hw = (size_t)dhw.d;
            int b, q; dhw.divmod((int)e, b, q);
            float p[OUTC_MAXCLS]; float m = -INFINITY;
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { p[k] = logits[((size_t)b * ncls + k) * hw + q]; m = fmaxf(m, p[k]); }
            float den = 0.f;
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { p[k] = expf(p[k] - m); den += p[k]; }
            const float inv = 1.f / den;                   // softmax as the criterion's statistics pass forms it
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls && k >= c0 && k < c1) acc += (double)(p[k] * inv) * (double)phi[k - c0];
            atomicAdd(&s_valid, 1);
        }
    }
    if (!logits) return;                                   // (uniform)
    dred[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) { if (tid < h) dred[tid] += dred[tid + h]; __syncthreads(); }
    if (tid == 0) { part[blockIdx.x] = dred[0]; pval[blockIdx.x] = s_valid; }
}

__global__ __launch_bounds__(256) void bnd_finish_kernel(const double* __restrict__ part, const int32_t* __restrict__ pval, int nb, float weight,
                                                         int accumulate, float* __restrict__ loss, float* __restrict__ term, float* __restrict__ scale) {
    __shared__ double dred[256];
    __shared__ long long nred[256];
    const int tid = threadIdx.x;
    double a = 0.0; long long n = 0;
    for (int i = tid; i < nb; i += 256) { a += part[i]; n += pval[i]; }
    dred[tid] = a; nred[tid] = n;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) { if (tid < h) { dred[tid] += dred[tid + h]; nred[tid] += nred[tid + h]; } __syncthreads(); }
    if (tid == 0) {
        const long long nv = nred[0];
        const float t = nv > 0 ? (float)(dred[0] / (double)nv) : 0.f;
        scale[0] = nv > 0 ? (float)(1.0 / (double)nv) : 0.f;
        if (term) *term = t;
        const float wt = __fmul_rn(weight, t);
        *loss = accumulate ? *loss + wt : wt;
    }
}

__global__ __launch_bounds__(256) void bnd_grad_kernel(const float* __restrict__ logits, const uint8_t* __restrict__ labels, int ignore,
                                                       const float* __restrict__ phi_ws, const float* __restrict__ scale, float weight,
                                                       int accumulate, float* __restrict__ dlogits, int npix, int ncls, int c0, FastDiv dhw) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= npix) return;
    const size_t hw = (size_t)dhw.d;
    int b, qi; dhw.divmod((int)e, b, qi);
    if ((int)labels[e] == ignore) {                        // nothing of this pixel's logits is read; an accumulated gradient stays as it is
        if (!accumulate) {
#pragma unroll
            for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) dlogits[((size_t)b * ncls + k) * hw + qi] = 0.f;
        }
        return;
    }
    float p[OUTC_MAXCLS], qq[OUTC_MAXCLS]; float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { p[k] = logits[((size_t)b * ncls + k) * hw + qi]; m = fmaxf(m, p[k]); }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) { p[k] = expf(p[k] - m); den += p[k]; }
    const float inv = 1.f / den, sc = scale[0];
    float dot = 0.f;
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) {
        p[k] *= inv;
        qq[k] = k >= c0 ? phi_ws[(size_t)(k - c0) * npix + (size_t)e] * sc : 0.f;
        dot += qq[k] * p[k];
    }
#pragma unroll
    for (int k = 0; k < OUTC_MAXCLS; k++) if (k < ncls) {
        const size_t o = ((size_t)b * ncls + k) * hw + qi;
        const float v = __fmul_rn(weight, p[k] * (qq[k] - dot));               // rounded before the add: accumulate = 1 is one float32 add of accumulate = 0's value
        dlogits[o] = accumulate ? dlogits[o] + v : v;
    }
}

// ws: [the transform's workspace for 2 * ninc * B images][d2 int32 2*ninc*npix][phi f32 ninc*npix][partials f64 nb][valid i32 nb][1 / n: 4 x f32]
struct BndPlan { int npix, nb; size_t o_d2, o_phi, o_part, o_pval, o_scale, total; };
static BndPlan bnd_plan(int B, int ninc, int H, int W) {
    BndPlan p;
    p.npix = B * H * W;
    p.nb = (int)grid_for((size_t)p.npix);
    p.o_d2 = edt_plan((size_t)2 * ninc * B, H, W).total;
    p.o_phi = p.o_d2 + edt_up16(sizeof(int32_t) * (size_t)2 * ninc * p.npix);
    p.o_part = p.o_phi + edt_up16(sizeof(float) * (size_t)ninc * p.npix);
    p.o_pval = p.o_part + edt_up16(sizeof(double) * (size_t)p.nb);
    p.o_scale = p.o_pval + edt_up16(sizeof(int32_t) * (size_t)p.nb);
    p.total = p.o_scale + 16;
    return p;
}

static bool bnd_shape_ok(int B, int ninc, int H, int W) {
    return B > 0 && H > 0 && W > 0 && H <= EDT_MAX_DIM && W <= EDT_MAX_DIM && (unsigned long long)B * H * W < (1ull << 31) &&
           edt_shape_ok((long long)2 * ninc * B, H, W);
}

extern "C" size_t bdn_boundary_workspace_bytes(int B, int ncls, int H, int W) {
    if (ncls < 2 || ncls > OUTC_MAXCLS || !bnd_shape_ok(B, ncls, H, W)) return 0;
    return bnd_plan(B, ncls, H, W).total;                  // sized for classes_all = 1: one workspace serves both settings
}

extern "C" int bdn_boundary_loss(const float* logits, const uint8_t* labels, int ignore_label, int classes_all, float max_dist, float weight,
                                 int accumulate, void* ws, float* loss, float* term, float* dlogits, float* phi_out,
                                 int B, int ncls, int H, int W, void* stream) {
    if (!logits || !labels || !ws || !loss) BDN_FAIL(BDN_E_ARG, "boundary_loss: null pointer");
    if (ignore_label < -1 || ignore_label > 255) BDN_FAIL(BDN_E_ARG, "boundary_loss: ignore_label=%d is neither -1 (none) nor a byte value (0..255)", ignore_label);
    if (!(weight >= 0.f)) BDN_FAIL(BDN_E_ARG, "boundary_loss: negative weight (%g)", weight);
    if (!(max_dist >= 0.f)) BDN_FAIL(BDN_E_ARG, "boundary_loss: negative max_dist (%g; 0 = no clamp)", max_dist);
    if (ncls < 2 || ncls > OUTC_MAXCLS) BDN_FAIL(BDN_E_ARG, "boundary_loss: ncls=%d unsupported (2..%d)", ncls, OUTC_MAXCLS);
    if (!bnd_shape_ok(B, ncls, H, W)) BDN_FAIL(BDN_E_ARG, "boundary_loss: bad shape (H, W <= 32767, 2*ncls*B*H*W must stay below 2^31)");
    if ((uintptr_t)ws & 15) BDN_FAIL(BDN_E_ARG, "boundary_loss: ws must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int c0 = classes_all ? 0 : 1, ninc = ncls - c0;
    const BndPlan p = bnd_plan(B, ninc, H, W);             // (never more than the size query's plan for every class)
    char* base = (char*)ws;
    int32_t* d2 = (int32_t*)(base + p.o_d2); float* phi = (float*)(base + p.o_phi);
    double* part = (double*)(base + p.o_part); int32_t* pval = (int32_t*)(base + p.o_pval); float* scale = (float*)(base + p.o_scale);
    // the ignored pixels leave both site sets: labels are their own validity raster (ignore_label = -1 matches no byte)
    const int rc = edt_run(labels, labels, ignore_label, EdtJobs{2 * ninc, c0, 1, 1}, INT_MAX, d2, ws, B, H, W, st);
    if (rc != BDN_OK) return rc;
    const FastDiv dhw(H * W);
    hipLaunchKernelGGL(bnd_phi_kernel, dim3(p.nb), dim3(256), 0, st, logits, labels, ignore_label, d2, max_dist, phi, phi_out, part, pval,
                       p.npix, ncls, c0, ncls, dhw);
    BDN_CHECK_LAUNCH("boundary_phi");
    hipLaunchKernelGGL(bnd_finish_kernel, dim3(1), dim3(256), 0, st, part, pval, p.nb, weight, accumulate, loss, term, scale);
    BDN_CHECK_LAUNCH("boundary_finish");
    if (dlogits) {
        hipLaunchKernelGGL(bnd_grad_kernel, dim3(p.nb), dim3(256), 0, st, logits, labels, ignore_label, phi, scale, weight, accumulate, dlogits,
                           p.npix, ncls, c0, dhw);
        BDN_CHECK_LAUNCH("boundary_grad");
    }
    return BDN_OK;
}

extern "C" size_t bdn_signed_distance_workspace_bytes(int N, int H, int W) {
    if (!bnd_shape_ok(N, 1, H, W)) return 0;
    return bnd_plan(N, 1, H, W).total;
}

extern "C" int bdn_signed_distance(const uint8_t* labels, int cls, int ignore_label, float max_dist, void* ws, float* phi, int N, int H, int W,
                                   void* stream) {
    if (!labels || !ws || !phi) BDN_FAIL(BDN_E_ARG, "signed_distance: null pointer");
    if (cls < 0 || cls > 255) BDN_FAIL(BDN_E_ARG, "signed_distance: cls=%d must be a byte value (0..255)", cls);
    if (ignore_label < -1 || ignore_label > 255) BDN_FAIL(BDN_E_ARG, "signed_distance: ignore_label=%d is neither -1 (none) nor a byte value (0..255)", ignore_label);
    if (!(max_dist >= 0.f)) BDN_FAIL(BDN_E_ARG, "signed_distance: negative max_dist (%g; 0 = no clamp)", max_dist);
    if (!bnd_shape_ok(N, 1, H, W)) BDN_FAIL(BDN_E_ARG, "signed_distance: bad shape (H, W <= 32767, 2*N*H*W must stay below 2^31)");
    if ((uintptr_t)ws & 15) BDN_FAIL(BDN_E_ARG, "signed_distance: ws must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const BndPlan p = bnd_plan(N, 1, H, W);
    int32_t* d2 = (int32_t*)((char*)ws + p.o_d2);
    const int rc = edt_run(labels, labels, ignore_label, EdtJobs{2, cls, 1, 1}, INT_MAX, d2, ws, N, H, W, st);
    if (rc != BDN_OK) return rc;
    hipLaunchKernelGGL(bnd_phi_kernel, dim3(p.nb), dim3(256), 0, st, (const float*)nullptr, labels, ignore_label, d2, max_dist, phi,
                       (float*)nullptr, (double*)nullptr, (int32_t*)nullptr, p.npix, 0, cls, cls + 1, FastDiv(H * W));
    BDN_CHECK_LAUNCH("signed_distance_phi");
    return BDN_OK;
}

// ---------------------------------------------------------------- boundary sets and scores
__global__ __launch_bounds__(256) void bnd_mask_kernel(const uint8_t* __restrict__ src, int fg_value, const uint8_t* __restrict__ valid,
                                                       int invalid_value, uint8_t* __restrict__ out, int H, int W) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)H * W) return;
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    auto ok = [&](long long k) { return !valid || valid[k] != invalid_value; };
    auto open = [&](int yy, int xx) {                      // a neighbour that is inside the image, valid and not foreground
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) return false;
        const long long k = (long long)yy * W + xx;
        return ok(k) && src[k] != fg_value;
    };
    out[i] = edt_on_boundary(ok(i), src[i] == fg_value, open(y - 1, x), open(y + 1, x), open(y, x - 1), open(y, x + 1)) ? 1 : 0;
}

// acc: u64[6] (the output, zeroed by the entry) ={n_pred, n_true, pred_hit, true_hit, 1 + max d2 pred -> true, 1 + max d2 true -> pred}
__global__ __launch_bounds__(256) void bnd_score_kernel(const uint8_t* __restrict__ bnd, const int32_t* __restrict__ d2, long long tol2,
                                                        unsigned long long* __restrict__ acc, long long hw) {
    __shared__ unsigned s_cnt[4];
    __shared__ unsigned s_max[2];
    const int tid = threadIdx.x;
    if (tid < 4) s_cnt[tid] = 0;
    if (tid < 2) s_max[tid] = 0;
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + tid;
    if (i < hw) {
        if (bnd[i]) {                                      // a predicted boundary pixel: its distance to the true boundary
            const int d = d2[hw + i];
            atomicAdd(&s_cnt[0], 1u); if (d <= tol2) atomicAdd(&s_cnt[2], 1u);
            atomicMax(&s_max[0], (unsigned)d + 1u);
        }
        if (bnd[hw + i]) {
            const int d = d2[i];
            atomicAdd(&s_cnt[1], 1u); if (d <= tol2) atomicAdd(&s_cnt[3], 1u);
            atomicMax(&s_max[1], (unsigned)d + 1u);
        }
    }
    __syncthreads();
    if (tid < 4 && s_cnt[tid]) atomicAdd(&acc[tid], (unsigned long long)s_cnt[tid]);
    if (tid < 2 && s_max[tid]) atomicMax(&acc[4 + tid], (unsigned long long)s_max[tid]);
}

__global__ void bnd_score_finish_kernel(long long* out) {   // the maxima were kept as 1 + d2; -1 when either set is empty
    if (threadIdx.x == 0) {
        const bool both = out[0] > 0 && out[1] > 0;
        out[4] = both ? out[4] - 1 : -1;
        out[5] = both ? out[5] - 1 : -1;
    }
}

extern "C" int bdn_boundary_mask(const uint8_t* src, int fg_value, const uint8_t* valid_src, int invalid_value, uint8_t* out, int H, int W,
                                 void* stream) {
    if (!src || !out) BDN_FAIL(BDN_E_ARG, "boundary_mask: null pointer");
    if (fg_value < 0 || fg_value > 255) BDN_FAIL(BDN_E_ARG, "boundary_mask: fg_value=%d must be a byte value (0..255)", fg_value);
    if (valid_src && (invalid_value < 0 || invalid_value > 255)) BDN_FAIL(BDN_E_ARG, "boundary_mask: invalid_value=%d must be a byte value (0..255)", invalid_value);
    if (!edt_shape_ok(1, H, W)) BDN_FAIL(BDN_E_ARG, "boundary_mask: bad shape %d x %d (1 <= H, W <= 32767, H*W < 2^31)", H, W);
    hipLaunchKernelGGL(bnd_mask_kernel, dim3(grid_for((size_t)H * W)), dim3(256), 0, (hipStream_t)stream, src, fg_value, valid_src, invalid_value,
                       out, H, W);
    BDN_CHECK_LAUNCH("boundary_mask");
    return BDN_OK;
}

extern "C" int bdn_boundary_score(const uint8_t* bnd, const int32_t* d2, long long tol2, long long* out, int H, int W, void* stream) {
    if (!bnd || !d2 || !out) BDN_FAIL(BDN_E_ARG, "boundary_score: null pointer");
    if (tol2 < 0) BDN_FAIL(BDN_E_ARG, "boundary_score: negative squared tolerance");
    if (!edt_shape_ok(2, H, W)) BDN_FAIL(BDN_E_ARG, "boundary_score: bad shape %d x %d (1 <= H, W <= 32767, 2*H*W < 2^31)", H, W);
    if ((uintptr_t)out & 7) BDN_FAIL(BDN_E_ARG, "boundary_score: out must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long* acc = (unsigned long long*)out;   // the sums and maxima gather in the output itself
    if (hipMemsetAsync(acc, 0, 6 * sizeof(unsigned long long), st) != hipSuccess) BDN_FAIL(BDN_E_HIP, "boundary_score: hipMemsetAsync failed");
    const long long hw = (long long)H * W;
    hipLaunchKernelGGL(bnd_score_kernel, dim3(grid_for((size_t)hw)), dim3(256), 0, st, bnd, d2, tol2, acc, hw);
    BDN_CHECK_LAUNCH("boundary_score");
    hipLaunchKernelGGL(bnd_score_finish_kernel, dim3(1), dim3(64), 0, st, out);
    BDN_CHECK_LAUNCH("boundary_score_finish");
    return BDN_OK;
}
