// libbidate_hip: cleaning a scene mask -- binary reconstruction (hysteresis thresholding, hole filling, border clearing) on the canonical
// labels of bdn_cc_label, and disc morphology as a threshold on the exact squared distances of bdn_edt.  The reference stops at the pixel
// mask of a scene (train.py:199); each of these would be a scipy.ndimage call (binary_propagation, binary_fill_holes, binary_dilation /
// binary_erosion) on the host after a device-to-host copy of the mask.  Here the mask stays on the device:
//   bdn_cc_mark         two launches: clear the flags, then every labelled pixel that is a seed (or lies on the image edge) stores 1 at its
//                       component's root.  Many threads store the same 1: the flags do not depend on the arrival order.
//   bdn_cc_select       one launch: keep the components by flag and by area, OR-ed onto a base mask.
//   bdn_d2_mask         one launch: d2 <= r2 (dilation) or d2 > r2 (erosion).
//   bdn_threshold_pair  one launch: the low and the high mask of one probability plane in one pass.
//   bdn_mask_not        one launch: out = src != 1 (the background raster of the hole filling).
// Streaming kernels in cc.hip's form: grid-strided under a block cap, four pixels per thread (16-byte label loads, 4-byte mask loads and
// stores) where W and the pointers allow, one pixel otherwise.  No loop waits for another thread; nothing is read back; integers only but
// for the two comparisons of bdn_threshold_pair.
#include "common.hpp"

constexpr int MO_THREADS = 256;
constexpr int MO_MAX_BLOCKS = 2048;                        // grid-strided kernels: 8 blocks per CU
constexpr long long MO_MAX_PIXELS = 2147483646LL;          // bdn_cc_label's limit: 1 + (largest index) still fits an int32 label

template <int PER> struct MoVec;
template <> struct MoVec<1> {
    __device__ __forceinline__ static void load(const int* p, int* v) { v[0] = p[0]; }
    __device__ __forceinline__ static void store(int* p, const int* v) { p[0] = v[0]; }
    __device__ __forceinline__ static void loadf(const float* p, float* v) { v[0] = p[0]; }
    __device__ __forceinline__ static void bytes(const uint8_t* p, int* v) { v[0] = p[0]; }
    __device__ __forceinline__ static void store_bytes(uint8_t* p, const int* v) { p[0] = (uint8_t)v[0]; }
};
template <> struct MoVec<4> {
    __device__ __forceinline__ static void load(const int* p, int* v) {
        const int4 u = *reinterpret_cast<const int4*>(p);
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    }
    __device__ __forceinline__ static void store(int* p, const int* v) { *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]); }
    __device__ __forceinline__ static void loadf(const float* p, float* v) {
        const float4 u = *reinterpret_cast<const float4*>(p);
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    }
    __device__ __forceinline__ static void bytes(const uint8_t* p, int* v) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
        v[0] = u & 255; v[1] = u >> 8 & 255; v[2] = u >> 16 & 255; v[3] = u >> 24;
    }
    __device__ __forceinline__ static void store_bytes(uint8_t* p, const int* v) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    }
};

static inline unsigned mo_grid(long long n_items) {
    const long long want = (n_items + MO_THREADS - 1) / MO_THREADS;
    return (unsigned)(want < 1 ? 1 : want < MO_MAX_BLOCKS ? want : MO_MAX_BLOCKS);
}
static inline bool mo_al(const void* p, uintptr_t a) { return (uintptr_t)p % a == 0; }
static inline bool mo_shape_ok(int H, int W) { return H >= 1 && W >= 1 && (long long)H * W <= MO_MAX_PIXELS; }

// ============================================================ mark
template <int PER>
__global__ __launch_bounds__(MO_THREADS) void mo_clear_kernel(int* __restrict__ mark, long long n_items) {
    const long long stride = (long long)gridDim.x * MO_THREADS;
    const int zero[4] = {0, 0, 0, 0};
    for (long long it = (long long)blockIdx.x * MO_THREADS + threadIdx.x; it < n_items; it += stride) MoVec<PER>::store(mark + it * PER, zero);
}

// An item is PER consecutive pixels; PER = 4 needs W % 4 == 0, so an item lies in one row.  A label is 0 or 1 + a pixel index below H W.
template <int PER>
__global__ __launch_bounds__(MO_THREADS) void mo_mark_kernel(const int* __restrict__ labels, const uint8_t* __restrict__ seed, int seed_value, int border,
                                                             int* mark, int H, int W, long long n_items) {
    const long long stride = (long long)gridDim.x * MO_THREADS;
    for (long long it = (long long)blockIdx.x * MO_THREADS + threadIdx.x; it < n_items; it += stride) {
        int lab[PER], s[PER];
        MoVec<PER>::load(labels + it * PER, lab);
#pragma unroll
        for (int j = 0; j < PER; j++) s[j] = -1;
        if (seed) MoVec<PER>::bytes(seed + it * PER, s);
        const int y = (int)(it * PER / W), x = (int)(it * PER - (long long)y * W);
        const bool edge_row = border && (y == 0 || y == H - 1);
#pragma unroll
        for (int j = 0; j < PER; j++) {
            const bool hit = (seed && s[j] == seed_value) || edge_row || (border && (x + j == 0 || x + j == W - 1));
            if (lab[j] != 0 && hit) mark[lab[j] - 1] = 1;
        }
    }
}

extern "C" int bdn_cc_mark(const int32_t* labels, const uint8_t* seed, int seed_value, int border, int32_t* mark, int H, int W, void* stream) {
    if (!labels || !mark) BDN_FAIL(BDN_E_ARG, "cc_mark: null pointer");
    if (!mo_al(labels, 4) || !mo_al(mark, 4)) BDN_FAIL(BDN_E_ARG, "cc_mark: labels / mark must be 4-byte aligned");
    if (labels == mark) BDN_FAIL(BDN_E_ARG, "cc_mark: mark must not alias labels");
    if (seed && (seed_value < 0 || seed_value > 255)) BDN_FAIL(BDN_E_ARG, "cc_mark: seed_value must be a byte 0..255, got %d", seed_value);
    if (!mo_shape_ok(H, W)) BDN_FAIL(BDN_E_ARG, "cc_mark: need 1 <= H, W and H * W <= 2^31 - 2, got %d x %d", H, W);
    const long long HW = (long long)H * W;
    const bool vec = W % 4 == 0 && mo_al(labels, 16) && mo_al(mark, 16) && mo_al(seed, 4);
    const long long n_items = vec ? HW / 4 : HW;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(mo_clear_kernel<4>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, mark, n_items);
    else hipLaunchKernelGGL(mo_clear_kernel<1>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, mark, n_items);
    BDN_CHECK_LAUNCH("cc_mark (clear)");
    if (vec) hipLaunchKernelGGL(mo_mark_kernel<4>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, labels, seed, seed_value, border != 0, mark, H, W, n_items);
    else hipLaunchKernelGGL(mo_mark_kernel<1>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, labels, seed, seed_value, border != 0, mark, H, W, n_items);
    BDN_CHECK_LAUNCH("cc_mark");
    return BDN_OK;
}

// ============================================================ select
// base and out may be the same raster: a thread reads its item of base before it writes the same item of out, and no other thread touches it.
template <int PER>
__global__ __launch_bounds__(MO_THREADS) void mo_select_kernel(const int* __restrict__ labels, const int* __restrict__ mark, int keep_marked,
                                                               const int* __restrict__ area, int min_area, int max_area, const uint8_t* base,
                                                               uint8_t* out, long long n_items) {
    const long long stride = (long long)gridDim.x * MO_THREADS;
    for (long long it = (long long)blockIdx.x * MO_THREADS + threadIdx.x; it < n_items; it += stride) {
        int lab[PER], b[PER], keep[PER];
        MoVec<PER>::load(labels + it * PER, lab);
#pragma unroll
        for (int j = 0; j < PER; j++) b[j] = 0;
        if (base) MoVec<PER>::bytes(base + it * PER, b);
#pragma unroll
        for (int j = 0; j < PER; j++) {
            bool sel = lab[j] != 0;
            if (sel && mark) sel = (mark[lab[j] - 1] != 0) == (keep_marked != 0);
            if (sel && area) { const int a = area[lab[j] - 1]; sel = a >= min_area && a <= max_area; }
            keep[j] = b[j] == 1 || sel;
        }
        MoVec<PER>::store_bytes(out + it * PER, keep);
    }
}

extern "C" int bdn_cc_select(const int32_t* labels, const int32_t* mark, int keep_marked, const int32_t* area, int min_area, int max_area,
                             const uint8_t* base, uint8_t* out, int H, int W, void* stream) {
    if (!labels || !out) BDN_FAIL(BDN_E_ARG, "cc_select: null pointer");
    if (!mo_al(labels, 4) || !mo_al(mark, 4) || !mo_al(area, 4)) BDN_FAIL(BDN_E_ARG, "cc_select: labels / mark / area must be 4-byte aligned");
    if (keep_marked != 0 && keep_marked != 1) BDN_FAIL(BDN_E_ARG, "cc_select: keep_marked must be 0 or 1, got %d", keep_marked);
    if (min_area < 1 || max_area < min_area) BDN_FAIL(BDN_E_ARG, "cc_select: need 1 <= min_area <= max_area, got %d and %d", min_area, max_area);
    if (!area && (min_area != 1 || max_area != 2147483647)) BDN_FAIL(BDN_E_ARG, "cc_select: area bounds other than 1 and 2^31 - 1 need the areas");
    if (!mo_shape_ok(H, W)) BDN_FAIL(BDN_E_ARG, "cc_select: need 1 <= H, W and H * W <= 2^31 - 2, got %d x %d", H, W);
    const long long HW = (long long)H * W;
    const bool vec = W % 4 == 0 && mo_al(labels, 16) && mo_al(base, 4) && mo_al(out, 4);
    const long long n_items = vec ? HW / 4 : HW;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(mo_select_kernel<4>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, labels, mark, keep_marked, area, min_area, max_area, base, out, n_items);
    else hipLaunchKernelGGL(mo_select_kernel<1>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, labels, mark, keep_marked, area, min_area, max_area, base, out, n_items);
    BDN_CHECK_LAUNCH("cc_select");
    return BDN_OK;
}

// ============================================================ d2_mask
template <int PER>
__global__ __launch_bounds__(MO_THREADS) void mo_d2_mask_kernel(const int* __restrict__ d2, int r2, int greater, uint8_t* __restrict__ out, long long n_items) {
    const long long stride = (long long)gridDim.x * MO_THREADS;
    for (long long it = (long long)blockIdx.x * MO_THREADS + threadIdx.x; it < n_items; it += stride) {
        int d[PER], o[PER];
        MoVec<PER>::load(d2 + it * PER, d);
#pragma unroll
        for (int j = 0; j < PER; j++) o[j] = greater ? d[j] > r2 : d[j] <= r2;
        MoVec<PER>::store_bytes(out + it * PER, o);
    }
}

extern "C" int bdn_d2_mask(const int32_t* d2, int r2, int greater, uint8_t* out, long long n, void* stream) {
    if (!d2 || !out) BDN_FAIL(BDN_E_ARG, "d2_mask: null pointer");
    if (!mo_al(d2, 4)) BDN_FAIL(BDN_E_ARG, "d2_mask: d2 must be 4-byte aligned");
    if (r2 < 0) BDN_FAIL(BDN_E_ARG, "d2_mask: r2 must be >= 0, got %d", r2);
    if (greater != 0 && greater != 1) BDN_FAIL(BDN_E_ARG, "d2_mask: greater must be 0 or 1, got %d", greater);
    if (n < 1 || n > 2147483647LL) BDN_FAIL(BDN_E_ARG, "d2_mask: need 1 <= n < 2^31, got %lld", n);
    const bool vec = n % 4 == 0 && mo_al(d2, 16) && mo_al(out, 4);
    const long long n_items = vec ? n / 4 : n;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(mo_d2_mask_kernel<4>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, d2, r2, greater, out, n_items);
    else hipLaunchKernelGGL(mo_d2_mask_kernel<1>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, d2, r2, greater, out, n_items);
    BDN_CHECK_LAUNCH("d2_mask");
    return BDN_OK;
}

// ============================================================ threshold_pair
// bdn_threshold_mask's comparison, twice on one load of the plane: a NaN probability gives 0 in both masks.
template <int PER>
__global__ __launch_bounds__(MO_THREADS) void mo_threshold_pair_kernel(const float* __restrict__ p, float low, float high, uint8_t* __restrict__ mask_low,
                                                                       uint8_t* __restrict__ mask_high, long long n_items) {
    const long long stride = (long long)gridDim.x * MO_THREADS;
    for (long long it = (long long)blockIdx.x * MO_THREADS + threadIdx.x; it < n_items; it += stride) {
        float v[PER];
        int lo[PER], hi[PER];
        MoVec<PER>::loadf(p + it * PER, v);
#pragma unroll
        for (int j = 0; j < PER; j++) { lo[j] = v[j] >= low; hi[j] = v[j] >= high; }
        MoVec<PER>::store_bytes(mask_low + it * PER, lo);
        MoVec<PER>::store_bytes(mask_high + it * PER, hi);
    }
}

extern "C" int bdn_threshold_pair(const float* proba, int pos_class, float low, float high, uint8_t* mask_low, uint8_t* mask_high, int ncls,
                                  long long HW, void* stream) {
    if (!proba || !mask_low || !mask_high) BDN_FAIL(BDN_E_ARG, "threshold_pair: null pointer");
    if (mask_low == mask_high) BDN_FAIL(BDN_E_ARG, "threshold_pair: mask_low and mask_high must be two rasters");
    if (!mo_al(proba, 4)) BDN_FAIL(BDN_E_ARG, "threshold_pair: proba must be 4-byte aligned");
    if (!(low >= 0.f && high <= 1.f && low <= high))
        BDN_FAIL(BDN_E_ARG, "threshold_pair: need 0 <= low <= high <= 1, got %g and %g", (double)low, (double)high);
    if (ncls < 2 || ncls > 256 || HW < 1 || HW > MO_MAX_PIXELS) BDN_FAIL(BDN_E_ARG, "threshold_pair: need 2 <= ncls <= 256, 1 <= HW <= 2^31 - 2");
    if (pos_class < 0 || pos_class >= ncls) BDN_FAIL(BDN_E_ARG, "threshold_pair: pos_class must be in 0..%d, got %d", ncls - 1, pos_class);
    const float* p = proba + (size_t)pos_class * HW;
    const bool vec = HW % 4 == 0 && mo_al(p, 16) && mo_al(mask_low, 4) && mo_al(mask_high, 4);
    const long long n_items = vec ? HW / 4 : HW;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(mo_threshold_pair_kernel<4>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, p, low, high, mask_low, mask_high, n_items);
    else hipLaunchKernelGGL(mo_threshold_pair_kernel<1>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, p, low, high, mask_low, mask_high, n_items);
    BDN_CHECK_LAUNCH("threshold_pair");
    return BDN_OK;
}

// ============================================================ complement
template <int PER>
__global__ __launch_bounds__(MO_THREADS) void mo_not_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ out, long long n_items) {
    const long long stride = (long long)gridDim.x * MO_THREADS;
    for (long long it = (long long)blockIdx.x * MO_THREADS + threadIdx.x; it < n_items; it += stride) {
        int s[PER];
        MoVec<PER>::bytes(src + it * PER, s);
#pragma unroll
        for (int j = 0; j < PER; j++) s[j] = s[j] != 1;
        MoVec<PER>::store_bytes(out + it * PER, s);
    }
}

extern "C" int bdn_mask_not(const uint8_t* src, uint8_t* out, long long n, void* stream) {
    if (!src || !out) BDN_FAIL(BDN_E_ARG, "mask_not: null pointer");
    if (src == out) BDN_FAIL(BDN_E_ARG, "mask_not: out must not alias src");
    if (n < 1 || n > 2147483647LL) BDN_FAIL(BDN_E_ARG, "mask_not: need 1 <= n < 2^31, got %lld", n);
    const bool vec = n % 4 == 0 && mo_al(src, 4) && mo_al(out, 4);
    const long long n_items = vec ? n / 4 : n;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(mo_not_kernel<4>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, src, out, n_items);
    else hipLaunchKernelGGL(mo_not_kernel<1>, dim3(mo_grid(n_items)), dim3(MO_THREADS), 0, st, src, out, n_items);
    BDN_CHECK_LAUNCH("mask_not");
    return BDN_OK;
}
