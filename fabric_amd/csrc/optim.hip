// Parameter updates over the flat float32 buffers: SGD, momentum SGD, Adam / AdamW, their grouped and _ex forms, EMA / SWA averaging and
// the buffer swap, gradient accumulation and the global gradient norm, and the layer-wise adaptive rules LAMB / LARS (per-tensor norms
// and trust ratios), and the perturbation and restore of sharpness-aware minimisation (SAM / ASAM).  Memory-bound float4 passes; no
// atomics, fixed-order reductions.
//
// Map of the file:
//   ungrouped kernels   sgd_kernel, sgdm_kernel, adam_kernel (with sgdm_elem / adam_elem, which every rule reuses), ema_multi_kernel,
//                       grad_accumulate_kernel: no table, and they alone handle n % 4 tails.
//   shared helpers      what every table-driven kernel is assembled from, each written once: flat_check / table_check (host), seg_step,
//                       stage_table (table and per-group parameters into LDS, *dev_scale applied), pass_lookup (grid-stride passes),
//                       chunk_span (the partial kernels' chunks), wave_sum / block_sum (fixed-order sums of doubles).
//   rules               RuleSgd / RuleSgdm / RuleAdam / RuleEma / RuleSwap (grouped_kernel), RuleLamb / RuleLars (lw_partial_kernel,
//                       lw_apply_kernel), sq_acc / sam_acc (the terms of the two norm partials), sam_elem (sam_apply_kernel).
//   entry points        each section ends with its own: bdn_sgd_step .. bdn_adam_step, the grouped updates and their _ex forms, EMA / swap,
//                       bdn_grad_accumulate and bdn_grad_norm, bdn_lamb_step / bdn_lars_step, bdn_sam_perturb / bdn_sam_restore.
#include "common.hpp"
#include <initializer_list>

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

// the rule's checks and kernel parameters, one place for bdn_sgd_momentum_step and the grouped launcher (per group): the same bits in both
static int sgdm_rule_check(const char* what, float momentum, const float* momentum_buf, float dampening, int nesterov) {
    if ((momentum != 0.f) != (momentum_buf != nullptr)) BDN_FAIL(BDN_E_ARG, "%s: momentum_buf must be given iff momentum != 0", what);
    if (nesterov && (momentum <= 0.f || dampening != 0.f)) BDN_FAIL(BDN_E_ARG, "%s: nesterov needs momentum > 0 and zero dampening", what);
    return BDN_OK;
}
static SgdmParams sgdm_params(float lr, float weight_decay, float grad_scale, float momentum, float dampening, int nesterov, int first_step) {
    return SgdmParams{lr, grad_scale, momentum, (float)(1.0 - (double)dampening), weight_decay, first_step ? 1 : 0, nesterov ? 1 : 0};
}

extern "C" int bdn_sgd_momentum_step(float* params, const float* grads, float* momentum_buf, float lr, float grad_scale, float momentum,
                                     float dampening, float weight_decay, int nesterov, int first_step, size_t n, void* stream) {
    if (!params || !grads) BDN_FAIL(BDN_E_ARG, "sgd_momentum_step: null pointer");
    if (int rc = sgdm_rule_check("sgd_momentum_step", momentum, momentum_buf, dampening, nesterov)) return rc;
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)momentum_buf) & 15)
        BDN_FAIL(BDN_E_ARG, "sgd_momentum_step: buffers must be 16-byte aligned");
    if (n == 0) return BDN_OK;
    const size_t n4 = n / 4;
    const SgdmParams a = sgdm_params(lr, weight_decay, grad_scale, momentum, dampening, nesterov, first_step);
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

// likewise for bdn_adam_step and the grouped launcher (bdn_adam_step has tested the state pointers before it asks)
static int adam_rule_check(const char* what, const float* exp_avg, const float* exp_avg_sq, long long step, double beta1, double beta2) {
    if (!exp_avg || !exp_avg_sq) BDN_FAIL(BDN_E_ARG, "%s: null pointer", what);
    if (step < 1) BDN_FAIL(BDN_E_ARG, "%s: step must be >= 1 (1-based, counted after the increment), got %lld", what, step);
    if (!(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0)) BDN_FAIL(BDN_E_ARG, "%s: betas must lie in [0, 1)", what);
    return BDN_OK;
}
// 1 - beta and the bias corrections in double on the host, as torch computes them from Python floats: no device sync
static AdamParams adam_params(float lr, float weight_decay, float grad_scale, double beta1, double beta2, float eps, int decoupled, long long step) {
    const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
    const float w1 = (float)(1.0 - beta1);
    const bool dec = decoupled != 0;
    return AdamParams{grad_scale, w1, (float)beta2, (float)(1.0 - beta2), eps, dec ? 0.f : weight_decay,
                      dec ? (float)(1.0 - (double)lr * (double)weight_decay) : 1.f, (float)((double)lr / bc1), (float)std::sqrt(bc2),
                      w1 >= 0.5f ? 1 : 0};
}

extern "C" int bdn_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float lr, float grad_scale,
                             double beta1, double beta2, float eps, float weight_decay, int decoupled_weight_decay, long long step,
                             size_t n, void* stream) {
    if (!params || !grads || !exp_avg || !exp_avg_sq) BDN_FAIL(BDN_E_ARG, "adam_step: null pointer");
    if (((uintptr_t)params | (uintptr_t)grads | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15)
        BDN_FAIL(BDN_E_ARG, "adam_step: buffers must be 16-byte aligned");
    if (int rc = adam_rule_check("adam_step", exp_avg, exp_avg_sq, step, beta1, beta2)) return rc;
    if (n == 0) return BDN_OK;
    const AdamParams a = adam_params(lr, weight_decay, grad_scale, beta1, beta2, eps, decoupled_weight_decay, step);
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

// ------------------------------------------------------------ shared helpers of the table-driven kernels
// Everything between an entry point's arguments and a rule's element function, written once: the grouped updates, EMA / swap, the
// gradient norm, LAMB / LARS and SAM below differ in their rule and in what they derive from a vector's table entry, not in this.
//
// Host side, flat buffers: `need` must not be null; `buffers` must be 16-byte aligned (a null entry -- a rule without that state -- passes);
// n is a multiple of 4 whose vector count fits the table's 32-bit ends.
static int flat_check(const char* what, std::initializer_list<const void*> need, std::initializer_list<const void*> buffers, size_t n) {
    for (const void* q : need)
        if (!q) BDN_FAIL(BDN_E_ARG, "%s: null pointer", what);
    uintptr_t bits = 0;
    for (const void* q : buffers) bits |= (uintptr_t)q;
    if (bits & 15) BDN_FAIL(BDN_E_ARG, "%s: buffers must be 16-byte aligned", what);
    if (n % 4 != 0 || n / 4 > 0xffffffffull)
        BDN_FAIL(BDN_E_ARG, "%s: n = %zu must be a multiple of 4 (tensors padded to a float4) below 2^34", what, n);
    return BDN_OK;
}

// Host side, a table of `count` entries of `noun` ("segment" / "tensor"): 1..OPT_MAX_SEGS of them, or 0.. where the entry point takes
// "no table" -- `every` then names what counts without one ("vector" / "element") and is nullptr otherwise; its arrays non-null and
// 4-byte aligned when there are entries; n_groups, where given, in 1..OPT_MAX_GROUPS.
static int table_check(const char* what, const char* noun, const char* every, int count, std::initializer_list<const void*> arrays,
                       const int* n_groups) {
    if (n_groups && (*n_groups < 1 || *n_groups > OPT_MAX_GROUPS))
        BDN_FAIL(BDN_E_ARG, "%s: %d groups (1..%d: their hyperparameters travel in the kernel arguments)", what, *n_groups, OPT_MAX_GROUPS);
    if (every && (count < 0 || count > OPT_MAX_SEGS))
        BDN_FAIL(BDN_E_ARG, "%s: %d %ss (0..%d; 0: no table, every %s counts)", what, count, noun, OPT_MAX_SEGS, every);
    if (!every && (count < 1 || count > OPT_MAX_SEGS)) BDN_FAIL(BDN_E_ARG, "%s: %d %ss (1..%d)", what, count, noun, OPT_MAX_SEGS);
    if (count == 0) return BDN_OK;
    uintptr_t bits = 0;
    for (const void* q : arrays) {
        if (!q && every) BDN_FAIL(BDN_E_ARG, "%s: null pointer (%s table of %d %ss)", what, noun, count, noun);
        if (!q) BDN_FAIL(BDN_E_ARG, "%s: null pointer", what);
        bits |= (uintptr_t)q;
    }
    if (bits & 3) BDN_FAIL(BDN_E_ARG, "%s: %s table must be 4-byte aligned", what, noun);
    return BDN_OK;
}

// One halving step of the lookup "first s with end[s] > i" over the LDS table, which is padded with UINT32_MAX to `cap` entries, a power
// of two: branch-free, so the OPT_VEC lookups of a pass advance side by side (their LDS reads are independent) and lanes never diverge.
__device__ __forceinline__ void seg_step(const uint32_t* s_end, int h, uint32_t i, int& s) {
    if (s_end[s + h - 1] <= i) s += h;
}

// The table's ends and groups into LDS, padded to `cap` entries, a power of two (seg_step's contract), which is returned; the caller
// places the barrier.  n == 0 -- no table: bdn_ema_update, bdn_swap_segments -- gives one segment of group 0 that covers everything; a
// pad entry is frozen otherwise.  third(k, in) fills a third per-entry array beside them (in: k is an entry, not a pad), or nothing.
struct NoThird { __device__ __forceinline__ void operator()(int, bool) const {} };
template <typename Third>
__device__ __forceinline__ int stage_table(const uint32_t* __restrict__ end, const int32_t* __restrict__ group, int n, uint32_t* s_end,
                                           int* s_grp, Third third) {
    int cap = 1;
    while (cap < n) cap <<= 1;
    for (int k = threadIdx.x; k < cap; k += 256) {
        const bool in = k < n;
        s_end[k] = in ? end[k] : 0xffffffffu;
        s_grp[k] = in ? group[k] : (n == 0 ? 0 : OPT_FROZEN);
        third(k, in);
    }
    return cap;
}

// The same, and the per-group parameters beside the table; with dev_scale (the _ex entry points, LAMB / LARS) grad_scale * *dev_scale is
// formed here, once per block.  dev_scale == nullptr never touches the staged parameters: the plain forms keep the bits they always gave.
template <typename Rule, typename Third>
__device__ __forceinline__ int stage_table(const uint32_t* __restrict__ end, const int32_t* __restrict__ group, int n, uint32_t* s_end,
                                           int* s_grp, Third third, const GroupArgs<typename Rule::Params>& a,
                                           const float* __restrict__ dev_scale, typename Rule::Params* s_par) {
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < OPT_MAX_GROUPS; k++) s_par[k] = a.g[k];
        if (dev_scale) {
            const float ds = *dev_scale;
#pragma unroll
            for (int k = 0; k < OPT_MAX_GROUPS; k++) Rule::scale(s_par[k], ds);
        }
    }
    return stage_table(end, group, n, s_end, s_grp, third);
}

// The table entry s of each of the OPT_VEC vectors i = b0 + u * stride + threadIdx.x of a grid-stride pass, as out[u] = entry(s, i), or
// -1 for a vector at or behind n4 or behind the table's last end: such a vector is neither read nor written, so a wrong table can not
// move an access out of the buffers.  EntryIndex yields s itself; a caller that wants more of the entry than its index -- SAM's count of
// real elements, which reads the entry's end again -- derives it here, where that end is already in a register.  A block's 256
// consecutive vectors almost always lie in one entry: one lookup of the first vector then serves the block (the first vector is clamped:
// a pass past the end yields -1 below); the lookup is per lane where they span a boundary or lie behind the table.
struct EntryIndex { __device__ __forceinline__ int operator()(int s, size_t) const { return s; } };
static_assert(OPT_FROZEN == -1, "grouped_kernel reads pass_lookup's 'no entry' as the frozen group id");
template <typename Entry>
__device__ __forceinline__ void pass_lookup(const uint32_t* s_end, int cap, size_t b0, size_t stride, size_t n4, int (&out)[OPT_VEC],
                                            Entry entry) {
    int head[OPT_VEC] = {};
    for (int h = cap >> 1; h > 0; h >>= 1) {
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t first = b0 + u * stride;
            seg_step(s_end, h, (uint32_t)(first < n4 ? first : n4 - 1), head[u]);
        }
    }
#pragma unroll
    for (int u = 0; u < OPT_VEC; u++) {
        const size_t first = b0 + u * stride, i = first + threadIdx.x;
        out[u] = -1;
        if (i < n4) {
            const size_t last = first + 255 < n4 ? first + 255 : n4 - 1;
            int s = head[u];
            if (!(s_end[s] > last)) {
                s = 0;
                for (int h = cap >> 1; h > 0; h >>= 1) seg_step(s_end, h, (uint32_t)i, s);
            }
            if (s_end[s] > i) out[u] = entry(s, i);
        }
    }
}

// The entries of the first and of the last vector of a partial kernel's chunk: equal where the chunk lies in one entry -- one lookup
// then serves the block -- and different where it spans a boundary, so that every vector (or every piece) looks its own up.
struct Span { int lo, hi; };
__device__ __forceinline__ Span chunk_span(const uint32_t* s_end, int cap, size_t first, size_t last) {
    Span sp{0, 0};
    for (int h = cap >> 1; h > 0; h >>= 1) { seg_step(s_end, h, (uint32_t)first, sp.lo); seg_step(s_end, h, (uint32_t)last, sp.hi); }
    return sp;
}

// Fixed-order sums of N doubles per lane.  wave_sum: the wave64 butterfly (__shfl_xor, the same tree in every wave); every lane ends
// with its wave's sums.  block_sum: the butterfly, then thread 0 adds the four wave sums in wave order and alone holds the block's sums.
template <int N>
__device__ __forceinline__ void wave_sum(double (&v)[N]) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
#pragma unroll
        for (int c = 0; c < N; c++) v[c] += __shfl_xor(v[c], m);
    }
}
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N]) {
    __shared__ double s_wave[4][N];
    wave_sum(v);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < N; c++) s_wave[threadIdx.x >> 6][c] = v[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < N; c++) v[c] = ((s_wave[0][c] + s_wave[1][c]) + s_wave[2][c]) + s_wave[3][c];
    }
}

// ------------------------------------------------------------ the grouped update kernel
template <typename Rule>
__global__ void __launch_bounds__(256) grouped_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                      float* __restrict__ s1, SegTable t, GroupArgs<typename Rule::Params> a,
                                                      const float* __restrict__ dev_scale, size_t n4) {
    __shared__ uint32_t s_end[OPT_MAX_SEGS];
    __shared__ int s_grp[OPT_MAX_SEGS];
    __shared__ typename Rule::Params s_par[OPT_MAX_GROUPS];
    const int cap = stage_table<Rule>(t.end, t.group, t.n_seg, s_end, s_grp, NoThird{}, a, dev_scale, s_par);
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t b0 = (size_t)blockIdx.x * 256; b0 < n4; b0 += stride * OPT_VEC) {
        int gid[OPT_VEC];                                    // the group of each vector; no entry (-1) is OPT_FROZEN
        pass_lookup(s_end, cap, b0, stride, n4, gid, [&](int s, size_t) { return s_grp[s]; });
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) gid[u] = (unsigned)gid[u] < (unsigned)t.n_groups ? gid[u] : OPT_FROZEN;
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
    if (int rc = flat_check(what, {params, grads, lr}, {params, grads, s0, s1}, n)) return rc;
    return table_check(what, "segment", nullptr, n_seg, {seg_end, seg_group}, &n_groups);
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
    if (int rc = sgdm_rule_check(what, momentum, momentum_buf, dampening, nesterov)) return rc;
    if (n == 0) return BDN_OK;
    GroupArgs<SgdmParams> a{};
    for (int k = 0; k < n_groups; k++) a.g[k] = sgdm_params(lr[k], weight_decay[k], grad_scale, momentum, dampening, nesterov, first_step);
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
    if (!weight_decay) BDN_FAIL(BDN_E_ARG, "%s: null pointer", what);
    if (int rc = adam_rule_check(what, exp_avg, exp_avg_sq, step, beta1, beta2)) return rc;
    if (n == 0) return BDN_OK;
    GroupArgs<AdamParams> a{};
    for (int k = 0; k < n_groups; k++) a.g[k] = adam_params(lr[k], weight_decay[k], grad_scale, beta1, beta2, eps, decoupled_weight_decay, step);
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
    if (int rc = flat_check(what, {a, b}, {a, b}, n)) return rc;
    return table_check(what, "segment", "vector", n_seg, {seg_end, seg_group}, nullptr);
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
    const size_t c0 = (size_t)blockIdx.x * NORM_CHUNK;
    // A block's 4096 consecutive vectors almost always lie in one segment: one lookup of its first and of its last vector then serves the
    // block (a frozen block reads nothing at all); a block that spans a boundary looks every vector up.  The sums are the same either way.
    int cap = 1;
    bool per_lane = false, whole = true;
    if (n_seg > 0) {                                         // no table: nothing is staged or looked up, every vector counts
        cap = stage_table(seg_end, seg_group, n_seg, s_end, s_grp, NoThird{});
        __syncthreads();
        const size_t last = (c0 + NORM_CHUNK < n4 ? c0 + NORM_CHUNK : n4) - 1;
        const Span sp = chunk_span(s_end, cap, c0, last);
        per_lane = sp.lo != sp.hi;
        whole = s_end[sp.lo] > last && s_grp[sp.lo] != OPT_FROZEN;
    }
    double acc[1] = {0.0};
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
        for (int u = 0; u < OPT_VEC; u++) acc[0] = sq_acc(acc[0], G[u]);     // a vector not taken adds +0.0: the sum is unchanged
    }
    block_sum(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

// the partials added in index order by thread 0 of a 256-thread block (staged through LDS 1024 at a time); the other threads return 0
__device__ __forceinline__ double sum_partials(const double* __restrict__ part, size_t nblk, double* s_part) {
    double sum = 0.0;
    for (size_t b0 = 0; b0 < nblk; b0 += 1024) {
        const size_t m = nblk - b0 < 1024 ? nblk - b0 : 1024;
        for (size_t k = threadIdx.x; k < m; k += 256) s_part[k] = part[b0 + k];
        __syncthreads();
        if (threadIdx.x == 0)
            for (size_t k = 0; k < m; k++) sum += s_part[k];
        __syncthreads();
    }
    return sum;
}

__global__ void __launch_bounds__(256) grad_norm_finish_kernel(const double* __restrict__ part, size_t nblk, float grad_scale, float max_norm,
                                                               float* __restrict__ out) {
    __shared__ double s_part[1024];
    const double sum = sum_partials(part, nblk, s_part);
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
    if (int rc = flat_check("grad_norm", {grads, workspace, out}, {grads}, n)) return rc;
    if (int rc = table_check("grad_norm", "segment", "element", n_seg, {seg_end, seg_group}, nullptr)) return rc;
    if ((uintptr_t)workspace & 7) BDN_FAIL(BDN_E_ARG, "grad_norm: workspace must be 8-byte aligned");
    if ((uintptr_t)out & 3) BDN_FAIL(BDN_E_ARG, "grad_norm: out must be 4-byte aligned");
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

// ============================================================ layer-wise adaptive rules: LAMB (You et al. 2020) and LARS (You et al. 2017)
// Both scale a tensor's update by a trust ratio formed from two norms of that tensor, so they need a norm per TENSOR between the moment
// update and the parameter update.  The table here is per tensor, not per segment: ten_end (sorted ends in float4 units, tiling [0, n/4)
// like seg_end), ten_len (the real element count: the last vector of a tensor is masked by it, a pad never enters a norm), ten_group
// (0..n_groups-1, OPT_FROZEN for frozen) and ten_adapt (0: ratio 1).  Three launches, fixed:
//   1 partial  block b owns the LW_CHUNK vectors [b LW_CHUNK, (b + 1) LW_CHUNK), as grad_norm_partial_kernel does, and writes one
//              pair of doubles {sum p^2, sum x^2} per PIECE, the intersection of its chunk with one tensor, to part[2 (b + t)] (b + t is
//              strictly increasing along the pieces, so no two pieces share a slot; there are fewer than blocks + tensors of them).  A
//              chunk inside one tensor -- a large tensor spans many blocks -- is summed by the whole block: each lane sums its vectors
//              in index order, a wave64 butterfly, thread 0 adds the four wave sums in wave order.  A chunk that holds several tensors
//              -- a bias is 16 vectors -- hands its pieces to its four waves round robin: lanes stride the piece, one butterfly, lane 0
//              writes.  Which path a piece takes depends on (n, table) alone.  LAMB: x = u, and the pass writes the new moments; LARS:
//              x = g, nothing is written.
//   2 finish   one wave per tensor: lane l adds the tensor's pieces l, l + 64, ... in chunk order, a butterfly, and lane 0 writes
//              trust_out[t] = {wn, xn, applied ratio} (float32, rounded once from double); a frozen tensor gets {0, 0, 0} and none of
//              its partials is read.
//   3 apply    the grouped kernels' pass shape (LDS-staged table, OPT_VEC float4s per thread, every load before the first store); each
//              vector takes its tensor's ratio from trust_out and its group's lr / weight_decay.  LAMB recomputes u from the NEW moments
//              and the still-OLD parameter through lamb_u, the function pass 1 summed: the same bits, and no n-sized scratch.
// No atomics, no memset, no host read-back, no block waits for another; a slot of `part` that no piece owns is never read, so the
// result does not depend on what the workspace or trust_out held.  Every float32 is converted to double before it is squared.
constexpr int LW_ROUNDS = 1;                                     // passes of OPT_VEC float4s per thread
constexpr size_t LW_CHUNK = (size_t)256 * OPT_VEC * LW_ROUNDS;   // vectors per block: 1024 (16 KiB per buffer).  A quarter of the gradient norm's chunk:
                                                                 // the pass does divisions and square roots between its loads and its sums, and
                                                                 // 3272 short blocks at the model's size overlap them where 818 long ones did not
static inline size_t lw_blocks(size_t n4) { return (n4 + LW_CHUNK - 1) / LW_CHUNK; }

struct TenTable { const uint32_t* end; const uint32_t* len; const int32_t* group; const int32_t* adapt; int n_ten, n_groups; };

struct LambParams { AdamParams a; float bc1, wd, lr; };
struct LarsParams { SgdmParams s; };

// LAMB's moments: adam_elem's statements for m and v, so that the state carries Adam's bits
__device__ __forceinline__ void lamb_moments(float gr, float& m, float& v, const AdamParams& a) {
    const float g = a.grad_scale * gr;
    m = a.lerp_hi ? g - (g - m) * (1.f - a.w1) : m + a.w1 * (g - m);
    v = a.beta2 * v + a.c2 * g * g;
}
// u = (m / bc1) / (sqrt(v)/sqrt(bc2) + eps) + wd * p: two IEEE divisions, a sqrt, an add and ONE explicit fma -- nothing the compiler may
// contract one way in pass 1 and another way in pass 3
__device__ __forceinline__ float lamb_u(float p, float m, float v, const LambParams& q) {
    const float den = sqrtf(v) / q.a.bc2_sqrt + q.a.eps;
    return fmaf(q.wd, p, (m / q.bc1) / den);
}
// LARS: sgdm_elem with d = local * (g + wd * p) in place of the decayed gradient (local == 1: sgdm_elem's bits)
template <bool MOM>
__device__ __forceinline__ void lars_elem(float& p, float gr, float& buf, float local, const SgdmParams& a) {
    float g = a.grad_scale * gr;
    if (a.weight_decay != 0.f) g = g + a.weight_decay * p;
    g = local * g;
    if (MOM) {
        buf = a.first ? g : a.momentum * buf + a.damp1 * g;
        g = a.nesterov ? g + a.momentum * buf : buf;
    }
    p = p - a.lr * g;
}

struct RuleLamb {
    using Params = LambParams;
    static constexpr bool LAMB = true, MOM = true;
    static __device__ __forceinline__ void scale(Params& q, float s) { q.a.grad_scale *= s; }
    static __device__ __forceinline__ bool reads_state(const Params&) { return true; }
    // pass 1: the new moments, and the value whose square is summed
    static __device__ __forceinline__ float first(float p, float gr, float& m, float& v, const Params& q) {
        lamb_moments(gr, m, v, q.a);
        return lamb_u(p, m, v, q);
    }
    static __device__ __forceinline__ void apply(float& p, float, float& m, float& v, float ratio, const Params& q) {
        p = p - (q.lr * ratio) * lamb_u(p, m, v, q);
    }
};
template <bool MOM_> struct RuleLars {
    using Params = LarsParams;
    static constexpr bool LAMB = false, MOM = MOM_;
    static __device__ __forceinline__ void scale(Params& q, float s) { q.s.grad_scale *= s; }
    static __device__ __forceinline__ bool reads_state(const Params& q) { return MOM_ && !q.s.first; }
    static __device__ __forceinline__ float first(float, float gr, float&, float&, const Params& q) { return q.s.grad_scale * gr; }
    static __device__ __forceinline__ void apply(float& p, float gr, float& buf, float&, float local, const Params& q) {
        lars_elem<MOM_>(p, gr, buf, local, q.s);
    }
};

// one vector of pass 1: the first `nvalid` elements enter the two sums (a pad is replaced by 0.0, whatever it holds)
template <typename Rule>
__device__ __forceinline__ void lw_sum_vec(const float4& P, const float4& G, float4& M, float4& V, int nvalid,
                                           const typename Rule::Params& q, double& aw, double& ax) {
    const float x0 = Rule::first(P.x, G.x, M.x, V.x, q), x1 = Rule::first(P.y, G.y, M.y, V.y, q);
    const float x2 = Rule::first(P.z, G.z, M.z, V.z, q), x3 = Rule::first(P.w, G.w, M.w, V.w, q);
    const double p0 = nvalid > 0 ? (double)P.x : 0.0, p1 = nvalid > 1 ? (double)P.y : 0.0;
    const double p2 = nvalid > 2 ? (double)P.z : 0.0, p3 = nvalid > 3 ? (double)P.w : 0.0;
    const double d0 = nvalid > 0 ? (double)x0 : 0.0, d1 = nvalid > 1 ? (double)x1 : 0.0;
    const double d2 = nvalid > 2 ? (double)x2 : 0.0, d3 = nvalid > 3 ? (double)x3 : 0.0;
    aw = fma(p0, p0, aw); aw = fma(p1, p1, aw); aw = fma(p2, p2, aw); aw = fma(p3, p3, aw);
    ax = fma(d0, d0, ax); ax = fma(d1, d1, ax); ax = fma(d2, d2, ax); ax = fma(d3, d3, ax);
}

template <typename Rule>
__global__ void __launch_bounds__(256) lw_partial_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                         float* __restrict__ s1, TenTable t, GroupArgs<typename Rule::Params> a,
                                                         const float* __restrict__ dev_scale, double* __restrict__ part, size_t n4) {
    __shared__ uint32_t s_end[OPT_MAX_SEGS];
    __shared__ int s_grp[OPT_MAX_SEGS];
    __shared__ typename Rule::Params s_par[OPT_MAX_GROUPS];
    const int cap = stage_table<Rule>(t.end, t.group, t.n_ten, s_end, s_grp, NoThird{}, a, dev_scale, s_par);
    __syncthreads();
    const size_t c0 = (size_t)blockIdx.x * LW_CHUNK, c1 = c0 + LW_CHUNK < n4 ? c0 + LW_CHUNK : n4;
    const Span sp = chunk_span(s_end, cap, c0, c1 - 1);
    const int t_lo = sp.lo, t_hi = sp.hi > t.n_ten - 1 ? t.n_ten - 1 : sp.hi;    // vectors behind the table's end belong to no tensor
    const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p);
    const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g);
    float4* __restrict__ m4 = reinterpret_cast<float4*>(s0);
    float4* __restrict__ v4 = reinterpret_cast<float4*>(s1);
    if (t_lo >= t_hi) {
        // ---- the chunk lies in one tensor: the whole block sums [lo, hi)
        const int k = t_lo;
        if (k > t.n_ten - 1) return;
        const size_t start = k ? s_end[k - 1] : 0, end = s_end[k];
        const size_t lo = start > c0 ? start : c0, hi = end < c1 ? end : c1;
        const int grp = s_grp[k];
        if (!(lo < hi) || (unsigned)grp >= (unsigned)t.n_groups) return;         // block-uniform: nobody reaches the barrier below
        const typename Rule::Params q = s_par[grp];
        const int tail = (int)(t.len[k] - 4u * (uint32_t)(end - 1 - start));      // real elements of the tensor's last vector
        double acc[2] = {0.0, 0.0};                          // {sum p^2, sum x^2}
        for (int r = 0; r < LW_ROUNDS; r++) {
            float4 P[OPT_VEC] = {}, G[OPT_VEC] = {}, M[OPT_VEC] = {}, V[OPT_VEC] = {};
#pragma unroll
            for (int u = 0; u < OPT_VEC; u++) {
                const size_t i = c0 + (size_t)(r * OPT_VEC + u) * 256 + threadIdx.x;
                if (i >= lo && i < hi) {
                    P[u] = p4[i]; G[u] = g4[i];
                    if (Rule::LAMB) { M[u] = m4[i]; V[u] = v4[i]; }
                }
            }
#pragma unroll
            for (int u = 0; u < OPT_VEC; u++) {
                const size_t i = c0 + (size_t)(r * OPT_VEC + u) * 256 + threadIdx.x;
                if (i >= lo && i < hi) {
                    lw_sum_vec<Rule>(P[u], G[u], M[u], V[u], i + 1 == end ? tail : 4, q, acc[0], acc[1]);
                    if (Rule::LAMB) { m4[i] = M[u]; v4[i] = V[u]; }
                }
            }
        }
        block_sum(acc);
        if (threadIdx.x == 0) {
            double* o = part + 2 * ((size_t)blockIdx.x + k);
            o[0] = acc[0]; o[1] = acc[1];
        }
        return;
    }
    // ---- the chunk holds several tensors: piece k goes to wave (k - t_lo) % 4
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int k = t_lo + wave; k <= t_hi; k += 4) {
        const size_t start = k ? s_end[k - 1] : 0, end = s_end[k];
        const size_t lo = start > c0 ? start : c0, hi = end < c1 ? end : c1;
        const int grp = s_grp[k];
        if (!(lo < hi) || (unsigned)grp >= (unsigned)t.n_groups) continue;        // wave-uniform
        const typename Rule::Params q = s_par[grp];
        const int tail = (int)(t.len[k] - 4u * (uint32_t)(end - 1 - start));
        double acc[2] = {0.0, 0.0};
        for (size_t i = lo + lane; i < hi; i += 64) {
            const float4 P = p4[i], G = g4[i];
            float4 M = {}, V = {};
            if (Rule::LAMB) { M = m4[i]; V = v4[i]; }
            lw_sum_vec<Rule>(P, G, M, V, i + 1 == end ? tail : 4, q, acc[0], acc[1]);
            if (Rule::LAMB) { m4[i] = M; v4[i] = V; }
        }
        wave_sum(acc);                                       // per wave, no barrier: the waves hold different pieces
        if (lane == 0) {
            double* o = part + 2 * ((size_t)blockIdx.x + k);
            o[0] = acc[0]; o[1] = acc[1];
        }
    }
}

struct TrustArgs { float wd[OPT_MAX_GROUPS]; float trust_coef, lars_eps, max_trust; };

// one wave per tensor: lane l adds the pieces l, l + 64, ... of its tensor in chunk order, then the butterfly (a serial chain over the 144
// pieces of a bottleneck filter is 144 dependent memory latencies on the update's critical path)
template <bool LAMB>
__global__ void __launch_bounds__(64) lw_finish_kernel(const double* __restrict__ part, TenTable t, TrustArgs a, size_t nblk, size_t n4,
                                                       float* __restrict__ trust_out) {
    const int k = blockIdx.x, lane = threadIdx.x;
    const int grp = t.group[k];
    float* o = trust_out + 3 * k;
    if ((unsigned)grp >= (unsigned)t.n_groups) {             // block-uniform
        if (lane == 0) { o[0] = 0.f; o[1] = 0.f; o[2] = 0.f; }
        return;
    }
    const size_t start = k ? t.end[k - 1] : 0;
    size_t end = t.end[k];
    if (end > n4) end = n4;
    double acc[2] = {0.0, 0.0};                              // {sum p^2, sum x^2}
    if (start < end) {
        size_t b_hi = (end - 1) / LW_CHUNK;
        if (b_hi > nblk - 1) b_hi = nblk - 1;
        for (size_t b = start / LW_CHUNK + lane; b <= b_hi; b += 64) { acc[0] += part[2 * (b + k)]; acc[1] += part[2 * (b + k) + 1]; }
    }
    wave_sum(acc);
    if (lane != 0) return;
    const double wn = sqrt(acc[0]), xn = sqrt(acc[1]);
    double ratio = 1.0;
    if (wn > 0.0 && xn > 0.0)
        ratio = LAMB ? wn / xn : (double)a.trust_coef * wn / (xn + (double)a.wd[grp] * wn + (double)a.lars_eps);
    if (a.max_trust > 0.f && ratio > (double)a.max_trust) ratio = (double)a.max_trust;
    if (t.adapt[k] == 0) ratio = 1.0;
    o[0] = (float)wn; o[1] = (float)xn; o[2] = (float)ratio;
}

template <typename Rule>
__global__ void __launch_bounds__(256) lw_apply_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ s0,
                                                       float* __restrict__ s1, TenTable t, GroupArgs<typename Rule::Params> a,
                                                       const float* __restrict__ dev_scale, const float* __restrict__ trust, size_t n4) {
    __shared__ uint32_t s_end[OPT_MAX_SEGS];
    __shared__ int s_grp[OPT_MAX_SEGS];
    __shared__ float s_ratio[OPT_MAX_SEGS];
    __shared__ typename Rule::Params s_par[OPT_MAX_GROUPS];
    const int cap = stage_table<Rule>(t.end, t.group, t.n_ten, s_end, s_grp,
                                      [&](int k, bool in) { s_ratio[k] = in ? trust[3 * k + 2] : 0.f; }, a, dev_scale, s_par);
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t b0 = (size_t)blockIdx.x * 256; b0 < n4; b0 += stride * OPT_VEC) {
        int gid[OPT_VEC], ten[OPT_VEC];
        pass_lookup(s_end, cap, b0, stride, n4, ten, EntryIndex{});
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const int grp = ten[u] >= 0 ? s_grp[ten[u]] : OPT_FROZEN;
            gid[u] = (unsigned)grp < (unsigned)t.n_groups ? grp : OPT_FROZEN;
        }
        float4 P[OPT_VEC], G[OPT_VEC] = {}, S0[OPT_VEC] = {}, S1[OPT_VEC] = {};
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = b0 + u * stride + threadIdx.x;
            if (gid[u] != OPT_FROZEN) {
                P[u] = reinterpret_cast<const float4*>(p)[i];
                if (!Rule::LAMB) G[u] = reinterpret_cast<const float4*>(g)[i];
                if (Rule::MOM && Rule::reads_state(s_par[0])) S0[u] = reinterpret_cast<const float4*>(s0)[i];
                if (Rule::LAMB) S1[u] = reinterpret_cast<const float4*>(s1)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = b0 + u * stride + threadIdx.x;
            if (gid[u] != OPT_FROZEN) {
                const typename Rule::Params q = s_par[gid[u]];
                const float r = s_ratio[ten[u]];
                Rule::apply(P[u].x, G[u].x, S0[u].x, S1[u].x, r, q); Rule::apply(P[u].y, G[u].y, S0[u].y, S1[u].y, r, q);
                Rule::apply(P[u].z, G[u].z, S0[u].z, S1[u].z, r, q); Rule::apply(P[u].w, G[u].w, S0[u].w, S1[u].w, r, q);
                reinterpret_cast<float4*>(p)[i] = P[u];
                if (!Rule::LAMB && Rule::MOM) reinterpret_cast<float4*>(s0)[i] = S0[u];
            }
        }
    }
}

static int layerwise_check(const char* what, const void* params, const void* grads, const void* s0, const void* s1, const uint32_t* ten_end,
                           const uint32_t* ten_len, const int32_t* ten_group, const int32_t* ten_adapt, int n_tensors, int n_groups,
                           const float* lr, const float* weight_decay, const float* dev_scale, float max_trust, const void* workspace,
                           const float* trust_out, size_t n) {
    if (int rc = flat_check(what, {params, grads, lr, weight_decay, workspace, trust_out}, {params, grads, s0, s1}, n)) return rc;
    if (int rc = table_check(what, "tensor", nullptr, n_tensors, {ten_end, ten_len, ten_group, ten_adapt}, &n_groups)) return rc;
    if ((uintptr_t)dev_scale & 3) BDN_FAIL(BDN_E_ARG, "%s: dev_scale must be 4-byte aligned", what);
    if ((uintptr_t)workspace & 7) BDN_FAIL(BDN_E_ARG, "%s: workspace must be 8-byte aligned", what);
    if ((uintptr_t)trust_out & 3) BDN_FAIL(BDN_E_ARG, "%s: trust_out must be 4-byte aligned", what);
    if (!(max_trust >= 0.f)) BDN_FAIL(BDN_E_ARG, "%s: max_trust = %g must be >= 0 (0: no clamp)", what, (double)max_trust);
    return BDN_OK;
}

extern "C" size_t bdn_layerwise_workspace_bytes(size_t n, int n_tensors) {
    const size_t slots = lw_blocks(n / 4) + (size_t)(n_tensors > 0 ? n_tensors : 0);
    return (slots ? slots : 1) * 2 * sizeof(double);
}

template <typename Rule>
static int layerwise_launch(const char* what, float* params, const float* grads, float* s0, float* s1, const TenTable& t,
                            const GroupArgs<typename Rule::Params>& a, const TrustArgs& ta, const float* dev_scale, void* workspace,
                            float* trust_out, size_t n, void* stream) {
    const size_t n4 = n / 4, nblk = lw_blocks(n4);
    hipLaunchKernelGGL(lw_partial_kernel<Rule>, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, (const float*)params, grads, s0, s1,
                       t, a, dev_scale, (double*)workspace, n4);
    BDN_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(lw_finish_kernel<Rule::LAMB>, dim3((unsigned)t.n_ten), dim3(64), 0, (hipStream_t)stream, (const double*)workspace, t, ta, nblk, n4,
                       trust_out);
    BDN_CHECK_LAUNCH(what);
    hipLaunchKernelGGL(lw_apply_kernel<Rule>, dim3(opt_grid(n4)), dim3(256), 0, (hipStream_t)stream, params, grads, s0, s1, t, a, dev_scale,
                       (const float*)trust_out, n4);
    BDN_CHECK_LAUNCH(what);
    return BDN_OK;
}

extern "C" int bdn_lamb_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, const uint32_t* ten_end,
                             const uint32_t* ten_len, const int32_t* ten_group, const int32_t* ten_adapt, int n_tensors, int n_groups,
                             const float* lr, const float* weight_decay, float grad_scale, const float* dev_scale, double beta1,
                             double beta2, float eps, float max_trust, long long step, void* workspace, float* trust_out, size_t n,
                             void* stream) {
    if (int rc = layerwise_check("lamb_step", params, grads, exp_avg, exp_avg_sq, ten_end, ten_len, ten_group, ten_adapt, n_tensors, n_groups,
                                 lr, weight_decay, dev_scale, max_trust, workspace, trust_out, n)) return rc;
    if (int rc = adam_rule_check("lamb_step", exp_avg, exp_avg_sq, step, beta1, beta2)) return rc;
    if (!(eps >= 0.f)) BDN_FAIL(BDN_E_ARG, "lamb_step: eps = %g must be >= 0", (double)eps);
    if (n == 0) return BDN_OK;
    GroupArgs<LambParams> a{};
    const double bc1 = 1.0 - std::pow(beta1, (double)step);
    for (int k = 0; k < n_groups; k++)
        a.g[k] = LambParams{adam_params(lr[k], weight_decay[k], grad_scale, beta1, beta2, eps, 1, step), (float)bc1, weight_decay[k], lr[k]};
    TrustArgs ta{};
    ta.max_trust = max_trust;
    const TenTable t{ten_end, ten_len, ten_group, ten_adapt, n_tensors, n_groups};
    return layerwise_launch<RuleLamb>("lamb_step", params, grads, exp_avg, exp_avg_sq, t, a, ta, dev_scale, workspace, trust_out, n, stream);
}

extern "C" int bdn_lars_step(float* params, const float* grads, float* momentum_buf, const uint32_t* ten_end, const uint32_t* ten_len,
                             const int32_t* ten_group, const int32_t* ten_adapt, int n_tensors, int n_groups, const float* lr,
                             const float* weight_decay, float grad_scale, const float* dev_scale, float momentum, float dampening,
                             int nesterov, int first_step, float trust_coef, float lars_eps, float max_trust, void* workspace,
                             float* trust_out, size_t n, void* stream) {
    if (int rc = layerwise_check("lars_step", params, grads, momentum_buf, nullptr, ten_end, ten_len, ten_group, ten_adapt, n_tensors,
                                 n_groups, lr, weight_decay, dev_scale, max_trust, workspace, trust_out, n)) return rc;
    if (int rc = sgdm_rule_check("lars_step", momentum, momentum_buf, dampening, nesterov)) return rc;
    if (!(trust_coef >= 0.f)) BDN_FAIL(BDN_E_ARG, "lars_step: trust_coef = %g must be >= 0", (double)trust_coef);
    if (!(lars_eps >= 0.f)) BDN_FAIL(BDN_E_ARG, "lars_step: lars_eps = %g must be >= 0", (double)lars_eps);
    if (n == 0) return BDN_OK;
    GroupArgs<LarsParams> a{};
    TrustArgs ta{};
    for (int k = 0; k < n_groups; k++) {
        a.g[k].s = sgdm_params(lr[k], weight_decay[k], grad_scale, momentum, dampening, nesterov, first_step);
        ta.wd[k] = weight_decay[k];
    }
    for (int k = n_groups; k < OPT_MAX_GROUPS; k++) a.g[k].s.first = first_step ? 1 : 0;      // reads_state() asks entry 0 only; keep all alike
    ta.trust_coef = trust_coef; ta.lars_eps = lars_eps; ta.max_trust = max_trust;
    const TenTable t{ten_end, ten_len, ten_group, ten_adapt, n_tensors, n_groups};
    if (momentum_buf)
        return layerwise_launch<RuleLars<true>>("lars_step", params, grads, momentum_buf, nullptr, t, a, ta, dev_scale, workspace, trust_out,
                                                n, stream);
    return layerwise_launch<RuleLars<false>>("lars_step", params, grads, nullptr, nullptr, t, a, ta, dev_scale, workspace, trust_out, n, stream);
}

// ============================================================ sharpness-aware minimisation: SAM (Foret et al. 2021), ASAM (Kwon et al. 2021)
// The ascent step w -> w + e of a SAM update and its undoing, on the layer-wise rules' per-tensor table (ten_end, ten_len, ten_group; no
// adapt flags, no groups: a group id >= 0 is trainable, OPT_FROZEN is not).  e = rho * t^2 * g / (||t * g|| + eps) with t = |w| (ASAM) or
// 1 (SAM); the norm runs over the real elements of every trainable tensor.  bdn_sam_perturb is three launches, fixed:
//   1 partial  grad_norm_partial_kernel's shape: block b owns the NORM_CHUNK vectors [b NORM_CHUNK, (b + 1) NORM_CHUNK) and writes ONE
//              double; a vector takes its tensor from the LDS table (one lookup per block where the chunk lies in one tensor), a frozen
//              vector or one behind the table is not read, and the last vector of a tensor is masked by the tensor's real length.
//   2 finish   one thread adds the partials in index order; out = {(float)norm, rho / (out[0] + eps)}, both float32.
//   3 apply    the update kernels' pass shape: saved = w, then w += ((out[1] * t) * t) * g on the real elements -- float32 products in
//              that order, one float32 add, none contracted.  A product that is exactly 0 leaves w's bits alone (-0.0 stays -0.0).
// bdn_sam_restore is one launch of the same pass shape that copies saved back: bits are moved, never computed.  Both passes move whole
// float4s; a pad element keeps its own bits throughout.
// stage_table's third array: the real elements of each tensor's last vector (4 without ten_len: bdn_sam_restore moves whole vectors)
struct SamTail {
    const uint32_t* __restrict__ ten_end;
    const uint32_t* __restrict__ ten_len;
    int* s_tail;
    __device__ __forceinline__ void operator()(int k, bool in) const {
        s_tail[k] = (in && ten_len) ? (int)(ten_len[k] - 4u * (ten_end[k] - 1u - (k ? ten_end[k - 1] : 0u))) : 4;
    }
};

// real elements of vector i in tensor s: 0 when it is frozen or lies behind the table (the vector is then neither read nor written)
__device__ __forceinline__ int sam_valid(const uint32_t* s_end, const int* s_grp, const int* s_tail, int s, size_t i) {
    if (!(s_end[s] > i) || s_grp[s] < 0) return 0;
    return i + 1 == s_end[s] ? s_tail[s] : 4;
}
struct SamValid {                                       // pass_lookup's entry: sam_valid of the vector's tensor
    const uint32_t* s_end;
    const int *s_grp, *s_tail;
    __device__ __forceinline__ int operator()(int s, size_t i) const { return sam_valid(s_end, s_grp, s_tail, s, i); }
};

template <bool ADAPT>
__device__ __forceinline__ double sam_acc(double acc, const float4& P, const float4& G, int nvalid) {
    double x0 = (double)G.x, x1 = (double)G.y, x2 = (double)G.z, x3 = (double)G.w;
    if (ADAPT) { x0 *= fabs((double)P.x); x1 *= fabs((double)P.y); x2 *= fabs((double)P.z); x3 *= fabs((double)P.w); }
    x0 = nvalid > 0 ? x0 : 0.0; x1 = nvalid > 1 ? x1 : 0.0; x2 = nvalid > 2 ? x2 : 0.0; x3 = nvalid > 3 ? x3 : 0.0;   // a pad is 0.0, whatever it holds
    acc = fma(x0, x0, acc); acc = fma(x1, x1, acc); acc = fma(x2, x2, acc); acc = fma(x3, x3, acc);
    return acc;
}

template <bool ADAPT>
__global__ void __launch_bounds__(256) sam_partial_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                          const uint32_t* __restrict__ ten_end, const uint32_t* __restrict__ ten_len,
                                                          const int32_t* __restrict__ ten_group, int n_ten, double* __restrict__ part, size_t n4) {
    __shared__ uint32_t s_end[OPT_MAX_SEGS];
    __shared__ int s_grp[OPT_MAX_SEGS], s_tail[OPT_MAX_SEGS];
    const int cap = stage_table(ten_end, ten_group, n_ten, s_end, s_grp, SamTail{ten_end, ten_len, s_tail});
    __syncthreads();
    const size_t c0 = (size_t)blockIdx.x * NORM_CHUNK, last = (c0 + NORM_CHUNK < n4 ? c0 + NORM_CHUNK : n4) - 1;
    const Span sp = chunk_span(s_end, cap, c0, last);
    const bool per_lane = sp.lo != sp.hi;                    // the chunk spans a tensor boundary: every vector looks its tensor up
    double acc[1] = {0.0};
    for (int r = 0; r < NORM_ROUNDS; r++) {
        int nv[OPT_VEC];
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = c0 + (size_t)(r * OPT_VEC + u) * 256 + threadIdx.x;
            nv[u] = 0;
            if (i < n4) {
                int s = sp.lo;
                if (per_lane) {
                    s = 0;
                    for (int h = cap >> 1; h > 0; h >>= 1) seg_step(s_end, h, (uint32_t)i, s);
                }
                nv[u] = sam_valid(s_end, s_grp, s_tail, s, i);
            }
        }
        float4 P[OPT_VEC] = {}, G[OPT_VEC] = {};
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = c0 + (size_t)(r * OPT_VEC + u) * 256 + threadIdx.x;
            if (nv[u] > 0) {
                G[u] = reinterpret_cast<const float4*>(g)[i];
                if (ADAPT) P[u] = reinterpret_cast<const float4*>(p)[i];
            }
        }
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) acc[0] = sam_acc<ADAPT>(acc[0], P[u], G[u], nv[u]);        // a vector not taken adds +0.0
    }
    block_sum(acc);
    if (threadIdx.x == 0) part[blockIdx.x] = acc[0];
}

__global__ void __launch_bounds__(256) sam_finish_kernel(const double* __restrict__ part, size_t nblk, float rho, float eps,
                                                         float* __restrict__ out) {
    __shared__ double s_part[1024];
    const double sum = sum_partials(part, nblk, s_part);
    if (threadIdx.x == 0) {
        const float norm32 = (float)sqrt(sum);
        out[0] = norm32;
        out[1] = rho / (norm32 + eps);
    }
}

template <bool ADAPT>
__device__ __forceinline__ float sam_elem(float w, float g, float scale) {
    float c = scale;
    if (ADAPT) { const float t = fabsf(w); c = __fmul_rn(__fmul_rn(scale, t), t); }
    const float e = __fmul_rn(c, g);
    return e == 0.f ? w : __fadd_rn(w, e);
}

template <bool ADAPT>
__global__ void __launch_bounds__(256) sam_apply_kernel(float* __restrict__ p, float* __restrict__ saved, const float* __restrict__ g,
                                                        const uint32_t* __restrict__ ten_end, const uint32_t* __restrict__ ten_len,
                                                        const int32_t* __restrict__ ten_group, int n_ten, const float* __restrict__ out,
                                                        size_t n4) {
    __shared__ uint32_t s_end[OPT_MAX_SEGS];
    __shared__ int s_grp[OPT_MAX_SEGS], s_tail[OPT_MAX_SEGS];
    const int cap = stage_table(ten_end, ten_group, n_ten, s_end, s_grp, SamTail{ten_end, ten_len, s_tail});
    __syncthreads();
    const float scale = out[1];
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t b0 = (size_t)blockIdx.x * 256; b0 < n4; b0 += stride * OPT_VEC) {
        int nv[OPT_VEC];                                     // the real elements of each of the pass's vectors (<= 0: not touched)
        pass_lookup(s_end, cap, b0, stride, n4, nv, SamValid{s_end, s_grp, s_tail});
        float4 P[OPT_VEC] = {}, G[OPT_VEC] = {};
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = b0 + u * stride + threadIdx.x;
            if (nv[u] > 0) { P[u] = reinterpret_cast<const float4*>(p)[i]; G[u] = reinterpret_cast<const float4*>(g)[i]; }
        }
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++) {
            const size_t i = b0 + u * stride + threadIdx.x;
            if (nv[u] > 0) {
                float4 w = P[u];
                w.x = sam_elem<ADAPT>(w.x, G[u].x, scale);
                if (nv[u] > 1) w.y = sam_elem<ADAPT>(w.y, G[u].y, scale);
                if (nv[u] > 2) w.z = sam_elem<ADAPT>(w.z, G[u].z, scale);
                if (nv[u] > 3) w.w = sam_elem<ADAPT>(w.w, G[u].w, scale);
                reinterpret_cast<float4*>(saved)[i] = P[u];
                reinterpret_cast<float4*>(p)[i] = w;
            }
        }
    }
}

__global__ void __launch_bounds__(256) sam_restore_kernel(float* __restrict__ p, const float* __restrict__ saved,
                                                          const uint32_t* __restrict__ ten_end, const int32_t* __restrict__ ten_group, int n_ten,
                                                          size_t n4) {
    __shared__ uint32_t s_end[OPT_MAX_SEGS];
    __shared__ int s_grp[OPT_MAX_SEGS], s_tail[OPT_MAX_SEGS];
    const int cap = stage_table(ten_end, ten_group, n_ten, s_end, s_grp, SamTail{ten_end, nullptr, s_tail});
    __syncthreads();
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t b0 = (size_t)blockIdx.x * 256; b0 < n4; b0 += stride * OPT_VEC) {
        int nv[OPT_VEC];
        pass_lookup(s_end, cap, b0, stride, n4, nv, SamValid{s_end, s_grp, s_tail});
        float4 S[OPT_VEC] = {};
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++)
            if (nv[u] > 0) S[u] = reinterpret_cast<const float4*>(saved)[b0 + u * stride + threadIdx.x];
#pragma unroll
        for (int u = 0; u < OPT_VEC; u++)
            if (nv[u] > 0) reinterpret_cast<float4*>(p)[b0 + u * stride + threadIdx.x] = S[u];
    }
}

static int sam_check(const char* what, const void* params, const void* saved, const uint32_t* ten_end, const int32_t* ten_group, int n_tensors,
                     size_t n) {
    if (int rc = flat_check(what, {params, saved}, {params, saved}, n)) return rc;
    if (params == saved) BDN_FAIL(BDN_E_ARG, "%s: params and saved are the same buffer", what);
    return table_check(what, "tensor", nullptr, n_tensors, {ten_end, ten_group}, nullptr);
}

extern "C" size_t bdn_sam_workspace_bytes(size_t n, int n_tensors) {
    (void)n_tensors;                                         // one partial per chunk, whatever the table
    return bdn_grad_norm_workspace_bytes(n);
}

extern "C" int bdn_sam_perturb(float* params, float* saved, const float* grads, const uint32_t* ten_end, const uint32_t* ten_len,
                               const int32_t* ten_group, int n_tensors, float rho, int adaptive, float eps, void* workspace, float* out,
                               size_t n, void* stream) {
    if (int rc = sam_check("sam_perturb", params, saved, ten_end, ten_group, n_tensors, n)) return rc;
    if (!grads || !ten_len || !workspace || !out) BDN_FAIL(BDN_E_ARG, "sam_perturb: null pointer");
    if ((uintptr_t)grads & 15) BDN_FAIL(BDN_E_ARG, "sam_perturb: buffers must be 16-byte aligned");
    if ((uintptr_t)ten_len & 3) BDN_FAIL(BDN_E_ARG, "sam_perturb: tensor table must be 4-byte aligned");
    if ((uintptr_t)workspace & 7) BDN_FAIL(BDN_E_ARG, "sam_perturb: workspace must be 8-byte aligned");
    if ((uintptr_t)out & 3) BDN_FAIL(BDN_E_ARG, "sam_perturb: out must be 4-byte aligned");
    if (!(rho > 0.f)) BDN_FAIL(BDN_E_ARG, "sam_perturb: rho = %g must be > 0", (double)rho);
    if (!(eps >= 0.f)) BDN_FAIL(BDN_E_ARG, "sam_perturb: eps = %g must be >= 0", (double)eps);
    if (adaptive != 0 && adaptive != 1) BDN_FAIL(BDN_E_ARG, "sam_perturb: adaptive must be 0 or 1, got %d", adaptive);
    if (n == 0) return BDN_OK;
    const size_t n4 = n / 4, nblk = norm_blocks(n4);
    hipStream_t st = (hipStream_t)stream;
    if (adaptive) {
        hipLaunchKernelGGL(sam_partial_kernel<true>, dim3((unsigned)nblk), dim3(256), 0, st, (const float*)params, grads, ten_end, ten_len,
                           ten_group, n_tensors, (double*)workspace, n4);
    } else {
        hipLaunchKernelGGL(sam_partial_kernel<false>, dim3((unsigned)nblk), dim3(256), 0, st, (const float*)params, grads, ten_end, ten_len,
                           ten_group, n_tensors, (double*)workspace, n4);
    }
    BDN_CHECK_LAUNCH("sam_perturb");
    hipLaunchKernelGGL(sam_finish_kernel, dim3(1), dim3(256), 0, st, (const double*)workspace, nblk, rho, eps, out);
    BDN_CHECK_LAUNCH("sam_perturb");
    if (adaptive) {
        hipLaunchKernelGGL(sam_apply_kernel<true>, dim3(opt_grid(n4)), dim3(256), 0, st, params, saved, grads, ten_end, ten_len, ten_group,
                           n_tensors, (const float*)out, n4);
    } else {
        hipLaunchKernelGGL(sam_apply_kernel<false>, dim3(opt_grid(n4)), dim3(256), 0, st, params, saved, grads, ten_end, ten_len, ten_group,
                           n_tensors, (const float*)out, n4);
    }
    BDN_CHECK_LAUNCH("sam_perturb");
    return BDN_OK;
}

extern "C" int bdn_sam_restore(float* params, const float* saved, const uint32_t* ten_end, const int32_t* ten_group, int n_tensors, size_t n,
                               void* stream) {
    if (int rc = sam_check("sam_restore", params, saved, ten_end, ten_group, n_tensors, n)) return rc;
    if (n == 0) return BDN_OK;
    hipLaunchKernelGGL(sam_restore_kernel, dim3(opt_grid(n / 4)), dim3(256), 0, (hipStream_t)stream, params, saved, ten_end, ten_group,
                       n_tensors, n / 4);
    BDN_CHECK_LAUNCH("sam_restore");
    return BDN_OK;
}
