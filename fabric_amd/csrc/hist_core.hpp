// What the histogram kernels share (curve.hip: bdn_score_hist; thresh.hip: bdn_raster_hist): the wave-aggregated add into a block's LDS
// histogram, and the one-pixel / four-pixel item loads.
#pragma once
#include "common.hpp"

// One add of the wave's pixels into the block's LDS histogram.  key = the cell, or < 0 for a lane without a pixel (tail, ignored).  On
// real data nearly every pixel lands in one cell (score_hist: a negative in bin 0), and 64 LDS atomics on one address serialise; so the
// wave first peels off, twice, the lanes that share the key of its first pending lane (a ballot and one add of their count by that lane) --
// all-equal waves need one add, a wave with a dominant cell and a few strays two -- and only the lanes still pending add for themselves.
// Must be called by all 64 lanes of the wave together.
__device__ __forceinline__ void wave_hist_add(unsigned* lds, int key, int lane) {
    bool pending = key >= 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const unsigned long long act = __ballot(pending);
        if (!act) return;                                                    // wave-uniform
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
        const int k = __builtin_amdgcn_readlane(key, leader);
        const bool mine = pending && key == k;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&lds[k], (unsigned)__popcll(same));
        pending = pending && !mine;
    }
    if (pending) atomicAdd(&lds[key], 1u);
}

template <int PER> struct PixVec;
template <> struct PixVec<1> {
    __device__ __forceinline__ static void load(const float* p, float* v) { v[0] = p[0]; }
    __device__ __forceinline__ static void store(float* p, const float* v) { p[0] = v[0]; }
    __device__ __forceinline__ static void labels(const uint8_t* p, int* l) { l[0] = p[0]; }
};
template <> struct PixVec<4> {
    __device__ __forceinline__ static void load(const float* p, float* v) {
        const float4 u = *reinterpret_cast<const float4*>(p);
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    }
    __device__ __forceinline__ static void store(float* p, const float* v) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
    __device__ __forceinline__ static void labels(const uint8_t* p, int* l) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
        l[0] = u & 255; l[1] = u >> 8 & 255; l[2] = u >> 16 & 255; l[3] = u >> 24;
    }
};
