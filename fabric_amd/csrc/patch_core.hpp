// What scene.hip (bdn_sample_patches and its augmenting kin) and mix.hip share: the city record the descriptors index, the output tile
// every patch kernel works on, and the host check behind every address a kernel forms from a descriptor.
#pragma once
#include "common.hpp"

struct SampleCity { const float* images; const uint8_t* labels; int32_t H, W; };       // bdn_sample_patches' city record, 24 bytes

constexpr int SP_TILE = 64, SP_WAVES = 4, SP_ROWS = SP_TILE / SP_WAVES;

// city_hw_host: int32 [n_cities][2] = (H, W); desc_host: int32 [n][4] = (city, row, col, sym).  Every S x S window must lie inside its
// city and sym in 0..7.  n, S and n_cities are positive (the caller's check); `who` names the entry in the message.
static int patch_desc_check(const char* who, const int32_t* city_hw_host, int n_cities, const int32_t* desc_host, int n, int S) {
    for (int k = 0; k < n_cities; k++)
        if (city_hw_host[2 * k] <= 0 || city_hw_host[2 * k + 1] <= 0)
            BDN_FAIL(BDN_E_SHAPE, "%s: city %d has shape %d x %d", who, k, city_hw_host[2 * k], city_hw_host[2 * k + 1]);
    for (int k = 0; k < n; k++) {                            // every address the kernel forms comes from a descriptor checked here
        const int32_t* e = desc_host + 4 * (size_t)k;
        const int city = e[0], row = e[1], col = e[2], sym = e[3];
        if (city < 0 || city >= n_cities) BDN_FAIL(BDN_E_ARG, "%s: descriptor %d: city %d outside [0, %d)", who, k, city, n_cities);
        if (sym < 0 || sym > 7) BDN_FAIL(BDN_E_ARG, "%s: descriptor %d: sym %d outside [0, 8)", who, k, sym);
        const long long H = city_hw_host[2 * city], W = city_hw_host[2 * city + 1];
        if (row < 0 || (long long)row + S > H)
            BDN_FAIL(BDN_E_ARG, "%s: descriptor %d: row %d + S %d outside H %lld of city %d", who, k, row, S, H, city);
        if (col < 0 || (long long)col + S > W)
            BDN_FAIL(BDN_E_ARG, "%s: descriptor %d: col %d + S %d outside W %lld of city %d", who, k, col, S, W, city);
    }
    return BDN_OK;
}
