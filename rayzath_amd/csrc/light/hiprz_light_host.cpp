// hiprz_light_host.cpp — the pure-host half of light baking (hiprz_light_host.hpp) and the host-only calls of include/hiprz_light.h.
// No HIP header.
#include "hiprz_light_host.hpp"

#include <cmath>
#include <cstddef>

#include "../query/hiprz_query_staging.hpp"
#include "hiprz_light.h"

namespace hiprz {

const char* light_table_refusal(const float* xy, uint32_t K, uint32_t S) {
    if (!xy) return "null pointer";
    if (!light_k_allowed(K)) return "K is not a power of two in 1..1024";
    if (!light_s_allowed(S)) return "S is not in 1..64";
    for (size_t i = 0; i < size_t(K) * S; ++i) {
        const float x = xy[2 * i], y = xy[2 * i + 1];
        if (!std::isfinite(x) || !std::isfinite(y)) return "a sample is not finite";
        const float xx = x * x, yy = y * y;  // (named: each product is rounded to float before the sum, whatever the host contracts)
        const float sq = xx + yy;
        if (sq > 1.0f) return "a sample lies outside the unit disk";
    }
    return nullptr;
}

const char* light_refusal(bool any_null, size_t n, uint32_t K, int* code) {
    *code = HIPRZ_ERR_INVALID;
    if (any_null) return "null pointer";
    *code = HIPRZ_ERR_STATE;
    if (K == 0u) return "no sample table has been set";
    *code = HIPRZ_ERR_INVALID;
    if (n >= kLightMaxRays / K) return "n*K is 2^31 or more";  // (K divides 2^31; no product that could wrap)
    *code = HIPRZ_OK;
    return nullptr;
}

const char* light_range_refusal(const hiprz_light_range* range, uint32_t n_spot, uint32_t n_direct, LightSpan* out) {
    *out = LightSpan{0u, n_spot, 0u, n_direct};
    if (!range) return nullptr;
    if (range->spot_first > n_spot) return "the range starts behind the last spot light";
    if (range->direct_first > n_direct) return "the range starts behind the last direct light";
    const uint32_t spots_left = n_spot - range->spot_first, directs_left = n_direct - range->direct_first;
    if (range->spot_count != HIPRZ_LIGHT_TO_END && range->spot_count > spots_left) return "the range ends behind the last spot light";
    if (range->direct_count != HIPRZ_LIGHT_TO_END && range->direct_count > directs_left) return "the range ends behind the last direct light";
    out->spot_first = range->spot_first, out->spots = range->spot_count == HIPRZ_LIGHT_TO_END ? spots_left : range->spot_count;
    out->direct_first = range->direct_first, out->directs = range->direct_count == HIPRZ_LIGHT_TO_END ? directs_left : range->direct_count;
    return nullptr;
}

const char* light_rays_refusal(size_t n, uint32_t K, uint32_t L) {
    if (L != 0u && n * K >= (kLightMaxRays + L - 1u) / L) return "n*L*K is 2^31 or more";  // n*K < 2^31: the product does not wrap
    return nullptr;
}

size_t light_capacity(size_t have, size_t need) { return staging_capacity(have, need, kLightMaxPoints); }

}  // namespace hiprz

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_light_texel) == 16 && sizeof(hiprz_light_range) == 16,
              "two 16-byte loads per point, one 16-byte store per texel");

extern "C" {

uint32_t hiprz_light_set_of(uint32_t i, uint32_t seed, uint32_t S) { return S ? hiprz::light_hash(i ^ seed) % S : 0u; }

int hiprz_light_disk_samples(uint32_t K, uint32_t S, float* xy_out) {
    if (!xy_out || !hiprz::light_k_allowed(K) || !hiprz::light_s_allowed(S)) return HIPRZ_ERR_INVALID;
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t k = 0; k < K; ++k) {
            const double r = std::sqrt((double(k) + 0.5) / double(K));
            const double turn = double(k) * 0.6180339887498949;
            const double phi = two_pi * ((turn - std::floor(turn)) + double(s) / double(S));
            float* o = xy_out + 2 * (size_t(s) * K + k);
            o[0] = float(r * std::cos(phi)), o[1] = float(r * std::sin(phi));
        }
    return HIPRZ_OK;
}

void hiprz_light_layout(uint32_t out[6]) {
    if (!out) return;
    out[0] = uint32_t(sizeof(hiprz_bake_point)), out[1] = uint32_t(sizeof(hiprz_light_texel)), out[2] = uint32_t(sizeof(hiprz_light_range));
    out[3] = uint32_t(offsetof(hiprz_light_texel, light)), out[4] = uint32_t(offsetof(hiprz_light_texel, shadowed));
    out[5] = uint32_t(offsetof(hiprz_light_range, direct_first));
}

}  // extern "C"
