// hiprz_bake_host.cpp — the pure-host half of occlusion baking (hiprz_bake_host.hpp) and the host-only calls of include/hiprz_bake.h.
// No HIP header.
#include "hiprz_bake_host.hpp"

#include <cmath>
#include <cstddef>

#include "../query/hiprz_query_staging.hpp"
#include "hiprz_bake.h"

namespace hiprz {

const char* bake_table_refusal(const float* xyz0, uint32_t K, uint32_t S) {
    if (!xyz0) return "null pointer";
    if (!bake_k_allowed(K)) return "K is not one of 16, 32, 64, 128, 256, 512, 1024";
    if (!bake_s_allowed(S)) return "S is not in 1..64";
    for (size_t i = 0; i < size_t(K) * S; ++i) {
        const float x = xyz0[4 * i], y = xyz0[4 * i + 1], z = xyz0[4 * i + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return "a direction is not finite";
        const float xx = x * x, yy = y * y, zz = z * z;  // (named: each product is rounded to float before the sums, whatever the host contracts)
        const float xy = xx + yy, sq = xy + zz;
        if (!(sq >= 0.999f && sq <= 1.001f)) return "a direction is not of unit length (squared length outside [0.999, 1.001])";
    }
    return nullptr;
}

const char* bake_refusal(bool any_null, size_t n, uint32_t K, int* code) {
    *code = HIPRZ_ERR_INVALID;
    if (any_null) return "null pointer";
    *code = HIPRZ_ERR_STATE;
    if (K == 0u) return "no direction table has been set";
    *code = HIPRZ_ERR_INVALID;
    if (n >= kBakeMaxRays / K) return "n*K is 2^31 or more";  // (K divides 2^31; no product that could wrap)
    *code = HIPRZ_OK;
    return nullptr;
}

size_t bake_capacity(size_t have, size_t need) { return staging_capacity(have, need, kBakeMaxPoints); }

}  // namespace hiprz

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_bake_texel) == 16, "two 16-byte loads per point, one 16-byte store per texel");
static_assert(offsetof(hiprz_bake_point, normal) == offsetof(hiprz_ray, direction) && offsetof(hiprz_bake_point, far_) == offsetof(hiprz_ray, far_),
              "a point is the ray along its normal");

extern "C" {

uint32_t hiprz_bake_set_of(uint32_t i, uint32_t seed, uint32_t S) { return S ? hiprz::bake_hash(i ^ seed) % S : 0u; }

int hiprz_bake_cosine_directions(uint32_t K, uint32_t S, float* xyz0_out) {
    if (!xyz0_out || !hiprz::bake_k_allowed(K) || !hiprz::bake_s_allowed(S)) return HIPRZ_ERR_INVALID;
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t k = 0; k < K; ++k) {
            const double u = (double(k) + 0.5) / double(K), r = std::sqrt(u);
            const double turn = double(k) * 0.6180339887498949;
            const double phi = two_pi * ((turn - std::floor(turn)) + double(s) / double(S));
            float* o = xyz0_out + 4 * (size_t(s) * K + k);
            o[0] = float(r * std::cos(phi)), o[1] = float(r * std::sin(phi)), o[2] = float(std::sqrt(1.0 - u)), o[3] = 0.0f;
        }
    return HIPRZ_OK;
}

void hiprz_bake_layout(uint32_t out[6]) {
    if (!out) return;
    out[0] = uint32_t(sizeof(hiprz_bake_point)), out[1] = uint32_t(sizeof(hiprz_bake_texel));
    out[2] = uint32_t(offsetof(hiprz_bake_point, normal)), out[3] = uint32_t(offsetof(hiprz_bake_point, far_));
    out[4] = uint32_t(offsetof(hiprz_bake_texel, bent)), out[5] = uint32_t(offsetof(hiprz_bake_texel, occluded));
}

}  // extern "C"
