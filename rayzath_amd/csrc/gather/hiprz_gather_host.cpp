// hiprz_gather_host.cpp — the pure-host half of bounce baking (hiprz_gather_host.hpp) and the host-only call of include/hiprz_gather.h.
// No HIP header.
#include "hiprz_gather_host.hpp"

#include <cmath>
#include <cstddef>

#include "../query/hiprz_query_staging.hpp"
#include "hiprz_gather.h"

namespace hiprz {

const char* gather_table_refusal(const float* xyz0, uint32_t K, uint32_t S) {
    if (!xyz0) return "null pointer";
    if (!gather_k_allowed(K)) return "K is not one of 16, 32, 64, 128, 256, 512, 1024";
    if (!gather_s_allowed(S)) return "S is not in 1..64";
    for (size_t i = 0; i < size_t(K) * S; ++i) {
        const float x = xyz0[4 * i], y = xyz0[4 * i + 1], z = xyz0[4 * i + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return "a direction is not finite";
        const float xx = x * x, yy = y * y, zz = z * z;  // (named: each product is rounded to float before the sums, whatever the host contracts)
        const float xy = xx + yy, sq = xy + zz;
        if (!(sq >= 0.999f && sq <= 1.001f)) return "a direction is not of unit length (squared length outside [0.999, 1.001])";
    }
    return nullptr;
}

const char* gather_charts_refusal(const uint32_t* base, uint32_t n_instances, const hiprz_gather_chart* uv, uint32_t n_charts) {
    if ((!base && n_instances != 0u) || (!uv && n_charts != 0u)) return "null pointer";
    if (n_charts > HIPRZ_GATHER_MAX_CHARTS) return "more charts than there are ids below the codes";
    for (size_t i = 0; i < n_charts; ++i) {
        const hiprz_gather_chart& c = uv[i];
        if (!std::isfinite(c.u1) || !std::isfinite(c.v1) || !std::isfinite(c.u2) || !std::isfinite(c.v2) || !std::isfinite(c.u3) || !std::isfinite(c.v3))
            return "a chart's UV is not finite";
    }
    return nullptr;
}

const char* gather_refusal(bool any_null, size_t n, uint32_t K, bool has_charts, int* code) {
    *code = HIPRZ_ERR_INVALID;
    if (any_null) return "null pointer";
    *code = HIPRZ_ERR_STATE;
    if (K == 0u) return "no direction table has been set";
    if (!has_charts) return "no chart map has been set";
    *code = HIPRZ_ERR_INVALID;
    if (n >= kGatherMaxRays / K) return "n*K is 2^31 or more";  // (K divides 2^31; no product that could wrap)
    *code = HIPRZ_OK;
    return nullptr;
}

const char* gather_size_refusal(uint32_t W, uint32_t H) {
    if (W < 1u || W > HIPRZ_GATHER_MAX_SIZE || H < 1u || H > HIPRZ_GATHER_MAX_SIZE) return "W or H is not in 1..16384";
    return nullptr;
}

const char* gather_compose_refusal(bool any_null, size_t n_texels) {
    if (any_null) return "null pointer";
    if (n_texels >= kGatherMaxRays) return "2^31 texels or more";
    return nullptr;
}

size_t gather_capacity(size_t have, size_t need) { return staging_capacity(have, need, kGatherMaxPoints); }

}  // namespace hiprz

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_gather_texel) == 16 && sizeof(hiprz_gather_sample) == 16 && sizeof(hiprz_gather_chart) == 32,
              "two 16-byte loads per point and chart, one 16-byte store per texel and sample");

extern "C" {

void hiprz_gather_layout(uint32_t out[8]) {
    if (!out) return;
    out[0] = uint32_t(sizeof(hiprz_bake_point)), out[1] = uint32_t(sizeof(hiprz_gather_texel)), out[2] = uint32_t(sizeof(hiprz_gather_sample));
    out[3] = uint32_t(sizeof(hiprz_gather_chart)), out[4] = uint32_t(offsetof(hiprz_gather_texel, counts));
    out[5] = uint32_t(offsetof(hiprz_gather_sample, bx)), out[6] = uint32_t(offsetof(hiprz_gather_sample, t)), out[7] = uint32_t(offsetof(hiprz_gather_chart, u3));
}

}  // extern "C"
