// hiprz_place_host.cpp — the pure-host half of probe placement (hiprz_place_host.hpp) and the host-only calls of include/hiprz_place.h.
// No HIP header.
#include "hiprz_place_host.hpp"

#include <cmath>
#include <cstddef>

#include "../query/hiprz_query_staging.hpp"
#include "hiprz_place.h"

namespace hiprz {

const char* place_table_refusal(const float* xyz0, uint32_t K, uint32_t S) {
    if (!xyz0) return "null pointer";
    if (!place_k_allowed(K)) return "K is not one of 64, 128, 256, 512, 1024";
    if (!place_s_allowed(S)) return "S is not in 1..64";
    for (size_t i = 0; i < size_t(K) * S; ++i) {
        const float x = xyz0[4 * i], y = xyz0[4 * i + 1], z = xyz0[4 * i + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return "a direction is not finite";
        const float xx = x * x, yy = y * y, zz = z * z;  // (named: each product is rounded to float before the sums, whatever the host contracts)
        const float xy = xx + yy, sq = xy + zz;
        if (!(sq >= 0.999f && sq <= 1.001f)) return "a direction is not of unit length (squared length outside [0.999, 1.001])";
    }
    return nullptr;
}

const char* place_params_refusal(const hiprz_place_params* params) {
    if (!params) return "null params";
    if (!std::isfinite(params->min_front) || !(params->min_front > 0.0f)) return "min_front is not a finite number > 0";
    if (!std::isfinite(params->reach) || !(params->reach > 0.0f)) return "reach is not a finite number > 0";
    for (int a = 0; a < 3; ++a)
        if (!std::isfinite(params->max_offset[a]) || !(params->max_offset[a] >= 0.0f)) return "a max_offset is not a finite number >= 0";
    if (params->iterations > HIPRZ_PLACE_MAX_ITERATIONS) return "iterations is above 16";
    if (params->reserved != 0u) return "reserved is not 0";
    return nullptr;
}

const char* place_probes_refusal(bool any_null, size_t n, uint32_t K, const hiprz_place_params* params, int* code) {
    *code = HIPRZ_ERR_INVALID;
    if (any_null) return "null pointer";
    *code = HIPRZ_ERR_STATE;
    if (K == 0u) return "no direction table has been set";
    *code = HIPRZ_ERR_INVALID;
    if (n >= kPlaceMaxRays / K) return "n*K is 2^31 or more";  // (K divides 2^31; no product that could wrap)
    if (const char* why = place_params_refusal(params)) return why;
    *code = HIPRZ_OK;
    return nullptr;
}

size_t place_capacity(size_t have, size_t need) { return staging_capacity(have, need, kPlaceMaxProbes); }

}  // namespace hiprz

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_place_params) == 32 && sizeof(hiprz_place_record) == 32, "two 16-byte words per probe, params and record");

extern "C" {

int hiprz_place_check_params(const hiprz_place_params* params) { return hiprz::place_params_refusal(params) ? HIPRZ_ERR_INVALID : HIPRZ_OK; }

void hiprz_place_layout(uint32_t out[8]) {
    if (!out) return;
    out[0] = uint32_t(sizeof(hiprz_bake_point)), out[1] = uint32_t(sizeof(hiprz_place_params)), out[2] = uint32_t(sizeof(hiprz_place_record));
    out[3] = uint32_t(offsetof(hiprz_place_params, max_offset)), out[4] = uint32_t(offsetof(hiprz_place_params, iterations));
    out[5] = uint32_t(offsetof(hiprz_place_params, max_back)), out[6] = uint32_t(offsetof(hiprz_place_record, word));
    out[7] = uint32_t(offsetof(hiprz_place_record, front));
}

}  // extern "C"
