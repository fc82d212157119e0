// hiprz_field_host.cpp — the pure-host half of probe fields (hiprz_field_host.hpp) and the host-only calls of include/hiprz_field.h.
// No HIP header.
#include "hiprz_field_host.hpp"

#include <cmath>
#include <cstddef>

#include "../query/hiprz_query_staging.hpp"
#include "hiprz_field.h"

namespace hiprz {

const char* field_table_refusal(const float* xyz0, uint32_t K, uint32_t S) {
    if (!xyz0) return "null pointer";
    if (!field_k_allowed(K)) return "K is not one of 64, 128, 256, 512, 1024";
    if (!field_s_allowed(S)) return "S is not in 1..64";
    for (size_t i = 0; i < size_t(K) * S; ++i) {
        const float x = xyz0[4 * i], y = xyz0[4 * i + 1], z = xyz0[4 * i + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return "a direction is not finite";
        const float xx = x * x, yy = y * y, zz = z * z;  // (named: each product is rounded to float before the sums, whatever the host contracts)
        const float xy = xx + yy, sq = xy + zz;
        if (!(sq >= 0.999f && sq <= 1.001f)) return "a direction is not of unit length (squared length outside [0.999, 1.001])";
    }
    return nullptr;
}

const char* field_visibility_refusal(bool any_null, size_t n, uint32_t K, float reach, int* code) {
    *code = HIPRZ_ERR_INVALID;
    if (any_null) return "null pointer";
    *code = HIPRZ_ERR_STATE;
    if (K == 0u) return "no direction table has been set";
    *code = HIPRZ_ERR_INVALID;
    if (n >= kFieldMaxRays / K) return "n*K is 2^31 or more";  // (K divides 2^31; no product that could wrap)
    if (!std::isfinite(reach) || !(reach > 0.0f)) return "reach is not a finite number > 0";
    *code = HIPRZ_OK;
    return nullptr;
}

const char* field_grid_refusal(const hiprz_field_grid* grid, size_t n_probes) {
    if (!grid) return "null grid";
    size_t product = 1u;
    for (int a = 0; a < 3; ++a) {
        if (grid->n[a] < 1u) return "a grid count is 0";
        if (grid->n[a] >= kFieldMaxPoints / product) return "the grid has 2^31 probes or more";  // (product <= 2^31 - 1: no wrap)
        product *= grid->n[a];
    }
    if (product != n_probes) return "the grid's counts do not multiply to the number of probes";
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(grid->lo[a])) return "the grid's corner is not finite";
        if (grid->n[a] > 1u && (!std::isfinite(grid->step[a]) || !(grid->step[a] > 0.0f))) return "a grid step is not a finite number > 0";
    }
    return nullptr;
}

const char* field_params_refusal(const hiprz_field_params* params) {
    if (!params) return "null params";
    if (!std::isfinite(params->bias) || !(params->bias >= 0.0f)) return "bias is not a finite number >= 0";
    return nullptr;
}

const char* field_lookup_refusal(bool any_null, const hiprz_field_grid* grid, size_t n_probes, const hiprz_field_params* params, size_t m) {
    if (any_null) return "null pointer";
    if (const char* why = field_grid_refusal(grid, n_probes)) return why;
    if (const char* why = field_params_refusal(params)) return why;
    if (m >= kFieldMaxPoints) return "2^31 points or more";
    return nullptr;
}

size_t field_capacity(size_t have, size_t need) { return staging_capacity(have, need, kFieldMaxPoints); }

}  // namespace hiprz

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_probe_sh) == 144 && sizeof(hiprz_field_vis) == 528 && sizeof(hiprz_field_grid) == 40 &&
                  sizeof(hiprz_field_params) == 16 && sizeof(hiprz_field_result) == 16,
              "two 16-byte loads per point, 33 per visibility record, one 16-byte store per result");

extern "C" {

int hiprz_field_texel_directions(float out[64][4]) {
    if (!out) return HIPRZ_ERR_INVALID;
    for (int iy = 0; iy < 8; ++iy)
        for (int ix = 0; ix < 8; ++ix) {
            const double ex = (double(ix) + 0.5) / 4.0 - 1.0, ey = (double(iy) + 0.5) / 4.0 - 1.0;
            const double z = 1.0 - std::fabs(ex) - std::fabs(ey);
            double x = ex, y = ey;
            if (z < 0.0) {
                x = (1.0 - std::fabs(ey)) * (ex < 0.0 ? -1.0 : 1.0);
                y = (1.0 - std::fabs(ex)) * (ey < 0.0 ? -1.0 : 1.0);
            }
            const double len = std::sqrt(x * x + y * y + z * z);
            float* o = out[8 * iy + ix];
            o[0] = float(x / len), o[1] = float(y / len), o[2] = float(z / len), o[3] = 0.0f;
        }
    return HIPRZ_OK;
}

int hiprz_field_check_grid(const hiprz_field_grid* grid, size_t n_probes) { return hiprz::field_grid_refusal(grid, n_probes) ? HIPRZ_ERR_INVALID : HIPRZ_OK; }

int hiprz_field_check_params(const hiprz_field_params* params) { return hiprz::field_params_refusal(params) ? HIPRZ_ERR_INVALID : HIPRZ_OK; }

void hiprz_field_layout(uint32_t out[8]) {
    if (!out) return;
    out[0] = uint32_t(sizeof(hiprz_bake_point)), out[1] = uint32_t(sizeof(hiprz_probe_sh)), out[2] = uint32_t(sizeof(hiprz_field_vis));
    out[3] = uint32_t(sizeof(hiprz_field_grid)), out[4] = uint32_t(sizeof(hiprz_field_params)), out[5] = uint32_t(sizeof(hiprz_field_result));
    out[6] = uint32_t(offsetof(hiprz_field_vis, words)), out[7] = uint32_t(RZ_FIELD_LOOKUP_WG);
}

}  // extern "C"
