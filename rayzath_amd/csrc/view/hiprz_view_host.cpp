// hiprz_view_host.cpp — the pure-host half of the baked view (hiprz_view_host.hpp) and the host-only calls of include/hiprz_view.h.
// No HIP header.
#include "hiprz_view_host.hpp"

#include <cmath>
#include <cstddef>

#include "../query/hiprz_query_staging.hpp"
#include "hiprz_view.h"

namespace hiprz {

const char* view_charts_refusal(const uint32_t* base, uint32_t n_instances, const hiprz_gather_chart* uv, uint32_t n_charts) {
    if ((!base && n_instances != 0u) || (!uv && n_charts != 0u)) return "null pointer";
    if (n_charts > HIPRZ_GATHER_MAX_CHARTS) return "more charts than there are ids below the codes";
    for (size_t i = 0; i < n_charts; ++i) {
        const hiprz_gather_chart& c = uv[i];
        if (!std::isfinite(c.u1) || !std::isfinite(c.v1) || !std::isfinite(c.u2) || !std::isfinite(c.v2) || !std::isfinite(c.u3) || !std::isfinite(c.v3))
            return "a chart's UV is not finite";
    }
    return nullptr;
}

const char* view_params_refusal(const hiprz_view_params* params) {
    if (!params) return "null params";
    if (params->filter != HIPRZ_VIEW_NEAREST && params->filter != HIPRZ_VIEW_BILINEAR) return "filter is neither NEAREST nor BILINEAR";
    if (params->reserved[0] != 0u || params->reserved[1] != 0u || params->reserved[2] != 0u) return "reserved is not 0";
    return nullptr;
}

const char* view_grid_refusal(const hiprz_field_grid* grid, size_t n_probes) {
    if (!grid) return "null grid";
    size_t product = 1u;
    for (int a = 0; a < 3; ++a) {
        if (grid->n[a] < 1u) return "a grid count is 0";
        if (grid->n[a] >= kViewMaxProbes / product) return "the grid has 2^31 probes or more";  // (product <= 2^31 - 1: no wrap)
        product *= grid->n[a];
    }
    if (product != n_probes) return "the grid's counts do not multiply to the number of probes";
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(grid->lo[a])) return "the grid's corner is not finite";
        if (grid->n[a] > 1u && (!std::isfinite(grid->step[a]) || !(grid->step[a] > 0.0f))) return "a grid step is not a finite number > 0";
    }
    return nullptr;
}

const char* view_field_params_refusal(const hiprz_field_params* params) {
    if (!params) return "null params";
    if (!std::isfinite(params->bias) || !(params->bias >= 0.0f)) return "bias is not a finite number >= 0";
    return nullptr;
}

const char* view_refusal(bool any_null, bool has_charts, uint32_t W, uint32_t H, const hiprz_view_params* params, const hiprz_view_field* field, int* code) {
    *code = HIPRZ_ERR_INVALID;
    if (any_null || (field && (!field->grid || !field->probes || !field->sh))) return "null pointer";
    *code = HIPRZ_ERR_STATE;
    if (!has_charts) return "no chart map has been set";
    *code = HIPRZ_ERR_INVALID;
    if (W < 1u || W > HIPRZ_GATHER_MAX_SIZE || H < 1u || H > HIPRZ_GATHER_MAX_SIZE) return "W or H is not in 1..16384";
    if (params)
        if (const char* why = view_params_refusal(params)) return why;
    if (field) {
        if (const char* why = view_grid_refusal(field->grid, field->n_probes)) return why;
        if (field->params)
            if (const char* why = view_field_params_refusal(field->params)) return why;
    }
    *code = HIPRZ_OK;
    return nullptr;
}

const char* view_pixels_refusal(uint32_t width, uint32_t height) {
    if (size_t(width) * height > kViewMaxPixels) return "more than 2^31 - 1 pixels";
    return nullptr;
}

uint32_t view_groups(uint32_t width, uint32_t height, bool rows) {
    if (rows) return uint32_t((size_t(width) * height + 63u) / 64u);
    return uint32_t(size_t((width + 7u) / 8u) * ((height + 7u) / 8u));  // (at most 2^31 - 1 pixels: fewer than 2^26 + 2^29 blocks)
}

size_t view_capacity(size_t have, size_t need) { return staging_capacity(have, need, kViewMaxPixels); }

}  // namespace hiprz

static_assert(sizeof(hiprz_view_pixel) == 16 && sizeof(hiprz_view_params) == 16 && sizeof(hiprz_view_field) == 48 && sizeof(hiprz_gather_sample) == 16 &&
                  sizeof(hiprz_gather_chart) == 32,
              "one 16-byte store per pixel and sample, two 16-byte loads per chart");

extern "C" {

int hiprz_view_check_params(const hiprz_view_params* params) { return hiprz::view_params_refusal(params) ? HIPRZ_ERR_INVALID : HIPRZ_OK; }

void hiprz_view_layout(uint32_t out[8]) {
    if (!out) return;
    out[0] = uint32_t(sizeof(hiprz_view_pixel)), out[1] = uint32_t(sizeof(hiprz_view_params)), out[2] = uint32_t(sizeof(hiprz_view_field));
    out[3] = uint32_t(sizeof(hiprz_gather_sample)), out[4] = uint32_t(sizeof(hiprz_gather_chart)), out[5] = uint32_t(offsetof(hiprz_view_pixel, word));
    out[6] = HIPRZ_VIEW_KIND_SHIFT, out[7] = RZ_VIEW_ROWS_BUILD;
}

}  // extern "C"
