// hiprz_atlas_host.cpp — the pure-host half of bake atlases (hiprz_atlas_host.hpp) and the layout report of include/hiprz_atlas.h.
// No HIP header.
#include "hiprz_atlas_host.hpp"

#include <cmath>
#include <cstddef>

#include "../query/hiprz_query_staging.hpp"
#include "hiprz_atlas.h"

namespace hiprz {

const char* atlas_size_refusal(uint32_t width, uint32_t height) {
    if (width < 1u || width > kAtlasMaxSize) return "width is not in 1..16384";
    if (height < 1u || height > kAtlasMaxSize) return "height is not in 1..16384";
    return nullptr;
}

const char* atlas_add_refusal(bool any_null, bool begun, size_t n, uint32_t triangle_base, float near_, float far_, int* code) {
    *code = HIPRZ_ERR_INVALID;
    if (any_null) return "null pointer";
    *code = HIPRZ_ERR_STATE;
    if (!begun) return "no atlas has been begun";
    *code = HIPRZ_ERR_INVALID;
    if (n >= size_t(kAtlasNone) - triangle_base) return "triangle_base + n is 0xFFFFFFFF or more";  // (no sum that could wrap)
    if (!std::isfinite(near_) || !std::isfinite(far_)) return "near_ or far_ is not finite: every point would be invalid";
    if (near_ < 0.0f) return "near_ < 0: every point would be invalid";
    if (!(far_ > near_)) return "far_ <= near_: every point would be invalid";
    *code = HIPRZ_OK;
    return nullptr;
}

const char* atlas_instance_refusal(uint32_t instance, uint32_t n_instances) {
    return instance >= n_instances ? "the scene has no such instance" : nullptr;
}

const char* atlas_dilate_refusal(bool any_null, bool built, uint32_t rings, int* code) {
    *code = HIPRZ_ERR_INVALID;
    if (any_null) return "null pointer";
    *code = HIPRZ_ERR_STATE;
    if (!built) return "nothing has been added since the atlas was begun";
    *code = HIPRZ_ERR_INVALID;
    if (rings > kAtlasMaxRings) return "more than 64 rings";
    *code = HIPRZ_OK;
    return nullptr;
}

size_t atlas_capacity(size_t have, size_t need) { return staging_capacity(have, need, kAtlasMaxUnits); }

}  // namespace hiprz

static_assert(sizeof(hiprz_atlas_tri) == 96 && sizeof(hiprz_atlas_sample) == 16 && sizeof(hiprz_bake_point) == 32,
              "six 16-byte loads per triangle, one 16-byte store per sample, two per point");
static_assert(HIPRZ_ATLAS_NONE == hiprz::kAtlasNone && HIPRZ_ATLAS_MAX_SIZE == hiprz::kAtlasMaxSize && HIPRZ_ATLAS_MAX_RINGS == hiprz::kAtlasMaxRings,
              "the header's constants are the host unit's");

extern "C" {

void hiprz_atlas_layout(uint32_t out[8]) {
    if (!out) return;
    out[0] = uint32_t(sizeof(hiprz_atlas_tri)), out[1] = uint32_t(sizeof(hiprz_atlas_sample)), out[2] = uint32_t(sizeof(hiprz_bake_point));
    out[3] = uint32_t(offsetof(hiprz_atlas_tri, n1)), out[4] = uint32_t(offsetof(hiprz_atlas_tri, v3));
    out[5] = uint32_t(offsetof(hiprz_atlas_sample, bx)), out[6] = uint32_t(offsetof(hiprz_atlas_sample, by)), out[7] = uint32_t(offsetof(hiprz_atlas_sample, zero));
}

}  // extern "C"
