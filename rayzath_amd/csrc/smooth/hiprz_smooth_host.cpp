// hiprz_smooth_host.cpp — the pure-host half of lightmap smoothing (hiprz_smooth_host.hpp) and the host-only calls of
// include/hiprz_smooth.h.  No HIP header.
#include "hiprz_smooth_host.hpp"

#include <cmath>
#include <cstddef>

#include "../query/hiprz_query_staging.hpp"
#include "hiprz_smooth.h"

namespace hiprz {

namespace {
constexpr size_t kSmoothMaxTexels = size_t(HIPRZ_SMOOTH_MAX_SIZE) * HIPRZ_SMOOTH_MAX_SIZE;
bool stop_allowed(float v) { return std::isfinite(v) && v >= 0.0f; }
}  // namespace

const char* smooth_params_refusal(const hiprz_smooth_params* p) {
    if (!p) return "null params";
    if (p->iterations < 1u || p->iterations > HIPRZ_SMOOTH_MAX_ITERATIONS) return "iterations is not in 1..8";
    if (!stop_allowed(p->radius)) return "radius is not a finite number >= 0";
    if (!stop_allowed(p->plane)) return "plane is not a finite number >= 0";
    if (!stop_allowed(p->sigma_colour)) return "sigma_colour is not a finite number >= 0";
    return nullptr;
}

const char* smooth_refusal(bool any_null, const hiprz_smooth_params* p, uint32_t W, uint32_t H) {
    if (any_null) return "null pointer";
    if (const char* why = smooth_params_refusal(p)) return why;
    if (W < 1u || W > HIPRZ_SMOOTH_MAX_SIZE || H < 1u || H > HIPRZ_SMOOTH_MAX_SIZE) return "W or H is not in 1..16384";
    return nullptr;
}

SmoothGrid smooth_grid(uint32_t W, uint32_t H, uint32_t step, bool staged) {
    const auto blocks = [](uint32_t n) { return (n + kSmoothBlock - 1u) / kSmoothBlock; };
    if (!staged) return SmoothGrid{blocks(W), blocks(H), blocks(W), blocks(H)};
    const uint32_t per_x = blocks((W + step - 1u) / step), per_y = blocks((H + step - 1u) / step);
    return SmoothGrid{(step < W ? step : W) * per_x, (step < H ? step : H) * per_y, per_x, per_y};
}

bool smooth_overlap(const void* a, const void* b, size_t bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y ? y - x < bytes : x - y < bytes;
}

size_t smooth_capacity(size_t have, size_t need) { return staging_capacity(have, need, kSmoothMaxTexels); }

}  // namespace hiprz

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_smooth_params) == 16, "two 16-byte loads per point, one 16-byte argument");

extern "C" {

int hiprz_smooth_check_params(const hiprz_smooth_params* params) { return hiprz::smooth_params_refusal(params) ? HIPRZ_ERR_INVALID : HIPRZ_OK; }

void hiprz_smooth_layout(uint32_t out[8]) {
    if (!out) return;
    out[0] = uint32_t(sizeof(hiprz_bake_point)), out[1] = 16u, out[2] = uint32_t(sizeof(hiprz_smooth_params)), out[3] = 12u;
    out[4] = uint32_t(offsetof(hiprz_smooth_params, radius)), out[5] = uint32_t(offsetof(hiprz_smooth_params, sigma_colour));
    out[6] = hiprz::smooth_staged(1u) ? 1u : 0u, out[7] = hiprz::smooth_staged(2u) ? 1u : 0u;
}

}  // extern "C"
