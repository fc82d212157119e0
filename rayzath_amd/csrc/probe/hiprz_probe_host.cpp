// hiprz_probe_host.cpp — the pure-host half of probe baking (hiprz_probe_host.hpp) and the host-only calls of include/hiprz_probe.h.
// No HIP header.
#include "hiprz_probe_host.hpp"

#include <cmath>
#include <cstddef>
#include <cstring>

#include "../query/hiprz_query_staging.hpp"
#include "hiprz_probe.h"

namespace hiprz {

const char* probe_table_refusal(const float* xyz0, uint32_t K, uint32_t S) {
    if (!xyz0) return "null pointer";
    if (!probe_k_allowed(K)) return "K is not one of 16, 32, 64, 128, 256, 512, 1024";
    if (!probe_s_allowed(S)) return "S is not in 1..64";
    for (size_t i = 0; i < size_t(K) * S; ++i) {
        const float x = xyz0[4 * i], y = xyz0[4 * i + 1], z = xyz0[4 * i + 2];
        if (!std::isfinite(x) || !std::isfinite(y) || !std::isfinite(z)) return "a direction is not finite";
        const float xx = x * x, yy = y * y, zz = z * z;  // (named: each product is rounded to float before the sums, whatever the host contracts)
        const float xy = xx + yy, sq = xy + zz;
        if (!(sq >= 0.999f && sq <= 1.001f)) return "a direction is not of unit length (squared length outside [0.999, 1.001])";
    }
    return nullptr;
}

const char* probe_samples_refusal(const float* xy, uint32_t K, uint32_t S) {
    if (!xy) return "null pointer";
    if (!probe_samples_k_allowed(K)) return "K is not a power of two in 1..1024";
    if (!probe_s_allowed(S)) return "S is not in 1..64";
    for (size_t i = 0; i < size_t(K) * S; ++i) {
        const float x = xy[2 * i], y = xy[2 * i + 1];
        if (!std::isfinite(x) || !std::isfinite(y)) return "a sample is not finite";
        const float xx = x * x, yy = y * y;
        const float sq = xx + yy;
        if (sq > 1.0f) return "a sample lies outside the unit disk";
    }
    return nullptr;
}

const char* probe_charts_refusal(const uint32_t* base, uint32_t n_instances, const hiprz_gather_chart* uv, uint32_t n_charts) {
    if ((!base && n_instances != 0u) || (!uv && n_charts != 0u)) return "null pointer";
    if (n_charts > HIPRZ_GATHER_MAX_CHARTS) return "more charts than there are ids below the codes";
    for (size_t i = 0; i < n_charts; ++i) {
        const hiprz_gather_chart& c = uv[i];
        if (!std::isfinite(c.u1) || !std::isfinite(c.v1) || !std::isfinite(c.u2) || !std::isfinite(c.v2) || !std::isfinite(c.u3) || !std::isfinite(c.v3))
            return "a chart's UV is not finite";
    }
    return nullptr;
}

const char* probe_gather_refusal(bool any_null, size_t n, uint32_t K, bool has_charts, int* code) {
    *code = HIPRZ_ERR_INVALID;
    if (any_null) return "null pointer";
    *code = HIPRZ_ERR_STATE;
    if (K == 0u) return "no direction table has been set";
    if (!has_charts) return "no chart map has been set";
    *code = HIPRZ_ERR_INVALID;
    if (n >= kProbeMaxRays / K) return "n*K is 2^31 or more";  // (K divides 2^31; no product that could wrap)
    *code = HIPRZ_OK;
    return nullptr;
}

const char* probe_light_refusal(bool any_null, size_t n, uint32_t K, int* code) {
    *code = HIPRZ_ERR_INVALID;
    if (any_null) return "null pointer";
    *code = HIPRZ_ERR_STATE;
    if (K == 0u) return "no sample table has been set";
    *code = HIPRZ_ERR_INVALID;
    if (n >= kProbeMaxRays / K) return "n*K is 2^31 or more";
    *code = HIPRZ_OK;
    return nullptr;
}

const char* probe_size_refusal(uint32_t W, uint32_t H) {
    if (W < 1u || W > HIPRZ_PROBE_MAX_SIZE || H < 1u || H > HIPRZ_PROBE_MAX_SIZE) return "W or H is not in 1..16384";
    return nullptr;
}

const char* probe_range_refusal(const hiprz_light_range* range, uint32_t n_spot, uint32_t n_direct, ProbeSpan* out) {
    *out = ProbeSpan{0u, n_spot, 0u, n_direct};
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

size_t probe_capacity(size_t have, size_t need) { return staging_capacity(have, need, kProbeMaxProbes); }

}  // namespace hiprz

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_probe_sh) == 144 && sizeof(hiprz_gather_sample) == 16 && sizeof(hiprz_gather_chart) == 32,
              "two 16-byte loads per probe and chart, nine 16-byte stores per record, one per sample");

extern "C" {

int hiprz_probe_sphere_directions(uint32_t K, uint32_t S, float* xyz0_out) {
    if (!xyz0_out || !hiprz::probe_k_allowed(K) || !hiprz::probe_s_allowed(S)) return HIPRZ_ERR_INVALID;
    const double two_pi = 6.283185307179586476925286766559;
    for (uint32_t s = 0; s < S; ++s)
        for (uint32_t k = 0; k < K; ++k) {
            const double z = 1.0 - 2.0 * (double(k) + 0.5) / double(K);
            const double r = std::sqrt(1.0 - z * z);
            const double turn = double(k) * 0.6180339887498949;
            const double phi = two_pi * ((turn - std::floor(turn)) + double(s) / double(S));
            float* o = xyz0_out + 4 * (size_t(s) * K + k);
            o[0] = float(r * std::cos(phi)), o[1] = float(r * std::sin(phi)), o[2] = float(z), o[3] = 0.0f;
        }
    return HIPRZ_OK;
}

void hiprz_probe_irradiance(const hiprz_probe_sh* sh, const float n[3], float out[3]) {
    if (!out) return;
    out[0] = out[1] = out[2] = 0.0f;
    if (!sh || !n) return;
    uint32_t word;
    std::memcpy(&word, &sh->sh[0][3], sizeof word);
    if (word == HIPRZ_PROBE_INVALID) return;
    const float x = n[0], y = n[1], z = n[2];
    // (named: each product is rounded to float before it is used, whatever the host contracts)
    const float xy = x * y, yz = y * z, zz = z * z, xz = x * z, xx = x * x, yy = y * y;
    const float zz3 = 3.0f * zz;
    const float basis[9] = {1.0f, y, z, x, xy, yz, zz3 - 1.0f, xz, xx - yy};
    const float weight[9] = {1.0f, 2.0f, 2.0f, 2.0f, 3.75f, 3.75f, 0.3125f, 3.75f, 0.9375f};
    for (int c = 0; c < 3; ++c) {
        float e = 0.0f;
        for (int b = 0; b < 9; ++b) {
            const float ws = weight[b] * sh->sh[b][c];
            const float term = ws * basis[b];
            e = e + term;
        }
        out[c] = e;
    }
}

void hiprz_probe_layout(uint32_t out[6]) {
    if (!out) return;
    out[0] = uint32_t(sizeof(hiprz_bake_point)), out[1] = uint32_t(sizeof(hiprz_probe_sh)), out[2] = uint32_t(sizeof(hiprz_gather_sample));
    out[3] = uint32_t(sizeof(hiprz_gather_chart)), out[4] = uint32_t(offsetof(hiprz_probe_sh, sh) + 3 * sizeof(float));
    out[5] = uint32_t(offsetof(hiprz_probe_sh, sh) + 7 * sizeof(float));
}

}  // extern "C"
