// hiprz_noise_host.cpp — the pure-host half of the noise meter (include/hiprz_noise.h "THE SUMMARY"): no HIP header, so that
// tests/test_noise_abi.py can compile it with g++ under sanitizers beside a main of its own.
#include <cmath>
#include <cstddef>

#include "hiprz_noise.h"

extern "C" {

int hiprz_noise_summarise(const float* tiles, uint32_t tiles_x, uint32_t tiles_y, uint32_t width, uint32_t height, hiprz_noise_summary* out) {
    if (!tiles || !out || !width || !height) return HIPRZ_ERR_INVALID;
    if (tiles_x != (width - 1u) / HIPRZ_NOISE_TILE_W + 1u || tiles_y != (height - 1u) / HIPRZ_NOISE_TILE_H + 1u) return HIPRZ_ERR_INVALID;
    hiprz_noise_summary s{};
    s.tiles_x = tiles_x, s.tiles_y = tiles_y;
    s.pixels = uint64_t(width) * height;
    double sum = 0.0;
    bool found = false;
    const size_t n = size_t(tiles_x) * tiles_y;
    for (size_t t = 0; t < n; ++t) {
        const float* r = tiles + 4u * t;
        const double tile_sum = double(r[0]);
        const uint64_t tile_n = uint64_t(r[2]);
        sum += tile_sum;
        s.estimated += tile_n;
        s.above += uint64_t(r[3]);
        if (r[1] > s.max) s.max = r[1];
        if (!tile_n) continue;
        const double tile_rms = std::sqrt(tile_sum / double(tile_n));
        if (!found || tile_rms > s.tile_rms_max) s.tile_rms_max = tile_rms, s.worst_tile = uint32_t(t), found = true;
    }
    s.rms = s.estimated ? std::sqrt(sum / double(s.estimated)) : 0.0;
    *out = s;
    return HIPRZ_OK;
}

void hiprz_noise_layout(uint32_t out[4]) {
    out[0] = uint32_t(sizeof(hiprz_noise_params));
    out[1] = uint32_t(sizeof(hiprz_noise_summary));
    out[2] = uint32_t(offsetof(hiprz_noise_summary, estimated));
    out[3] = uint32_t(offsetof(hiprz_noise_summary, tiles_x));
}

}  // extern "C"
