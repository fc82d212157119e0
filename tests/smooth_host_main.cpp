// smooth_host_main.cpp — the pure-host unit of lightmap smoothing (rayzath_amd/csrc/smooth/hiprz_smooth_host.cpp) as a program of its
// own: tests/test_smooth_abi.py builds it with -fsanitize=address,undefined and reads what it prints.  The params check, every refusal
// in the header's order, the launch grids, the overlap test, the growth rule and the layout.
#include <cstdint>
#include <cstdio>
#include <limits>

#include "hiprz_smooth.h"
#include "hiprz_smooth_host.hpp"

using namespace hiprz;

static const char* text(const char* why) { return why ? why : "none"; }

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const hiprz_smooth_params good{3u, 0.5f, 0.02f, 0.8f};
    // the params check: the C call and the reason
    const hiprz_smooth_params cases[] = {good, {1u, 0.0f, 0.0f, 0.0f}, {8u, 0.0f, -0.0f, 3.0e38f}, {0u, 0.5f, 0.02f, 0.8f}, {9u, 0.5f, 0.02f, 0.8f}, {0xFFFFFFFFu, 0.5f, 0.02f, 0.8f},
                                         {3u, nan, 0.02f, 0.8f}, {3u, -1.0f, 0.02f, 0.8f}, {3u, inf, 0.02f, 0.8f}, {3u, 0.5f, nan, 0.8f}, {3u, 0.5f, -1.0e-30f, 0.8f}, {3u, 0.5f, inf, 0.8f},
                                         {3u, 0.5f, 0.02f, nan}, {3u, 0.5f, 0.02f, -inf}, {3u, 0.5f, 0.02f, inf}, {0u, nan, nan, nan}};
    for (const hiprz_smooth_params& p : cases) std::printf("params: %d %s\n", hiprz_smooth_check_params(&p), text(smooth_params_refusal(&p)));
    std::printf("params null: %d %s\n", hiprz_smooth_check_params(nullptr), text(smooth_params_refusal(nullptr)));
    // a call's refusals, in order: a null pointer before bad params before a bad size
    const hiprz_smooth_params bad{0u, nan, 0.0f, 0.0f};
    struct { bool any_null; const hiprz_smooth_params* p; uint32_t W, H; } calls[] = {
        {false, &good, 1u, 1u}, {false, &good, 16384u, 16384u}, {true, &bad, 0u, 0u}, {true, &good, 4u, 4u}, {false, &bad, 0u, 0u}, {false, nullptr, 0u, 0u}, {false, &good, 0u, 4u},
        {false, &good, 4u, 0u}, {false, &good, 16385u, 1u}, {false, &good, 1u, 16385u}, {false, &good, 0xFFFFFFFFu, 0xFFFFFFFFu}};
    for (const auto& c : calls) std::printf("call: %s\n", text(smooth_refusal(c.any_null, c.p, c.W, c.H)));
    // the grids: (W, H, step, staged) -> workgroups and blocks per residue
    struct { uint32_t W, H, step; bool staged; } grids[] = {{1u, 1u, 1u, false}, {1u, 1u, 1u, true}, {1u, 7u, 4u, true}, {17u, 33u, 1u, false}, {17u, 33u, 1u, true}, {17u, 33u, 2u, true},
                                                            {67u, 131u, 16u, true}, {16384u, 16384u, 1u, true}, {16384u, 16384u, 128u, true}, {16384u, 16384u, 128u, false}};
    for (const auto& g : grids) {
        const SmoothGrid r = smooth_grid(g.W, g.H, g.step, g.staged);
        std::printf("grid %u %u %u %d: %u %u %u %u\n", g.W, g.H, g.step, int(g.staged), r.x, r.y, r.per_x, r.per_y);
    }
    char bytes[64];
    std::printf("overlap: %d %d %d %d %d\n", int(smooth_overlap(bytes, bytes, 16)), int(smooth_overlap(bytes, bytes + 15, 16)), int(smooth_overlap(bytes + 15, bytes, 16)),
                int(smooth_overlap(bytes, bytes + 16, 16)), int(smooth_overlap(bytes + 32, bytes, 32)));
    std::printf("capacity %zu %zu %zu %zu\n", smooth_capacity(0, 1), smooth_capacity(4096, 4097), smooth_capacity(100, 50), smooth_capacity(size_t(1) << 27, (size_t(1) << 27) + 1));
    uint32_t layout[8];
    hiprz_smooth_layout(layout);
    hiprz_smooth_layout(nullptr);
    std::printf("layout %u %u %u %u %u %u\n", layout[0], layout[1], layout[2], layout[3], layout[4], layout[5]);
    std::printf("forms %u %u %d %d\n", layout[6], layout[7], int(smooth_staged(1u)), int(smooth_staged(64u)));
    return 0;
}
