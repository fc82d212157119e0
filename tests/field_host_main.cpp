// field_host_main.cpp — the pure-host unit of probe fields (rayzath_amd/csrc/field/hiprz_field_host.cpp) as a program of its own:
// tests/test_field_abi.py builds it with -fsanitize=address,undefined and reads what it prints.  The table check, every refusal in the
// header's order, the grid and params checks, the texel directions, the hash, the growth rule and the layout.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "hiprz_field.h"
#include "hiprz_field_host.hpp"

using namespace hiprz;

static const char* text(const char* why) { return why ? why : "none"; }

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the table: K and S before the floats
    std::vector<float> table(4 * 64 * 2, 0.0f);
    for (size_t i = 0; i < table.size(); i += 4) table[i + 2] = (i / 4) % 2 ? -1.0f : 1.0f, table[i + 3] = nan;  // w is ignored
    std::printf("table: %s\n", text(field_table_refusal(table.data(), 64u, 2u)));
    std::printf("table: %s\n", text(field_table_refusal(nullptr, 64u, 2u)));
    for (uint32_t K : {0u, 16u, 32u, 63u, 96u, 2048u}) std::printf("table K %u: %s\n", K, text(field_table_refusal(table.data(), K, 1u)));
    for (uint32_t S : {0u, 65u}) std::printf("table S %u: %s\n", S, text(field_table_refusal(table.data(), 64u, S)));
    table[4 * 70] = inf;
    std::printf("table: %s\n", text(field_table_refusal(table.data(), 64u, 2u)));
    table[4 * 70] = 0.1f;
    std::printf("table: %s\n", text(field_table_refusal(table.data(), 64u, 2u)));
    std::printf("table: %s\n", text(field_table_refusal(table.data(), 64u, 1u)));  // the first set alone is sound
    // a bake's refusals, in order
    struct { bool any_null; size_t n; uint32_t K; float reach; } bakes[] = {{false, 5u, 64u, 1.0f}, {false, 0u, 1024u, 3.0e38f}, {true, size_t(1) << 40, 0u, nan}, {false, size_t(1) << 40, 0u, nan},
                                                                           {false, size_t(1) << 25, 64u, nan}, {false, (size_t(1) << 25) - 1u, 64u, 1.0f}, {false, 1u, 64u, 0.0f},
                                                                           {false, 1u, 64u, -1.0f}, {false, 1u, 64u, nan}, {false, 1u, 64u, inf}};
    for (const auto& b : bakes) {
        int code = -1;
        const char* why = field_visibility_refusal(b.any_null, b.n, b.K, b.reach, &code);
        std::printf("bake: %d %s\n", code, text(why));
    }
    // the grid
    const hiprz_field_grid good{{-1.0f, 0.0f, 0.5f}, {1.0f, 1.0f, 1.0f}, {3u, 2u, 3u}, 0u};
    std::printf("grid: %d %s\n", hiprz_field_check_grid(&good, 18u), text(field_grid_refusal(&good, 18u)));
    std::printf("grid: %d %s\n", hiprz_field_check_grid(&good, 17u), text(field_grid_refusal(&good, 17u)));
    std::printf("grid: %d %s\n", hiprz_field_check_grid(nullptr, 18u), text(field_grid_refusal(nullptr, 18u)));
    hiprz_field_grid g = good;
    g.n[1] = 0u;
    std::printf("grid: %s\n", text(field_grid_refusal(&g, 0u)));
    g = good, g.n[0] = g.n[1] = g.n[2] = 0xFFFFFFFFu;
    std::printf("grid: %s\n", text(field_grid_refusal(&g, size_t(0xFFFFFFFFu))));
    g = good, g.n[0] = 1u << 16, g.n[1] = 1u << 15, g.n[2] = 1u;
    std::printf("grid: %s\n", text(field_grid_refusal(&g, size_t(1) << 31)));
    g = good, g.n[0] = 1u << 15, g.n[1] = 1u << 15, g.n[2] = 1u;
    std::printf("grid: %s\n", text(field_grid_refusal(&g, size_t(1) << 30)));
    for (float step : {0.0f, -1.0f, nan, inf}) {
        g = good, g.step[2] = step;
        std::printf("grid step: %s\n", text(field_grid_refusal(&g, 18u)));
    }
    g = good, g.n[1] = 1u, g.step[1] = nan;  // a count of 1: the step is not read
    std::printf("grid: %s\n", text(field_grid_refusal(&g, 9u)));
    g = good, g.lo[0] = inf;
    std::printf("grid: %s\n", text(field_grid_refusal(&g, 18u)));
    // the params
    for (float bias : {0.0f, -0.0f, 0.5f, 3.0e38f, -1.0e-30f, nan, inf}) {
        const hiprz_field_params p{bias, 7u, {0u, 0u}};
        std::printf("params: %d %s\n", hiprz_field_check_params(&p), text(field_params_refusal(&p)));
    }
    std::printf("params null: %d\n", hiprz_field_check_params(nullptr));
    // a lookup's refusals, in order: a null pointer before the grid before the params before m
    const hiprz_field_params fine{0.0f, 0u, {0u, 0u}}, negative{-1.0f, 0u, {0u, 0u}};
    g = good, g.step[0] = 0.0f;
    std::printf("lookup: %s\n", text(field_lookup_refusal(false, &good, 18u, &fine, 1000u)));
    std::printf("lookup: %s\n", text(field_lookup_refusal(false, &good, 18u, &fine, 0u)));
    std::printf("lookup: %s\n", text(field_lookup_refusal(true, &g, 18u, &negative, size_t(1) << 31)));
    std::printf("lookup: %s\n", text(field_lookup_refusal(false, &g, 18u, &negative, size_t(1) << 31)));
    std::printf("lookup: %s\n", text(field_lookup_refusal(false, &good, 18u, &negative, size_t(1) << 31)));
    std::printf("lookup: %s\n", text(field_lookup_refusal(false, &good, 18u, &fine, size_t(1) << 31)));
    std::printf("lookup: %s\n", text(field_lookup_refusal(false, &good, 18u, &fine, (size_t(1) << 31) - 1u)));
    // the texel directions: unit vectors, the equator and both hemispheres, w = 0
    float o[64][4];
    std::printf("texels: %d %d\n", hiprz_field_texel_directions(o), hiprz_field_texel_directions(nullptr));
    int up = 0, down = 0;
    double worst = 0.0;
    for (const auto& d : o) {
        up += d[2] > 1.0e-6f, down += d[2] < -1.0e-6f;
        worst = std::fmax(worst, std::fabs(std::sqrt(double(d[0]) * d[0] + double(d[1]) * d[1] + double(d[2]) * d[2]) - 1.0) + std::fabs(double(d[3])));
    }
    std::printf("texels: %d up %d down unit %d\n", up, down, int(worst < 1.0e-6));
    std::printf("hash %u %u %u\n", field_hash(0u), field_hash(1u), field_hash(0xFFFFFFFFu));
    std::printf("allowed %d %d %d %d %d %d\n", int(field_k_allowed(64u)), int(field_k_allowed(1024u)), int(field_k_allowed(32u)), int(field_k_allowed(192u)), int(field_s_allowed(64u)),
                int(field_s_allowed(0u)));
    std::printf("capacity %zu %zu %zu %zu\n", field_capacity(0, 1), field_capacity(4096, 4097), field_capacity(100, 50), field_capacity(size_t(1) << 30, (size_t(1) << 30) + 1));
    uint32_t layout[8];
    hiprz_field_layout(layout);
    hiprz_field_layout(nullptr);
    std::printf("layout %u %u %u %u %u %u %u\n", layout[0], layout[1], layout[2], layout[3], layout[4], layout[5], layout[6]);
    return 0;
}
