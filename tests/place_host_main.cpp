// place_host_main.cpp — the pure-host unit of probe placement (rayzath_amd/csrc/place/hiprz_place_host.cpp) as a program of its own:
// tests/test_place_abi.py builds it with -fsanitize=address,undefined and reads what it prints.  The table check, the params check case by
// case, every refusal in the header's order, the hash, the growth rule and the layout.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "hiprz_place.h"
#include "hiprz_place_host.hpp"

using namespace hiprz;

static const char* text(const char* why) { return why ? why : "none"; }

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the table: K and S before the floats
    std::vector<float> table(4 * 64 * 2, 0.0f);
    for (size_t i = 0; i < table.size(); i += 4) table[i + 2] = (i / 4) % 2 ? -1.0f : 1.0f, table[i + 3] = nan;  // w is ignored
    std::printf("table: %s\n", text(place_table_refusal(table.data(), 64u, 2u)));
    std::printf("table: %s\n", text(place_table_refusal(nullptr, 64u, 2u)));
    for (uint32_t K : {0u, 16u, 32u, 63u, 96u, 2048u}) std::printf("table K %u: %s\n", K, text(place_table_refusal(table.data(), K, 1u)));
    for (uint32_t S : {0u, 65u}) std::printf("table S %u: %s\n", S, text(place_table_refusal(table.data(), 64u, S)));
    table[4 * 70] = inf;
    std::printf("table: %s\n", text(place_table_refusal(table.data(), 64u, 2u)));
    table[4 * 70] = 0.1f;
    std::printf("table: %s\n", text(place_table_refusal(table.data(), 64u, 2u)));
    std::printf("table: %s\n", text(place_table_refusal(table.data(), 64u, 1u)));  // the first set alone is sound
    // the params, case by case
    const hiprz_place_params good{0.2f, 4.0f, {0.36f, 0.0f, 3.0e38f}, 16u, 0xFFFFFFFFu, 0u};
    std::printf("params: %d %s\n", hiprz_place_check_params(&good), text(place_params_refusal(&good)));
    std::printf("params: %d %s\n", hiprz_place_check_params(nullptr), text(place_params_refusal(nullptr)));
    for (float v : {0.0f, -0.0f, -1.0f, nan, inf}) {
        hiprz_place_params p = good;
        p.min_front = v;
        std::printf("min_front: %d %s\n", hiprz_place_check_params(&p), text(place_params_refusal(&p)));
    }
    for (float v : {0.0f, -1.0f, nan, inf}) {
        hiprz_place_params p = good;
        p.reach = v;
        std::printf("reach: %d %s\n", hiprz_place_check_params(&p), text(place_params_refusal(&p)));
    }
    for (int a = 0; a < 3; ++a)
        for (float v : {-1.0e-30f, nan, inf}) {
            hiprz_place_params p = good;
            p.max_offset[a] = v;
            std::printf("max_offset %d: %d %s\n", a, hiprz_place_check_params(&p), text(place_params_refusal(&p)));
        }
    {
        hiprz_place_params p = good;
        p.max_offset[0] = p.max_offset[1] = p.max_offset[2] = -0.0f, p.iterations = 0u, p.max_back = 0u;  // -0 is >= 0
        std::printf("params: %d %s\n", hiprz_place_check_params(&p), text(place_params_refusal(&p)));
        p.iterations = 17u;
        std::printf("iterations: %d %s\n", hiprz_place_check_params(&p), text(place_params_refusal(&p)));
        p.iterations = 16u, p.reserved = 1u;
        std::printf("reserved: %d %s\n", hiprz_place_check_params(&p), text(place_params_refusal(&p)));
        p.min_front = nan, p.reach = nan, p.iterations = 99u;  // the first thing wrong is named
        std::printf("params: %d %s\n", hiprz_place_check_params(&p), text(place_params_refusal(&p)));
    }
    // a placement's refusals, in order
    hiprz_place_params bad = good;
    bad.reach = 0.0f;
    struct { bool any_null; size_t n; uint32_t K; const hiprz_place_params* params; } calls[] = {
        {false, 5u, 64u, &good}, {false, 0u, 1024u, &good}, {true, size_t(1) << 40, 0u, &bad}, {false, size_t(1) << 40, 0u, &bad}, {false, size_t(1) << 25, 64u, &bad},
        {false, (size_t(1) << 25) - 1u, 64u, &bad}, {false, (size_t(1) << 25) - 1u, 64u, &good}, {false, 1u, 64u, nullptr}};
    for (const auto& c : calls) {
        int code = -1;
        const char* why = place_probes_refusal(c.any_null, c.n, c.K, c.params, &code);
        std::printf("place: %d %s\n", code, text(why));
    }
    std::printf("hash %u %u %u\n", place_hash(0u), place_hash(1u), place_hash(0xFFFFFFFFu));
    std::printf("allowed %d %d %d %d %d %d\n", int(place_k_allowed(64u)), int(place_k_allowed(1024u)), int(place_k_allowed(32u)), int(place_k_allowed(192u)), int(place_s_allowed(64u)),
                int(place_s_allowed(0u)));
    std::printf("capacity %zu %zu %zu %zu\n", place_capacity(0, 1), place_capacity(4096, 4097), place_capacity(100, 50), place_capacity(size_t(1) << 30, (size_t(1) << 30) + 1));
    uint32_t layout[8];
    hiprz_place_layout(layout);
    hiprz_place_layout(nullptr);
    std::printf("layout %u %u %u %u %u %u %u %u\n", layout[0], layout[1], layout[2], layout[3], layout[4], layout[5], layout[6], layout[7]);
    return 0;
}
