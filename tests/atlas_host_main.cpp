// atlas_host_main.cpp — the pure-host unit of bake atlases (rayzath_amd/csrc/atlas/hiprz_atlas_host.cpp) as a process of its own, for
// tests/test_atlas_abi.py to build under sanitizers: reads "have need" pairs from stdin, prints atlas_capacity of each (a buffer of that
// many 16-byte units is allocated and touched where `need` ends, as grow_staging uses the figure), then the size rule on a fixed list of
// sizes, the refusals of a fixed list of adds and dilations in the order they are looked at, and the layout report.
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hiprz_atlas.h"
#include "hiprz_atlas_host.hpp"

int main() {
    unsigned long long have, need;
    size_t pairs = 0;
    while (std::scanf("%llu %llu", &have, &need) == 2) {
        const size_t cap = hiprz::atlas_capacity(size_t(have), size_t(need));
        std::printf("%zu\n", cap);
        if (cap && cap <= (1u << 16)) {
            std::vector<hiprz_atlas_sample> units(cap);
            if (need) std::memset(&units[need - 1], 0, sizeof(hiprz_atlas_sample));
        }
        ++pairs;
    }
    const uint32_t sizes[][2] = {{1, 1}, {16384, 16384}, {0, 4}, {4, 0}, {16385, 4}, {4, 16385}, {0xFFFFFFFFu, 1}, {7, 5}};
    for (const auto& s : sizes) {
        const char* why = hiprz::atlas_size_refusal(s[0], s[1]);
        std::printf("size %u %u: %s\n", s[0], s[1], why ? why : "none");
    }
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const struct {
        bool any_null, begun;
        size_t n;
        uint32_t base;
        float near_, far_;
    } adds[] = {{false, true, 0, 0, 1e-3f, 3e38f},
                {false, true, 12, 0, 0.0f, 1.0f},
                {true, false, ~size_t(0), 0, nan, nan},             // a null pointer is looked at first
                {false, false, ~size_t(0), 0, nan, nan},            // then the missing begin
                {false, false, 0, 0, 1e-3f, 1.0f},                  //   ... even for nothing to do
                {false, true, 0xFFFFFFFEull, 0, 1e-3f, 1.0f},       // ids 0 .. 0xFFFFFFFD
                {false, true, 0xFFFFFFFFull, 0, 1e-3f, 1.0f},       // the id 0xFFFFFFFE is the last one allowed
                {false, true, 1, 0xFFFFFFFEu, 1e-3f, 1.0f},
                {false, true, 0, 0xFFFFFFFEu, 1e-3f, 1.0f},
                {false, true, 0, 0xFFFFFFFFu, 1e-3f, 1.0f},
                {false, true, ~size_t(0), 7, 1e-3f, 1.0f},          // no sum that wraps
                {false, true, (size_t(1) << 32) + 1, 0, 1e-3f, 1.0f},
                {false, true, 1, 0, nan, 1.0f},
                {false, true, 1, 0, 1e-3f, inf},
                {false, true, 1, 0, -inf, 1.0f},
                {false, true, 1, 0, -1e-3f, 1.0f},
                {false, true, 1, 0, -0.0f, 1.0f},                   // -0 is not < 0
                {false, true, 1, 0, 1.0f, 1.0f},
                {false, true, 1, 0, 2.0f, 1.0f}};
    for (const auto& c : adds) {
        int code = -1;
        const char* why = hiprz::atlas_add_refusal(c.any_null, c.begun, c.n, c.base, c.near_, c.far_, &code);
        std::printf("add: %d %s\n", code, why ? why : "none");
    }
    const uint32_t instances[][2] = {{0, 1}, {0, 0}, {3, 3}, {2, 3}, {0xFFFFFFFFu, 0xFFFFFFFFu}};
    for (const auto& i : instances) {
        const char* why = hiprz::atlas_instance_refusal(i[0], i[1]);
        std::printf("instance %u of %u: %s\n", i[0], i[1], why ? why : "none");
    }
    const struct {
        bool any_null, built;
        uint32_t rings;
    } dilations[] = {{false, true, 0}, {false, true, 64}, {false, true, 65}, {true, false, 65}, {false, false, 65}, {false, false, 0}, {false, true, 0xFFFFFFFFu}};
    for (const auto& d : dilations) {
        int code = -1;
        const char* why = hiprz::atlas_dilate_refusal(d.any_null, d.built, d.rings, &code);
        std::printf("dilate: %d %s\n", code, why ? why : "none");
    }
    uint32_t layout[8];
    hiprz_atlas_layout(layout);
    hiprz_atlas_layout(nullptr);
    std::printf("layout %u %u %u %u %u %u %u %u\n", layout[0], layout[1], layout[2], layout[3], layout[4], layout[5], layout[6], layout[7]);
    std::printf("pairs %zu\n", pairs);
    return 0;
}
