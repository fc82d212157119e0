// query_host_main.cpp — the pure-host units of the ray queries (rayzath_amd/csrc/query/hiprz_query_staging.hpp, hiprz_query_host.cpp) as a
// process of its own, for tests/test_query_abi.py to build under sanitizers: reads "have need" pairs from stdin, prints
// query_staging_capacity of each (a staging of that capacity is allocated and touched where `need` ends), then the query's refusals of the
// calls tests/order_host_main.cpp lists (under the query's limit of 2^31 - 1 rays), then the layout words.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hiprz_query.h"
#include "hiprz_query_staging.hpp"

int main() {
    unsigned long long have, need;
    size_t pairs = 0;
    while (std::scanf("%llu %llu", &have, &need) == 2) {
        const size_t cap = hiprz::query_staging_capacity(size_t(have), size_t(need));
        std::printf("%zu\n", cap);
        if (cap && cap <= (1u << 16)) {  // what grow_staging does with the figure: room for `need` rays and hits
            std::vector<hiprz_ray> rays(cap);
            std::vector<hiprz_hit> hits(cap);
            if (need) std::memset(&rays[need - 1], 0, sizeof(hiprz_ray)), std::memset(&hits[need - 1], 0, sizeof(hiprz_hit));
        }
        ++pairs;
    }
    const struct {
        bool any_null;
        size_t n;
        uint32_t flags;
    } calls[] = {{false, 0, 0},           {false, 1, HIPRZ_QUERY_NORMALIZE}, {true, 1, 0},  {false, 1, 2},       {false, 1, 3},
                 {false, size_t(1) << 30, 0}, {false, (size_t(1) << 30) + 1, 0}, {true, 0, 2}, {false, ~size_t(0), 1}};
    for (const auto& c : calls) {
        const char* why = hiprz::query_refusal(c.any_null, c.n, c.flags);
        std::printf("refusal: %s\n", why ? why : "none");
    }
    uint32_t layout[7];
    hiprz_query_layout(layout);
    std::printf("layout %u %u %u %u %u %u %u\npairs %zu\n", layout[0], layout[1], layout[2], layout[3], layout[4], layout[5], layout[6], pairs);
    return 0;
}
