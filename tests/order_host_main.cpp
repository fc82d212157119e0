// order_host_main.cpp — the pure-host unit of the ordered ray queries (rayzath_amd/csrc/order/hiprz_order_host.cpp) as a process of its own,
// for tests/test_order_abi.py to build under sanitizers: reads "have need" pairs from stdin, prints order_capacity of each (buffers of that
// capacity are allocated and touched where `need` ends, as grow_work and grow_staging use the figure), then the refusals of a fixed list
// of calls.
#include <cstdio>
#include <cstring>
#include <vector>

#include "hiprz_order_host.hpp"
#include "hiprz_query.h"

int main() {
    unsigned long long have, need;
    size_t pairs = 0;
    while (std::scanf("%llu %llu", &have, &need) == 2) {
        const size_t cap = hiprz::order_capacity(size_t(have), size_t(need));
        std::printf("%zu\n", cap);
        if (cap && cap <= (1u << 16)) {
            std::vector<uint32_t> keys(cap), perm(cap);
            std::vector<hiprz_ray> rays(cap);
            std::vector<hiprz_hit> hits(cap);
            if (need) {
                keys[need - 1] = perm[need - 1] = 0u;
                std::memset(&rays[need - 1], 0, sizeof(hiprz_ray)), std::memset(&hits[need - 1], 0, sizeof(hiprz_hit));
            }
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
        const char* why = hiprz::order_refusal(c.any_null, c.n, c.flags);
        std::printf("refusal: %s\n", why ? why : "none");
    }
    std::printf("pairs %zu\n", pairs);
    return 0;
}
