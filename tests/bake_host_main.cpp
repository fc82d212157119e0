// bake_host_main.cpp — the pure-host unit of occlusion baking (rayzath_amd/csrc/bake/hiprz_bake_host.cpp) as a process of its own, for
// tests/test_bake_abi.py to build under sanitizers: reads "have need" pairs from stdin, prints bake_capacity of each (buffers of that
// capacity are allocated and touched where `need` ends, as grow_staging uses the figure), then the refusals of a fixed list of calls in
// the order they are looked at, the verdicts of the table validator on a fixed list of tables, and the host-only calls of the header.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hiprz_bake.h"
#include "hiprz_bake_host.hpp"

namespace {
// a table of K * S copies of (x, y, z, 9): a good one has x*x + y*y + z*z = 1; the fourth component is not read
std::vector<float> table_of(uint32_t K, uint32_t S, float x, float y, float z) {
    std::vector<float> t(4 * size_t(K) * S);
    for (size_t i = 0; i < t.size(); i += 4) t[i] = x, t[i + 1] = y, t[i + 2] = z, t[i + 3] = 9.0f;
    return t;
}
void verdict(const char* name, const float* xyz0, uint32_t K, uint32_t S) {
    const char* why = hiprz::bake_table_refusal(xyz0, K, S);
    std::printf("table %s: %s\n", name, why ? why : "none");
}
}  // namespace

int main() {
    unsigned long long have, need;
    size_t pairs = 0;
    while (std::scanf("%llu %llu", &have, &need) == 2) {
        const size_t cap = hiprz::bake_capacity(size_t(have), size_t(need));
        std::printf("%zu\n", cap);
        if (cap && cap <= (1u << 16)) {
            std::vector<hiprz_bake_point> points(cap);
            std::vector<hiprz_bake_texel> texels(cap);
            if (need) std::memset(&points[need - 1], 0, sizeof(hiprz_bake_point)), std::memset(&texels[need - 1], 0, sizeof(hiprz_bake_texel));
        }
        ++pairs;
    }
    const struct {
        bool any_null;
        size_t n;
        uint32_t K;
    } calls[] = {{false, 0, 16},
                 {false, 1, 64},
                 {true, 1, 64},                     // a null pointer is looked at first
                 {true, 1, 0},                      //   ... before the missing table
                 {true, ~size_t(0), 0},             //   ... and before the size
                 {false, 1, 0},                     // no table
                 {false, 0, 0},                     //   ... even for nothing to do
                 {false, ~size_t(0), 0},            //   ... before the size
                 {false, (size_t(1) << 27) - 1, 16},  // n*K = 2^31 - 16
                 {false, size_t(1) << 27, 16},      // n*K = 2^31
                 {false, (size_t(1) << 21) - 1, 1024},
                 {false, size_t(1) << 21, 1024},
                 {false, ~size_t(0), 64},           // no product that wraps
                 {false, (size_t(1) << 58) + 1, 64}};  // n*K = 2^64 + 64 wraps to 64
    for (const auto& c : calls) {
        int code = -1;
        const char* why = hiprz::bake_refusal(c.any_null, c.n, c.K, &code);
        std::printf("refusal: %d %s\n", code, why ? why : "none");
    }

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> good = table_of(16, 3, 0.6f, 0.0f, 0.8f);
    verdict("good", good.data(), 16, 3);
    std::vector<float> t = good;
    t[4 * 47 + 1] = nan;  // the last direction of the table
    verdict("nan", t.data(), 16, 3);
    t = good, t[0] = inf;
    verdict("inf", t.data(), 16, 3);
    t = good, t[3] = nan;  // the fourth component is not read
    verdict("nan in w", t.data(), 16, 3);
    const float l1002 = std::sqrt(1.002f), l0998 = std::sqrt(0.998f);
    t = table_of(16, 1, 0.0f, l1002, 0.0f);
    verdict("squared length 1.002", t.data(), 16, 1);
    t = table_of(16, 1, 0.0f, 0.0f, -l0998);
    verdict("squared length 0.998", t.data(), 16, 1);
    t = table_of(16, 1, 0.0f, 1.002f, 0.0f);
    verdict("length 1.002", t.data(), 16, 1);
    t = table_of(16, 1, 0.0f, 0.0f, 0.998f);
    verdict("length 0.998", t.data(), 16, 1);
    t = table_of(16, 1, 0.0f, 0.0f, -1.0004f);  // inside: a sign of z is not required
    verdict("length 1.0004 downwards", t.data(), 16, 1);
    t = table_of(16, 1, 0.0f, 0.0f, 0.0f);
    verdict("zero", t.data(), 16, 1);
    t = table_of(48, 1, 0.0f, 0.0f, 1.0f);
    verdict("K = 48", t.data(), 48, 1);
    verdict("K = 8", t.data(), 8, 1);
    t = table_of(1024, 2, 0.0f, 0.0f, 1.0f);
    verdict("K = 1024", t.data(), 1024, 2);
    verdict("K = 2048", t.data(), 2048, 1);
    verdict("S = 0", good.data(), 16, 0);
    verdict("S = 65", good.data(), 16, 65);
    t = table_of(16, 64, 1.0f, 0.0f, 0.0f);
    verdict("S = 64", t.data(), 16, 64);
    verdict("null", nullptr, 16, 1);

    // the host-only calls of the header: the cosine table passes the validator, a refused call writes nothing, the layout, the set
    std::vector<float> cosine(4 * size_t(1024) * 64 + 4, 7.0f);
    const int rc = hiprz_bake_cosine_directions(1024, 64, cosine.data());
    std::printf("cosine 1024 64: %d, behind %g\n", rc, double(cosine[4 * size_t(1024) * 64]));
    verdict("cosine", cosine.data(), 1024, 64);
    float one[4] = {7.0f, 7.0f, 7.0f, 7.0f};
    std::printf("cosine 48 1: %d, wrote %d\n", hiprz_bake_cosine_directions(48, 1, one), int(one[0] != 7.0f));
    uint32_t layout[6];
    hiprz_bake_layout(layout);
    std::printf("layout %u %u %u %u %u %u\n", layout[0], layout[1], layout[2], layout[3], layout[4], layout[5]);
    std::printf("set_of %u %u %u %u\n", hiprz_bake_set_of(1, 0, 64), hiprz_bake_set_of(0, 1, 7), hiprz_bake_set_of(9, 9, 5), hiprz_bake_set_of(4, 2, 0));
    std::printf("pairs %zu\n", pairs);
    return 0;
}
