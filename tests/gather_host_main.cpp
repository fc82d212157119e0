// gather_host_main.cpp — the pure-host unit of bounce baking (rayzath_amd/csrc/gather/hiprz_gather_host.cpp) as a process of its own, for
// tests/test_gather_abi.py to build under sanitizers: reads "have need" pairs from stdin, prints gather_capacity of each (buffers of that
// capacity are allocated and touched where `need` ends, as grow_staging uses the figure), then the refusals of a fixed list of calls in
// the order they are looked at, the verdicts of the table validator on a fixed list of tables, of the chart check on a fixed list of
// maps, the size and compose rules, the hash and the layout.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hiprz_gather.h"
#include "hiprz_gather_host.hpp"

namespace {
// a table of K * S copies of (x, y, z, w)
std::vector<float> table_of(uint32_t K, uint32_t S, float x, float y, float z, float w) {
    std::vector<float> t(4 * size_t(K) * S);
    for (size_t i = 0; i < t.size(); i += 4) t[i] = x, t[i + 1] = y, t[i + 2] = z, t[i + 3] = w;
    return t;
}
void verdict(const char* name, const float* xyz0, uint32_t K, uint32_t S) {
    const char* why = hiprz::gather_table_refusal(xyz0, K, S);
    std::printf("table %s: %s\n", name, why ? why : "none");
}
void charts(const char* name, const uint32_t* base, uint32_t n_instances, const hiprz_gather_chart* uv, uint32_t n_charts) {
    const char* why = hiprz::gather_charts_refusal(base, n_instances, uv, n_charts);
    std::printf("charts %s: %s\n", name, why ? why : "none");
}
}  // namespace

int main() {
    unsigned long long have, need;
    size_t pairs = 0;
    while (std::scanf("%llu %llu", &have, &need) == 2) {
        const size_t cap = hiprz::gather_capacity(size_t(have), size_t(need));
        std::printf("%zu\n", cap);
        if (cap && cap <= (1u << 16)) {
            std::vector<hiprz_bake_point> points(cap);
            std::vector<hiprz_gather_texel> texels(cap);
            if (need) std::memset(&points[need - 1], 0, sizeof(hiprz_bake_point)), std::memset(&texels[need - 1], 0, sizeof(hiprz_gather_texel));
        }
        ++pairs;
    }
    const struct {
        bool any_null;
        size_t n;
        uint32_t K;
        bool has_charts;
    } calls[] = {{false, 0, 16, true},
                 {false, 1, 1024, true},
                 {true, 1, 64, true},                        // a null pointer is looked at first
                 {true, 1, 0, false},                        //   ... before the missing table and map
                 {true, ~size_t(0), 0, true},                //   ... and before the size
                 {false, 1, 0, true},                        // no table
                 {false, 1, 0, false},                       //   ... before the missing map
                 {false, 0, 16, false},                      // no map, even for nothing to do
                 {false, ~size_t(0), 16, false},             //   ... before the size
                 {false, (size_t(1) << 27) - 1, 16, true},   // n*K = 2^31 - 16
                 {false, size_t(1) << 27, 16, true},         // n*K = 2^31
                 {false, (size_t(1) << 21) - 1, 1024, true},
                 {false, size_t(1) << 21, 1024, true},
                 {false, ~size_t(0), 64, true},              // no product that wraps
                 {false, (size_t(1) << 58) + 1, 64, true}};  // n*K = 2^64 + 64 wraps to 64
    for (const auto& c : calls) {
        int code = -1;
        const char* why = hiprz::gather_refusal(c.any_null, c.n, c.K, c.has_charts, &code);
        std::printf("refusal: %d %s\n", code, why ? why : "none");
    }

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> good = table_of(16, 3, 0.6f, 0.0f, 0.8f, 7.0f);
    verdict("good", good.data(), 16, 3);
    std::vector<float> t = good;
    t[4 * 47 + 2] = nan;  // the last direction of the table
    verdict("nan", t.data(), 16, 3);
    t = good, t[0] = inf;
    verdict("inf", t.data(), 16, 3);
    t = good, t[4 * 47 + 3] = nan;  // the fourth component is not read
    verdict("nan w", t.data(), 16, 3);
    t = table_of(16, 1, 0.0f, 0.0f, 1.0006f, 0.0f);  // squared 1.0012
    verdict("long", t.data(), 16, 1);
    t = table_of(16, 1, 0.0f, 0.0f, 0.9994f, 0.0f);  // squared 0.9988
    verdict("short", t.data(), 16, 1);
    t = table_of(16, 1, 0.0f, -1.0f, 0.0f, 0.0f);
    verdict("below", t.data(), 16, 1);
    t = table_of(8, 1, 0.0f, 0.0f, 1.0f, 0.0f);
    verdict("K = 8", t.data(), 8, 1);
    t = table_of(48, 1, 0.0f, 0.0f, 1.0f, 0.0f);
    verdict("K = 48", t.data(), 48, 1);
    t = table_of(1024, 2, 0.0f, 0.0f, 1.0f, 0.0f);
    verdict("K = 1024", t.data(), 1024, 2);
    verdict("K = 2048", t.data(), 2048, 1);
    verdict("S = 0", good.data(), 16, 0);
    verdict("S = 65", good.data(), 16, 65);
    verdict("null", nullptr, 16, 1);

    const uint32_t base[3] = {0, HIPRZ_GATHER_NONE, 2};
    std::vector<hiprz_gather_chart> uv(5);
    for (size_t i = 0; i < uv.size(); ++i) uv[i] = hiprz_gather_chart{0.1f * float(i), 0.2f, 0.3f, 0.4f, -2.0f, 7.5f, {0.0f, 0.0f}};
    charts("good", base, 3, uv.data(), 5);
    charts("empty", nullptr, 0, nullptr, 0);
    charts("no charts", base, 3, nullptr, 0);
    charts("no instances", nullptr, 0, uv.data(), 5);
    charts("null base", nullptr, 3, uv.data(), 5);
    charts("null uv", base, 3, nullptr, 5);
    charts("too many", base, 3, uv.data(), 0xFFFFFFFDu);  // refused before a chart is read
    std::vector<hiprz_gather_chart> bad = uv;
    bad[4].v3 = nan;  // the last float that is read
    charts("nan", base, 3, bad.data(), 5);
    bad = uv, bad[0].u1 = -inf;
    charts("inf", base, 3, bad.data(), 5);
    bad = uv, bad[4].zero[1] = nan;  // the padding is not read
    charts("nan padding", base, 3, bad.data(), 5);

    const uint32_t sizes[][2] = {{1, 1}, {16384, 16384}, {0, 4}, {4, 0}, {16385, 1}, {1, 16385}, {0xFFFFFFFFu, 0xFFFFFFFFu}};
    for (const auto& s : sizes) {
        const char* why = hiprz::gather_size_refusal(s[0], s[1]);
        std::printf("size %u %u: %s\n", s[0], s[1], why ? why : "none");
    }
    const struct {
        bool any_null;
        size_t n;
    } composes[] = {{false, 0}, {true, 0}, {false, (size_t(1) << 31) - 1}, {false, size_t(1) << 31}, {true, ~size_t(0)}};
    for (const auto& c : composes) {
        const char* why = hiprz::gather_compose_refusal(c.any_null, c.n);
        std::printf("compose: %s\n", why ? why : "none");
    }

    uint32_t layout[8];
    hiprz_gather_layout(layout);
    hiprz_gather_layout(nullptr);
    std::printf("layout %u %u %u %u %u %u %u %u\n", layout[0], layout[1], layout[2], layout[3], layout[4], layout[5], layout[6], layout[7]);
    std::printf("hash %u %u %u\n", hiprz::gather_hash(0u), hiprz::gather_hash(1u), hiprz::gather_hash(0xFFFFFFFFu));
    std::printf("pairs %zu\n", pairs);
    return 0;
}
