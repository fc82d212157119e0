// light_host_main.cpp — the pure-host unit of light baking (rayzath_amd/csrc/light/hiprz_light_host.cpp) as a process of its own, for
// tests/test_light_abi.py to build under sanitizers: reads "have need" pairs from stdin, prints light_capacity of each (buffers of that
// capacity are allocated and touched where `need` ends, as grow_staging uses the figure), then the refusals of a fixed list of calls in
// the order they are looked at, the verdicts of the table validator on a fixed list of tables, the range rule on a fixed list of ranges,
// and the host-only calls of the header.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hiprz_light.h"
#include "hiprz_light_host.hpp"

namespace {
// a table of K * S copies of (x, y)
std::vector<float> table_of(uint32_t K, uint32_t S, float x, float y) {
    std::vector<float> t(2 * size_t(K) * S);
    for (size_t i = 0; i < t.size(); i += 2) t[i] = x, t[i + 1] = y;
    return t;
}
void verdict(const char* name, const float* xy, uint32_t K, uint32_t S) {
    const char* why = hiprz::light_table_refusal(xy, K, S);
    std::printf("table %s: %s\n", name, why ? why : "none");
}
void range(const char* name, const hiprz_light_range* r, uint32_t n_spot, uint32_t n_direct) {
    hiprz::LightSpan span;
    const char* why = hiprz::light_range_refusal(r, n_spot, n_direct, &span);
    if (why) std::printf("range %s: %s\n", name, why);
    else std::printf("range %s: %u %u %u %u\n", name, span.spot_first, span.spots, span.direct_first, span.directs);
}
}  // namespace

int main() {
    unsigned long long have, need;
    size_t pairs = 0;
    while (std::scanf("%llu %llu", &have, &need) == 2) {
        const size_t cap = hiprz::light_capacity(size_t(have), size_t(need));
        std::printf("%zu\n", cap);
        if (cap && cap <= (1u << 16)) {
            std::vector<hiprz_bake_point> points(cap);
            std::vector<hiprz_light_texel> texels(cap);
            if (need) std::memset(&points[need - 1], 0, sizeof(hiprz_bake_point)), std::memset(&texels[need - 1], 0, sizeof(hiprz_light_texel));
        }
        ++pairs;
    }
    const struct {
        bool any_null;
        size_t n;
        uint32_t K;
    } calls[] = {{false, 0, 16},
                 {false, 1, 1},
                 {true, 1, 64},                       // a null pointer is looked at first
                 {true, 1, 0},                        //   ... before the missing table
                 {true, ~size_t(0), 0},               //   ... and before the size
                 {false, 1, 0},                       // no table
                 {false, 0, 0},                       //   ... even for nothing to do
                 {false, ~size_t(0), 0},              //   ... before the size
                 {false, (size_t(1) << 31) - 1, 1},   // n*K = 2^31 - 1
                 {false, size_t(1) << 31, 1},         // n*K = 2^31
                 {false, (size_t(1) << 21) - 1, 1024},
                 {false, size_t(1) << 21, 1024},
                 {false, ~size_t(0), 64},             // no product that wraps
                 {false, (size_t(1) << 58) + 1, 64}};  // n*K = 2^64 + 64 wraps to 64
    for (const auto& c : calls) {
        int code = -1;
        const char* why = hiprz::light_refusal(c.any_null, c.n, c.K, &code);
        std::printf("refusal: %d %s\n", code, why ? why : "none");
    }
    const struct {
        size_t n;
        uint32_t K, L;
    } rays[] = {{1, 1, 0}, {(size_t(1) << 31) - 1, 1, 0}, {(size_t(1) << 31) - 1, 1, 1}, {size_t(1) << 30, 1, 2}, {(size_t(1) << 30) - 1, 1, 2}, {715827882, 1, 3},
                {715827883, 1, 3}, {(size_t(1) << 21) - 1, 1024, 1}, {size_t(1) << 20, 1024, 2}, {1, 1024, 0xFFFFFFFFu}, {1, 1, 0x7FFFFFFFu}, {1, 1, 0x80000000u}};
    for (const auto& c : rays) {
        const char* why = hiprz::light_rays_refusal(c.n, c.K, c.L);
        std::printf("rays: %s\n", why ? why : "none");
    }

    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    std::vector<float> good = table_of(16, 3, 0.75f, -0.5f);
    verdict("good", good.data(), 16, 3);
    std::vector<float> t = good;
    t[2 * 47 + 1] = nan;  // the last sample of the table
    verdict("nan", t.data(), 16, 3);
    t = good, t[0] = inf;
    verdict("inf", t.data(), 16, 3);
    t = good, t[2 * 47] = std::nextafter(1.0f, 2.0f), t[2 * 47 + 1] = 0.0f;  // the last sample, one ulp outside
    verdict("just outside", t.data(), 16, 3);
    t = table_of(16, 1, 0.0f, 1.0f);
    verdict("on the rim", t.data(), 16, 1);
    t = table_of(16, 1, 0.0f, -1.0000001f);
    verdict("behind the rim", t.data(), 16, 1);
    t = table_of(16, 1, 0.0f, 0.0f);
    verdict("centre", t.data(), 16, 1);
    t = table_of(1, 1, 0.5f, 0.5f);
    verdict("K = 1", t.data(), 1, 1);
    t = table_of(48, 1, 0.0f, 0.0f);
    verdict("K = 48", t.data(), 48, 1);
    verdict("K = 0", t.data(), 0, 1);
    t = table_of(1024, 2, 0.0f, 0.0f);
    verdict("K = 1024", t.data(), 1024, 2);
    verdict("K = 2048", t.data(), 2048, 1);
    verdict("S = 0", good.data(), 16, 0);
    verdict("S = 65", good.data(), 16, 65);
    t = table_of(16, 64, 1.0f, 0.0f);
    verdict("S = 64", t.data(), 16, 64);
    verdict("null", nullptr, 16, 1);

    const hiprz_light_range all = {0, HIPRZ_LIGHT_TO_END, 0, HIPRZ_LIGHT_TO_END}, one = {1, 1, 0, 0}, tail = {2, HIPRZ_LIGHT_TO_END, 1, 1}, none = {3, 0, 2, HIPRZ_LIGHT_TO_END},
                            behind = {4, 0, 0, 0}, long_ = {1, 3, 0, 0}, dbehind = {0, 0, 3, HIPRZ_LIGHT_TO_END}, dlong = {0, 0, 1, 2}, wrap = {2, 0xFFFFFFFEu, 0, 0};
    range("null", nullptr, 3, 2);
    range("all", &all, 3, 2);
    range("one", &one, 3, 2);
    range("tail", &tail, 3, 2);
    range("none", &none, 3, 2);
    range("no lights", &all, 0, 0);
    range("behind", &behind, 3, 2);
    range("long", &long_, 3, 2);
    range("direct behind", &dbehind, 3, 2);
    range("direct long", &dlong, 3, 2);
    range("wrap", &wrap, 3, 2);

    // the host-only calls of the header: the disk table passes the validator, a refused call writes nothing, the layout, the set
    std::vector<float> disk(2 * size_t(1024) * 64 + 2, 7.0f);
    const int rc = hiprz_light_disk_samples(1024, 64, disk.data());
    std::printf("disk 1024 64: %d, behind %g\n", rc, double(disk[2 * size_t(1024) * 64]));
    verdict("disk", disk.data(), 1024, 64);
    float one_sample[2] = {7.0f, 7.0f};
    const int rc_one = hiprz_light_disk_samples(1, 1, one_sample);  // (before its output is read: arguments are evaluated in no fixed order)
    std::printf("disk 1 1: %d, %.9g %.9g\n", rc_one, double(one_sample[0]), double(one_sample[1]));
    float untouched[2] = {7.0f, 7.0f};
    const int rc_bad = hiprz_light_disk_samples(48, 1, untouched);
    std::printf("disk 48 1: %d, wrote %d\n", rc_bad, int(untouched[0] != 7.0f));
    std::printf("disk null: %d\n", hiprz_light_disk_samples(16, 1, nullptr));
    uint32_t layout[6];
    hiprz_light_layout(layout);
    hiprz_light_layout(nullptr);
    std::printf("layout %u %u %u %u %u %u\n", layout[0], layout[1], layout[2], layout[3], layout[4], layout[5]);
    std::printf("set_of %u %u %u %u\n", hiprz_light_set_of(1, 0, 64), hiprz_light_set_of(0, 1, 7), hiprz_light_set_of(9, 9, 5), hiprz_light_set_of(4, 2, 0));
    std::printf("pairs %zu\n", pairs);
    return 0;
}
