// probe_host_main.cpp — the pure-host unit of probe baking (rayzath_amd/csrc/probe/hiprz_probe_host.cpp) as a program of its own:
// tests/test_probe_abi.py builds it with -fsanitize=address,undefined and reads what it prints.  Every refusal in the header's order, the
// table, sample and chart checks, the range rule, the sphere table, the evaluation and the layout.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "hiprz_probe.h"
#include "hiprz_probe_host.hpp"

using namespace hiprz;

static const char* text(const char* why) { return why ? why : "none"; }

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the gather's refusals, in order: (any_null, n, K, has_charts)
    struct { bool any_null; size_t n; uint32_t K; bool charts; } gathers[] = {
        {false, 0, 16, true}, {false, 5, 64, true}, {true, 5, 64, true}, {true, 5, 0, false}, {false, 5, 0, true}, {false, 5, 0, false}, {false, 5, 16, false},
        {false, (size_t(1) << 27) - 1, 16, true}, {false, size_t(1) << 27, 16, true}, {false, (size_t(1) << 21) - 1, 1024, true}, {false, size_t(1) << 21, 1024, true}};
    for (const auto& g : gathers) {
        int code = -99;
        const char* why = probe_gather_refusal(g.any_null, g.n, g.K, g.charts, &code);
        std::printf("gather: %d %s\n", code, text(why));
    }
    struct { bool any_null; size_t n; uint32_t K; } lights[] = {{false, 0, 1}, {true, 1, 1}, {true, 1, 0}, {false, 1, 0}, {false, (size_t(1) << 31) - 1, 1}, {false, size_t(1) << 31, 1},
                                                                 {false, size_t(1) << 21, 1024}};
    for (const auto& l : lights) {
        int code = -99;
        const char* why = probe_light_refusal(l.any_null, l.n, l.K, &code);
        std::printf("light: %d %s\n", code, text(why));
    }
    // the direction table
    {
        std::vector<float> good(4 * 16 * 2);
        if (hiprz_probe_sphere_directions(16, 2, good.data()) != HIPRZ_OK) return 1;
        std::printf("table good: %s\n", text(probe_table_refusal(good.data(), 16, 2)));
        auto with = [&](size_t at, float v) { std::vector<float> t = good; t[at] = v; return t; };
        std::printf("table nan: %s\n", text(probe_table_refusal(with(5, nan).data(), 16, 2)));
        std::printf("table inf: %s\n", text(probe_table_refusal(with(4 * 17 + 2, inf).data(), 16, 2)));
        std::printf("table nan w: %s\n", text(probe_table_refusal(with(7, nan).data(), 16, 2)));
        std::vector<float> longer = good;
        for (int c = 0; c < 3; ++c) longer[4 * 3 + c] *= 1.01f;
        std::printf("table long: %s\n", text(probe_table_refusal(longer.data(), 16, 2)));
        std::vector<float> down = good;
        for (size_t i = 2; i < down.size(); i += 4) down[i] = -std::fabs(down[i]);
        std::printf("table below: %s\n", text(probe_table_refusal(down.data(), 16, 2)));
        std::printf("table K = 8: %s\n", text(probe_table_refusal(good.data(), 8, 2)));
        std::printf("table K = 2048: %s\n", text(probe_table_refusal(good.data(), 2048, 1)));
        std::printf("table S = 0: %s\n", text(probe_table_refusal(good.data(), 16, 0)));
        std::printf("table S = 65: %s\n", text(probe_table_refusal(good.data(), 16, 65)));
        std::printf("table null: %s\n", text(probe_table_refusal(nullptr, 16, 1)));
        std::printf("sphere refusals: %d %d %d\n", hiprz_probe_sphere_directions(16, 1, nullptr), hiprz_probe_sphere_directions(48, 1, good.data()),
                    hiprz_probe_sphere_directions(16, 0, good.data()));
        // the formula, for a few entries: z = 1 - 2 (k + 0.5) / K, the squared length 1 within a float's rounding, w = 0
        double worst = 0.0;
        for (int k = 0; k < 16; ++k) {
            const float* d = &good[4 * (16 + k)];
            worst = std::fmax(worst, std::fabs(double(d[2]) - (1.0 - 2.0 * (k + 0.5) / 16.0)));
            worst = std::fmax(worst, std::fabs(double(d[0]) * d[0] + double(d[1]) * d[1] + double(d[2]) * d[2] - 1.0));
            if (d[3] != 0.0f) return 2;
        }
        std::printf("sphere worst: %s\n", worst < 3e-7 ? "ok" : "off");
    }
    // the light's samples
    {
        const float good[8] = {0.0f, 0.0f, 0.5f, 0.5f, -1.0f, 0.0f, 0.6f, -0.8f};
        float outside[8], bad[8];
        std::memcpy(outside, good, sizeof good), std::memcpy(bad, good, sizeof good);
        outside[2] = 0.8f, outside[3] = 0.7f, bad[6] = nan;
        std::printf("samples good: %s\n", text(probe_samples_refusal(good, 4, 1)));
        std::printf("samples K = 1: %s\n", text(probe_samples_refusal(good, 1, 4)));
        std::printf("samples outside: %s\n", text(probe_samples_refusal(outside, 4, 1)));
        std::printf("samples nan: %s\n", text(probe_samples_refusal(bad, 4, 1)));
        std::printf("samples K = 3: %s\n", text(probe_samples_refusal(good, 3, 1)));
        std::printf("samples K = 2048: %s\n", text(probe_samples_refusal(good, 2048, 1)));
        std::printf("samples S = 0: %s\n", text(probe_samples_refusal(good, 4, 0)));
        std::printf("samples null: %s\n", text(probe_samples_refusal(nullptr, 4, 1)));
    }
    // the chart map
    {
        const uint32_t base[2] = {0u, HIPRZ_GATHER_NONE};
        hiprz_gather_chart uv[2];
        std::memset(uv, 0, sizeof uv);
        uv[1].u2 = 0.5f;
        std::printf("charts good: %s\n", text(probe_charts_refusal(base, 2, uv, 2)));
        std::printf("charts empty: %s\n", text(probe_charts_refusal(nullptr, 0, nullptr, 0)));
        std::printf("charts null base: %s\n", text(probe_charts_refusal(nullptr, 2, uv, 2)));
        std::printf("charts null uv: %s\n", text(probe_charts_refusal(base, 2, nullptr, 2)));
        std::printf("charts too many: %s\n", text(probe_charts_refusal(base, 2, uv, HIPRZ_GATHER_MAX_CHARTS + 1u)));
        uv[0].v3 = inf;
        std::printf("charts inf: %s\n", text(probe_charts_refusal(base, 2, uv, 2)));
        uv[0].v3 = 0.0f, uv[1].zero[1] = nan;
        std::printf("charts nan padding: %s\n", text(probe_charts_refusal(base, 2, uv, 2)));
    }
    // the source size
    const uint32_t sizes[][2] = {{1, 1}, {16384, 16384}, {0, 4}, {4, 0}, {16385, 1}, {1, 16385}, {0xFFFFFFFFu, 0xFFFFFFFFu}};
    for (const auto& s : sizes) std::printf("size %u %u: %s\n", s[0], s[1], text(probe_size_refusal(s[0], s[1])));
    // the light range over 3 spot and 2 direct lights
    {
        const hiprz_light_range ranges[] = {{0, HIPRZ_LIGHT_TO_END, 0, HIPRZ_LIGHT_TO_END}, {1, 2, 2, 0}, {3, 0, 0, 1}, {4, 0, 0, 0}, {0, 4, 0, 0}, {0, 0, 3, 0}, {0, 0, 1, 2}};
        ProbeSpan span;
        std::printf("range null: %s", text(probe_range_refusal(nullptr, 3, 2, &span)));
        std::printf(" %u %u %u %u\n", span.spot_first, span.spots, span.direct_first, span.directs);
        for (const auto& r : ranges) {
            const char* why = probe_range_refusal(&r, 3, 2, &span);
            std::printf("range: %s", text(why));
            if (!why) std::printf(" %u %u %u %u", span.spot_first, span.spots, span.direct_first, span.directs);
            std::printf("\n");
        }
    }
    // the evaluation: e = e + ((w_b * sh[b].c) * B_b(n)) in order, +0 for an invalid record
    {
        hiprz_probe_sh rec;
        std::memset(&rec, 0, sizeof rec);
        for (int b = 0; b < 9; ++b)
            for (int c = 0; c < 3; ++c) rec.sh[b][c] = 0.25f * float(b + 1) - 0.5f * float(c);
        const float n[3] = {0.48f, 0.6f, 0.64f};
        float out[3] = {9.0f, 9.0f, 9.0f};
        hiprz_probe_irradiance(&rec, n, out);
        std::printf("irradiance %a %a %a\n", out[0], out[1], out[2]);
        const uint32_t invalid = HIPRZ_PROBE_INVALID;
        std::memcpy(&rec.sh[0][3], &invalid, 4);
        hiprz_probe_irradiance(&rec, n, out);
        std::printf("irradiance invalid %a %a %a\n", out[0], out[1], out[2]);
        hiprz_probe_irradiance(nullptr, n, out);
        hiprz_probe_irradiance(&rec, n, nullptr);
    }
    uint32_t layout[6];
    hiprz_probe_layout(layout);
    hiprz_probe_layout(nullptr);
    std::printf("layout %u %u %u %u %u %u\n", layout[0], layout[1], layout[2], layout[3], layout[4], layout[5]);
    std::printf("hash %u %u %u\n", probe_hash(0u), probe_hash(1u), probe_hash(0xFFFFFFFFu));
    std::printf("capacity %zu %zu %zu\n", probe_capacity(0, 1), probe_capacity(4096, 4097), probe_capacity(100, 50));
    return 0;
}
