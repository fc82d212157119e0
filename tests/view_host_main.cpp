// view_host_main.cpp — the pure-host unit of the baked view (rayzath_amd/csrc/view/hiprz_view_host.cpp) as a program of its own:
// tests/test_view_abi.py builds it with -fsanitize=address,undefined and reads what it prints.  The chart check, the params check case by
// case, the field's grid and params, every refusal in the header's order, the pixel count, the launch grid, the growth rule and the layout.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "hiprz_view.h"
#include "hiprz_view_host.hpp"

using namespace hiprz;

static const char* text(const char* why) { return why ? why : "none"; }

int main() {
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    // the chart map: hiprz_gather_set_charts's checks
    std::vector<uint32_t> base{0u, HIPRZ_GATHER_NONE, 2u};
    std::vector<hiprz_gather_chart> uv(4, hiprz_gather_chart{0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 1.0f, {nan, inf}});  // the padding is not looked at
    std::printf("charts: %s\n", text(view_charts_refusal(base.data(), 3u, uv.data(), 4u)));
    std::printf("charts: %s\n", text(view_charts_refusal(nullptr, 0u, nullptr, 0u)));
    std::printf("charts: %s\n", text(view_charts_refusal(nullptr, 3u, uv.data(), 4u)));
    std::printf("charts: %s\n", text(view_charts_refusal(base.data(), 3u, nullptr, 4u)));
    std::printf("charts: %s\n", text(view_charts_refusal(base.data(), 3u, uv.data(), 0xFFFFFFFDu)));  // (refused before a chart is read)
    uv[3].v2 = nan;
    std::printf("charts: %s\n", text(view_charts_refusal(base.data(), 3u, uv.data(), 4u)));
    std::printf("charts: %s\n", text(view_charts_refusal(base.data(), 3u, uv.data(), 3u)));  // the first three alone are sound
    // the params, case by case
    hiprz_view_params good{HIPRZ_VIEW_BILINEAR, {0u, 0u, 0u}};
    std::printf("params: %d %s\n", hiprz_view_check_params(&good), text(view_params_refusal(&good)));
    std::printf("params: %d %s\n", hiprz_view_check_params(nullptr), text(view_params_refusal(nullptr)));
    for (uint32_t f : {0u, 1u, 2u, 0xFFFFFFFFu}) {
        hiprz_view_params p = good;
        p.filter = f;
        std::printf("filter %u: %d %s\n", f, hiprz_view_check_params(&p), text(view_params_refusal(&p)));
    }
    for (int k = 0; k < 3; ++k) {
        hiprz_view_params p = good;
        p.reserved[k] = 1u;
        std::printf("reserved %d: %d %s\n", k, hiprz_view_check_params(&p), text(view_params_refusal(&p)));
    }
    // the field's grid and params: hiprz_field_check_grid's and hiprz_field_check_params's rules
    hiprz_field_grid grid{{-1.0f, 0.0f, 0.5f}, {1.0f, 1.0f, 0.0f}, {3u, 2u, 1u}, 0u};
    std::printf("grid: %s\n", text(view_grid_refusal(&grid, 6u)));
    std::printf("grid: %s\n", text(view_grid_refusal(nullptr, 6u)));
    std::printf("grid: %s\n", text(view_grid_refusal(&grid, 5u)));
    {
        hiprz_field_grid g = grid;
        g.n[2] = 0u;
        std::printf("grid: %s\n", text(view_grid_refusal(&g, 0u)));
        g = grid, g.n[0] = 65536u, g.n[1] = 32768u;
        std::printf("grid: %s\n", text(view_grid_refusal(&g, size_t(1) << 31)));
        g = grid, g.lo[1] = inf;
        std::printf("grid: %s\n", text(view_grid_refusal(&g, 6u)));
        for (float v : {0.0f, -1.0f, nan, inf}) {
            g = grid, g.step[1] = v;
            std::printf("grid step: %s\n", text(view_grid_refusal(&g, 6u)));
        }
        g = grid, g.step[2] = nan;  // a step of an axis with one probe is not read
        std::printf("grid: %s\n", text(view_grid_refusal(&g, 6u)));
    }
    hiprz_field_params fp{0.02f, 4u, {0u, 0u}};
    std::printf("field params: %s\n", text(view_field_params_refusal(&fp)));
    std::printf("field params: %s\n", text(view_field_params_refusal(nullptr)));
    for (float v : {-1.0e-30f, nan, inf}) {
        hiprz_field_params p = fp;
        p.bias = v;
        std::printf("field params: %s\n", text(view_field_params_refusal(&p)));
    }
    // a view's refusals, in the header's order: each call is wrong in everything that follows what it is refused for
    const int dummy = 0;
    const hiprz_bake_point* probes = reinterpret_cast<const hiprz_bake_point*>(&dummy);  // never read
    const hiprz_probe_sh* sh = reinterpret_cast<const hiprz_probe_sh*>(&dummy);
    hiprz_view_params bad_params{7u, {0u, 0u, 0u}};
    hiprz_field_grid bad_grid = grid;
    bad_grid.step[0] = 0.0f;
    hiprz_field_params bad_fp{-1.0f, 0u, {0u, 0u}};
    const hiprz_view_field whole{&grid, probes, sh, nullptr, 6u, &fp}, no_probes{&grid, nullptr, sh, nullptr, 6u, &fp}, no_grid{nullptr, probes, sh, nullptr, 6u, &fp};
    const hiprz_view_field wrong_grid{&bad_grid, probes, sh, nullptr, 6u, &bad_fp}, wrong_fp{&grid, probes, sh, nullptr, 6u, &bad_fp}, defaults{&grid, probes, sh, nullptr, 6u, nullptr};
    struct { bool any_null, has_charts; uint32_t W, H; const hiprz_view_params* params; const hiprz_view_field* field; } calls[] = {
        {false, true, 64u, 48u, &good, &whole},     {false, true, 1u, 16384u, nullptr, nullptr}, {false, true, 4u, 3u, nullptr, &defaults},
        {true, false, 0u, 0u, &bad_params, &wrong_grid}, {false, false, 0u, 0u, &bad_params, &no_probes}, {false, false, 0u, 0u, &bad_params, &no_grid},
        {false, false, 0u, 0u, &bad_params, &wrong_grid}, {false, true, 0u, 48u, &bad_params, &wrong_grid}, {false, true, 64u, 16385u, &bad_params, &wrong_grid},
        {false, true, 64u, 48u, &bad_params, &wrong_grid}, {false, true, 64u, 48u, &good, &wrong_grid},  {false, true, 64u, 48u, &good, &wrong_fp}};
    for (const auto& c : calls) {
        int code = -1;
        const char* why = view_refusal(c.any_null, c.has_charts, c.W, c.H, c.params, c.field, &code);
        std::printf("view: %d %s\n", code, text(why));
    }
    std::printf("pixels: %s | %s | %s | %s\n", text(view_pixels_refusal(0u, 0u)), text(view_pixels_refusal(46341u, 46340u)), text(view_pixels_refusal(65536u, 32768u)),
                text(view_pixels_refusal(0xFFFFFFFFu, 0xFFFFFFFFu)));
    std::printf("groups %u %u %u %u %u %u\n", view_groups(32u, 24u, false), view_groups(33u, 19u, false), view_groups(1u, 1u, false), view_groups(32u, 24u, true),
                view_groups(33u, 19u, true), view_groups(1u, 1u, true));
    std::printf("capacity %zu %zu %zu %zu\n", view_capacity(0, 1), view_capacity(4096, 4097), view_capacity(100, 50), view_capacity(size_t(1) << 30, (size_t(1) << 30) + 1));
    uint32_t layout[8];
    hiprz_view_layout(layout);
    hiprz_view_layout(nullptr);
    std::printf("layout %u %u %u %u %u %u %u %u\n", layout[0], layout[1], layout[2], layout[3], layout[4], layout[5], layout[6], layout[7]);
    return 0;
}
