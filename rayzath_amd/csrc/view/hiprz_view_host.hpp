// hiprz_view_host.hpp — the pure-host half of the baked view (include/hiprz_view.h): what a call is refused for before a device is asked
// anything, the checks of the chart map, the params and the field, the launch grid and the growth rule of the handle's staging.  No HIP
// header: tests/test_view_abi.py compiles hiprz_view_host.cpp with g++ under sanitizers beside a main of its own.  Not part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

struct hiprz_gather_chart;
struct hiprz_view_params;
struct hiprz_view_field;
struct hiprz_field_grid;
struct hiprz_field_params;

// 1: thread i of the view's kernels is pixel i of the row-major frame, as in the query's kernels; 0 (shipped): a wave is an 8 x 8 block of
// pixels.  The same bytes either way (make VIEW_DEFS=-DRZ_VIEW_ROWS).
#ifdef RZ_VIEW_ROWS
#define RZ_VIEW_ROWS_BUILD 1
#else
#define RZ_VIEW_ROWS_BUILD 0
#endif

namespace hiprz {

constexpr size_t kViewMaxPixels = 0x7FFFFFFFull;  // 2^31 - 1, the most pixels hiprz_query_pixel_rays takes
constexpr size_t kViewMaxProbes = size_t(1) << 31;

// nullptr when set_charts takes the map, else what is wrong with it: hiprz_gather_set_charts's checks
const char* view_charts_refusal(const uint32_t* base, uint32_t n_instances, const hiprz_gather_chart* uv, uint32_t n_charts);

// nullptr when a view takes the params, else what is wrong (a null pointer included)
const char* view_params_refusal(const hiprz_view_params* params);

// hiprz_field_check_grid's and hiprz_field_check_params's rules, restated: nullptr or what is wrong (a null pointer included)
const char* view_grid_refusal(const hiprz_field_grid* grid, size_t n_probes);
const char* view_field_params_refusal(const hiprz_field_params* params);

// nullptr when a view may go on to ask for the context's view, else what is wrong with it and the return code in *code.  In the header's
// order: a null pointer (any_null, or a field without grid, probes or records), no chart map (HIPRZ_ERR_STATE), W or H outside
// 1 .. 16384, the params (null: the defaults), the field's grid, the field's params (null: the defaults).
const char* view_refusal(bool any_null, bool has_charts, uint32_t W, uint32_t H, const hiprz_view_params* params, const hiprz_view_field* field, int* code);

// nullptr when a frame of width x height pixels can be viewed (at most 2^31 - 1 pixels)
const char* view_pixels_refusal(uint32_t width, uint32_t height);

// workgroups of 64 threads for a frame: 8 x 8 blocks (rows == false) or 64 consecutive pixels (rows)
uint32_t view_groups(uint32_t width, uint32_t height, bool rows);

// the capacity (in records) a staging of `have` takes on to hold `need`: the query staging's rule (doubling, at least 4096)
size_t view_capacity(size_t have, size_t need);

}  // namespace hiprz
