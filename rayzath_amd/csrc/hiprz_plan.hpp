// hiprz_plan.hpp — the launch plan: which kernel instantiation every launch of a render call selects, with which grid and how much
// dynamic LDS, as ONE pure function of a plain record of settings, scene facts and frame facts.  No HIP header: hiprz_plan.cpp builds
// with any C++17 compiler and tests/test_launch_plan.py runs it over its whole input space without a GPU.  hiprz_api.hip fills the
// inputs from a context (plan_inputs) and computes the plan once per render call; the launch units only dispatch on it, and the key of
// a captured graph holds its bytes.
#pragma once
#include <cstdint>

#include "hiprz.h"
#include "hiprz_lds.hpp"

namespace hiprz {

// the HIPRZ_COMPAT_* flags that change the integration (everything but the reprojection of history at a restart)
constexpr uint32_t kIntegratorFlags = HIPRZ_MODE_CUDA_COMPAT & ~HIPRZ_COMPAT_REPROJECTION;

// Everything the selection reads, and nothing else.  Booleans are 0 / 1.
struct PlanInputs {
    // settings (hiprz_set_*, HIPRZ_* environment)
    int32_t pipeline_setting, traversal_mode, lds_scene_override, walk_order, sort_rays, sort_bits, shadow_sort, shadow_packet;
    int32_t defer_shadow_rays, nolight_kernels, trace_waves, batch_waves, batch_segments;
    uint32_t wave_resident_max, xcd_swizzle, heavy_first, mode_flags, spot_samples, direct_samples;
    // the uploaded scene
    uint32_t have_scene, scene_tree, lds_scene, hot_bytes, stack_entries, world_stack_entries, mesh_stack_entries;
    uint32_t n_instances, n_lights, n_textures, n_nodes, top_count, flat_world;
    // the selected camera's frame
    uint32_t have_camera, n_local_tiles;
};

// kernel families; 0 everywhere: the render call does not make this launch
enum : uint32_t { TRACE_NONE, TRACE_COMPAT, TRACE_COOP, TRACE_SKIP, TRACE_WORKGROUP };
enum : uint32_t { SHADOWS_NONE, SHADOWS_PACKET, SHADOWS_PACKET_COLOUR, SHADOWS_COOP3_COLOUR, SHADOWS_COOP4, SHADOWS_SKIP4, SHADOWS_SKIP6 };
enum : uint32_t { FUSED_NONE, FUSED_COMPAT, FUSED_PASS };
enum : uint32_t { BATCH_NONE, BATCH_WAVE, BATCH_WORKGROUP };

struct TraceVariant {    // rz_trace_coop_compat_kernel | rz_trace_coop_kernel<waves, one_leaf> | rz_trace_skip_kernel<waves> | rz_trace_kernel<mode, lds_scene>
    uint32_t family, waves, one_leaf, mode, lds_scene;
    uint32_t grid, block, lds, top_n;
};
struct ShadeVariant {    // rz_shade_kernel<lds_scene, shadow> and, behind the sorts, the kernel that walks the deferred shadow rays
    uint32_t active, lds_scene, shadow;  // shadow: 1 / 3 inline walks, RZ_SHADOW_*
    uint32_t grid, block, lds, top_n;
    uint32_t follow, follow_grid, follow_block, follow_lds, follow_top_n;  // SHADOWS_*
};
struct FusedVariant {    // rz_compat_pass_kernel | rz_pass_kernel<mode, lds_scene>
    uint32_t family, mode, lds_scene;
    uint32_t grid, block, lds;
};
struct BatchVariant {    // rz_wave_batch_kernel<shading, 4, one_leaf> | rz_batch_kernel / rz_batch_seg_kernel<mode, lds_scene, shading, five ? 5 : RZ_MIN_WAVES>
    uint32_t family;
    uint32_t mode;         // 1 LDS stack, 2 workgroup-binned, 4 binned with the one-leaf world
    uint32_t lds_scene;    // the hot blob is staged into LDS
    uint32_t shading;      // 1 general, RZ_SHADOW_NONE, RZ_SHADOW_PLAIN
    uint32_t five;         // the 5-wave build (plain shading only)
    uint32_t one_leaf;
    uint32_t grid, block;  // (the segmented kernel's grid is what the chip holds at once: hiprz_launch_batch_seg.hip)
    uint32_t units;        // tiles of the (swizzle-padded) grid
    uint32_t lds;          // dynamic LDS per workgroup
    uint32_t park_offset;  // where the parked state starts behind the scene blob
    uint32_t segment_cap;  // pass segments per tile; the launcher keeps min(n_passes, cap), 1: the unsegmented kernel
};

// A value: every member is a 32-bit integer, so there is no padding, and plan_launches zero-fills it first — two plans are equal
// exactly when memcmp says so.  No pointers.
struct LaunchPlan {
    uint32_t pipeline;        // 0 fused, 1 split, 2 resident (choose_pipeline)
    uint32_t reported_mode;   // what hiprz_traversal_mode reports
    uint32_t walk_mode;       // walk of the 256-thread pass kernels: 1 LDS stack, 2 workgroup-binned, 3 skip links (the variants hold each launch's own)
    uint32_t lds_scene, blob; // the hot blob is staged into LDS by every workgroup; its bytes (0 when not staged)
    uint32_t tile_grid;       // one workgroup per owned 32x8 tile, padded to a multiple of 8 under the XCD swizzle (the extra ones find no tile)
    uint32_t wave_grid;       // one single-wave workgroup per wave of the shard
    uint32_t stack_lds;       // LDS stack columns of the MODE 1 walk (and of inline shadow rays)
    uint32_t walk_lds;        // workspace of the closest-hit walk
    uint32_t sort_enabled, sort_bits, shadow_sort;
    uint32_t defer_shadows, nee_quads;
    uint32_t wave_resident;   // resident pipeline on a scene that is not staged in LDS: rz_wave_batch_kernel
    uint32_t heavy_units;     // resident kernels, heaviest first: units whose cost is collected and ordered (0: not in this call)
    TraceVariant trace;
    ShadeVariant shade;
    FusedVariant fused;
    BatchVariant batch;
};

int choose_pipeline(const PlanInputs& in);
// `counted`: the instrumented instantiations (hiprz_render_counted).  renderFirstPass or renderCumulativePass never enters a choice.
LaunchPlan plan_launches(const PlanInputs& in, bool counted);

}  // namespace hiprz
