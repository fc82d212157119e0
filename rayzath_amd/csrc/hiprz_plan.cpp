// hiprz_plan.cpp — the launch plan (hiprz_plan.hpp): every "which kernel when" rule of the library, stated once, with the measurement
// that justifies it.  Plain integer logic, no HIP header.
#include "hiprz_plan.hpp"

#include <algorithm>

namespace hiprz {
namespace {

constexpr uint32_t kBatchSegments = 2u;  // pass segments per tile where the grid oversubscribes the chip (B: S = 2 +2.0 %, 3 +0.6 %, 4 -0.5 %, 8 -7.6 %)

bool lights(const PlanInputs& in) { return in.n_lights != 0u; }
bool integrator(const PlanInputs& in) { return (in.mode_flags & kIntegratorFlags) != 0u; }
bool rebuilt_trees(const PlanInputs& in) { return in.scene_tree != HIPRZ_TREE_REFERENCE; }

bool use_lds_scene(const PlanInputs& in) {
    if (in.lds_scene_override == 0 || rebuilt_trees(in) || integrator(in)) return false;
    if (in.lds_scene_override == 1) return uint64_t(in.hot_bytes) + uint64_t(in.stack_entries) * 1024u <= kLdsPerCu;
    return in.lds_scene != 0u;
}

// what the per-wave chains of passes (rz_wave_batch_kernel) need besides the resident pipeline: a scene that is not staged in LDS, the
// front-to-back walk (mode 3) and no lights (shadow rays are deferred to a kernel of their own otherwise)
bool dark_capable(const PlanInputs& in) {
    return !use_lds_scene(in) && !lights(in) && in.nolight_kernels && in.walk_order != 0 && (in.traversal_mode == -1 || in.traversal_mode == 3);
}

// The binned walk pays off when a mesh visit is short and uniform (every mesh tree is a single leaf, e.g. the
// Cornell configs: 329 vs 370 us per pass); with deep mesh trees a round lasts as long as its slowest item
// and the nested walk is faster (config C: 1 668 vs 2 450 us).
int reported_mode(const PlanInputs& in, int pipeline) {
    if (rebuilt_trees(in) || integrator(in)) return 3;  // rebuilt trees: the front-to-back cooperative walks only; compat integrator: the cooperative walk, or the fused kernel's skip-link walk
    if (in.traversal_mode >= 0) return in.traversal_mode;
    // records do not fit LDS: skip-link walks in single-wave workgroups
    if (!in.lds_scene && pipeline == 1) return 3;
    return in.mesh_stack_entries <= 2u ? 2 : 1;
}

// front-to-back mesh walks on per-octant skip links (the cooperative kernels) against the reference's child order, which the work
// counters are anchored on: counted renders keep that order unless asked otherwise (hiprz_set_walk_order(2))
bool front_to_back(const PlanInputs& in, bool counted) { return (counted ? in.walk_order == 2 : in.walk_order != 0) || rebuilt_trees(in); }

// the reference's child order, tree tops cached in LDS: 160 KiB over 24 (6 waves per SIMD: big trees want occupancy) or 16 (4)
// single-wave workgroups per CU
bool big_trees(const PlanInputs& in) { return in.trace_waves > 0 ? in.trace_waves >= 6 : in.n_nodes > kLatencyBoundNodes; }
uint32_t skip_top_n(const PlanInputs& in) { return std::min<uint32_t>(in.top_count, big_trees(in) ? 170u : 272u); }

// the plain one-step world level (the general world level costs D's 5-wave build 3.5 %, C's 4-wave build 0.5 %)
bool one_leaf_world(const PlanInputs& in) { return in.n_instances != 0u && in.flat_world; }

// mode of a 256-thread kernel that has the binned walk: with the whole scene in LDS and a one-leaf world the instance boxes are tested up front
uint32_t workgroup_mode(const PlanInputs& in, const LaunchPlan& p, uint32_t mode) { return mode == 2u ? (p.lds_scene && in.flat_world ? 4u : 2u) : 1u; }

void plan_trace(const PlanInputs& in, bool counted, const LaunchPlan& p, TraceVariant& t) {
    t.grid = p.wave_grid, t.block = 64u, t.lds = kCoopLdsBytes;
    if (integrator(in)) {  // CUDA-compat integrator on the split pipeline: the cooperative walk + the medium's scattering distance
        t.family = TRACE_COMPAT;
    } else if (p.walk_mode == 3u && front_to_back(in, counted)) {
        // one wave per workgroup: a workgroup's slot is free as soon as ITS slowest ray is done.  Front-to-back mesh walks on per-octant
        // skip links with the cooperative triangle phase.  Register budget: 112 VGPRs are what the kernel wants (4 waves per SIMD, no
        // scratch); trees that do not live in L1 / L2 are bound by the latency of their node fetches and take a fifth wave at the price
        // of 52 B of scratch (D: 1 014 -> 964 us; C 342 -> 351, E 3 082 -> 3 279 us)
        const int waves = in.trace_waves > 0 ? in.trace_waves : (in.n_nodes > kLatencyBoundNodes ? 5 : 4);
        t.family = TRACE_COOP;
        t.waves = waves == 5 ? 5u : waves >= 6 ? 6u : 4u;
        t.one_leaf = one_leaf_world(in) && t.waves != 6u;
    } else if (p.walk_mode == 3u) {
        t.family = TRACE_SKIP;
        t.waves = big_trees(in) ? 6u : 4u;
        t.top_n = skip_top_n(in), t.lds = t.top_n * kTopNodeBytes;
    } else {
        t.family = TRACE_WORKGROUP;
        t.mode = workgroup_mode(in, p, p.walk_mode), t.lds_scene = p.lds_scene;
        t.grid = p.tile_grid, t.block = 256u, t.lds = p.blob + p.walk_lds;
    }
}

// The deferred shadow rays in their own sorted order (slot set, light, origin cell) reach the kernel as BEAMS — 64 rays from one cell towards
// one light — and the wave walks the trees for all of them at once (rz_shadow_packet_kernel; round 4, config E: shadow kernel 1 449 ->
// about 1 160 us, step 37.5 -> 35.2 ms, identical frames).  Not for counted passes (the work counters are anchored on the per-lane walks)
// not where the shadow rays follow the next pass's ray order (HIPRZ_SHADOW_SORT=0: no beams), and not for small frames of many instances (wide
// beams: below).  HIPRZ_SHADOW_PACKET=0 / 1: never / always.
bool shadow_beams(const PlanInputs& in, bool counted, const LaunchPlan& p) {
    if (counted || in.shadow_packet == 0 || !p.shadow_sort) return false;
    // how narrow the beams are goes with the rays per light and cell: the living room at 40 instances 1.09x (4K) / 1.06x (1080p) / 1.05x (960 x 540) /
    // 0.97x (480 x 270) of the cooperative walk's pass, at 300 instances 0.98x (1080p) / 0.88x (480 x 270) — tools/ab_shadow_walks.py
    return in.shadow_packet > 0 || uint64_t(in.n_local_tiles) * 256u >= uint64_t(8192) * in.n_instances;
}

void plan_shade(const PlanInputs& in, bool counted, const LaunchPlan& p, ShadeVariant& s) {
    s.active = 1u, s.grid = p.tile_grid, s.block = 256u;
    const bool colour = (in.mode_flags & HIPRZ_COMPAT_SHADOW_COLOR) != 0u;
    if (integrator(in)) {
        // CUDA-compat integrator: the same packaging as below — shading, then (scenes with lights) the pass's shadow rays in the lean
        // cooperative kernel in their own sorted order; with HIPRZ_COMPAT_SHADOW_COLOR its mask-collecting instantiation (round 4):
        // the rays go through what they cross and collect the opacity colours
        s.shadow = p.defer_shadows ? RZ_SHADOW_COMPAT_DEFER : RZ_SHADOW_COMPAT;
        if (p.defer_shadows) s.follow = colour ? (shadow_beams(in, counted, p) ? SHADOWS_PACKET_COLOUR : SHADOWS_COOP3_COLOUR) : (shadow_beams(in, counted, p) ? SHADOWS_PACKET : SHADOWS_COOP4);
    } else if (!lights(in) && in.nolight_kernels) {
        // no next-event estimation: the instantiation without it (no shadow walk, no LDS stack); no maps either: the one without
        // texture fetches and normal mapping
        s.shadow = in.n_textures == 0u ? RZ_SHADOW_PLAIN : RZ_SHADOW_NONE;
        s.lds_scene = p.lds_scene, s.lds = p.blob;
    } else if (p.lds_scene) {  // shadow rays inline: LDS-stack walk on the staged scene
        s.shadow = 1u, s.lds_scene = 1u, s.lds = p.blob + p.stack_lds;
    } else if (p.defer_shadows) {
        // shading without shadow walks, then every shadow ray of the pass in a lean single-wave kernel
        s.shadow = RZ_SHADOW_DEFER;
        s.follow = shadow_beams(in, counted, p) ? SHADOWS_PACKET : front_to_back(in, counted) ? SHADOWS_COOP4 : big_trees(in) ? SHADOWS_SKIP6 : SHADOWS_SKIP4;
    } else {  // shadow rays inline on skip links with the tree tops staged in LDS
        s.shadow = 3u;
        s.top_n = std::min<uint32_t>(in.top_count, kTopCacheNodes), s.lds = s.top_n * kTopNodeBytes;
    }
    if (s.follow == SHADOWS_NONE) return;
    s.follow_grid = p.wave_grid, s.follow_block = 64u;
    if (s.follow == SHADOWS_SKIP4 || s.follow == SHADOWS_SKIP6) s.follow_top_n = skip_top_n(in), s.follow_lds = s.follow_top_n * kTopNodeBytes;
    else s.follow_lds = s.follow == SHADOWS_PACKET ? kPacketLdsBytes : s.follow == SHADOWS_PACKET_COLOUR ? kPacketMaskLdsBytes : kCoopLdsBytes;
}

void plan_fused(const PlanInputs& in, const LaunchPlan& p, FusedVariant& f) {
    f.grid = p.tile_grid, f.block = 256u;
    if (integrator(in)) {  // CUDA-compat mode: its own fused kernel on the global scene
        f.family = FUSED_COMPAT;
        return;
    }
    // the fused kernel's shadow rays use the stack walk: its columns must exist in every mode
    f.family = FUSED_PASS;
    f.mode = workgroup_mode(in, p, p.walk_mode), f.lds_scene = p.lds_scene;
    f.lds = p.blob + p.walk_lds + (p.walk_mode == 2u ? kFusedParkBytes : 0u);  // mode 2: + the parked path state
}

void plan_batch(const PlanInputs& in, bool counted, const LaunchPlan& p, BatchVariant& b) {
    b.segment_cap = 1u;
    // counted renders report the work of the reference's visiting order unless asked otherwise (hiprz_set_walk_order): those keep the
    // workgroup kernel with its stack walk in that order
    const bool reference_counters = counted && in.walk_order != 2 && !rebuilt_trees(in);
    // scenes without lights run the instantiation whose next-event-estimation code is compiled out (RZ_SHADOW_NONE), scenes that
    // have no maps either the one without texture fetches and normal mapping (RZ_SHADOW_PLAIN)
    const bool dark = !lights(in) && in.nolight_kernels;
    const bool plain = dark && in.n_textures == 0u;
    if (p.wave_resident && !reference_counters) {  // scenes that are not staged in LDS, without lights: single-wave workgroups walk cooperatively, pass after pass
        b.family = BATCH_WAVE;
        b.mode = 3u, b.shading = plain ? RZ_SHADOW_PLAIN : RZ_SHADOW_NONE, b.one_leaf = one_leaf_world(in);
        b.grid = b.units = p.wave_grid, b.block = 64u, b.lds = kCoopLdsBytes;
        return;
    }
    const uint32_t mode = p.wave_resident ? 1u : p.walk_mode, walk_lds = p.wave_resident ? p.stack_lds : p.walk_lds;
    b.family = BATCH_WORKGROUP;
    b.mode = workgroup_mode(in, p, mode), b.lds_scene = p.lds_scene;
    b.shading = plain ? RZ_SHADOW_PLAIN : dark ? RZ_SHADOW_NONE : 1u;
    b.grid = b.units = p.tile_grid, b.block = 256u;
    b.lds = p.blob + walk_lds + kBatchParkBytes, b.park_offset = walk_lds;
    // 5 workgroups per CU must fit LDS, and the grid must be more than two full loads of the chip (256 CUs x 5)
    b.five = plain && uint64_t(b.lds) * 5u <= kLdsPerCu && b.grid > 2u * 5u * 256u && in.batch_waves != 4;
    // Pass segments (rz_batch_seg_kernel): where the grid oversubscribes the chip, the launch otherwise ends on whole tiles' chains of
    // passes; measured on config B.  A grid that fits the chip in one round has no such tail.  HIPRZ_BATCH_SEGMENTS
    // forces S everywhere (1: the unsegmented kernel).
    b.segment_cap = in.batch_segments > 0 ? uint32_t(in.batch_segments) : (b.five ? kBatchSegments : 1u);
}

}  // namespace

// 0 fused (one kernel per pass), 1 split (trace kernel -> shade kernel per pass), 2 resident (one kernel per batch of passes).
// Setting -1: resident when the scene is staged in LDS (config B: as fast as split on a whole frame, 2.26 ms per 8 passes, and 0.34 vs
// 0.45 ms on an eighth of it — per-pass launch/ramp/tail costs vanish), else split (10-20 % faster than fused on configs C, D; the
// resident kernel has no LDS room for the tree-top cache).
int choose_pipeline(const PlanInputs& in) {
    // a shard small enough to be ONE round of waves on the chip pays the slowest wave of every kernel of every pass in the split
    // pipeline; without lights it runs per-wave chains of passes instead (hiprz_kernels.hpp: rz_wave_batch_kernel).
    // HIPRZ_WAVE_RESIDENT_MAX: scenes without lights that are not staged in LDS run the resident pipeline (rz_wave_batch_kernel) while
    // a shard has at most this many waves — no limit since the end of round 3.  Measured on MI355X, split / resident, ms per step of 8
    // passes: an eighth of a 1080p frame C 1.18 / 0.61, D 3.78 / 2.69; half C 2.46 / 1.86, D 5.79 / 3.91; a whole frame (32 400 waves),
    // since the walk's instance level: C 3.69 / 3.38, D 7.28 / 7.19 (it was C 3.78 / 3.82 before); a 4K frame (129 600 waves): C 14.26
    // / 12.73, D 27.26 / 27.18.  (The kernel keeps the register budget of 4 waves per SIMD: with 5 — what D's trace kernel likes — the
    // shading spills: D 7.18 -> 7.51, C 3.38 -> 3.81 ms per step.)
    const bool dark = in.have_scene && dark_capable(in);
    const bool small_dark_shard = dark && in.have_camera && in.n_local_tiles != 0u && in.n_local_tiles * 4u <= in.wave_resident_max;
    if (integrator(in)) return in.pipeline_setting == 0 ? 0 : 1;  // CUDA-compat integrator: split (sorted rays, cooperative walks, deferred shadow rays); 0 = one fused kernel per pass
    if (rebuilt_trees(in))  // rebuilt trees: the front-to-back cooperative walks only (split, or per-wave resident)
        return dark && (in.pipeline_setting == 2 || (in.pipeline_setting < 0 && small_dark_shard)) ? 2 : 1;
    if (in.pipeline_setting >= 0) return in.pipeline_setting;
    if (small_dark_shard) return 2;
    // resident needs blob + walk workspace + 8 KiB of parked state per workgroup, four workgroups per CU
    const uint64_t lds = uint64_t(in.hot_bytes) + uint64_t(in.stack_entries) * 1024u + kBinnedFixedBytes + kBatchParkBytes;
    const bool mode_ok = in.traversal_mode == -1 || in.traversal_mode == 1 || in.traversal_mode == 2;  // walks the batch kernel has
    return in.have_scene && in.lds_scene && in.lds_scene_override != 0 && mode_ok && lds <= 40u * 1024u ? 2 : 1;
}

LaunchPlan plan_launches(const PlanInputs& in, bool counted) {
    LaunchPlan p{};
    const int pipeline = choose_pipeline(in);
    p.pipeline = uint32_t(pipeline);
    p.lds_scene = use_lds_scene(in), p.blob = p.lds_scene ? in.hot_bytes : 0u;
    p.wave_resident = pipeline == 2 && dark_capable(in);
    p.reported_mode = p.walk_mode = uint32_t(reported_mode(in, pipeline));
    if (p.walk_mode >= 3u && (p.lds_scene || (pipeline != 1 && !p.wave_resident))) p.walk_mode = 1u;  // skip links are for scenes that are not staged whole: trace kernel, wave batch kernel
    p.tile_grid = in.xcd_swizzle ? ((in.n_local_tiles + 7u) / 8u) * 8u : in.n_local_tiles;
    p.wave_grid = in.n_local_tiles * 4u;
    p.stack_lds = in.stack_entries * 1024u;
    p.walk_lds = p.walk_mode == 2u ? kBinnedFixedBytes + (in.world_stack_entries + in.mesh_stack_entries) * kBinnedEntryBytes : p.walk_mode == 1u ? p.stack_lds : 0u;
    // Shadow rays get their own kernel when the scene has lights, is not staged in LDS (split pipeline) and the sample slots of a
    // segment fit the 30-bit mask of the hand-over record.
    p.defer_shadows = in.defer_shadow_rays && pipeline == 1 && !p.lds_scene && lights(in) && in.spot_samples + in.direct_samples <= 30u;
    p.nee_quads = 4u + 2u * (in.spot_samples + in.direct_samples);
    // Rays are reordered where the walk is bound by scattered fetches: scenes not staged in LDS, split pipeline.  Measured (1920x1080+,
    // MODE 3; the sort itself costs ~0.12 ms per pass at 1080p): many small instances (config E, 46) 33.9 -> 26.5 ms per pass; one
    // mid-size mesh (config C, 12 k nodes) trace kernel 853 -> 645 us, step 7.70 -> 6.98 ms; one big mesh (config D, 600 k nodes) trace
    // kernel 2 656 -> 2 586 us but step 22.5 -> 23.2 ms.  So: on for many instances, and for trees small enough that a coherent wave
    // finds its nodes in LDS / L2.
    p.sort_enabled = pipeline == 1 && in.sort_rays != 0 &&
                     (in.sort_rays == 1 || (!p.lds_scene && p.reported_mode >= 3u && (in.n_instances >= 16u || in.n_nodes <= kLatencyBoundNodes)));
    // Two radix passes (16 key bits) are enough while a bin of the coarser order still holds a wave's worth of rays: up to ~2 M owned
    // pixels (config C: step 4.53 -> 4.33 ms, the sort 88 -> 59 us per pass).  Bigger frames and scenes with lights (whose shadow rays
    // follow a sorted order of their own) keep all 24 bits (config E: 16 bits 55.9 ms per step against 51.0).
    p.sort_bits = in.sort_bits > 0 ? uint32_t(in.sort_bits) : (!lights(in) && uint64_t(in.n_local_tiles) * 256u <= (uint64_t(32) << 16)) ? 16u : 24u;
    p.shadow_sort = p.sort_enabled && in.shadow_sort != 0 && p.defer_shadows;
    // resident kernels, heaviest first: a tile of rz_batch_kernel, a wave of rz_wave_batch_kernel; costs are not collected while counting
    p.heavy_units = pipeline == 2 && in.heavy_first && !counted ? (p.wave_resident ? p.wave_grid : in.n_local_tiles) : 0u;
    if (pipeline == 1 || p.wave_resident) {  // (the first pass of a wave-resident frame: the split kernels)
        plan_trace(in, counted, p, p.trace);
        plan_shade(in, counted, p, p.shade);
    } else {
        plan_fused(in, p, p.fused);
    }
    if (pipeline == 2) plan_batch(in, counted, p, p.batch);
    return p;
}

}  // namespace hiprz
