// hiprz_lds.hpp — the sizes and ids the launch plan (hiprz_plan.cpp, which includes no HIP header) shares with the device code that
// carves dynamic LDS and is instantiated per shading variant (hiprz_device.hpp, hiprz_kernels.hpp): one definition for both sides.
#pragma once
#include <cstdint>

#ifndef RZ_MIN_WAVES
#define RZ_MIN_WAVES 4
#endif
// shadow-ray handling of a shading instantiation (hiprz_device.hpp describes each where the walks are defined); 1 and 3 are the walk
// MODEs of inline shadow rays
#define RZ_SHADOW_DEFER 4
#define RZ_SHADOW_NONE 5
#define RZ_SHADOW_PLAIN 6
#define RZ_SHADOW_COMPAT 8
#define RZ_SHADOW_COMPAT_DEFER 9

namespace hiprz {

constexpr uint32_t kBinnedFixedBytes = 15u * 1024u;  // BinnedLds: rays, hits, items, bins of a 256-lane workgroup ...
constexpr uint32_t kBinnedEntryBytes = 1024u;        // ... + one stack column per lane for every world and mesh stack entry
constexpr uint32_t kTopNodeBytes = 36u;              // TopCache: two float4 + one skip link per staged node
constexpr uint32_t kCoopLdsBytes = 8u * 1024u;       // CoopLds: per single-wave workgroup
constexpr uint32_t kBatchParkBytes = 8u * 1024u;     // rz_batch_kernel: the parked path state behind scene blob and walk workspace
constexpr uint32_t kFusedParkBytes = 4u * 1024u;     // rz_pass_kernel, binned modes: four words of parked path state per lane behind the walk's workspace
constexpr uint32_t kPacketLdsBytes = 2u * 1024u;     // any_hit_packet: the 64 rays of a leaf's triangle phase, two float4 each ...
constexpr uint32_t kPacketMaskLdsBytes = 3u * 1024u; // ... + one float4 per lane for the crossed triangles' colours (coloured masks)
constexpr uint32_t kLdsPerCu = 160u * 1024u;

constexpr uint32_t kLatencyBoundNodes = 32768u;  // trees beyond ~1 MiB of nodes: fetches come from L2 / HBM, occupancy hides them
constexpr uint32_t kTopCacheNodes = 682u;        // 682 x 36 B = 24 KiB per workgroup: ~9 levels of every tree, 5 workgroups per CU

}  // namespace hiprz
