// hiprz_end.hpp — "no node": the end of every skip-link walk, for the device code (hiprz_device.hpp) and for the host code that writes
// the links it follows (hiprz_scene_host.hpp), which includes no HIP header.  And the other figures both sides must agree on: the
// size of a pair record (hiprz_scene_host.hpp: PackedScene::pair_section), the size and the flags of a surface record
// (hiprz_scene_host.hpp: pack_surface_section).
#pragma once
#define RZ_END 0xFFFFFFFFu
#define RZ_PAIR_RECORD_BYTES 72u  // nine float2, 8-byte aligned: four reads of two 8-byte values and one of one
#define RZ_SURFACE_RECORD_BYTES 32u  // two float4: normal.xyz, bits(surface_material); mapped_normal.xyz, bits(flags)
#define RZ_SURFACE_NORMAL_VALID 1u   // the record's normal is what the device would compute
#define RZ_SURFACE_MAPPED_VALID 2u   // ... and so is its mapped normal, for a hit whose material has no normal map
