// hiprz_end.hpp — "no node": the end of every skip-link walk, for the device code (hiprz_device.hpp) and for the host code that writes
// the links it follows (hiprz_scene_host.hpp), which includes no HIP header.  And the one other figure both sides must agree on: the
// size of a pair record (hiprz_scene_host.hpp: PackedScene::pair_section).
#pragma once
#define RZ_END 0xFFFFFFFFu
#define RZ_PAIR_RECORD_BYTES 72u  // nine float2, 8-byte aligned: four reads of two 8-byte values and one of one
