// hiprz_end.hpp — "no node": the end of every skip-link walk, for the device code (hiprz_device.hpp) and for the host code that writes
// the links it follows (hiprz_scene_host.hpp), which includes no HIP header.
#pragma once
#define RZ_END 0xFFFFFFFFu
