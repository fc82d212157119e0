// hiprz_atlas_host.hpp — the pure-host half of bake atlases (include/hiprz_atlas.h): what a call is refused for before a device is asked
// anything, the size rule of an atlas and the growth rule of the handle's staging.  No HIP header: tests/test_atlas_abi.py compiles
// hiprz_atlas_host.cpp with g++ under sanitizers beside a main of its own.  Not part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hiprz {

constexpr uint32_t kAtlasMaxSize = 16384u;                                // texels per side
constexpr uint32_t kAtlasMaxRings = 64u;
constexpr uint32_t kAtlasNone = 0xFFFFFFFFu;                              // no id reaches it: triangle_base + n < 0xFFFFFFFF
constexpr size_t kAtlasMaxUnits = size_t(6) * 0xFFFFFFFFull;              // the staging counts 16-byte units: six per triangle, one per texel

// nullptr when width x height is an atlas begin takes (1 .. 16384 each), else what is wrong with it
const char* atlas_size_refusal(uint32_t width, uint32_t height);

// nullptr when an add of n triangles may go on to fetch a view, else what is wrong with it and the return code in *code.  In this order:
// a null pointer (any_null; the caller leaves it false for n == 0), no begin (HIPRZ_ERR_STATE), triangle_base + n >= 0xFFFFFFFF, a near_
// or far_ under which every point is invalid (hiprz_query.h "AN INVALID RAY": not finite, near_ < 0, far_ <= near_).
const char* atlas_add_refusal(bool any_null, bool begun, size_t n, uint32_t triangle_base, float near_, float far_, int* code);

// the one refusal that needs the view: nullptr when the view has the instance
const char* atlas_instance_refusal(uint32_t instance, uint32_t n_instances);

// nullptr when a dilation may go on: a null pointer, no add since the begin (HIPRZ_ERR_STATE), rings > 64
const char* atlas_dilate_refusal(bool any_null, bool built, uint32_t rings, int* code);

// the capacity (in 16-byte units) a staging of `have` takes on to hold `need`: the query staging's rule (doubling, at least 4096)
size_t atlas_capacity(size_t have, size_t need);

}  // namespace hiprz
