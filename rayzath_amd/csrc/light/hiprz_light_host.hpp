// hiprz_light_host.hpp — the pure-host half of light baking (include/hiprz_light.h): what a call is refused for before a device is asked
// anything, the check of a sample table, the rule of a light range, the hash that picks a point's set and the growth rule of the handle's
// staging.  No HIP header: tests/test_light_abi.py compiles hiprz_light_host.cpp with g++ under sanitizers beside a main of its own.  Not
// part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

struct hiprz_light_range;

namespace hiprz {

constexpr size_t kLightMaxRays = size_t(1) << 31;    // a call takes n*K < 2^31 (the rays: n*L*K): the kernels index them on uint32_t
constexpr size_t kLightMaxPoints = size_t(1) << 31;  // K = 1: no accepted call has more points

// include/hiprz_light.h "THE SET OF A POINT"; constexpr, so the kernels call the same text
constexpr uint32_t light_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// 1, 2, 4, ..., 1024
constexpr bool light_k_allowed(uint32_t K) { return K >= 1u && K <= 1024u && (K & (K - 1u)) == 0u; }
constexpr bool light_s_allowed(uint32_t S) { return S >= 1u && S <= 64u; }

// nullptr when S*K float2 at xy are a table set_samples takes, else what is wrong with it (K and S are looked at before the floats)
const char* light_table_refusal(const float* xy, uint32_t K, uint32_t S);

// nullptr when a call over n points may go on, else what is wrong with it and the return code in *code.  In this order: a null pointer
// (any_null), no table (K == 0: HIPRZ_ERR_STATE), n*K >= 2^31.
const char* light_refusal(bool any_null, size_t n, uint32_t K, int* code);

// the lights a call works on: `spots` spot lights from spot_first on, then `directs` direct lights from direct_first on
struct LightSpan {
    uint32_t spot_first, spots, direct_first, directs;
};

// nullptr and the span in *out when `range` (nullptr: every light) lies within n_spot spot and n_direct direct lights, else what is wrong
const char* light_range_refusal(const hiprz_light_range* range, uint32_t n_spot, uint32_t n_direct, LightSpan* out);

// nullptr when the n*L*K rays of a rays call can be indexed on uint32_t (K != 0, n*K < 2^31 already)
const char* light_rays_refusal(size_t n, uint32_t K, uint32_t L);

// the capacity (in points) a staging of `have` points takes on to hold `need`: the query staging's rule (doubling, at least 4096), never
// beyond 2^31
size_t light_capacity(size_t have, size_t need);

}  // namespace hiprz
