// hiprz_bake_host.hpp — the pure-host half of occlusion baking (include/hiprz_bake.h): what a call is refused for before a device is asked
// anything, the check of a direction table, the hash that picks a point's set and the growth rule of the handle's staging.  No HIP header:
// tests/test_bake_abi.py compiles hiprz_bake_host.cpp with g++ under sanitizers beside a main of its own.  Not part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hiprz {

constexpr size_t kBakeMaxRays = size_t(1) << 31;    // a call takes n*K < 2^31: the rays kernel indexes them on uint32_t
constexpr size_t kBakeMaxPoints = size_t(1) << 27;  // (2^31 - 1) / 16 rounded up: no accepted call has more points

// include/hiprz_bake.h "THE SET OF A POINT"; constexpr, so the kernels call the same text
constexpr uint32_t bake_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// 16, 32, 64, 128, 256, 512, 1024
constexpr bool bake_k_allowed(uint32_t K) { return K >= 16u && K <= 1024u && (K & (K - 1u)) == 0u; }
constexpr bool bake_s_allowed(uint32_t S) { return S >= 1u && S <= 64u; }

// nullptr when S*K float4 at xyz0 are a table set_directions takes, else what is wrong with it (K and S are looked at before the floats)
const char* bake_table_refusal(const float* xyz0, uint32_t K, uint32_t S);

// nullptr when a call over n points may go on, else what is wrong with it and the return code in *code.  In this order: a null pointer
// (any_null), no table (K == 0: HIPRZ_ERR_STATE), n*K >= 2^31.
const char* bake_refusal(bool any_null, size_t n, uint32_t K, int* code);

// the capacity (in points) a staging of `have` points takes on to hold `need`: the query staging's rule (doubling, at least 4096), never
// beyond 2^27
size_t bake_capacity(size_t have, size_t need);

}  // namespace hiprz
