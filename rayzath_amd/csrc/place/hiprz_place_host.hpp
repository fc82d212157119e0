// hiprz_place_host.hpp — the pure-host half of probe placement (include/hiprz_place.h): what a call is refused for before a device is
// asked anything, the checks of the direction table and the params, the hash that picks a probe's set and the growth rule of the handle's
// staging.  No HIP header: tests/test_place_abi.py compiles hiprz_place_host.cpp with g++ under sanitizers beside a main of its own.  Not
// part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

struct hiprz_place_params;

namespace hiprz {

constexpr size_t kPlaceMaxRays = size_t(1) << 31;    // a placement takes n*K < 2^31
constexpr size_t kPlaceMaxProbes = size_t(1) << 31;  // the staging's cap (n < 2^31 / 64 anyway)

// include/hiprz_probe.h "THE SET OF A PROBE" (hiprz_bake.h's, restated); constexpr, so the kernel calls the same text
constexpr uint32_t place_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// 64, 128, ..., 1024: one ray per lane and round
constexpr bool place_k_allowed(uint32_t K) { return K >= 64u && K <= 1024u && (K & (K - 1u)) == 0u; }
constexpr bool place_s_allowed(uint32_t S) { return S >= 1u && S <= 64u; }

// nullptr when S*K float4 at xyz0 are a table set_directions takes, else what is wrong with it (K and S are looked at before the floats)
const char* place_table_refusal(const float* xyz0, uint32_t K, uint32_t S);

// nullptr when a placement takes the params, else what is wrong with them (a null pointer included)
const char* place_params_refusal(const hiprz_place_params* params);

// nullptr when a placement of n probes may go on, else what is wrong with it and the return code in *code.  In this order: a null pointer
// (any_null), no table (K == 0: HIPRZ_ERR_STATE), n*K >= 2^31, the params.
const char* place_probes_refusal(bool any_null, size_t n, uint32_t K, const hiprz_place_params* params, int* code);

// the capacity (in records) a staging of `have` takes on to hold `need`: the query staging's rule (doubling, at least 4096)
size_t place_capacity(size_t have, size_t need);

}  // namespace hiprz
