// hiprz_gather_host.hpp — the pure-host half of bounce baking (include/hiprz_gather.h): what a call is refused for before a device is asked
// anything, the checks of a direction table and of a chart map, the hash that picks a point's set and the growth rule of the handle's
// staging.  No HIP header: tests/test_gather_abi.py compiles hiprz_gather_host.cpp with g++ under sanitizers beside a main of its own.  Not
// part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

struct hiprz_gather_chart;

namespace hiprz {

constexpr size_t kGatherMaxRays = size_t(1) << 31;    // a call takes n*K < 2^31: the samples kernel indexes them on uint32_t
constexpr size_t kGatherMaxPoints = size_t(1) << 27;  // (2^31 - 1) / 16 rounded up: no accepted call has more points

// include/hiprz_gather.h "THE SET OF A POINT" (hiprz_bake.h's, restated); constexpr, so the kernels call the same text
constexpr uint32_t gather_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// 16, 32, 64, 128, 256, 512, 1024
constexpr bool gather_k_allowed(uint32_t K) { return K >= 16u && K <= 1024u && (K & (K - 1u)) == 0u; }
constexpr bool gather_s_allowed(uint32_t S) { return S >= 1u && S <= 64u; }

// nullptr when S*K float4 at xyz0 are a table set_directions takes, else what is wrong with it (K and S are looked at before the floats):
// the check of hiprz_bake_set_directions
const char* gather_table_refusal(const float* xyz0, uint32_t K, uint32_t S);

// nullptr when the arrays are a chart map set_charts takes, else what is wrong with it (the pointers and the count before the floats)
const char* gather_charts_refusal(const uint32_t* base, uint32_t n_instances, const hiprz_gather_chart* uv, uint32_t n_charts);

// nullptr when a call over n points may go on, else what is wrong with it and the return code in *code.  In this order: a null pointer
// (any_null), no table (K == 0: HIPRZ_ERR_STATE), no chart map (HIPRZ_ERR_STATE), n*K >= 2^31.
const char* gather_refusal(bool any_null, size_t n, uint32_t K, bool has_charts, int* code);

// nullptr when W x H is a source size the gather takes
const char* gather_size_refusal(uint32_t W, uint32_t H);

// nullptr when a compose over n_texels may go on (any_null: direct, albedo or out is null)
const char* gather_compose_refusal(bool any_null, size_t n_texels);

// the capacity (in points) a staging of `have` points takes on to hold `need`: the query staging's rule (doubling, at least 4096), never
// beyond 2^27
size_t gather_capacity(size_t have, size_t need);

}  // namespace hiprz
