// hiprz_probe_host.hpp — the pure-host half of probe baking (include/hiprz_probe.h): what a call is refused for before a device is asked
// anything, the checks of the two tables and of a chart map, the rule of a light range, the hash that picks a probe's set and the growth
// rule of the handle's staging.  No HIP header: tests/test_probe_abi.py compiles hiprz_probe_host.cpp with g++ under sanitizers beside a
// main of its own.  Not part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

struct hiprz_gather_chart;
struct hiprz_light_range;

namespace hiprz {

constexpr size_t kProbeMaxRays = size_t(1) << 31;    // a call takes n*K < 2^31: the samples kernel indexes them on uint32_t
constexpr size_t kProbeMaxProbes = size_t(1) << 31;  // K = 1 of the light term: no accepted call has more probes

// include/hiprz_probe.h "THE SET OF A PROBE" (hiprz_bake.h's, restated); constexpr, so the kernels call the same text
constexpr uint32_t probe_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// 16, 32, ..., 1024 for the directions; 1, 2, ..., 1024 for the light's samples
constexpr bool probe_k_allowed(uint32_t K) { return K >= 16u && K <= 1024u && (K & (K - 1u)) == 0u; }
constexpr bool probe_samples_k_allowed(uint32_t K) { return K >= 1u && K <= 1024u && (K & (K - 1u)) == 0u; }
constexpr bool probe_s_allowed(uint32_t S) { return S >= 1u && S <= 64u; }

// nullptr when S*K float4 at xyz0 are a table set_directions takes, else what is wrong with it (K and S are looked at before the floats)
const char* probe_table_refusal(const float* xyz0, uint32_t K, uint32_t S);

// nullptr when S*K float2 at xy are a table set_samples takes, else what is wrong with it
const char* probe_samples_refusal(const float* xy, uint32_t K, uint32_t S);

// nullptr when the arrays are a chart map set_charts takes, else what is wrong with it (the pointers and the count before the floats)
const char* probe_charts_refusal(const uint32_t* base, uint32_t n_instances, const hiprz_gather_chart* uv, uint32_t n_charts);

// nullptr when a gather or samples call over n probes may go on, else what is wrong with it and the return code in *code.  In this order:
// a null pointer (any_null), no table (K == 0: HIPRZ_ERR_STATE), no chart map (HIPRZ_ERR_STATE), n*K >= 2^31.
const char* probe_gather_refusal(bool any_null, size_t n, uint32_t K, bool has_charts, int* code);

// the same for the light term: a null pointer, no sample table (K == 0: HIPRZ_ERR_STATE), n*K >= 2^31
const char* probe_light_refusal(bool any_null, size_t n, uint32_t K, int* code);

// nullptr when W x H is a source size the gather takes
const char* probe_size_refusal(uint32_t W, uint32_t H);

// the lights a call works on: `spots` spot lights from spot_first on, then `directs` direct lights from direct_first on
struct ProbeSpan {
    uint32_t spot_first, spots, direct_first, directs;
};

// nullptr and the span in *out when `range` (nullptr: every light) lies within n_spot spot and n_direct direct lights, else what is wrong
const char* probe_range_refusal(const hiprz_light_range* range, uint32_t n_spot, uint32_t n_direct, ProbeSpan* out);

// the capacity (in probes) a staging of `have` probes takes on to hold `need`: the query staging's rule (doubling, at least 4096)
size_t probe_capacity(size_t have, size_t need);

}  // namespace hiprz
