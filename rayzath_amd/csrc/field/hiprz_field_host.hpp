// hiprz_field_host.hpp — the pure-host half of probe fields (include/hiprz_field.h): what a call is refused for before a device is asked
// anything, the checks of the direction table, the grid and the params, the hash that picks a probe's set and the growth rule of the
// handle's staging.  No HIP header: tests/test_field_abi.py compiles hiprz_field_host.cpp with g++ under sanitizers beside a main of its
// own.  Not part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

struct hiprz_field_grid;
struct hiprz_field_params;

// threads per workgroup of rz_field_lookup_kernel: 64 or 256.  On the MI355X the two timed the same within their spread (DESIGN.md §6
// "Probe fields"); 64 ships, as in the query library.  make FIELD_DEFS="-DRZ_FIELD_LOOKUP_WG=256" builds the other, which writes the
// same bytes
#ifndef RZ_FIELD_LOOKUP_WG
#define RZ_FIELD_LOOKUP_WG 64
#endif

namespace hiprz {

constexpr size_t kFieldMaxRays = size_t(1) << 31;    // a bake takes n*K < 2^31
constexpr size_t kFieldMaxPoints = size_t(1) << 31;  // a lookup takes fewer points and fewer probes: both are indexed on uint32_t

// include/hiprz_probe.h "THE SET OF A PROBE" (hiprz_bake.h's, restated); constexpr, so the kernel calls the same text
constexpr uint32_t field_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// 64, 128, ..., 1024: one ray per lane and round, and no map from fewer rays than texels
constexpr bool field_k_allowed(uint32_t K) { return K >= 64u && K <= 1024u && (K & (K - 1u)) == 0u; }
constexpr bool field_s_allowed(uint32_t S) { return S >= 1u && S <= 64u; }

// nullptr when S*K float4 at xyz0 are a table set_directions takes, else what is wrong with it (K and S are looked at before the floats)
const char* field_table_refusal(const float* xyz0, uint32_t K, uint32_t S);

// nullptr when a bake over n probes may go on, else what is wrong with it and the return code in *code.  In this order: a null pointer
// (any_null), no table (K == 0: HIPRZ_ERR_STATE), n*K >= 2^31, a reach that is not finite or not > 0.
const char* field_visibility_refusal(bool any_null, size_t n, uint32_t K, float reach, int* code);

// nullptr when the lookup takes the grid for n_probes probes / the params, else what is wrong (a null pointer included)
const char* field_grid_refusal(const hiprz_field_grid* grid, size_t n_probes);
const char* field_params_refusal(const hiprz_field_params* params);

// nullptr when a lookup of m points may go on, else what is wrong with it (always HIPRZ_ERR_INVALID).  In this order: a null pointer
// (any_null), the grid, the params, m >= 2^31.
const char* field_lookup_refusal(bool any_null, const hiprz_field_grid* grid, size_t n_probes, const hiprz_field_params* params, size_t m);

// the capacity (in records) a staging of `have` takes on to hold `need`: the query staging's rule (doubling, at least 4096)
size_t field_capacity(size_t have, size_t need);

}  // namespace hiprz
