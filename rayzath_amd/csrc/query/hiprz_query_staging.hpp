// hiprz_query_staging.hpp — what the ray libraries (query, order, bake) share on the pure-host side: the growth rule of a handle's buffers
// and what a call over rays is refused for before a device is asked anything.  Header-only and no HIP header, so that tests/test_query_abi.py
// (and, through the order's and the bake's host units, tests/test_{order,bake}_abi.py) compile it with g++ under sanitizers beside a main
// of their own.  Not part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

#include "hiprz_query.h"

namespace hiprz {

constexpr size_t kQueryMaxRays = 0x7FFFFFFFull;  // 2^31 - 1, the most rays one query call takes

// the capacity (in records) buffers of `have` records take on to hold `need`: `have` while it is enough, else the larger of `need` and
// twice `have`, at least 4096 and never beyond `most` (the most records one call of the library takes)
inline size_t staging_capacity(size_t have, size_t need, size_t most) {
    const size_t least = 4096u;
    if (need <= have) return have;
    size_t cap = have > most / 2u ? most : 2u * have;
    if (cap < need) cap = need;
    if (cap < least) cap = least;
    return cap > most ? most : cap;
}

inline size_t query_staging_capacity(size_t have, size_t need) { return staging_capacity(have, need, kQueryMaxRays); }

// nullptr when a call over n rays with these flags may go on, else what is wrong with it; any_null: a required pointer is null;
// `too_many`: the text for n > most
inline const char* ray_call_refusal(bool any_null, size_t n, uint32_t flags, size_t most, const char* too_many) {
    if (any_null) return "null pointer";
    if (flags & ~uint32_t(HIPRZ_QUERY_NORMALIZE)) return "unknown flag";
    if (n > most) return too_many;
    return nullptr;
}

inline const char* query_refusal(bool any_null, size_t n, uint32_t flags) {
    return ray_call_refusal(any_null, n, flags, kQueryMaxRays, "more than 2^31 - 1 rays");
}

}  // namespace hiprz
