// hiprz_order_host.hpp — the pure-host half of the ordered ray queries (include/hiprz_order.h): what a call is refused for before a device
// is asked anything, and the growth rule of the handle's buffers.  No HIP header: tests/test_order_abi.py compiles hiprz_order_host.cpp
// with g++ under sanitizers beside a main of its own.  Not part of the C-ABI.
#pragma once
#include <cstddef>
#include <cstdint>

namespace hiprz {

constexpr size_t kOrderMaxRays = size_t(1) << 30;  // hiprz_sort_u32_device's limit

// nullptr when a call over n rays with these flags may go on, else what is wrong with it; any_null: a required pointer is null
const char* order_refusal(bool any_null, size_t n, uint32_t flags);

// the capacity (in rays) buffers of `have` rays take on to hold `need`: `have` while it is enough, else the larger of `need` and twice
// `have`, at least 4096 and never beyond 2^30
size_t order_capacity(size_t have, size_t need);

}  // namespace hiprz
