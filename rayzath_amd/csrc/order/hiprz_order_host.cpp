// hiprz_order_host.cpp — the pure-host half of the ordered ray queries (hiprz_order_host.hpp).  No HIP header.
#include "hiprz_order_host.hpp"

#include "../query/hiprz_query_staging.hpp"

namespace hiprz {

const char* order_refusal(bool any_null, size_t n, uint32_t flags) { return ray_call_refusal(any_null, n, flags, kOrderMaxRays, "more than 2^30 rays"); }

// the shared rule (doubling, at least 4096) under the sort's limit
size_t order_capacity(size_t have, size_t need) { return staging_capacity(have, need, kOrderMaxRays); }

}  // namespace hiprz
