// hiprz_order_host.cpp — the pure-host half of the ordered ray queries (hiprz_order_host.hpp).  No HIP header.
#include "hiprz_order_host.hpp"

#include "../query/hiprz_query_staging.hpp"
#include "hiprz_query.h"

namespace hiprz {

const char* order_refusal(bool any_null, size_t n, uint32_t flags) {
    if (any_null) return "null pointer";
    if (flags & ~uint32_t(HIPRZ_QUERY_NORMALIZE)) return "unknown flag";
    if (n > kOrderMaxRays) return "more than 2^30 rays";
    return nullptr;
}

// the query staging's rule (doubling, at least 4096) under the sort's limit
size_t order_capacity(size_t have, size_t need) {
    if (need <= have) return have;
    const size_t cap = query_staging_capacity(have, need);
    return cap > kOrderMaxRays ? kOrderMaxRays : cap;
}

}  // namespace hiprz
