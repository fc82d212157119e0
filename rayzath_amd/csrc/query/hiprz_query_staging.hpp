// hiprz_query_staging.hpp — the growth rule of the query's pinned staging (hiprz_query.hip: grow_staging), pure host and header-only so that
// tests/test_query_abi.py can compile it with g++ under sanitizers beside a main of its own.  Not part of the C-ABI.
#pragma once
#include <cstddef>

namespace hiprz {

// the capacity (in rays) a staging of `have` rays takes on to hold `need`: `have` while it is enough, else the larger of `need` and twice
// `have`, at least 4096 and never beyond 2^31 - 1 (the most rays one call takes)
inline size_t query_staging_capacity(size_t have, size_t need) {
    const size_t most = 0x7FFFFFFFull, least = 4096u;
    if (need <= have) return have;
    size_t cap = have > most / 2u ? most : 2u * have;
    if (cap < need) cap = need;
    if (cap < least) cap = least;
    return cap > most ? most : cap;
}

}  // namespace hiprz
