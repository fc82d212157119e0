// hiprz_query_host.cpp — the pure-host half of the ray queries (include/hiprz_query.h): the record layouts as compiled (the staging's
// growth rule is the header hiprz_query_staging.hpp).
// No HIP header, so that tests/test_query_abi.py can compile it with g++ under sanitizers beside a main of its own.
#include <cstddef>

#include "hiprz_query.h"

extern "C" {

void hiprz_query_layout(uint32_t out[7]) {
    out[0] = uint32_t(sizeof(hiprz_ray));
    out[1] = uint32_t(sizeof(hiprz_hit));
    out[2] = uint32_t(offsetof(hiprz_ray, direction));
    out[3] = uint32_t(offsetof(hiprz_hit, flags));
    out[4] = uint32_t(offsetof(hiprz_hit, instance));
    out[5] = uint32_t(offsetof(hiprz_hit, normal));
    out[6] = uint32_t(offsetof(hiprz_hit, scene_triangle));
}

}  // extern "C"
