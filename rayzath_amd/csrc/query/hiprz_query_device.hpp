// hiprz_query_device.hpp — what the kernels of the two query libraries share (libhiprz_query.so: query/hiprz_query.hip, libhiprz_order.so:
// order/hiprz_order.hip): the invalid-ray rule and the walks with the packing of their records, once.  RZ_DEV functions only and no
// __global__: including it adds no kernel to a library.
#pragma once
#include "hiprz_device.hpp"
#include "hiprz_query.h"

namespace hiprz {

// include/hiprz_query.h "AN INVALID RAY"; on a valid ray under NORMALIZE the direction is replaced by normalized()'s
RZ_DEV bool take_ray(const float4 r0, const float4 r1, uint32_t flags, Ray& ray) {
    ray.o = xyz(r0), ray.d = xyz(r1), ray.near_ = r0.w, ray.far_ = r1.w;
    bool ok = isfinite(r0.x) && isfinite(r0.y) && isfinite(r0.z) && isfinite(r0.w) && isfinite(r1.x) && isfinite(r1.y) && isfinite(r1.z) && isfinite(r1.w);
    ok = ok && !(ray.near_ < 0.0f) && ray.far_ > ray.near_;
    const float sq = ray.d.x * ray.d.x + ray.d.y * ray.d.y + ray.d.z * ray.d.z;
    if (flags & HIPRZ_QUERY_NORMALIZE) {
        const float len = sqrtf(sq), rcp = 1.0f / len;
        ok = ok && len > 0.0f && isfinite(len) && isfinite(rcp);
        if (ok) ray.d = ray.d * rcp;  // normalized(): a * rcp_magnitude(a)
    } else {
        ok = ok && sq >= 0.99f && sq <= 1.01f;
    }
    return ok;
}

// the closest hit of the ray (r0, r1) as the three float4 of a hiprz_hit: the walk and the record of include/hiprz_query.h "THE HIT"
RZ_DEV void closest_record(const DScene& s, const float4 r0, const float4 r1, uint32_t flags, float4& h0, float4& h1, float4& h2) {
    Ray ray;
    const bool valid = take_ray(r0, r1, flags, ray);
    Hit hit;
    hit.instance = -1, hit.triangle = 0u, hit.bx = hit.by = 0.0f, hit.external = true;
    Counters cnt;
    int found = 0;
    if (valid && s.n_instances != 0u) found = closest_hit_skip<false, false, true>(s, TopCache{nullptr, nullptr, 0u}, ray, hit, cnt);
    h0 = make_float4(r1.w, 0.0f, 0.0f, __uint_as_float(valid ? 0u : HIPRZ_HIT_INVALID));
    h1 = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __uint_as_float(0u));
    h2 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
    if (found == 2) {  // hit.instance / hit.triangle are in range only here
        Surface sf;
        sf.u = sf.v = 0.0f;
        Material m;
        analyze_intersection<false, true>(s, hit, sf, m, cnt, false);
        const uint32_t inst = uint32_t(hit.instance);
        const float4 ta = s.tris[3 * hit.triangle], tb = s.tris[3 * hit.triangle + 1], tc = s.tris[3 * hit.triangle + 2];
        uint32_t slot = __float_as_uint(ta.w) & HIPRZ_TRI_MATERIAL_MASK;
        if (slot > 63u) slot = 63u;
        const int32_t material = sf.surface_material == HIPRZ_MATERIAL_DEFAULT ? -1 : int32_t(sf.surface_material);
        h0 = make_float4(ray.far_, sf.u, sf.v, __uint_as_float(HIPRZ_HIT_FOUND | (hit.external ? HIPRZ_HIT_EXTERNAL : 0u)));
        h1 = make_float4(__int_as_float(int32_t(inst)), __int_as_float(int32_t(slot)), __int_as_float(material), tb.w);  // tb.w: hiprz_tri::source_index
        h2 = make_float4(sf.mapped_normal.x, sf.mapped_normal.y, sf.mapped_normal.z, tc.w);                          // tc.w: position in the uploaded order
    }
}

// include/hiprz_query.h "OCCLUSION": 1 = some triangle lies within the ray's range; 0 for an invalid ray and in an empty world
RZ_DEV uint32_t occluded_word(const DScene& s, const float4 r0, const float4 r1, uint32_t flags) {
    Ray ray;
    const bool valid = take_ray(r0, r1, flags, ray);
    Counters cnt;
    uint32_t occluded = 0u;
    if (valid && s.n_instances != 0u) occluded = any_hit_skip<false, false>(s, TopCache{nullptr, nullptr, 0u}, ray, cnt) == 0.0f ? 1u : 0u;
    return occluded;
}

}  // namespace hiprz
