// hiprz_light.hip — light baking (include/hiprz_light.h): per surface point and light of the scene, K shadow rays are made from a table of
// disk samples, weighted, walked by the query's occlusion walk and summed across the wave in a fixed order, 16 bytes out per point.  A
// library of its own (libhiprz_light.so) beside the six whose kernels and ABI are pinned; the ray rule and the walk are the query's device
// functions (query/hiprz_query_device.hpp, no __global__), so a ray's verdict is hiprz_query_occluded's.  The context, its lights
// included, is read through hiprz_device_view on every call.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hiprz_light.h"
#include "hiprz_light_host.hpp"
#include "query/hiprz_query_device.hpp"
#include "query/hiprz_session.hpp"  // the handle, its errors, the view, the staging and its round trip

// threads per workgroup: one wave — the ballot and the butterfly span exactly the workgroup
#define RZ_LIGHT_WG 64

namespace hiprz {

// what a point gives every one of its samples: the two words of the point, whether it is valid, its set and its normalised normal
struct LightPoint {
    float4 p0, p1;  // position, near_ | normal as given, far_
    v3 n;           // normalized(normal) (read on a valid point only)
    uint32_t set;
    bool valid;
};

RZ_DEV LightPoint take_light_point(const float4* __restrict__ points, uint32_t i, uint32_t seed, uint32_t S) {
    LightPoint p;
    p.p0 = points[2 * size_t(i)], p.p1 = points[2 * size_t(i) + 1];
    Ray along;
    p.valid = take_ray(p.p0, p.p1, HIPRZ_QUERY_NORMALIZE, along);  // valid: along.d = normalized(normal)
    p.set = light_hash(i ^ seed) % S;
    p.n = along.d;
    return p;
}

// include/hiprz_light.h "THE FRAME"
RZ_DEV void light_frame(const v3 a, v3& t, v3& bt) {
    const float s = copysignf(1.0f, a.z);
    const float e = -1.0f / (s + a.z);
    const float b = (a.x * a.y) * e;
    t = V3(1.0f + ((s * a.x) * a.x) * e, s * b, (-s) * a.x);
    bt = V3(b, s + (a.y * a.y) * e, -a.y);
}

RZ_DEV bool all_finite(const v3 a, float b, float c) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b) && isfinite(c); }

// The sample (x, y) of light l of the span (spot lights first) seen from the point: its weight w, +0 for a skipped sample, the shadow ray
// as the two float4 of a hiprz_ray (direction +0 when skipped or the point invalid) and the light's colour * emission.  l comes from a loop
// counter or a kernel argument in the bake, so the record is loaded once per wave.
RZ_DEV float light_sample(const DScene& s, const LightSpan span, uint32_t l, const LightPoint& p, const float2 xy, float4& r0, float4& r1, v3& ce) {
    const bool spot = l < span.spots;
    const v3 position = xyz(p.p0);
    float w = 0.0f, far_ = p.p1.w, emission;
    uint32_t rgba;
    v3 w3;
    if (spot) {
        const uint32_t li = span.spot_first + l;
        const float4 l0 = s.spot_lights[3 * li], l1 = s.spot_lights[3 * li + 1], l2 = s.spot_lights[3 * li + 2];
        const v3 lpos = xyz(l0), ldir = xyz(l1);
        const float size = l0.w, cos_angle = l2.z;
        emission = l1.w, rgba = __float_as_uint(l2.x);
        const v3 a = normalized(lpos - position);
        v3 t, bt;
        light_frame(a, t, bt);
        const v3 q = V3(lpos.x + ((t.x * xy.x + bt.x * xy.y) * size), lpos.y + ((t.y * xy.x + bt.y * xy.y) * size), lpos.z + ((t.z * xy.x + bt.z * xy.y) * size));
        const v3 vPL = q - position;
        const float dPL = magnitude(vPL);
        w3 = normalized(vPL);
        const float c = dot(p.n, w3);
        const float A = (size * size) * RZ_PI_F;
        const float d1 = dPL + 1.0f;
        const bool inside = cos_angle < similarity(-vPL, ldir);
        if (c > 0.0f && inside) w = c * (A / (d1 * d1));
        far_ = dPL;
    } else {
        const uint32_t li = span.direct_first + (l - span.spots);
        const float4 l0 = s.direct_lights[2 * li], l1 = s.direct_lights[2 * li + 1];
        const float ca = l1.z;
        emission = l0.w, rgba = __float_as_uint(l1.x);
        const v3 a = -xyz(l0);
        v3 t, bt;
        light_frame(a, t, bt);
        const float r2 = xy.x * xy.x + xy.y * xy.y;
        const float z = 1.0f - r2 * (1.0f - ca);
        const float h = sqrtf(fmaxf(0.0f, 1.0f - z * z));
        const float g = r2 > 0.0f ? h / sqrtf(r2) : 0.0f;
        const float xg = xy.x * g, yg = xy.y * g;
        const v3 d = V3((t.x * xg + bt.x * yg) + a.x * z, (t.y * xg + bt.y * yg) + a.y * z, (t.z * xg + bt.z * yg) + a.z * z);
        w3 = normalized(d);
        const float c = dot(p.n, w3);
        if (c > 0.0f) w = c * ((2.0f * RZ_PI_F) * (1.0f - ca));
    }
    const col4 colour = from_u8(rgba);
    ce = V3(colour.r * emission, colour.g * emission, colour.b * emission);
    const bool kept = p.valid && w > 0.0f && emission > 0.0f && all_finite(w3, far_, w);
    if (!kept) w = 0.0f, w3 = V3(0.0f, 0.0f, 0.0f), far_ = p.p1.w;
    r0 = p.p0;
    r1 = make_float4(w3.x, w3.y, w3.z, far_);
    return w;
}

// One wave per workgroup.  K >= 64: the wave bakes point blockIdx.x in K / 64 rounds per light, lane j takes samples j, 64 + j, ...  K < 64:
// it bakes the 64 / K points from blockIdx.x * (64 / K) on, lane j takes sample j % K of point j / K.  A lane whose point is >= n or
// invalid, or whose sample is skipped, walks nothing and adds +0, but takes part in every ballot and shuffle: nothing returns before them.
// Five waves per SIMD: 91 VGPRs instead of 100 and still no scratch; 1 - 7 % sooner than the four-wave build (DESIGN.md §6 "Light baking").
__global__ void __launch_bounds__(RZ_LIGHT_WG, 5) rz_light_bake_kernel(const DScene s, const float4* __restrict__ points, uint32_t n,
                                                                  const float2* __restrict__ samples, uint32_t K, uint32_t S, uint32_t seed,
                                                                  const LightSpan span, float4* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const uint32_t seg = K < 64u ? K : 64u;      // lanes per point, a power of two
    const uint32_t first = lane & ~(seg - 1u);  // the first lane of this lane's point
    const uint32_t point = blockIdx.x * (64u / seg) + lane / seg;
    const bool inside = point < n;
    LightPoint p;
    p.valid = false, p.set = 0u;
    p.p0 = p.p1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p.n = V3(0.0f, 0.0f, 0.0f);
    if (inside) p = take_light_point(points, point, seed, S);
    const unsigned long long segment = (seg == 64u ? ~0ull : (1ull << seg) - 1ull) << first;
    uint32_t count = 0u;
    v3 sum = V3(0.0f, 0.0f, 0.0f);
    const uint32_t lights = span.spots + span.directs;  // of kernel arguments alone: the same trip counts on every lane
    const uint32_t rounds = K < 64u ? 1u : K / 64u;
    for (uint32_t l = 0u; l < lights; ++l) {
        for (uint32_t r = 0u; r < rounds; ++r) {
            const uint32_t k = 64u * r + (lane - first);
            const float2 xy = samples[size_t(p.set) * K + k];  // (set 0 on a lane without a point: inside the table)
            float4 r0, r1;
            v3 ce;
            const float w = light_sample(s, span, l, p, xy, r0, r1, ce);
            uint32_t occluded = 0u;
            if (w > 0.0f) occluded = occluded_word(s, r0, r1, 0u);
            count += uint32_t(__popcll(__ballot(occluded != 0u) & segment));
            const bool adds = w > 0.0f && !occluded;
            sum.x = sum.x + (adds ? ce.x * w : 0.0f);
            sum.y = sum.y + (adds ? ce.y * w : 0.0f);
            sum.z = sum.z + (adds ? ce.z * w : 0.0f);
        }
    }
    for (uint32_t off = 1u; off < seg; off <<= 1) {
        sum.x = sum.x + __shfl_xor(sum.x, int(off));
        sum.y = sum.y + __shfl_xor(sum.y, int(off));
        sum.z = sum.z + __shfl_xor(sum.z, int(off));
    }
    const float rcp = 1.0f / float(K);
    if (inside && lane == first)
        out[point] = p.valid ? make_float4(sum.x * rcp, sum.y * rcp, sum.z * rcp, __uint_as_float(count)) : make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(HIPRZ_LIGHT_INVALID));
}

// thread i: ray i = ((point, light), sample) = (i / K / L, i / K % L, i % K), the ray the bake walks for that triple, and its weight
__global__ void __launch_bounds__(RZ_LIGHT_WG) rz_light_rays_kernel(const DScene s, const float4* __restrict__ points, uint32_t n_rays,
                                                                  const float2* __restrict__ samples, uint32_t K, uint32_t S, uint32_t seed,
                                                                  const LightSpan span, float4* __restrict__ rays, float* __restrict__ weights) {
    const uint32_t i = blockIdx.x * RZ_LIGHT_WG + threadIdx.x;
    if (i >= n_rays) return;
    const uint32_t lights = span.spots + span.directs, pair = i / K;
    const LightPoint p = take_light_point(points, pair / lights, seed, S);
    float4 r0, r1;
    v3 ce;
    const float w = light_sample(s, span, pair % lights, p, samples[size_t(p.set) * K + i % K], r0, r1, ce);
    rays[2 * size_t(i)] = r0, rays[2 * size_t(i) + 1] = r1;
    weights[i] = w;
}

}  // namespace hiprz

using namespace hiprz;

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_light_texel) == 16 && sizeof(hiprz_ray) == 32, "two 16-byte loads per point, one 16-byte store per texel");
static_assert(sizeof(LightSpan) == sizeof(hiprz_light_range), "four words either way");

struct hiprz_light : Session {
    std::vector<float> table;  // the samples as set, S*K float2; K == 0: none yet
    uint32_t K = 0, S = 0;
    float2* samples = nullptr;  // the device copy, made by the first call after set_samples (`stale`)
    bool stale = false;
};

namespace {
// what every call refuses before a view is asked for; *empty: nothing to do (n == 0 is HIPRZ_OK without a view or a launch)
int refuse(hiprz_light* h, bool any_null, size_t n, const char* what, bool* empty) {
    *empty = false;
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null light");
    int code;
    if (const char* why = light_refusal(any_null, n, h->K, &code)) return fail(h, code, std::string(what) + ": " + why);
    *empty = n == 0u;
    return HIPRZ_OK;
}

// the view of the call and the lights of it that `range` selects
int view_and_span(hiprz_light* h, const hiprz_light_range* range, const char* what, DScene& s, LightSpan& span) {
    if (const int rc = view(h, what, s); rc != HIPRZ_OK) return rc;
    if (const char* why = light_range_refusal(range, s.n_spot_lights, s.n_direct_lights, &span)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    return HIPRZ_OK;
}

// the table a set_samples left on the host goes to the device, ordered on the call's stream before its kernel (the head device is current:
// a view was just taken).  A new buffer each time: hipFree waits for whatever still reads the old one.
int place_table(hiprz_light* h, hipStream_t stream, const char* what) {
    if (!h->stale) return HIPRZ_OK;
    if (h->samples) (void)hipFree(h->samples);
    h->samples = nullptr;
    const size_t bytes = h->table.size() * sizeof(float);
    if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->samples), bytes); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipMemcpyAsync(h->samples, h->table.data(), bytes, hipMemcpyHostToDevice, stream); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return fail_hip(h, what, e);  // h->table is pageable and may be replaced
    h->stale = false;
    return HIPRZ_OK;
}

// the bake of n device points on the view and the span the call has fetched
int launch_bake(hiprz_light* h, const DScene& s, const LightSpan& span, const hiprz_bake_point* points, size_t n, uint32_t seed, hiprz_light_texel* out,
                hipStream_t stream, const char* what) {
    if (const int rc = place_table(h, stream, what); rc != HIPRZ_OK) return rc;
    const uint32_t per_wave = h->K < 64u ? 64u / h->K : 1u;
    const uint32_t grid = uint32_t((n + per_wave - 1u) / per_wave);
    hipLaunchKernelGGL(rz_light_bake_kernel, dim3(grid), dim3(RZ_LIGHT_WG), 0, stream, s, reinterpret_cast<const float4*>(points), uint32_t(n), h->samples, h->K, h->S,
                       seed, span, reinterpret_cast<float4*>(out));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}
}  // namespace

extern "C" {

int hiprz_light_create(hiprz_light** out, hiprz_ctx* ctx) { return create(out, ctx, "light_create"); }

int hiprz_light_destroy(hiprz_light* h) {
    return destroy(h, h && h->samples, [h] { if (h->samples) (void)hipFree(h->samples); });
}

const char* hiprz_light_last_error(const hiprz_light* h) { return last_error(h); }

int hiprz_light_set_samples(hiprz_light* h, const float* xy_host, uint32_t K, uint32_t S) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, "light_set_samples: null light");
    if (const char* why = light_table_refusal(xy_host, K, S)) return fail(h, HIPRZ_ERR_INVALID, std::string("light_set_samples: ") + why);
    h->table.assign(xy_host, xy_host + 2 * size_t(K) * S);
    h->K = K, h->S = S, h->stale = true;
    return HIPRZ_OK;
}

int hiprz_light_count(hiprz_light* h, const hiprz_light_range* range, uint32_t* spots, uint32_t* directs) {
    const char* what = "light_count";
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null light");
    if (!spots || !directs) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": null pointer");
    DScene s;
    LightSpan span;
    if (const int rc = view_and_span(h, range, what, s, span); rc != HIPRZ_OK) return rc;
    *spots = span.spots, *directs = span.directs;
    return HIPRZ_OK;
}

int hiprz_light_bake(hiprz_light* h, const hiprz_bake_point* points_device, size_t n, uint32_t seed, const hiprz_light_range* range, hiprz_light_texel* out_device,
                     void* stream) {
    const char* what = "light_bake";
    bool empty;
    if (const int rc = refuse(h, !points_device || !out_device, n, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    LightSpan span;
    if (const int rc = view_and_span(h, range, what, s, span); rc != HIPRZ_OK) return rc;
    return launch_bake(h, s, span, points_device, n, seed, out_device, stream_of(h, stream), what);
}

int hiprz_light_rays(hiprz_light* h, const hiprz_bake_point* points_device, size_t n, uint32_t seed, const hiprz_light_range* range, hiprz_ray* rays_out_device,
                     float* weights_out_device, void* stream) {
    const char* what = "light_rays";
    bool empty;
    if (const int rc = refuse(h, !points_device || !rays_out_device || !weights_out_device, n, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    LightSpan span;
    if (const int rc = view_and_span(h, range, what, s, span); rc != HIPRZ_OK) return rc;
    const uint32_t L = span.spots + span.directs;
    if (const char* why = light_rays_refusal(n, h->K, L)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    if (L == 0u) return HIPRZ_OK;  // no ray to write
    hipStream_t st = stream_of(h, stream);
    if (const int rc = place_table(h, st, what); rc != HIPRZ_OK) return rc;
    const uint32_t n_rays = uint32_t(n * h->K * L);  // < 2^31
    hipLaunchKernelGGL(rz_light_rays_kernel, dim3((n_rays + RZ_LIGHT_WG - 1u) / RZ_LIGHT_WG), dim3(RZ_LIGHT_WG), 0, st, s, reinterpret_cast<const float4*>(points_device),
                       n_rays, h->samples, h->K, h->S, seed, span, reinterpret_cast<float4*>(rays_out_device), weights_out_device);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

int hiprz_light_bake_host(hiprz_light* h, const hiprz_bake_point* points, size_t n, uint32_t seed, const hiprz_light_range* range, hiprz_light_texel* out) {
    const char* what = "light_bake_host";
    bool empty;
    if (const int rc = refuse(h, !points || !out, n, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    LightSpan span;
    if (const int rc = view_and_span(h, range, what, s, span); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the staging
    if (const int rc = grow_staging(h, what, n, sizeof(hiprz_bake_point), sizeof(hiprz_light_texel), light_capacity); rc != HIPRZ_OK) return rc;
    return round_trip(h, what, points, n, sizeof(hiprz_bake_point), out, sizeof(hiprz_light_texel), [&](void* dev_points, void* dev_out, hipStream_t st) {
        return launch_bake(h, s, span, static_cast<const hiprz_bake_point*>(dev_points), n, seed, static_cast<hiprz_light_texel*>(dev_out), st, what);
    });
}

}  // extern "C"
