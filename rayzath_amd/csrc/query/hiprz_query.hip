// hiprz_query.hip — ray queries (include/hiprz_query.h): closest hit and occlusion for caller-supplied rays, the selected camera's pixel
// rays, and the C-ABI around them.  A library of its own (libhiprz_query.so): libhiprz.so's kernel set is pinned (tests/test_launch_plan.py),
// and a caller that never queries runs none of this.  Only hiprz_device.hpp is shared with libhiprz.so — it defines no __global__, so no
// kernel of that library is duplicated here; the context is read through hiprz_device_view on every call.
#include <hip/hip_runtime.h>

#include <string>

#include "hiprz_query_device.hpp"  // hiprz_device.hpp, hiprz_query.h, and the ray rule and records shared with libhiprz_order.so
#include "hiprz_query_staging.hpp"
#include "hiprz_session.hpp"  // the handle, its errors, the view, the staging and its round trip

// threads per workgroup.  One wave: ray costs are heavy-tailed, and a single-wave workgroup gives its slot back as soon as ITS slowest ray
// is done instead of waiting for the slowest of four waves (DESIGN.md "Ray queries" has both measurements).
#ifndef RZ_QUERY_WG
#define RZ_QUERY_WG 64
#endif

namespace hiprz {

__global__ void __launch_bounds__(RZ_QUERY_WG) rz_query_closest_kernel(const DScene s, const float4* __restrict__ rays, size_t n, uint32_t flags,
                                                                     float4* __restrict__ hits) {
    const size_t i = size_t(blockIdx.x) * RZ_QUERY_WG + threadIdx.x;
    if (i >= n) return;
    const float4 r0 = rays[2 * i], r1 = rays[2 * i + 1];
    float4 h0, h1, h2;
    closest_record(s, r0, r1, flags, h0, h1, h2);
    float4* h = hits + 3 * i;
    h[0] = h0, h[1] = h1, h[2] = h2;
}

__global__ void __launch_bounds__(RZ_QUERY_WG) rz_query_occluded_kernel(const DScene s, const float4* __restrict__ rays, size_t n, uint32_t flags,
                                                                      uint32_t* __restrict__ out) {
    const size_t i = size_t(blockIdx.x) * RZ_QUERY_WG + threadIdx.x;
    if (i >= n) return;
    const float4 r0 = rays[2 * i], r1 = rays[2 * i + 1];
    out[i] = occluded_word(s, r0, r1, flags);
}

// thread i = pixel i of the row-major frame: 64 consecutive lanes write 2 KiB of contiguous records
__global__ void __launch_bounds__(RZ_QUERY_WG) rz_query_pixel_rays_kernel(const DCamera cam, float4* __restrict__ rays) {
    const size_t i = size_t(blockIdx.x) * RZ_QUERY_WG + threadIdx.x;
    if (i >= size_t(cam.width) * cam.height) return;
    Ray ray;
    generate_simple_ray(cam, ray, uint32_t(i % cam.width), uint32_t(i / cam.width));
    rays[2 * i] = make_float4(ray.o.x, ray.o.y, ray.o.z, ray.near_);
    rays[2 * i + 1] = make_float4(ray.d.x, ray.d.y, ray.d.z, ray.far_);
}

}  // namespace hiprz

using namespace hiprz;

static_assert(sizeof(hiprz_ray) == 32 && sizeof(hiprz_hit) == 48, "two 16-byte loads per ray, three 16-byte stores per hit");

struct hiprz_query : Session {};  // the staging holds rays and, on the out side, hits: occlusion words fit in it

namespace {
uint32_t grid_of(size_t n) { return uint32_t((n + RZ_QUERY_WG - 1u) / RZ_QUERY_WG); }

// what every call refuses before anything is launched or copied; *empty: nothing to do (n == 0 is HIPRZ_OK without a view or a launch)
int refuse(hiprz_query* q, const void* rays, size_t n, uint32_t flags, const void* out, const char* what, bool* empty) {
    *empty = false;
    if (!q) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null query");
    if (const char* why = query_refusal(!rays || !out, n, flags)) return fail(q, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    *empty = n == 0u;
    return HIPRZ_OK;
}

// one launch over device arrays on the view the call has fetched
template <typename Out>
int launch(hiprz_query* q, const DScene& s, const hiprz_ray* rays, size_t n, uint32_t flags, Out* out, hipStream_t stream, const char* what) {
    const float4* r = reinterpret_cast<const float4*>(rays);
    if constexpr (sizeof(Out) == sizeof(hiprz_hit))
        hipLaunchKernelGGL(rz_query_closest_kernel, dim3(grid_of(n)), dim3(RZ_QUERY_WG), 0, stream, s, r, n, flags, reinterpret_cast<float4*>(out));
    else
        hipLaunchKernelGGL(rz_query_occluded_kernel, dim3(grid_of(n)), dim3(RZ_QUERY_WG), 0, stream, s, r, n, flags, out);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(q, what, e);
    return HIPRZ_OK;
}

template <typename Out>
int enqueue(hiprz_query* q, const hiprz_ray* rays, size_t n, uint32_t flags, Out* out, void* stream, const char* what) {
    bool empty;
    if (const int rc = refuse(q, rays, n, flags, out, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(q, what, s); rc != HIPRZ_OK) return rc;
    return launch(q, s, rays, n, flags, out, stream_of(q, stream), what);
}

template <typename Out>
int host_call(hiprz_query* q, const hiprz_ray* rays, size_t n, uint32_t flags, Out* out, const char* what) {
    bool empty;
    if (const int rc = refuse(q, rays, n, flags, out, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(q, what, s); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the staging
    if (const int rc = grow_staging(q, what, n, sizeof(hiprz_ray), sizeof(hiprz_hit), query_staging_capacity); rc != HIPRZ_OK) return rc;
    return round_trip(q, what, rays, n, sizeof(hiprz_ray), out, sizeof(Out), [&](void* dev_rays, void* dev_out, hipStream_t st) {
        return launch(q, s, static_cast<const hiprz_ray*>(dev_rays), n, flags, static_cast<Out*>(dev_out), st, what);
    });
}
}  // namespace

extern "C" {

int hiprz_query_create(hiprz_query** out, hiprz_ctx* ctx) { return create(out, ctx, "query_create"); }

int hiprz_query_destroy(hiprz_query* q) { return destroy(q); }

const char* hiprz_query_last_error(const hiprz_query* q) { return last_error(q); }

int hiprz_query_closest(hiprz_query* q, const hiprz_ray* rays_device, size_t n, uint32_t flags, hiprz_hit* hits_out_device, void* stream) {
    return enqueue(q, rays_device, n, flags, hits_out_device, stream, "query_closest");
}

int hiprz_query_occluded(hiprz_query* q, const hiprz_ray* rays_device, size_t n, uint32_t flags, uint32_t* out_device, void* stream) {
    return enqueue(q, rays_device, n, flags, out_device, stream, "query_occluded");
}

int hiprz_query_closest_host(hiprz_query* q, const hiprz_ray* rays, size_t n, uint32_t flags, hiprz_hit* hits_out) {
    return host_call(q, rays, n, flags, hits_out, "query_closest_host");
}

int hiprz_query_occluded_host(hiprz_query* q, const hiprz_ray* rays, size_t n, uint32_t flags, uint32_t* out) {
    return host_call(q, rays, n, flags, out, "query_occluded_host");
}

int hiprz_query_pixel_rays(hiprz_query* q, hiprz_ray* rays_out_device, void* stream) {
    if (!q) return fail(nullptr, HIPRZ_ERR_INVALID, "query_pixel_rays: null query");
    if (!rays_out_device) return fail(q, HIPRZ_ERR_INVALID, "query_pixel_rays: null output");
    DScene s;
    DCamera cam;
    if (const int rc = view(q, "query_pixel_rays", s, &cam); rc != HIPRZ_OK) return rc;
    const size_t n = size_t(cam.width) * cam.height;
    if (n == 0u) return HIPRZ_OK;
    if (n > kQueryMaxRays) return fail(q, HIPRZ_ERR_INVALID, "query_pixel_rays: more than 2^31 - 1 pixels");
    hipLaunchKernelGGL(rz_query_pixel_rays_kernel, dim3(grid_of(n)), dim3(RZ_QUERY_WG), 0, stream_of(q, stream), cam, reinterpret_cast<float4*>(rays_out_device));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(q, "query_pixel_rays", e);
    return HIPRZ_OK;
}

}  // extern "C"
