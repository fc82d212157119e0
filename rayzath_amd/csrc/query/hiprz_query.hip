// hiprz_query.hip — ray queries (include/hiprz_query.h): closest hit and occlusion for caller-supplied rays, the selected camera's pixel
// rays, and the C-ABI around them.  A library of its own (libhiprz_query.so): libhiprz.so's kernel set is pinned (tests/test_launch_plan.py),
// and a caller that never queries runs none of this.  Only hiprz_device.hpp is shared with libhiprz.so — it defines no __global__, so no
// kernel of that library is duplicated here; the context is read through hiprz_device_view on every call.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "hiprz_query_device.hpp"  // hiprz_device.hpp, hiprz_query.h, and the ray rule and records shared with libhiprz_order.so
#include "hiprz_query_staging.hpp"

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

struct hiprz_query {
    hiprz_ctx* ctx = nullptr;
    int device = -1;            // the context's head device, known from the first view on (hiprz_device_view makes it current)
    void* pinned_rays = nullptr;  // host-pointer calls: pinned staging and its device twin, `capacity` rays each
    void* pinned_out = nullptr;
    void* dev_rays = nullptr;
    void* dev_out = nullptr;
    size_t capacity = 0;
    std::string error;
};

namespace {
thread_local std::string g_error;  // of calls without a query

constexpr size_t kMaxRays = 0x7FFFFFFFull;

int fail(hiprz_query* q, int code, const std::string& message) {
    (q ? q->error : g_error) = message;
    return code;
}
int fail_hip(hiprz_query* q, const char* what, hipError_t e) { return fail(q, HIPRZ_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

// the context's device views, fetched on every call; the sizes are the guard against a libhiprz.so built from other headers
int view(hiprz_query* q, const char* what, DScene& s, DCamera* cam) {
    const int rc = hiprz_device_view(q->ctx, &s, sizeof s, cam, cam ? sizeof *cam : 0u);
    if (rc != HIPRZ_OK) {
        const char* why = hiprz_last_error(q->ctx);
        return fail(q, rc, std::string(what) + ": " + (why && *why ? why : "the context gave no device view"));
    }
    if (const hipError_t e = hipGetDevice(&q->device); e != hipSuccess) return fail_hip(q, what, e);
    return HIPRZ_OK;
}

hipStream_t stream_of(hiprz_query* q, void* stream) { return static_cast<hipStream_t>(stream ? stream : hiprz_stream(q->ctx)); }

uint32_t grid_of(size_t n) { return uint32_t((n + RZ_QUERY_WG - 1u) / RZ_QUERY_WG); }

// what every call refuses before anything is launched or copied; *empty: nothing to do (n == 0 is HIPRZ_OK without a view or a launch)
int refuse(hiprz_query* q, const void* rays, size_t n, uint32_t flags, const void* out, const char* what, bool* empty) {
    *empty = false;
    if (!q) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null query");
    if (!rays || !out) return fail(q, HIPRZ_ERR_INVALID, std::string(what) + ": null pointer");
    if (flags & ~HIPRZ_QUERY_NORMALIZE) return fail(q, HIPRZ_ERR_INVALID, std::string(what) + ": unknown flag");
    if (n > kMaxRays) return fail(q, HIPRZ_ERR_INVALID, std::string(what) + ": more than 2^31 - 1 rays");
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
    if (const int rc = view(q, what, s, nullptr); rc != HIPRZ_OK) return rc;
    return launch(q, s, rays, n, flags, out, stream_of(q, stream), what);
}

void release_staging(hiprz_query* q) {
    if (q->dev_rays) (void)hipFree(q->dev_rays);  // (hipFree waits for whatever still uses the buffer)
    if (q->dev_out) (void)hipFree(q->dev_out);
    if (q->pinned_rays) (void)hipHostFree(q->pinned_rays);
    if (q->pinned_out) (void)hipHostFree(q->pinned_out);
    q->dev_rays = q->dev_out = q->pinned_rays = q->pinned_out = nullptr, q->capacity = 0;
}

// the output side is sized for hits: occlusion words fit in it
int grow_staging(hiprz_query* q, size_t n, const char* what) {
    if (n <= q->capacity) return HIPRZ_OK;
    const size_t cap = query_staging_capacity(q->capacity, n);
    release_staging(q);
    hipError_t e = hipMalloc(&q->dev_rays, cap * sizeof(hiprz_ray));
    if (e == hipSuccess) e = hipMalloc(&q->dev_out, cap * sizeof(hiprz_hit));
    if (e == hipSuccess) e = hipHostMalloc(&q->pinned_rays, cap * sizeof(hiprz_ray), hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostMalloc(&q->pinned_out, cap * sizeof(hiprz_hit), hipHostMallocDefault);
    if (e != hipSuccess) {
        release_staging(q);
        return fail_hip(q, what, e);
    }
    q->capacity = cap;
    return HIPRZ_OK;
}

template <typename Out>
int host_call(hiprz_query* q, const hiprz_ray* rays, size_t n, uint32_t flags, Out* out, const char* what) {
    bool empty;
    if (const int rc = refuse(q, rays, n, flags, out, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(q, what, s, nullptr); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the staging
    if (const int rc = grow_staging(q, n, what); rc != HIPRZ_OK) return rc;
    hipStream_t st = stream_of(q, nullptr);
    std::memcpy(q->pinned_rays, rays, n * sizeof(hiprz_ray));
    if (const hipError_t e = hipMemcpyAsync(q->dev_rays, q->pinned_rays, n * sizeof(hiprz_ray), hipMemcpyHostToDevice, st); e != hipSuccess)
        return fail_hip(q, what, e);
    if (const int rc = launch(q, s, static_cast<const hiprz_ray*>(q->dev_rays), n, flags, static_cast<Out*>(q->dev_out), st, what); rc != HIPRZ_OK) return rc;
    if (const hipError_t e = hipMemcpyAsync(q->pinned_out, q->dev_out, n * sizeof(Out), hipMemcpyDeviceToHost, st); e != hipSuccess) return fail_hip(q, what, e);
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(q, what, e);
    std::memcpy(out, q->pinned_out, n * sizeof(Out));
    return HIPRZ_OK;
}
}  // namespace

extern "C" {

int hiprz_query_create(hiprz_query** out, hiprz_ctx* ctx) {
    if (!out) return fail(nullptr, HIPRZ_ERR_INVALID, "query_create: null output");
    *out = nullptr;
    int n = 0;
    if (const hipError_t e = hipGetDeviceCount(&n); e != hipSuccess || n <= 0)
        return fail(nullptr, HIPRZ_ERR_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    if (!ctx) return fail(nullptr, HIPRZ_ERR_INVALID, "query_create: null context");
    hiprz_query* q = new hiprz_query;
    q->ctx = ctx;
    *out = q;
    return HIPRZ_OK;
}

int hiprz_query_destroy(hiprz_query* q) {
    if (!q) return HIPRZ_ERR_INVALID;
    if (q->capacity) {
        (void)hipSetDevice(q->device);
        release_staging(q);
    }
    delete q;
    return HIPRZ_OK;
}

const char* hiprz_query_last_error(const hiprz_query* q) { return q ? q->error.c_str() : g_error.c_str(); }

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
    if (n > kMaxRays) return fail(q, HIPRZ_ERR_INVALID, "query_pixel_rays: more than 2^31 - 1 pixels");
    hipLaunchKernelGGL(rz_query_pixel_rays_kernel, dim3(grid_of(n)), dim3(RZ_QUERY_WG), 0, stream_of(q, stream), cam, reinterpret_cast<float4*>(rays_out_device));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(q, "query_pixel_rays", e);
    return HIPRZ_OK;
}

}  // extern "C"
