// hiprz_order.hip — ordered ray queries (include/hiprz_order.h): the renderer's sort key per caller ray, the renderer's radix sort through
// libhiprz.so's hiprz_sort_u32_device, and the query walks on ray perm[i].  A library of its own (libhiprz_order.so) beside
// libhiprz_query.so, whose kernels and ABI are pinned; the ray rule, the walks and the records are that library's device functions
// (query/hiprz_query_device.hpp, no __global__), so the bytes are its bytes.  The context is read through hiprz_device_view on every call.
#include <hip/hip_runtime.h>

#include <string>

#include "hiprz_order.h"
#include "hiprz_order_host.hpp"
#include "query/hiprz_query_device.hpp"
#include "query/hiprz_session.hpp"  // the handle, its errors, the view, the staging and its round trip

// threads per workgroup: one wave, as RZ_QUERY_WG measured for the same walks (DESIGN.md "Ray queries")
#ifndef RZ_ORDER_WG
#define RZ_ORDER_WG 64
#endif

namespace hiprz {

// thread i: ray i's key in caller order (0 for an invalid ray); `copy`, unless null, receives the same word — the sort destroys `keys`.
// (hiprz_api.hip has a kernel of the same name in the global namespace, the launch order of the resident kernels: another symbol in
// another library; in a kernel trace the two are told apart by the namespace.)
__global__ void __launch_bounds__(RZ_ORDER_WG) rz_order_keys_kernel(const DScene s, const float4* __restrict__ rays, uint32_t n, uint32_t flags,
                                                                  uint32_t* __restrict__ keys, uint32_t* __restrict__ copy) {
    const uint32_t i = blockIdx.x * RZ_ORDER_WG + threadIdx.x;
    if (i >= n) return;
    const float4 r0 = rays[2 * size_t(i)], r1 = rays[2 * size_t(i) + 1];
    Ray ray;
    const uint32_t key = take_ray(r0, r1, flags, ray) ? ray_sort_key(s, ray.o, ray.d, 4u) : 0u;
    keys[i] = key;
    if (copy) copy[i] = key;
}

// thread i walks ray perm[i] and writes record perm[i]; an index outside [0, n) is skipped (include/hiprz_order.h: the _by calls)
__global__ void __launch_bounds__(RZ_ORDER_WG) rz_order_closest_kernel(const DScene s, const float4* __restrict__ rays, const uint32_t* __restrict__ perm,
                                                                     uint32_t n, uint32_t flags, float4* __restrict__ hits) {
    const uint32_t i = blockIdx.x * RZ_ORDER_WG + threadIdx.x;
    if (i >= n) return;
    const size_t at = perm[i];
    if (at >= n) return;
    const float4 r0 = rays[2 * at], r1 = rays[2 * at + 1];
    float4 h0, h1, h2;
    closest_record(s, r0, r1, flags, h0, h1, h2);
    float4* h = hits + 3 * at;
    h[0] = h0, h[1] = h1, h[2] = h2;
}

__global__ void __launch_bounds__(RZ_ORDER_WG) rz_order_occluded_kernel(const DScene s, const float4* __restrict__ rays, const uint32_t* __restrict__ perm,
                                                                      uint32_t n, uint32_t flags, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * RZ_ORDER_WG + threadIdx.x;
    if (i >= n) return;
    const size_t at = perm[i];
    if (at >= n) return;
    const float4 r0 = rays[2 * at], r1 = rays[2 * at + 1];
    out[at] = occluded_word(s, r0, r1, flags);
}

}  // namespace hiprz

using namespace hiprz;

static_assert(sizeof(hiprz_ray) == 32 && sizeof(hiprz_hit) == 48, "two 16-byte loads per ray, three 16-byte stores per hit");

struct hiprz_order : Session {
    uint32_t* keys = nullptr;  // fused calls: the keys the sort consumes and the order it leaves, `work_capacity` words each
    uint32_t* perm = nullptr;
    size_t work_capacity = 0;
};

namespace {
uint32_t grid_of(size_t n) { return uint32_t((n + RZ_ORDER_WG - 1u) / RZ_ORDER_WG); }

// what every call refuses before anything is launched or copied; *empty: nothing to do (n == 0 is HIPRZ_OK without a view or a launch)
int refuse(hiprz_order* o, bool any_null, size_t n, uint32_t flags, const char* what, bool* empty) {
    *empty = false;
    if (!o) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null order");
    if (const char* why = order_refusal(any_null, n, flags)) return fail(o, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    *empty = n == 0u;
    return HIPRZ_OK;
}

void release_work(hiprz_order* o) {
    if (o->keys) (void)hipFree(o->keys);  // (hipFree waits for whatever still uses the buffer)
    if (o->perm) (void)hipFree(o->perm);
    o->keys = o->perm = nullptr, o->work_capacity = 0;
}

int grow_work(hiprz_order* o, size_t n, const char* what) {
    if (n <= o->work_capacity) return HIPRZ_OK;
    const size_t cap = order_capacity(o->work_capacity, n);
    release_work(o);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&o->keys), cap * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&o->perm), cap * sizeof(uint32_t));
    if (e != hipSuccess) {
        release_work(o);
        return fail_hip(o, what, e);
    }
    o->work_capacity = cap;
    return HIPRZ_OK;
}

// keys of the rays -> the stable order of the keys, on the view the call has fetched; `perm` is the handle's or the caller's
int order_rays(hiprz_order* o, const DScene& s, const hiprz_ray* rays, size_t n, uint32_t flags, uint32_t* keys_copy, uint32_t* perm, hipStream_t stream,
               const char* what) {
    hipLaunchKernelGGL(rz_order_keys_kernel, dim3(grid_of(n)), dim3(RZ_ORDER_WG), 0, stream, s, reinterpret_cast<const float4*>(rays), uint32_t(n), flags, o->keys,
                       keys_copy);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(o, what, e);
    if (const int rc = hiprz_sort_u32_device(o->ctx, o->keys, uint32_t(n), 24, perm, stream); rc != HIPRZ_OK) {
        const char* why = hiprz_last_error(o->ctx);
        return fail(o, rc, std::string(what) + ": " + (why && *why ? why : "the sort failed"));
    }
    return HIPRZ_OK;
}

// one ordered walk over device arrays
template <typename Out>
int walk(hiprz_order* o, const DScene& s, const hiprz_ray* rays, const uint32_t* perm, size_t n, uint32_t flags, Out* out, hipStream_t stream, const char* what) {
    const float4* r = reinterpret_cast<const float4*>(rays);
    if constexpr (sizeof(Out) == sizeof(hiprz_hit))
        hipLaunchKernelGGL(rz_order_closest_kernel, dim3(grid_of(n)), dim3(RZ_ORDER_WG), 0, stream, s, r, perm, uint32_t(n), flags, reinterpret_cast<float4*>(out));
    else
        hipLaunchKernelGGL(rz_order_occluded_kernel, dim3(grid_of(n)), dim3(RZ_ORDER_WG), 0, stream, s, r, perm, uint32_t(n), flags, out);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(o, what, e);
    return HIPRZ_OK;
}

// keys + sort + walk on one stream
template <typename Out>
int fused(hiprz_order* o, const DScene& s, const hiprz_ray* rays, size_t n, uint32_t flags, Out* out, hipStream_t stream, const char* what) {
    if (const int rc = grow_work(o, n, what); rc != HIPRZ_OK) return rc;
    if (const int rc = order_rays(o, s, rays, n, flags, nullptr, o->perm, stream, what); rc != HIPRZ_OK) return rc;
    return walk(o, s, rays, o->perm, n, flags, out, stream, what);
}

template <typename Out>
int enqueue(hiprz_order* o, const hiprz_ray* rays, const uint32_t* perm, bool by, size_t n, uint32_t flags, Out* out, void* stream, const char* what) {
    bool empty;
    if (const int rc = refuse(o, !rays || !out || (by && !perm), n, flags, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(o, what, s); rc != HIPRZ_OK) return rc;
    if (by) return walk(o, s, rays, perm, n, flags, out, stream_of(o, stream), what);
    return fused(o, s, rays, n, flags, out, stream_of(o, stream), what);
}

template <typename Out>
int host_call(hiprz_order* o, const hiprz_ray* rays, size_t n, uint32_t flags, Out* out, const char* what) {
    bool empty;
    if (const int rc = refuse(o, !rays || !out, n, flags, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(o, what, s); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the staging
    // the output side is sized for hits: occlusion words fit in it
    if (const int rc = grow_staging(o, what, n, sizeof(hiprz_ray), sizeof(hiprz_hit), order_capacity); rc != HIPRZ_OK) return rc;
    return round_trip(o, what, rays, n, sizeof(hiprz_ray), out, sizeof(Out), [&](void* dev_rays, void* dev_out, hipStream_t st) {
        return fused(o, s, static_cast<const hiprz_ray*>(dev_rays), n, flags, static_cast<Out*>(dev_out), st, what);
    });
}
}  // namespace

extern "C" {

int hiprz_order_create(hiprz_order** out, hiprz_ctx* ctx) { return create(out, ctx, "order_create"); }

int hiprz_order_destroy(hiprz_order* o) {
    return destroy(o, o && o->work_capacity, [o] { release_work(o); });
}

const char* hiprz_order_last_error(const hiprz_order* o) { return last_error(o); }

int hiprz_order_permutation(hiprz_order* o, const hiprz_ray* rays_device, size_t n, uint32_t flags, uint32_t* keys_out_device, uint32_t* perm_out_device,
                            void* stream) {
    const char* what = "order_permutation";
    bool empty;
    if (const int rc = refuse(o, !rays_device || !perm_out_device, n, flags, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(o, what, s); rc != HIPRZ_OK) return rc;
    if (const int rc = grow_work(o, n, what); rc != HIPRZ_OK) return rc;
    return order_rays(o, s, rays_device, n, flags, keys_out_device, perm_out_device, stream_of(o, stream), what);
}

int hiprz_order_closest(hiprz_order* o, const hiprz_ray* rays_device, size_t n, uint32_t flags, hiprz_hit* hits_out_device, void* stream) {
    return enqueue(o, rays_device, nullptr, false, n, flags, hits_out_device, stream, "order_closest");
}

int hiprz_order_occluded(hiprz_order* o, const hiprz_ray* rays_device, size_t n, uint32_t flags, uint32_t* out_device, void* stream) {
    return enqueue(o, rays_device, nullptr, false, n, flags, out_device, stream, "order_occluded");
}

int hiprz_order_closest_by(hiprz_order* o, const hiprz_ray* rays_device, const uint32_t* perm_device, size_t n, uint32_t flags, hiprz_hit* hits_out_device,
                           void* stream) {
    return enqueue(o, rays_device, perm_device, true, n, flags, hits_out_device, stream, "order_closest_by");
}

int hiprz_order_occluded_by(hiprz_order* o, const hiprz_ray* rays_device, const uint32_t* perm_device, size_t n, uint32_t flags, uint32_t* out_device,
                            void* stream) {
    return enqueue(o, rays_device, perm_device, true, n, flags, out_device, stream, "order_occluded_by");
}

int hiprz_order_closest_host(hiprz_order* o, const hiprz_ray* rays, size_t n, uint32_t flags, hiprz_hit* hits_out) {
    return host_call(o, rays, n, flags, hits_out, "order_closest_host");
}

int hiprz_order_occluded_host(hiprz_order* o, const hiprz_ray* rays, size_t n, uint32_t flags, uint32_t* out) {
    return host_call(o, rays, n, flags, out, "order_occluded_host");
}

}  // extern "C"
