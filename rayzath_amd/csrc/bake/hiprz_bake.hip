// hiprz_bake.hip — occlusion baking (include/hiprz_bake.h): the K rays of a surface point are made from a table of local directions, walked
// by the query's occlusion walk and counted across the wave, 16 bytes out per point.  A library of its own (libhiprz_bake.so) beside
// libhiprz_query.so and libhiprz_order.so, whose kernels and ABI are pinned; the ray rule and the walk are that library's device functions
// (query/hiprz_query_device.hpp, no __global__), so a ray's verdict is hiprz_query_occluded's.  The context is read through
// hiprz_device_view on every call.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hiprz_bake.h"
#include "hiprz_bake_host.hpp"
#include "query/hiprz_query_device.hpp"
#include "query/hiprz_session.hpp"  // the handle, its errors, the view, the staging and its round trip

// threads per workgroup: one wave — the ballot and the butterfly span exactly the workgroup
#define RZ_BAKE_WG 64

namespace hiprz {

// what a point gives every one of its rays: the two words of the point, whether it is valid, its set and its frame
struct BakePoint {
    float4 p0, p1;  // position, near_ | normal as given, far_
    v3 n, t, bt;    // include/hiprz_bake.h "THE FRAME" of the normalised normal (read on a valid point only)
    uint32_t set;
    bool valid;
};

RZ_DEV BakePoint take_point(const float4* __restrict__ points, uint32_t i, uint32_t seed, uint32_t S) {
    BakePoint p;
    p.p0 = points[2 * size_t(i)], p.p1 = points[2 * size_t(i) + 1];
    Ray along;
    p.valid = take_ray(p.p0, p.p1, HIPRZ_QUERY_NORMALIZE, along);  // valid: along.d = normalized(normal)
    p.set = bake_hash(i ^ seed) % S;
    const v3 n = along.d;
    const float s = copysignf(1.0f, n.z);
    const float a = -1.0f / (s + n.z);
    const float b = (n.x * n.y) * a;
    p.n = n;
    p.t = V3(1.0f + ((s * n.x) * n.x) * a, s * b, (-s) * n.x);
    p.bt = V3(b, s + (n.y * n.y) * a, -n.y);
    return p;
}

// the ray of (point, direction k) as the two float4 of a hiprz_ray; `d` is its direction once more.  An invalid point: direction +0.
RZ_DEV void bake_ray(const BakePoint& p, const float4* __restrict__ dirs, uint32_t K, uint32_t k, float4& r0, float4& r1, v3& d) {
    d = V3(0.0f, 0.0f, 0.0f);
    if (p.valid) {
        const float4 l = dirs[size_t(p.set) * K + k];
        d.x = (p.t.x * l.x + p.bt.x * l.y) + p.n.x * l.z;
        d.y = (p.t.y * l.x + p.bt.y * l.y) + p.n.y * l.z;
        d.z = (p.t.z * l.x + p.bt.z * l.y) + p.n.z * l.z;
    }
    r0 = p.p0;
    r1 = make_float4(d.x, d.y, d.z, p.p1.w);
}

// One wave per workgroup.  K >= 64: the wave bakes point blockIdx.x in K / 64 rounds, lane l walks rays l, 64 + l, ...  K < 64: it bakes
// the 64 / K points from blockIdx.x * (64 / K) on, lane l walks ray l % K of point l / K.  A lane whose point is >= n or invalid walks
// nothing and contributes "not occluded, direction +0", but takes part in every ballot and shuffle: nothing returns before them.
__global__ void __launch_bounds__(RZ_BAKE_WG) rz_bake_occlusion_kernel(const DScene s, const float4* __restrict__ points, uint32_t n,
                                                                     const float4* __restrict__ dirs, uint32_t K, uint32_t S, uint32_t seed,
                                                                     float4* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const uint32_t seg = K < 64u ? K : 64u;  // lanes per point, a power of two
    const uint32_t first = lane & ~(seg - 1u);  // the first lane of this lane's point
    const uint32_t point = blockIdx.x * (64u / seg) + lane / seg;
    const bool inside = point < n;
    BakePoint p;
    p.valid = false;
    if (inside) p = take_point(points, point, seed, S);
    const bool walks = inside && p.valid;
    const unsigned long long segment = (seg == 64u ? ~0ull : (1ull << seg) - 1ull) << first;
    uint32_t count = 0u;
    v3 sum = V3(0.0f, 0.0f, 0.0f);
    const uint32_t rounds = K < 64u ? 1u : K / 64u;  // of a kernel argument alone: the same trip count on every lane
    for (uint32_t r = 0u; r < rounds; ++r) {
        const uint32_t k = 64u * r + (lane - first);
        uint32_t occluded = 0u;
        v3 d = V3(0.0f, 0.0f, 0.0f);
        if (walks) {
            float4 r0, r1;
            bake_ray(p, dirs, K, k, r0, r1, d);
            occluded = occluded_word(s, r0, r1, 0u);
        }
        count += uint32_t(__popcll(__ballot(occluded != 0u) & segment));
        sum.x = sum.x + (occluded ? 0.0f : d.x);
        sum.y = sum.y + (occluded ? 0.0f : d.y);
        sum.z = sum.z + (occluded ? 0.0f : d.z);
    }
    for (uint32_t off = 1u; off < seg; off <<= 1) {
        sum.x = sum.x + __shfl_xor(sum.x, int(off));
        sum.y = sum.y + __shfl_xor(sum.y, int(off));
        sum.z = sum.z + __shfl_xor(sum.z, int(off));
    }
    if (inside && lane == first)
        out[point] = p.valid ? make_float4(sum.x, sum.y, sum.z, __uint_as_float(count)) : make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(HIPRZ_BAKE_INVALID));
}

// thread i: ray i = (point i / K, direction i % K), the ray the bake walks for that pair
__global__ void __launch_bounds__(RZ_BAKE_WG) rz_bake_rays_kernel(const float4* __restrict__ points, uint32_t n_rays, const float4* __restrict__ dirs, uint32_t K,
                                                                uint32_t S, uint32_t seed, float4* __restrict__ rays) {
    const uint32_t i = blockIdx.x * RZ_BAKE_WG + threadIdx.x;
    if (i >= n_rays) return;
    const BakePoint p = take_point(points, i / K, seed, S);
    float4 r0, r1;
    v3 d;
    bake_ray(p, dirs, K, i % K, r0, r1, d);
    rays[2 * size_t(i)] = r0, rays[2 * size_t(i) + 1] = r1;
}

}  // namespace hiprz

using namespace hiprz;

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_bake_texel) == 16 && sizeof(hiprz_ray) == 32, "two 16-byte loads per point, one 16-byte store per texel");

struct hiprz_bake : Session {
    std::vector<float> table;  // the directions as set, S*K float4 with w = 0; K == 0: none yet
    uint32_t K = 0, S = 0;
    float4* dirs = nullptr;    // the device copy, made by the first call after set_directions (`stale`)
    bool stale = false;
};

namespace {
// what every call refuses before anything is launched or copied; *empty: nothing to do (n == 0 is HIPRZ_OK without a view or a launch)
int refuse(hiprz_bake* b, bool any_null, size_t n, const char* what, bool* empty) {
    *empty = false;
    if (!b) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null bake");
    int code;
    if (const char* why = bake_refusal(any_null, n, b->K, &code)) return fail(b, code, std::string(what) + ": " + why);
    *empty = n == 0u;
    return HIPRZ_OK;
}

// the table a set_directions left on the host goes to the device, ordered on the call's stream before its kernel (the head device is current:
// a view was just taken).  A new buffer each time: hipFree waits for whatever still reads the old one.
int place_table(hiprz_bake* b, hipStream_t stream, const char* what) {
    if (!b->stale) return HIPRZ_OK;
    if (b->dirs) (void)hipFree(b->dirs);
    b->dirs = nullptr;
    const size_t bytes = b->table.size() * sizeof(float);
    if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(&b->dirs), bytes); e != hipSuccess) return fail_hip(b, what, e);
    if (const hipError_t e = hipMemcpyAsync(b->dirs, b->table.data(), bytes, hipMemcpyHostToDevice, stream); e != hipSuccess) return fail_hip(b, what, e);
    if (const hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return fail_hip(b, what, e);  // b->table is pageable and may be replaced
    b->stale = false;
    return HIPRZ_OK;
}

// the bake of n device points on the view the call has fetched
int launch_occlusion(hiprz_bake* b, const DScene& s, const hiprz_bake_point* points, size_t n, uint32_t seed, hiprz_bake_texel* out, hipStream_t stream,
                     const char* what) {
    if (const int rc = place_table(b, stream, what); rc != HIPRZ_OK) return rc;
    const uint32_t per_wave = b->K < 64u ? 64u / b->K : 1u;
    const uint32_t grid = uint32_t((n + per_wave - 1u) / per_wave);
    hipLaunchKernelGGL(rz_bake_occlusion_kernel, dim3(grid), dim3(RZ_BAKE_WG), 0, stream, s, reinterpret_cast<const float4*>(points), uint32_t(n), b->dirs, b->K, b->S,
                       seed, reinterpret_cast<float4*>(out));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(b, what, e);
    return HIPRZ_OK;
}
}  // namespace

extern "C" {

int hiprz_bake_create(hiprz_bake** out, hiprz_ctx* ctx) { return create(out, ctx, "bake_create"); }

int hiprz_bake_destroy(hiprz_bake* b) {
    return destroy(b, b && b->dirs, [b] { if (b->dirs) (void)hipFree(b->dirs); });
}

const char* hiprz_bake_last_error(const hiprz_bake* b) { return last_error(b); }

int hiprz_bake_set_directions(hiprz_bake* b, const float* xyz0_host, uint32_t K, uint32_t S) {
    if (!b) return fail(nullptr, HIPRZ_ERR_INVALID, "bake_set_directions: null bake");
    if (const char* why = bake_table_refusal(xyz0_host, K, S)) return fail(b, HIPRZ_ERR_INVALID, std::string("bake_set_directions: ") + why);
    b->table.assign(xyz0_host, xyz0_host + 4 * size_t(K) * S);
    for (size_t i = 3; i < b->table.size(); i += 4) b->table[i] = 0.0f;
    b->K = K, b->S = S, b->stale = true;
    return HIPRZ_OK;
}

int hiprz_bake_occlusion(hiprz_bake* b, const hiprz_bake_point* points_device, size_t n, uint32_t seed, hiprz_bake_texel* out_device, void* stream) {
    const char* what = "bake_occlusion";
    bool empty;
    if (const int rc = refuse(b, !points_device || !out_device, n, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(b, what, s); rc != HIPRZ_OK) return rc;
    return launch_occlusion(b, s, points_device, n, seed, out_device, stream_of(b, stream), what);
}

int hiprz_bake_rays(hiprz_bake* b, const hiprz_bake_point* points_device, size_t n, uint32_t seed, hiprz_ray* rays_out_device, void* stream) {
    const char* what = "bake_rays";
    bool empty;
    if (const int rc = refuse(b, !points_device || !rays_out_device, n, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(b, what, s); rc != HIPRZ_OK) return rc;  // the rays read no scene; the view refuses what the bake refuses and makes the device current
    hipStream_t st = stream_of(b, stream);
    if (const int rc = place_table(b, st, what); rc != HIPRZ_OK) return rc;
    const uint32_t n_rays = uint32_t(n * b->K);  // < 2^31
    hipLaunchKernelGGL(rz_bake_rays_kernel, dim3((n_rays + RZ_BAKE_WG - 1u) / RZ_BAKE_WG), dim3(RZ_BAKE_WG), 0, st, reinterpret_cast<const float4*>(points_device), n_rays,
                       b->dirs, b->K, b->S, seed, reinterpret_cast<float4*>(rays_out_device));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(b, what, e);
    return HIPRZ_OK;
}

int hiprz_bake_occlusion_host(hiprz_bake* b, const hiprz_bake_point* points, size_t n, uint32_t seed, hiprz_bake_texel* out) {
    const char* what = "bake_occlusion_host";
    bool empty;
    if (const int rc = refuse(b, !points || !out, n, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(b, what, s); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the staging
    if (const int rc = grow_staging(b, what, n, sizeof(hiprz_bake_point), sizeof(hiprz_bake_texel), bake_capacity); rc != HIPRZ_OK) return rc;
    return round_trip(b, what, points, n, sizeof(hiprz_bake_point), out, sizeof(hiprz_bake_texel), [&](void* dev_points, void* dev_out, hipStream_t st) {
        return launch_occlusion(b, s, static_cast<const hiprz_bake_point*>(dev_points), n, seed, static_cast<hiprz_bake_texel*>(dev_out), st, what);
    });
}

}  // extern "C"
