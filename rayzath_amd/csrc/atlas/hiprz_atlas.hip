// hiprz_atlas.hip — bake atlases (include/hiprz_atlas.h): the caller's UV charts rasterised into one hiprz_bake_point per texel, and the
// dilation of what was baked per texel.  A library of its own (libhiprz_atlas.so) beside libhiprz_query.so, libhiprz_order.so and
// libhiprz_bake.so, whose kernels and ABI are pinned.  The context is read through hiprz_device_view on every add: only the instance
// records of the view are used, with the renderer's own vector functions (hiprz_device.hpp).
#include <hip/hip_runtime.h>

#include <string>

#include "hiprz_atlas.h"
#include "hiprz_atlas_host.hpp"
#include "query/hiprz_session.hpp"  // the handle, its errors, the view and the staging

// threads per workgroup: one wave.  In the cover kernel a wave is a block of RZ_ATLAS_BLOCK_W x (64 / RZ_ATLAS_BLOCK_W) texels and
// RZ_ATLAS_HELPERS waves share the blocks of one triangle's bounding box (DESIGN.md §6 "Bake atlases" has what was timed).
#define RZ_ATLAS_WG 64
#ifndef RZ_ATLAS_BLOCK_W
#define RZ_ATLAS_BLOCK_W 8
#endif
#ifndef RZ_ATLAS_HELPERS
#define RZ_ATLAS_HELPERS 8
#endif
#define RZ_ATLAS_BLOCK_H (RZ_ATLAS_WG / RZ_ATLAS_BLOCK_W)
static_assert(RZ_ATLAS_BLOCK_W * RZ_ATLAS_BLOCK_H == RZ_ATLAS_WG && RZ_ATLAS_HELPERS >= 1, "a wave is one block of texels");

namespace hiprz {

struct uv2 {
    float x, y;
};

// include/hiprz_atlas.h "THE EDGE VALUE": the edge walked from P to Q, valued at (px, py)
RZ_DEV float edge_value(uv2 P, uv2 Q, float px, float py) {
    const bool swap = Q.x < P.x || (Q.x == P.x && Q.y < P.y);
    const uv2 A = swap ? Q : P, B = swap ? P : Q;
    const float e = (B.x - A.x) * (py - A.y) - (B.y - A.y) * (px - A.x);
    return swap ? -e : e;
}

// a triangle in texel space: "TEXEL SPACE" and "ORIENTATION"
struct AtlasTri {
    uv2 a1, a2, a3;
    float area, s;
    bool degenerate;
};

RZ_DEV bool finite4(float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w); }

RZ_DEV AtlasTri take_tri(const float4* __restrict__ r, float fw, float fh, float4 row[6]) {
    for (int k = 0; k < 6; ++k) row[k] = r[k];
    AtlasTri t;
    t.a1 = uv2{row[0].w * fw - 0.5f, row[3].w * fh - 0.5f};
    t.a2 = uv2{row[1].w * fw - 0.5f, row[4].w * fh - 0.5f};
    t.a3 = uv2{row[2].w * fw - 0.5f, row[5].w * fh - 0.5f};
    t.area = edge_value(t.a1, t.a2, t.a3.x, t.a3.y);
    const bool finite = finite4(row[0]) && finite4(row[1]) && finite4(row[2]) && finite4(row[3]) && finite4(row[4]) && finite4(row[5]);
    t.degenerate = !finite || !isfinite(t.area) || t.area == 0.0f;
    t.s = t.area > 0.0f ? 1.0f : -1.0f;
    return t;
}

__global__ void __launch_bounds__(RZ_ATLAS_WG) rz_atlas_clear_kernel(uint32_t* __restrict__ owner, uint32_t texels) {
    const uint32_t t = blockIdx.x * RZ_ATLAS_WG + threadIdx.x;
    if (t < texels) owner[t] = kAtlasNone;
}

// grid.x strides over the triangles, grid.y = helpers: helper h takes the blocks h, h + grid.y, ... of the triangle's clipped bounding box.
// Every texel written lies in [x0, x1] x [y0, y1], which lies in the atlas.
__global__ void __launch_bounds__(RZ_ATLAS_WG) rz_atlas_cover_kernel(const float4* __restrict__ tris, uint32_t n, uint32_t base, uint32_t W, uint32_t H,
                                                                   uint32_t* __restrict__ owner) {
    const uint32_t lx = threadIdx.x % RZ_ATLAS_BLOCK_W, ly = threadIdx.x / RZ_ATLAS_BLOCK_W;
    for (unsigned long long i = blockIdx.x; i < n; i += gridDim.x) {
        float4 row[6];
        const AtlasTri t = take_tri(tris + 6ull * i, float(W), float(H), row);
        if (t.degenerate) continue;  // uniform: a wave has one triangle
        const float fx0 = fmaxf(fminf(fminf(t.a1.x, t.a2.x), t.a3.x), 0.0f), fx1 = fminf(fmaxf(fmaxf(t.a1.x, t.a2.x), t.a3.x), float(W - 1u));
        const float fy0 = fmaxf(fminf(fminf(t.a1.y, t.a2.y), t.a3.y), 0.0f), fy1 = fminf(fmaxf(fmaxf(t.a1.y, t.a2.y), t.a3.y), float(H - 1u));
        if (!(fx0 <= fx1 && fy0 <= fy1)) continue;
        const uint32_t x0 = uint32_t(ceilf(fx0)), x1 = uint32_t(floorf(fx1)), y0 = uint32_t(ceilf(fy0)), y1 = uint32_t(floorf(fy1));  // 0 <= .. <= W - 1, H - 1
        if (x0 > x1 || y0 > y1) continue;
        const uint32_t bx0 = x0 / RZ_ATLAS_BLOCK_W, by0 = y0 / RZ_ATLAS_BLOCK_H;
        const uint32_t nbx = x1 / RZ_ATLAS_BLOCK_W - bx0 + 1u, nby = y1 / RZ_ATLAS_BLOCK_H - by0 + 1u;
        const uint32_t blocks = nbx * nby;  // <= 2^28 / 64
        for (uint32_t b = blockIdx.y; b < blocks; b += gridDim.y) {
            const uint32_t x = (bx0 + b % nbx) * RZ_ATLAS_BLOCK_W + lx, y = (by0 + b / nbx) * RZ_ATLAS_BLOCK_H + ly;
            if (x < x0 || x > x1 || y < y0 || y > y1) continue;
            const float px = float(x), py = float(y);
            const float w1 = edge_value(t.a2, t.a3, px, py), w2 = edge_value(t.a3, t.a1, px, py), w3 = edge_value(t.a1, t.a2, px, py);
            if (t.s * w1 >= 0.0f && t.s * w2 >= 0.0f && t.s * w3 >= 0.0f) atomicMin(&owner[size_t(y) * W + x], base + uint32_t(i));
        }
    }
}

// thread t: texel (t % W, t / W).  first: every texel is written; otherwise only those whose owner is one of this add's n triangles.
__global__ void __launch_bounds__(RZ_ATLAS_WG) rz_atlas_points_kernel(const float4* __restrict__ tris, uint32_t n, uint32_t base, uint32_t W, uint32_t H,
                                                                    const uint32_t* __restrict__ owner, const float4* __restrict__ instances, uint32_t instance,
                                                                    float near_, float far_, uint32_t first, float4* __restrict__ points,
                                                                    uint4* __restrict__ samples) {
    const uint32_t t = blockIdx.x * RZ_ATLAS_WG + threadIdx.x;
    if (t >= W * H) return;
    const uint32_t o = owner[t];
    const bool mine = o != kAtlasNone && o >= base && o - base < n;
    if (!mine) {
        if (first) {
            points[2 * size_t(t)] = points[2 * size_t(t) + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            samples[t] = make_uint4(kAtlasNone, 0u, 0u, 0u);
        }
        return;
    }
    float4 row[6];
    const AtlasTri tri = take_tri(tris + 6 * size_t(o - base), float(W), float(H), row);
    const float px = float(t % W), py = float(t / W);
    const float w2 = edge_value(tri.a3, tri.a1, px, py), w3 = edge_value(tri.a1, tri.a2, px, py);
    const float sa = tri.s * tri.area;
    const float bx = (tri.s * w2) / sa, by = (tri.s * w3) / sa;
    const float b1 = (1.0f - bx) - by;

    const float4 i0 = instances[7 * size_t(instance)], i1 = instances[7 * size_t(instance) + 1], i2 = instances[7 * size_t(instance) + 2],
                 i3 = instances[7 * size_t(instance) + 3], i4 = instances[7 * size_t(instance) + 4];
    const v3 position = xyz(i0), scale = xyz(i1), xa = xyz(i2), ya = xyz(i3), za = xyz(i4);

    const v3 p1 = xyz(row[0]), p2 = xyz(row[1]), p3 = xyz(row[2]), n1 = xyz(row[3]), n2 = xyz(row[4]), n3 = xyz(row[5]);
    const v3 p = p1 * b1 + p2 * bx + p3 * by;
    const v3 world = transform_forward(xa, ya, za, p * scale) + position;
    const bool flat = n1.x == 0.0f && n1.y == 0.0f && n1.z == 0.0f && n2.x == 0.0f && n2.y == 0.0f && n2.z == 0.0f && n3.x == 0.0f && n3.y == 0.0f && n3.z == 0.0f;
    v3 nn = flat ? normalized(cross(p2 - p3, p2 - p1)) : n1 * b1 + n2 * bx + n3 * by;
    nn = normalized(transform_forward(xa, ya, za, normalized(nn) / scale));
    if (!(isfinite(nn.x) && isfinite(nn.y) && isfinite(nn.z)) || (nn.x == 0.0f && nn.y == 0.0f && nn.z == 0.0f)) nn = V3(0.0f, 0.0f, 0.0f);
    points[2 * size_t(t)] = make_float4(world.x, world.y, world.z, near_);
    points[2 * size_t(t) + 1] = make_float4(nn.x, nn.y, nn.z, far_);
    samples[t] = make_uint4(o, __float_as_uint(bx), __float_as_uint(by), 0u);
}

// thread t: texel t in ring r, reading (rec_src, ring_src) and writing (rec_dst, ring_dst).  r == 0: only ring_dst, from the samples.
__global__ void __launch_bounds__(RZ_ATLAS_WG) rz_atlas_dilate_kernel(const uint4* __restrict__ samples, const uint4* __restrict__ rec_src,
                                                                    const uint32_t* __restrict__ ring_src, uint4* __restrict__ rec_dst,
                                                                    uint32_t* __restrict__ ring_dst, uint32_t W, uint32_t H, uint32_t r) {
    const uint32_t t = blockIdx.x * RZ_ATLAS_WG + threadIdx.x;
    if (t >= W * H) return;
    if (r == 0u) {
        ring_dst[t] = samples[t].x == kAtlasNone ? kAtlasNone : 0u;
        return;
    }
    uint32_t ring = ring_src[t];
    uint4 rec = rec_src[t];
    if (ring == kAtlasNone) {
        const int x = int(t % W), y = int(t / W);
        constexpr int dx[8] = {-1, 1, 0, 0, -1, 1, -1, 1}, dy[8] = {0, 0, -1, 1, -1, -1, 1, 1};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int nx = x + dx[k], ny = y + dy[k];
            if (nx < 0 || ny < 0 || nx >= int(W) || ny >= int(H)) continue;
            const size_t at = size_t(ny) * W + size_t(nx);
            if (ring_src[at] != kAtlasNone) {
                rec = rec_src[at], ring = r;
                break;
            }
        }
    }
    rec_dst[t] = rec, ring_dst[t] = ring;
}

}  // namespace hiprz

using namespace hiprz;

struct hiprz_atlas : Session {
    uint32_t W = 0, H = 0;
    bool begun = false;  // a begin has set the size
    bool fresh = false;  // the next add is the first after a begin: it clears the owner map and writes every texel
    bool built = false;  // an add has run since the begin: the arrays hold this atlas
    uint32_t* owner = nullptr;
    float4* points = nullptr;
    uint4* samples = nullptr;
    uint4* records = nullptr;  // 16 bytes per texel for what the caller bakes: hiprz_atlas_records_device
    size_t capacity = 0;       // texels the four arrays hold
    uint4* scratch_records = nullptr;  // the dilation's other side
    uint32_t *ring_a = nullptr, *ring_b = nullptr;
    size_t scratch_capacity = 0;
    const uint32_t* last_ring = nullptr;  // the ring map of the last dilation since the begin (ring_a or ring_b)

    size_t texels() const { return size_t(W) * H; }
    void release_scratch() {
        if (scratch_records) (void)hipFree(scratch_records);
        if (ring_a) (void)hipFree(ring_a);
        if (ring_b) (void)hipFree(ring_b);
        scratch_records = nullptr, ring_a = ring_b = nullptr, scratch_capacity = 0, last_ring = nullptr;
    }
    void release_arrays() {
        if (owner) (void)hipFree(owner);  // (hipFree waits for whatever still uses the buffer)
        if (points) (void)hipFree(points);
        if (samples) (void)hipFree(samples);
        if (records) (void)hipFree(records);
        owner = nullptr, points = nullptr, samples = records = nullptr, capacity = 0;
    }
};

namespace {
uint32_t waves_for(size_t texels) { return uint32_t((texels + RZ_ATLAS_WG - 1u) / RZ_ATLAS_WG); }

// room for the atlas of the last begin on the current device (call it after a view); all four arrays or none
int grow_arrays(hiprz_atlas* a, const char* what) {
    const size_t need = a->texels();
    if (need <= a->capacity) return HIPRZ_OK;
    a->release_arrays();
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&a->owner), need * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&a->points), need * sizeof(hiprz_bake_point));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&a->samples), need * sizeof(hiprz_atlas_sample));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&a->records), need * 16u);
    if (e != hipSuccess) {
        a->release_arrays();
        return fail_hip(a, what, e);
    }
    a->capacity = need;
    return HIPRZ_OK;
}

int grow_scratch(hiprz_atlas* a, const char* what) {
    const size_t need = a->texels();
    if (need <= a->scratch_capacity) return HIPRZ_OK;
    a->release_scratch();
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&a->scratch_records), need * 16u);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&a->ring_a), need * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&a->ring_b), need * sizeof(uint32_t));
    if (e != hipSuccess) {
        a->release_scratch();
        return fail_hip(a, what, e);
    }
    a->scratch_capacity = need;
    return HIPRZ_OK;
}

// what an add refuses before anything is launched or copied; on HIPRZ_OK the view is in `s` and the head device is current
int refuse_add(hiprz_atlas* a, const void* tris, size_t n, uint32_t base, uint32_t instance, float near_, float far_, const char* what, DScene& s) {
    if (!a) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null atlas");
    int code;
    if (const char* why = atlas_add_refusal(!tris && n != 0u, a->begun, n, base, near_, far_, &code)) return fail(a, code, std::string(what) + ": " + why);
    if (const int rc = view(a, what, s); rc != HIPRZ_OK) return rc;
    if (const char* why = atlas_instance_refusal(instance, s.n_instances)) return fail(a, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    return HIPRZ_OK;
}

// the add of n device triangles on the view the call has fetched
int launch_add(hiprz_atlas* a, const DScene& s, const hiprz_atlas_tri* tris, size_t n, uint32_t base, uint32_t instance, float near_, float far_,
               hipStream_t stream, const char* what) {
    if (const int rc = grow_arrays(a, what); rc != HIPRZ_OK) return rc;
    const uint32_t waves = waves_for(a->texels());
    const float4* rows = reinterpret_cast<const float4*>(tris);
    if (a->fresh) hipLaunchKernelGGL(rz_atlas_clear_kernel, dim3(waves), dim3(RZ_ATLAS_WG), 0, stream, a->owner, uint32_t(a->texels()));
    if (n) {
        const uint32_t grid_x = uint32_t(n < (size_t(1) << 22) ? n : size_t(1) << 22);
        hipLaunchKernelGGL(rz_atlas_cover_kernel, dim3(grid_x, RZ_ATLAS_HELPERS), dim3(RZ_ATLAS_WG), 0, stream, rows, uint32_t(n), base, a->W, a->H, a->owner);
    }
    if (n || a->fresh)
        hipLaunchKernelGGL(rz_atlas_points_kernel, dim3(waves), dim3(RZ_ATLAS_WG), 0, stream, rows, uint32_t(n), base, a->W, a->H, a->owner, s.instances, instance, near_,
                           far_, a->fresh ? 1u : 0u, a->points, a->samples);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(a, what, e);
    a->fresh = false, a->built = true;
    return HIPRZ_OK;
}

int refuse_dilate(hiprz_atlas* a, bool any_null, uint32_t rings, const char* what) {
    if (!a) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null atlas");
    int code;
    if (const char* why = atlas_dilate_refusal(any_null, a->built, rings, &code)) return fail(a, code, std::string(what) + ": " + why);
    if (const hipError_t e = hipSetDevice(a->device); e != hipSuccess) return fail_hip(a, what, e);  // (known: an add has fetched a view)
    return HIPRZ_OK;
}

// `rings` rings in place on `records`; the ring map to ring_out when it is not null
int launch_dilate(hiprz_atlas* a, uint4* records, uint32_t rings, uint32_t* ring_out, hipStream_t stream, const char* what) {
    if (const int rc = grow_scratch(a, what); rc != HIPRZ_OK) return rc;
    const size_t texels = a->texels();
    const uint32_t waves = waves_for(texels);
    uint4 *rec = records, *rec_other = a->scratch_records;
    uint32_t *ring = a->ring_a, *ring_other = a->ring_b;
    hipLaunchKernelGGL(rz_atlas_dilate_kernel, dim3(waves), dim3(RZ_ATLAS_WG), 0, stream, a->samples, static_cast<const uint4*>(nullptr),
                       static_cast<const uint32_t*>(nullptr), static_cast<uint4*>(nullptr), ring, a->W, a->H, 0u);  // r == 0: the ring map of the samples
    for (uint32_t r = 1u; r <= rings; ++r) {
        hipLaunchKernelGGL(rz_atlas_dilate_kernel, dim3(waves), dim3(RZ_ATLAS_WG), 0, stream, a->samples, rec, ring, rec_other, ring_other, a->W, a->H, r);
        uint4* t = rec;
        rec = rec_other, rec_other = t;
        uint32_t* u = ring;
        ring = ring_other, ring_other = u;
    }
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(a, what, e);
    if (rec != records)
        if (const hipError_t e = hipMemcpyAsync(records, rec, texels * 16u, hipMemcpyDeviceToDevice, stream); e != hipSuccess) return fail_hip(a, what, e);
    a->last_ring = ring;
    if (ring_out)
        if (const hipError_t e = hipMemcpyAsync(ring_out, ring, texels * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream); e != hipSuccess) return fail_hip(a, what, e);
    return HIPRZ_OK;
}
}  // namespace

extern "C" {

int hiprz_atlas_create(hiprz_atlas** out, hiprz_ctx* ctx) { return create(out, ctx, "atlas_create"); }

int hiprz_atlas_destroy(hiprz_atlas* a) {
    return destroy(a, a && (a->capacity || a->scratch_capacity), [a] { a->release_arrays(), a->release_scratch(); });
}

const char* hiprz_atlas_last_error(const hiprz_atlas* a) { return last_error(a); }

int hiprz_atlas_begin(hiprz_atlas* a, uint32_t width, uint32_t height) {
    if (!a) return fail(nullptr, HIPRZ_ERR_INVALID, "atlas_begin: null atlas");
    if (const char* why = atlas_size_refusal(width, height)) return fail(a, HIPRZ_ERR_INVALID, std::string("atlas_begin: ") + why);
    a->W = width, a->H = height, a->begun = a->fresh = true, a->built = false, a->last_ring = nullptr;
    return HIPRZ_OK;
}

int hiprz_atlas_add(hiprz_atlas* a, const hiprz_atlas_tri* tris_device, size_t n, uint32_t triangle_base, uint32_t instance, float near_, float far_, void* stream) {
    const char* what = "atlas_add";
    DScene s;
    if (const int rc = refuse_add(a, tris_device, n, triangle_base, instance, near_, far_, what, s); rc != HIPRZ_OK) return rc;
    return launch_add(a, s, tris_device, n, triangle_base, instance, near_, far_, stream_of(a, stream), what);
}

int hiprz_atlas_add_host(hiprz_atlas* a, const hiprz_atlas_tri* tris, size_t n, uint32_t triangle_base, uint32_t instance, float near_, float far_) {
    const char* what = "atlas_add_host";
    DScene s;
    if (const int rc = refuse_add(a, tris, n, triangle_base, instance, near_, far_, what, s); rc != HIPRZ_OK) return rc;
    hipStream_t st = stream_of(a, nullptr);
    if (n == 0u) return launch_add(a, s, nullptr, 0u, triangle_base, instance, near_, far_, st, what);
    if (const int rc = grow_staging(a, what, 6u * n, 16u, sizeof(uint32_t), atlas_capacity); rc != HIPRZ_OK) return rc;
    const Staging& g = a->staging;
    std::memcpy(g.pinned_in, tris, n * sizeof(hiprz_atlas_tri));
    if (const hipError_t e = hipMemcpyAsync(g.dev_in, g.pinned_in, n * sizeof(hiprz_atlas_tri), hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(a, what, e);
    if (const int rc = launch_add(a, s, static_cast<const hiprz_atlas_tri*>(g.dev_in), n, triangle_base, instance, near_, far_, st, what); rc != HIPRZ_OK) return rc;
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(a, what, e);  // the staging is free for the next call
    return HIPRZ_OK;
}

const hiprz_bake_point* hiprz_atlas_points_device(const hiprz_atlas* a) { return a && a->built ? reinterpret_cast<const hiprz_bake_point*>(a->points) : nullptr; }

const hiprz_atlas_sample* hiprz_atlas_samples_device(const hiprz_atlas* a) { return a && a->built ? reinterpret_cast<const hiprz_atlas_sample*>(a->samples) : nullptr; }

int hiprz_atlas_read_host(hiprz_atlas* a, hiprz_bake_point* points_out, hiprz_atlas_sample* samples_out) {
    const char* what = "atlas_read_host";
    if (!a) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null atlas");
    if (!points_out && !samples_out) return fail(a, HIPRZ_ERR_INVALID, std::string(what) + ": null pointer");
    if (!a->built) return fail(a, HIPRZ_ERR_STATE, std::string(what) + ": nothing has been added since the atlas was begun");
    if (const hipError_t e = hipSetDevice(a->device); e != hipSuccess) return fail_hip(a, what, e);
    hipStream_t st = stream_of(a, nullptr);
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(a, what, e);
    if (points_out)
        if (const hipError_t e = hipMemcpy(points_out, a->points, a->texels() * sizeof(hiprz_bake_point), hipMemcpyDeviceToHost); e != hipSuccess) return fail_hip(a, what, e);
    if (samples_out)
        if (const hipError_t e = hipMemcpy(samples_out, a->samples, a->texels() * sizeof(hiprz_atlas_sample), hipMemcpyDeviceToHost); e != hipSuccess) return fail_hip(a, what, e);
    return HIPRZ_OK;
}

void* hiprz_atlas_records_device(const hiprz_atlas* a) { return a && a->built ? a->records : nullptr; }

int hiprz_atlas_read_records_host(hiprz_atlas* a, void* records16_out, uint32_t* ring_out) {
    const char* what = "atlas_read_records_host";
    if (!a) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null atlas");
    if (!records16_out && !ring_out) return fail(a, HIPRZ_ERR_INVALID, std::string(what) + ": null pointer");
    if (!a->built) return fail(a, HIPRZ_ERR_STATE, std::string(what) + ": nothing has been added since the atlas was begun");
    if (ring_out && !a->last_ring) return fail(a, HIPRZ_ERR_STATE, std::string(what) + ": nothing has been dilated since the atlas was begun");
    if (const hipError_t e = hipSetDevice(a->device); e != hipSuccess) return fail_hip(a, what, e);
    if (const hipError_t e = hipStreamSynchronize(stream_of(a, nullptr)); e != hipSuccess) return fail_hip(a, what, e);
    if (records16_out)
        if (const hipError_t e = hipMemcpy(records16_out, a->records, a->texels() * 16u, hipMemcpyDeviceToHost); e != hipSuccess) return fail_hip(a, what, e);
    if (ring_out)
        if (const hipError_t e = hipMemcpy(ring_out, a->last_ring, a->texels() * sizeof(uint32_t), hipMemcpyDeviceToHost); e != hipSuccess) return fail_hip(a, what, e);
    return HIPRZ_OK;
}

int hiprz_atlas_dilate(hiprz_atlas* a, void* records16_device, uint32_t rings, uint32_t* ring_out_device, void* stream) {
    const char* what = "atlas_dilate";
    if (const int rc = refuse_dilate(a, !records16_device, rings, what); rc != HIPRZ_OK) return rc;
    return launch_dilate(a, static_cast<uint4*>(records16_device), rings, ring_out_device, stream_of(a, stream), what);
}

int hiprz_atlas_dilate_host(hiprz_atlas* a, void* records16, uint32_t rings, uint32_t* ring_out) {
    const char* what = "atlas_dilate_host";
    if (const int rc = refuse_dilate(a, !records16, rings, what); rc != HIPRZ_OK) return rc;
    const size_t texels = a->texels();
    if (const int rc = grow_staging(a, what, texels, 16u, sizeof(uint32_t), atlas_capacity); rc != HIPRZ_OK) return rc;
    const Staging& g = a->staging;
    hipStream_t st = stream_of(a, nullptr);
    std::memcpy(g.pinned_in, records16, texels * 16u);
    if (const hipError_t e = hipMemcpyAsync(g.dev_in, g.pinned_in, texels * 16u, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(a, what, e);
    if (const int rc = launch_dilate(a, static_cast<uint4*>(g.dev_in), rings, static_cast<uint32_t*>(g.dev_out), st, what); rc != HIPRZ_OK) return rc;
    if (const hipError_t e = hipMemcpyAsync(g.pinned_in, g.dev_in, texels * 16u, hipMemcpyDeviceToHost, st); e != hipSuccess) return fail_hip(a, what, e);
    if (const hipError_t e = hipMemcpyAsync(g.pinned_out, g.dev_out, texels * sizeof(uint32_t), hipMemcpyDeviceToHost, st); e != hipSuccess) return fail_hip(a, what, e);
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(a, what, e);
    std::memcpy(records16, g.pinned_in, texels * 16u);
    if (ring_out) std::memcpy(ring_out, g.pinned_out, texels * sizeof(uint32_t));
    return HIPRZ_OK;
}

}  // extern "C"
