// hiprz_gather.hip — bounce baking (include/hiprz_gather.h): the K hemisphere rays of a surface point are made from a table of local
// directions, walked to their closest hits by the query's closest-hit walk, looked up in an atlas that holds light through the caller's
// chart map and averaged across the wave in a fixed order, 16 bytes out per point.  A library of its own (libhiprz_gather.so) beside the
// seven whose kernels and ABI are pinned; the ray rule is the query's device function (query/hiprz_query_device.hpp, no __global__) and
// the walk is closest_hit_skip as closest_record calls it, so a ray's t, instance and triangle are hiprz_query_closest's.  The frame and
// the ray of hiprz_bake.h are restated here.  The context is read through hiprz_device_view on every call.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hiprz_gather.h"
#include "hiprz_gather_host.hpp"
#include "query/hiprz_query_device.hpp"
#include "query/hiprz_session.hpp"  // the handle, its errors, the view, the staging and its round trip

// threads per workgroup: one wave — the ballots and the butterfly span exactly the workgroup
#define RZ_GATHER_WG 64

namespace hiprz {

// what a point gives every one of its rays: the two words of the point, whether it is valid, its set and its frame
struct GatherPoint {
    float4 p0, p1;  // position, near_ | normal as given, far_
    v3 n, t, bt;    // include/hiprz_gather.h "THE FRAME" of the normalised normal (read on a valid point only)
    uint32_t set;
    bool valid;
};

RZ_DEV GatherPoint gather_point(const float4* __restrict__ points, uint32_t i, uint32_t seed, uint32_t S) {
    GatherPoint p;
    p.p0 = points[2 * size_t(i)], p.p1 = points[2 * size_t(i) + 1];
    Ray along;
    p.valid = take_ray(p.p0, p.p1, HIPRZ_QUERY_NORMALIZE, along);  // valid: along.d = normalized(normal)
    p.set = gather_hash(i ^ seed) % S;
    const v3 n = along.d;
    const float s = copysignf(1.0f, n.z);
    const float a = -1.0f / (s + n.z);
    const float b = (n.x * n.y) * a;
    p.n = n;
    p.t = V3(1.0f + ((s * n.x) * n.x) * a, s * b, (-s) * n.x);
    p.bt = V3(b, s + (n.y * n.y) * a, -n.y);
    return p;
}

// the ray of (point, direction k) as the two float4 of a hiprz_ray.  An invalid point: direction +0, which the ray rule refuses.
RZ_DEV void gather_ray(const GatherPoint& p, const float4* __restrict__ dirs, uint32_t K, uint32_t k, float4& r0, float4& r1) {
    v3 d = V3(0.0f, 0.0f, 0.0f);
    if (p.valid) {
        const float4 l = dirs[size_t(p.set) * K + k];
        d.x = (p.t.x * l.x + p.bt.x * l.y) + p.n.x * l.z;
        d.y = (p.t.y * l.x + p.bt.y * l.y) + p.n.y * l.z;
        d.z = (p.t.z * l.x + p.bt.z * l.y) + p.n.z * l.z;
    }
    r0 = p.p0;
    r1 = make_float4(d.x, d.y, d.z, p.p1.w);
}

// the chart map on the device: one base per instance of the view (the host holds the two counts against each other), two float4 per chart
struct GatherMap {
    const uint32_t* base;
    const float4* uv;  // (u1, v1, u2, v2) (u3, v3, 0, 0)
    uint32_t n_charts;
};

// include/hiprz_gather.h "THE SAMPLES": the walk of one ray and the chart under its hit.  closest_record's walk without its
// analyze_intersection: no material, texture or normal is fetched, only the hit triangle's second word for its source index.
RZ_DEV hiprz_gather_sample gather_walk(const DScene& s, const GatherMap& map, const float4 r0, const float4 r1) {
    hiprz_gather_sample g;
    g.id = HIPRZ_GATHER_INVALID_RAY, g.bx = g.by = 0.0f, g.t = r1.w;
    Ray ray;
    if (!take_ray(r0, r1, 0u, ray)) return g;
    g.id = HIPRZ_GATHER_MISS;
    Hit hit;
    hit.instance = -1, hit.triangle = 0u, hit.bx = hit.by = 0.0f, hit.external = true;
    Counters cnt;
    int found = 0;
    if (s.n_instances != 0u) found = closest_hit_skip<false, false, true>(s, TopCache{nullptr, nullptr, 0u}, ray, hit, cnt);
    if (found == 2) {  // hit.instance / hit.triangle are in range only here
        g.bx = hit.bx, g.by = hit.by, g.t = ray.far_;
        g.id = HIPRZ_GATHER_BACK;
        if (hit.external) {
            const uint32_t base = map.base[uint32_t(hit.instance)];
            const unsigned long long id = (unsigned long long)base + __float_as_uint(s.tris[3 * hit.triangle + 1].w);  // hiprz_tri::source_index
            g.id = (base == HIPRZ_GATHER_NONE || id >= map.n_charts) ? HIPRZ_GATHER_UNMAPPED : uint32_t(id);
        }
    }
    return g;
}

// include/hiprz_gather.h "THE LOOKUP": true and the texel's RGB when the sample lies on a chart and its texel has a value
RZ_DEV bool gather_lookup(const GatherMap& map, const hiprz_gather_sample& g, const float4* __restrict__ source, uint32_t W, uint32_t H, v3& rgb) {
    if (g.id >= HIPRZ_GATHER_MAX_CHARTS) return false;  // one of the codes
    const float4 c0 = map.uv[2 * size_t(g.id)], c1 = map.uv[2 * size_t(g.id) + 1];
    const float b1 = (1.0f - g.bx) - g.by;
    const float u = (c0.x * b1 + c0.z * g.bx) + c1.x * g.by;
    const float v = (c0.y * b1 + c0.w * g.bx) + c1.y * g.by;
    if (!isfinite(u) || !isfinite(v)) return false;
    float fx = floorf(u * float(W)), fy = floorf(v * float(H));  // (finite or an infinity, never NaN: the clamps below are total)
    fx = fx < 0.0f ? 0.0f : (fx > float(W - 1u) ? float(W - 1u) : fx);
    fy = fy < 0.0f ? 0.0f : (fy > float(H - 1u) ? float(H - 1u) : fy);
    const float4 texel = source[size_t(uint32_t(fy)) * W + uint32_t(fx)];
    if (__float_as_uint(texel.w) == HIPRZ_GATHER_INVALID) return false;
    rgb = xyz(texel);
    return true;
}

// One wave per workgroup.  K >= 64: the wave gathers point blockIdx.x in K / 64 rounds, lane l walks rays l, 64 + l, ...  K < 64: it gathers
// the 64 / K points from blockIdx.x * (64 / K) on, lane l walks ray l % K of point l / K.  A lane whose point is >= n or invalid walks
// nothing and contributes +0, but takes part in every ballot and shuffle: nothing returns before them.
// Five waves per SIMD: 96 VGPRs and 24 bytes of scratch per lane instead of 118 VGPRs and none, and 3 - 10 % sooner than the four-wave build
// in every row measured (DESIGN.md §6 "Bounce baking"); make GATHER_DEFS=-DRZ_GATHER_WAVES=4 builds the other one.
#ifndef RZ_GATHER_WAVES
#define RZ_GATHER_WAVES 5
#endif
__global__ void __launch_bounds__(RZ_GATHER_WG, RZ_GATHER_WAVES) rz_gather_kernel(const DScene s, const float4* __restrict__ points, uint32_t n, const float4* __restrict__ dirs,
                                                                uint32_t K, uint32_t S, uint32_t seed, const GatherMap map,
                                                                const float4* __restrict__ source, uint32_t W, uint32_t H, const float4 sky,
                                                                float4* __restrict__ out) {
    const uint32_t lane = threadIdx.x;
    const uint32_t seg = K < 64u ? K : 64u;      // lanes per point, a power of two
    const uint32_t first = lane & ~(seg - 1u);  // the first lane of this lane's point
    const uint32_t point = blockIdx.x * (64u / seg) + lane / seg;
    const bool inside = point < n;
    GatherPoint p;
    p.valid = false;
    if (inside) p = gather_point(points, point, seed, S);
    const bool walks = inside && p.valid;
    const unsigned long long segment = (seg == 64u ? ~0ull : (1ull << seg) - 1ull) << first;
    uint32_t n_read = 0u, n_missed = 0u;
    v3 sum = V3(0.0f, 0.0f, 0.0f);
    const uint32_t rounds = K < 64u ? 1u : K / 64u;  // of a kernel argument alone: the same trip count on every lane
    for (uint32_t r = 0u; r < rounds; ++r) {
        const uint32_t k = 64u * r + (lane - first);
        bool read = false, missed = false;
        v3 c = V3(0.0f, 0.0f, 0.0f);
        if (walks) {
            float4 r0, r1;
            gather_ray(p, dirs, K, k, r0, r1);
            const hiprz_gather_sample g = gather_walk(s, map, r0, r1);
            missed = g.id == HIPRZ_GATHER_MISS || g.id == HIPRZ_GATHER_INVALID_RAY;
            if (missed) c = V3(sky.x, sky.y, sky.z);
            else read = gather_lookup(map, g, source, W, H, c);
        }
        n_read += uint32_t(__popcll(__ballot(read) & segment));
        n_missed += uint32_t(__popcll(__ballot(missed) & segment));
        sum.x = sum.x + c.x;
        sum.y = sum.y + c.y;
        sum.z = sum.z + c.z;
    }
    for (uint32_t off = 1u; off < seg; off <<= 1) {
        sum.x = sum.x + __shfl_xor(sum.x, int(off));
        sum.y = sum.y + __shfl_xor(sum.y, int(off));
        sum.z = sum.z + __shfl_xor(sum.z, int(off));
    }
    const float rcp = 1.0f / float(K);
    if (inside && lane == first)
        out[point] = p.valid ? make_float4(sum.x * rcp, sum.y * rcp, sum.z * rcp, __uint_as_float(n_read | (n_missed << 16)))
                             : make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(HIPRZ_GATHER_INVALID));
}

// thread i: sample i = (point i / K, direction i % K), the record the gather makes for that pair
__global__ void __launch_bounds__(RZ_GATHER_WG) rz_gather_samples_kernel(const DScene s, const float4* __restrict__ points, uint32_t n_rays,
                                                                        const float4* __restrict__ dirs, uint32_t K, uint32_t S, uint32_t seed, const GatherMap map,
                                                                        float4* __restrict__ samples) {
    const uint32_t i = blockIdx.x * RZ_GATHER_WG + threadIdx.x;
    if (i >= n_rays) return;
    const GatherPoint p = gather_point(points, i / K, seed, S);
    float4 r0, r1;
    gather_ray(p, dirs, K, i % K, r0, r1);
    const hiprz_gather_sample g = gather_walk(s, map, r0, r1);
    samples[i] = make_float4(__uint_as_float(g.id), g.bx, g.by, g.t);
}

// thread i: include/hiprz_gather.h "COMPOSE" on texel i; a null indirect or emission reads +0
__global__ void __launch_bounds__(RZ_GATHER_WG) rz_gather_compose_kernel(const float4* direct, const float4* indirect, const float4* albedo, const float4* emission,
                                                                        float4* out, uint32_t n_texels) {
    const uint32_t i = blockIdx.x * RZ_GATHER_WG + threadIdx.x;
    if (i >= n_texels) return;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 d = direct[i], a = albedo[i], g = indirect ? indirect[i] : zero, e = emission ? emission[i] : zero;
    out[i] = make_float4((a.x * (d.x + g.x)) + e.x, (a.y * (d.y + g.y)) + e.y, (a.z * (d.z + g.z)) + e.z, d.w);
}

}  // namespace hiprz

using namespace hiprz;

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_gather_texel) == 16 && sizeof(hiprz_gather_sample) == 16 && sizeof(hiprz_gather_chart) == 32,
              "two 16-byte loads per point and chart, one 16-byte store per texel and sample");

struct hiprz_gather : Session {
    std::vector<float> table;  // the directions as set, S*K float4 with w = 0; K == 0: none yet
    uint32_t K = 0, S = 0;
    float4* dirs = nullptr;    // the device copy, made by the first call after set_directions (`stale`)
    bool stale = false;
    std::vector<uint32_t> base;            // the chart map as set
    std::vector<hiprz_gather_chart> uv;
    bool has_charts = false, charts_stale = false;
    uint32_t* base_dev = nullptr;          // its device copy, made by the first call after set_charts
    float4* uv_dev = nullptr;
    float4* source_dev = nullptr;          // the device copy of a host source, source_capacity records
    size_t source_capacity = 0;
};

namespace {
// what every call over points refuses before a view is asked for; *empty: nothing to do (n == 0 is HIPRZ_OK without a view or a launch)
int refuse(hiprz_gather* h, bool any_null, size_t n, const char* what, bool* empty) {
    *empty = false;
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null gather");
    int code;
    if (const char* why = gather_refusal(any_null, n, h->K, h->has_charts, &code)) return fail(h, code, std::string(what) + ": " + why);
    *empty = n == 0u;
    return HIPRZ_OK;
}

// the view of the call, held against the chart map's number of instances
int view_and_map(hiprz_gather* h, const char* what, DScene& s) {
    if (const int rc = view(h, what, s); rc != HIPRZ_OK) return rc;
    if (s.n_instances != h->base.size()) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": the chart map is for another number of instances than the scene has");
    return HIPRZ_OK;
}

// a host array goes to a new device buffer, ordered on the call's stream (the head device is current: a view was just taken); at least 16
// bytes, so that an empty array has an address too.  hipFree waits for whatever still reads the old buffer.
template <typename T>
hipError_t replace(T*& dev, const void* host, size_t bytes, hipStream_t stream) {
    if (dev) (void)hipFree(dev);
    dev = nullptr;
    if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), bytes < 16u ? 16u : bytes); e != hipSuccess) return e;
    return bytes ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream) : hipSuccess;
}

// the table and the chart map a set_* left on the host go to the device before the call's kernel; the stream is waited for, since the host
// arrays are pageable and may be replaced
int place_tables(hiprz_gather* h, hipStream_t stream, const char* what) {
    if (!h->stale && !h->charts_stale) return HIPRZ_OK;
    if (h->stale)
        if (const hipError_t e = replace(h->dirs, h->table.data(), h->table.size() * sizeof(float), stream); e != hipSuccess) return fail_hip(h, what, e);
    if (h->charts_stale) {
        if (const hipError_t e = replace(h->base_dev, h->base.data(), h->base.size() * sizeof(uint32_t), stream); e != hipSuccess) return fail_hip(h, what, e);
        if (const hipError_t e = replace(h->uv_dev, h->uv.data(), h->uv.size() * sizeof(hiprz_gather_chart), stream); e != hipSuccess) return fail_hip(h, what, e);
    }
    if (const hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return fail_hip(h, what, e);
    h->stale = h->charts_stale = false;
    return HIPRZ_OK;
}

GatherMap map_of(const hiprz_gather* h) { return GatherMap{h->base_dev, h->uv_dev, uint32_t(h->uv.size())}; }

// the gather of n device points on the view the call has fetched
int launch_gather(hiprz_gather* h, const DScene& s, const hiprz_bake_point* points, size_t n, uint32_t seed, const void* source, uint32_t W, uint32_t H,
                  const float sky[3], hiprz_gather_texel* out, hipStream_t stream, const char* what) {
    if (const int rc = place_tables(h, stream, what); rc != HIPRZ_OK) return rc;
    const uint32_t per_wave = h->K < 64u ? 64u / h->K : 1u;
    const uint32_t grid = uint32_t((n + per_wave - 1u) / per_wave);
    hipLaunchKernelGGL(rz_gather_kernel, dim3(grid), dim3(RZ_GATHER_WG), 0, stream, s, reinterpret_cast<const float4*>(points), uint32_t(n), h->dirs, h->K, h->S, seed,
                       map_of(h), static_cast<const float4*>(source), W, H, make_float4(sky[0], sky[1], sky[2], 0.0f), reinterpret_cast<float4*>(out));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}
}  // namespace

extern "C" {

int hiprz_gather_create(hiprz_gather** out, hiprz_ctx* ctx) { return create(out, ctx, "gather_create"); }

int hiprz_gather_destroy(hiprz_gather* h) {
    return destroy(h, h && (h->dirs || h->base_dev || h->uv_dev || h->source_dev), [h] {
        for (void* p : {static_cast<void*>(h->dirs), static_cast<void*>(h->base_dev), static_cast<void*>(h->uv_dev), static_cast<void*>(h->source_dev)})
            if (p) (void)hipFree(p);
    });
}

const char* hiprz_gather_last_error(const hiprz_gather* h) { return last_error(h); }

int hiprz_gather_set_directions(hiprz_gather* h, const float* xyz0_host, uint32_t K, uint32_t S) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, "gather_set_directions: null gather");
    if (const char* why = gather_table_refusal(xyz0_host, K, S)) return fail(h, HIPRZ_ERR_INVALID, std::string("gather_set_directions: ") + why);
    h->table.assign(xyz0_host, xyz0_host + 4 * size_t(K) * S);
    for (size_t i = 3; i < h->table.size(); i += 4) h->table[i] = 0.0f;
    h->K = K, h->S = S, h->stale = true;
    return HIPRZ_OK;
}

int hiprz_gather_set_charts(hiprz_gather* h, const uint32_t* base_host, uint32_t n_instances, const hiprz_gather_chart* uv_host, uint32_t n_charts) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, "gather_set_charts: null gather");
    if (const char* why = gather_charts_refusal(base_host, n_instances, uv_host, n_charts)) return fail(h, HIPRZ_ERR_INVALID, std::string("gather_set_charts: ") + why);
    h->base.assign(base_host, base_host + n_instances);
    h->uv.assign(uv_host, uv_host + n_charts);
    h->has_charts = h->charts_stale = true;
    return HIPRZ_OK;
}

int hiprz_gather_texels(hiprz_gather* h, const hiprz_bake_point* points_device, size_t n, uint32_t seed, const void* source16_device, uint32_t W, uint32_t H,
                        const float sky[3], hiprz_gather_texel* out_device, void* stream) {
    const char* what = "gather_texels";
    bool empty;
    if (const int rc = refuse(h, !points_device || !source16_device || !sky || !out_device, n, what, &empty); rc != HIPRZ_OK) return rc;
    if (const char* why = gather_size_refusal(W, H)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    if (empty) return HIPRZ_OK;
    DScene s;
    if (const int rc = view_and_map(h, what, s); rc != HIPRZ_OK) return rc;
    return launch_gather(h, s, points_device, n, seed, source16_device, W, H, sky, out_device, stream_of(h, stream), what);
}

int hiprz_gather_samples(hiprz_gather* h, const hiprz_bake_point* points_device, size_t n, uint32_t seed, hiprz_gather_sample* samples_out_device, void* stream) {
    const char* what = "gather_samples";
    bool empty;
    if (const int rc = refuse(h, !points_device || !samples_out_device, n, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view_and_map(h, what, s); rc != HIPRZ_OK) return rc;
    hipStream_t st = stream_of(h, stream);
    if (const int rc = place_tables(h, st, what); rc != HIPRZ_OK) return rc;
    const uint32_t n_rays = uint32_t(n * h->K);  // < 2^31
    hipLaunchKernelGGL(rz_gather_samples_kernel, dim3((n_rays + RZ_GATHER_WG - 1u) / RZ_GATHER_WG), dim3(RZ_GATHER_WG), 0, st, s,
                       reinterpret_cast<const float4*>(points_device), n_rays, h->dirs, h->K, h->S, seed, map_of(h), reinterpret_cast<float4*>(samples_out_device));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

int hiprz_gather_texels_host(hiprz_gather* h, const hiprz_bake_point* points, size_t n, uint32_t seed, const void* source16, uint32_t W, uint32_t H, const float sky[3],
                             hiprz_gather_texel* out) {
    const char* what = "gather_texels_host";
    bool empty;
    if (const int rc = refuse(h, !points || !source16 || !sky || !out, n, what, &empty); rc != HIPRZ_OK) return rc;
    if (const char* why = gather_size_refusal(W, H)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    if (empty) return HIPRZ_OK;
    DScene s;
    if (const int rc = view_and_map(h, what, s); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the buffers
    if (const int rc = grow_staging(h, what, n, sizeof(hiprz_bake_point), sizeof(hiprz_gather_texel), gather_capacity); rc != HIPRZ_OK) return rc;
    const size_t texels = size_t(W) * H;
    hipStream_t st = stream_of(h, nullptr);
    if (texels > h->source_capacity) {
        if (h->source_dev) (void)hipFree(h->source_dev);
        h->source_dev = nullptr, h->source_capacity = 0;
        if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->source_dev), texels * 16u); e != hipSuccess) return fail_hip(h, what, e);
        h->source_capacity = texels;
    }
    if (const hipError_t e = hipMemcpyAsync(h->source_dev, source16, texels * 16u, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(h, what, e);  // the source is pageable and the caller's
    return round_trip(h, what, points, n, sizeof(hiprz_bake_point), out, sizeof(hiprz_gather_texel), [&](void* dev_points, void* dev_out, hipStream_t stream) {
        return launch_gather(h, s, static_cast<const hiprz_bake_point*>(dev_points), n, seed, h->source_dev, W, H, sky, static_cast<hiprz_gather_texel*>(dev_out), stream, what);
    });
}

int hiprz_gather_compose(hiprz_gather* h, const void* direct16_device, const void* indirect16_device, const void* albedo16_device, const void* emission16_device,
                         void* out16_device, size_t n_texels, void* stream) {
    const char* what = "gather_compose";
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null gather");
    if (const char* why = gather_compose_refusal(!direct16_device || !albedo16_device || !out16_device, n_texels)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    if (n_texels == 0u) return HIPRZ_OK;
    if (h->device >= 0) (void)hipSetDevice(h->device);  // (no view is taken here: the head device is known from the handle's first view on)
    hipLaunchKernelGGL(rz_gather_compose_kernel, dim3(uint32_t((n_texels + RZ_GATHER_WG - 1u) / RZ_GATHER_WG)), dim3(RZ_GATHER_WG), 0, stream_of(h, stream),
                       static_cast<const float4*>(direct16_device), static_cast<const float4*>(indirect16_device), static_cast<const float4*>(albedo16_device),
                       static_cast<const float4*>(emission16_device), static_cast<float4*>(out16_device), uint32_t(n_texels));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

int hiprz_gather_compose_host(hiprz_gather* h, const void* direct16, const void* indirect16, const void* albedo16, const void* emission16, void* out16, size_t n_texels) {
    const char* what = "gather_compose_host";
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null gather");
    if (const char* why = gather_compose_refusal(!direct16 || !albedo16 || !out16, n_texels)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    if (n_texels == 0u) return HIPRZ_OK;
    DScene s;
    if (const int rc = view(h, what, s); rc != HIPRZ_OK) return rc;  // makes the head device current for the buffers
    hipStream_t st = stream_of(h, nullptr);
    const size_t bytes = n_texels * 16u;
    const void* host[4] = {direct16, indirect16, albedo16, emission16};
    float4* dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // the four inputs (null where the host's is) and the output
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev[4]), bytes);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) {
        if (!host[i]) continue;
        e = hipMalloc(reinterpret_cast<void**>(&dev[i]), bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(dev[i], host[i], bytes, hipMemcpyHostToDevice, st);
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(rz_gather_compose_kernel, dim3(uint32_t((n_texels + RZ_GATHER_WG - 1u) / RZ_GATHER_WG)), dim3(RZ_GATHER_WG), 0, st, dev[0], dev[1], dev[2], dev[3], dev[4],
                           uint32_t(n_texels));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out16, dev[4], bytes, hipMemcpyDeviceToHost, st);
    const hipError_t waited = hipStreamSynchronize(st);  // in any case: the buffers go, and the host arrays are the caller's
    for (float4* p : dev)
        if (p) (void)hipFree(p);
    if (e == hipSuccess) e = waited;
    return e == hipSuccess ? HIPRZ_OK : fail_hip(h, what, e);
}

}  // extern "C"
