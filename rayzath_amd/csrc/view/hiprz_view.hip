// hiprz_view.hip — baked view (include/hiprz_view.h): one thread per pixel of the selected camera casts the pixel-centre ray, walks it to
// its closest hit by the query's closest-hit walk, and shades the hit from a lit atlas through the gather's chart map or — on an object
// outside the atlas — from a probe field and the surface's colour; 16 bytes and / or a float4 out per pixel.  A library of its own
// (libhiprz_view.so) beside the twelve whose kernels and ABI are pinned; the ray is generate_simple_ray's, the ray rule and the walk are the
// query's device functions (query/hiprz_query_device.hpp, no __global__), so a pixel's t, instance, triangle and side are
// hiprz_query_closest's on hiprz_query_pixel_rays's ray.  The lookups of hiprz_gather.h and hiprz_field.h are restated here.  The context
// is read through hiprz_device_view on every call.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hiprz_view.h"
#include "hiprz_view_host.hpp"
#include "query/hiprz_query_device.hpp"
#include "query/hiprz_session.hpp"  // the handle, its errors, the view and the staging

// threads per workgroup: one wave, an 8 x 8 block of pixels (or 64 consecutive pixels under RZ_VIEW_ROWS)
#define RZ_VIEW_WG 64

namespace hiprz {

// the chart map on the device: one base per instance of the view (the host holds the two counts against each other), two float4 per chart
struct ViewMap {
    const uint32_t* base;
    const float4* uv;  // (u1, v1, u2, v2) (u3, v3, 0, 0)
    uint32_t n_charts;
};

// the field of a call: the grid by value, the three arrays of its probes (vis may be null) and the params; probes == nullptr: no field
struct ViewField {
    hiprz_field_grid grid;
    const float4* probes;  // two float4 per probe
    const float4* sh;      // nine per probe
    const float4* vis;     // 33 per probe, or null
    float bias;
    uint32_t max_back;
};

// include/hiprz_view.h "THE KERNELS": the pixel of this thread; false when it lies outside the frame
RZ_DEV bool view_pixel_of(uint32_t width, uint32_t height, uint32_t& x, uint32_t& y) {
#if RZ_VIEW_ROWS_BUILD
    const size_t i = size_t(blockIdx.x) * RZ_VIEW_WG + threadIdx.x;
    if (i >= size_t(width) * height) return false;
    x = uint32_t(i % width), y = uint32_t(i / width);
    return true;
#else
    const uint32_t blocks_x = (width + 7u) / 8u;
    x = 8u * (blockIdx.x % blocks_x) + (threadIdx.x & 7u);
    y = 8u * (blockIdx.x / blocks_x) + (threadIdx.x >> 3);
    return x < width && y < height;
#endif
}

// include/hiprz_view.h "THE SAMPLES": the pixel's ray, its walk and the chart under its hit — hiprz_gather.h's record.  `ray` is the ray as
// walked (far_ = t of a hit), `hit` is in range only for an id below the codes, HIPRZ_GATHER_UNMAPPED or HIPRZ_GATHER_BACK.
RZ_DEV hiprz_gather_sample view_walk(const DScene& s, const DCamera& cam, const ViewMap& map, uint32_t x, uint32_t y, Ray& ray, Hit& hit) {
    Ray made;
    generate_simple_ray(cam, made, x, y);
    const float4 r0 = make_float4(made.o.x, made.o.y, made.o.z, made.near_), r1 = make_float4(made.d.x, made.d.y, made.d.z, made.far_);  // hiprz_query_pixel_rays's record
    hiprz_gather_sample g;
    g.id = HIPRZ_GATHER_INVALID_RAY, g.bx = g.by = 0.0f, g.t = r1.w;
    hit.instance = -1, hit.triangle = 0u, hit.bx = hit.by = 0.0f, hit.external = true;
    if (!take_ray(r0, r1, 0u, ray)) return g;
    g.id = HIPRZ_GATHER_MISS;
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

// one tap of the source: true and w * rgb added when (x, y) lies in the atlas and its texel has a value
RZ_DEV bool view_tap(const float4* __restrict__ source, uint32_t W, uint32_t H, int x, int y, float w, v3& acc, float& sw) {
    if (x < 0 || y < 0 || x >= int(W) || y >= int(H)) return false;
    const float4 texel = source[size_t(uint32_t(y)) * W + uint32_t(x)];
    if (__float_as_uint(texel.w) == HIPRZ_GATHER_INVALID) return false;
    acc.x = acc.x + (w * texel.x);
    acc.y = acc.y + (w * texel.y);
    acc.z = acc.z + (w * texel.z);
    sw = sw + w;
    return true;
}

// include/hiprz_view.h "A FRONT-FACE HIT ON A MAPPED ID": the taps used (0: kind NONE) and the RGB
RZ_DEV uint32_t view_atlas(const ViewMap& map, const hiprz_gather_sample& g, const float4* __restrict__ source, uint32_t W, uint32_t H, uint32_t filter, v3& rgb) {
    const float4 c0 = map.uv[2 * size_t(g.id)], c1 = map.uv[2 * size_t(g.id) + 1];
    const float b1 = (1.0f - g.bx) - g.by;
    const float u = (c0.x * b1 + c0.z * g.bx) + c1.x * g.by;
    const float v = (c0.y * b1 + c0.w * g.bx) + c1.y * g.by;
    if (!isfinite(u) || !isfinite(v)) return 0u;
    if (filter == HIPRZ_VIEW_NEAREST) {
        float fx = floorf(u * float(W)), fy = floorf(v * float(H));  // (finite or an infinity, never NaN: the clamps below are total)
        fx = fx < 0.0f ? 0.0f : (fx > float(W - 1u) ? float(W - 1u) : fx);
        fy = fy < 0.0f ? 0.0f : (fy > float(H - 1u) ? float(H - 1u) : fy);
        const float4 texel = source[size_t(uint32_t(fy)) * W + uint32_t(fx)];
        if (__float_as_uint(texel.w) == HIPRZ_GATHER_INVALID) return 0u;
        rgb = xyz(texel);
        return 1u;
    }
    const float gx = u * float(W) - 0.5f, gy = v * float(H) - 0.5f;
    const float flx = floorf(gx), fly = floorf(gy);
    const float fx = gx - flx, fy = gy - fly;
    const int x0 = int(flx < -1.0f ? -1.0f : (flx > float(W) ? float(W) : flx));  // (an infinity clamps like any other; never NaN)
    const int y0 = int(fly < -1.0f ? -1.0f : (fly > float(H) ? float(H) : fly));
    const float wx0 = 1.0f - fx, wy0 = 1.0f - fy;
    v3 acc = V3(0.0f, 0.0f, 0.0f);
    float sw = 0.0f;
    uint32_t used = 0u;
    used += view_tap(source, W, H, x0, y0, wx0 * wy0, acc, sw) ? 1u : 0u;
    used += view_tap(source, W, H, x0 + 1, y0, fx * wy0, acc, sw) ? 1u : 0u;
    used += view_tap(source, W, H, x0, y0 + 1, wx0 * fy, acc, sw) ? 1u : 0u;
    used += view_tap(source, W, H, x0 + 1, y0 + 1, fx * fy, acc, sw) ? 1u : 0u;
    if (!(sw > 0.0f)) return 0u;
    rgb = V3(acc.x / sw, acc.y / sw, acc.z / sw);
    return used;
}

// include/hiprz_probe.h "THE EVALUATION" of the record at `sh` for the normal n
RZ_DEV v3 view_irradiance(const float4* __restrict__ sh, const v3 n) {
    const float B[9] = {1.0f, n.y, n.z, n.x, n.x * n.y, n.y * n.z, (3.0f * (n.z * n.z)) - 1.0f, n.x * n.z, (n.x * n.x) - (n.y * n.y)};
    const float W[9] = {1.0f, 2.0f, 2.0f, 2.0f, 3.75f, 3.75f, 0.3125f, 3.75f, 0.9375f};
    v3 e = V3(0.0f, 0.0f, 0.0f);
#pragma unroll
    for (int b = 0; b < 9; ++b) {
        const float4 m = sh[b];
        e.x = e.x + ((W[b] * m.x) * B[b]);
        e.y = e.y + ((W[b] * m.y) * B[b]);
        e.z = e.z + ((W[b] * m.z) * B[b]);
    }
    return e;
}

// include/hiprz_field.h "THE CORNERS", the factor a visibility record gives the probe at P for the point p with normal n
RZ_DEV float view_visible(const float4* __restrict__ vis, const v3 P, const v3 p, const v3 n, float bias) {
    const v3 v = V3((p.x + (bias * n.x)) - P.x, (p.y + (bias * n.y)) - P.y, (p.z + (bias * n.z)) - P.z);
    const float dist = sqrtf((v.x * v.x + v.y * v.y) + v.z * v.z);
    float wb = 1.0f, ch = 1.0f;
    if (dist != 0.0f) {
        const v3 u = V3(P.x - p.x, P.y - p.y, P.z - p.z);
        const float len = sqrtf((u.x * u.x + u.y * u.y) + u.z * u.z);
        if (len != 0.0f) {
            const float b = ((((u.x / len) * n.x + (u.y / len) * n.y) + (u.z / len) * n.z) + 1.0f) * 0.5f;
            wb = (b * b) + 0.2f;
        }
        const float x = v.x / dist, y = v.y / dist, z = v.z / dist;
        const float sum = (fabsf(x) + fabsf(y)) + fabsf(z);
        const float ex = x / sum, ey = y / sum;
        float fx = ex, fy = ey;
        if (z < 0.0f) {
            fx = (1.0f - fabsf(ey)) * copysignf(1.0f, ex);
            fy = (1.0f - fabsf(ex)) * copysignf(1.0f, ey);
        }
        const uint32_t tx = uint32_t(fminf(fmaxf(floorf((fx * 0.5f + 0.5f) * 8.0f), 0.0f), 7.0f));  // (fmaxf(NaN, 0) is 0: the clamp is total)
        const uint32_t ty = uint32_t(fminf(fmaxf(floorf((fy * 0.5f + 0.5f) * 8.0f), 0.0f), 7.0f));
        const uint32_t j = 8u * ty + tx;
        const float4 pair = vis[j >> 1];  // two texels per float4
        const float mean = (j & 1u) ? pair.z : pair.x, mean2 = (j & 1u) ? pair.w : pair.y;
        if (dist > mean) {
            const float var = fabsf(mean2 - mean * mean);
            const float dd = dist - mean;
            ch = var / (var + dd * dd);
            ch = (ch * ch) * ch;
        }
    }
    float w = fmaxf(wb * ch, 1.0e-6f);
    if (w < 0.2f) w = w * ((w * w) * 25.0f);
    return w;
}

// include/hiprz_field.h §2 "THE LOOKUP" for the point (p, n): the probes counted (0: the lookup is invalid or counts none) and E
RZ_DEV uint32_t view_field_lookup(const ViewField& a, const v3 p, const v3 n, v3& E) {
    const float sq = (n.x * n.x + n.y * n.y) + n.z * n.z;
    const bool valid = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(n.x) && isfinite(n.y) && isfinite(n.z) && sq >= 0.99f && sq <= 1.01f;
    if (!valid) return 0u;
    const float pos[3] = {p.x, p.y, p.z};
    uint32_t cell[3];
    float frac[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const uint32_t count = a.grid.n[c];
        float g = 0.0f;
        if (count > 1u) g = (pos[c] - a.grid.lo[c]) / a.grid.step[c];
        g = fminf(fmaxf(g, 0.0f), float(count - 1u));
        const uint32_t fl = uint32_t(floorf(g));
        cell[c] = count > 1u ? (fl < count - 2u ? fl : count - 2u) : 0u;
        frac[c] = g - float(cell[c]);
    }
    v3 acc = V3(0.0f, 0.0f, 0.0f);
    float sw = 0.0f;
    uint32_t counted = 0u;
    for (uint32_t corner = 0u; corner < 8u; ++corner) {
        uint32_t at[3];
        float wa[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const uint32_t up = (corner >> c) & 1u;
            const uint32_t k = cell[c] + up;
            at[c] = k < a.grid.n[c] - 1u ? k : a.grid.n[c] - 1u;
            wa[c] = up ? frac[c] : 1.0f - frac[c];
        }
        const float tri = (wa[0] * wa[1]) * wa[2];
        const size_t index = (size_t(at[0]) * a.grid.n[1] + at[1]) * a.grid.n[2] + at[2];  // < the probe count, which the host held to the grid
        const float4* record = a.sh + 9u * index;
        bool left_out = __float_as_uint(record[0].w) == HIPRZ_PROBE_INVALID;
        float w = tri;
        if (a.vis && !left_out) {
            const float4* map = a.vis + 33u * index;
            const float4 words = map[32];
            left_out = __float_as_uint(words.w) == HIPRZ_FIELD_INVALID || __float_as_uint(words.y) > a.max_back;
            if (!left_out) w = view_visible(map, xyz(a.probes[2u * index]), p, n, a.bias) * tri;
        }
        if (left_out) continue;
        const v3 e = view_irradiance(record, n);
        acc.x = acc.x + (w * e.x);
        acc.y = acc.y + (w * e.y);
        acc.z = acc.z + (w * e.z);
        sw = sw + w;
        if (w > 0.0f) ++counted;
    }
    if (!(sw > 0.0f)) return 0u;
    E = V3(acc.x / sw, acc.y / sw, acc.z / sw);
    return counted;
}

// include/hiprz_view.h "A FRONT-FACE HIT ON AN UNMAPPED INSTANCE OR ID": the probes counted (0: kind NONE) and the RGB.  The surface is
// analyze_intersection's; the colour and the emission are the reference rule of the renderer's fetch_color_emission, restated (including
// hiprz_kernels.hpp would add the renderer's kernels to this library).
RZ_DEV uint32_t view_field(const DScene& s, const ViewField& field, const Ray& ray, const Hit& hit, v3& rgb) {
    Counters cnt;
    Surface sf;
    sf.u = sf.v = 0.0f;
    Material m;
    analyze_intersection<false, true>(s, hit, sf, m, cnt, false);
    const v3 p = V3(ray.o.x + (ray.far_ * ray.d.x), ray.o.y + (ray.far_ * ray.d.y), ray.o.z + (ray.far_ * ray.d.z));
    v3 E = V3(0.0f, 0.0f, 0.0f);
    const uint32_t counted = view_field_lookup(field, p, sf.mapped_normal, E);
    if (counted == 0u) return 0u;
    col4 color = from_u8(m.color);
    if (m.texture >= 0) color = fetch_rgba8<false>(s, m.texture, sf.u, sf.v, cnt);
    const float emission = m.emission_map >= 0 ? fetch_r32f<false>(s, m.emission_map, sf.u, sf.v, cnt) : m.emission;
    rgb = V3(color.r * E.x, color.g * E.y, color.b * E.z);
    if (emission > 0.0f) rgb = V3(rgb.x + (color.r * emission), rgb.y + (color.g * emission), rgb.z + (color.b * emission));
    return counted;
}

// One thread per pixel.  The walk's state is dead once view_walk has returned its sample: the atlas taps and the field's lookup run in the
// registers the walk has given back.  RZ_VIEW_WAVES: the waves per SIMD the kernel is held to (make VIEW_DEFS=-DRZ_VIEW_WAVES=..).
#ifndef RZ_VIEW_WAVES
#define RZ_VIEW_WAVES 5
#endif
__global__ void __launch_bounds__(RZ_VIEW_WG, RZ_VIEW_WAVES) rz_view_kernel(const DScene s, const DCamera cam, const ViewMap map, const ViewField field,
                                                                           const float4* __restrict__ source, uint32_t W, uint32_t H, uint32_t filter, const float4 sky,
                                                                           float4* __restrict__ pixels, float4* __restrict__ image) {
    uint32_t x, y;
    if (!view_pixel_of(cam.width, cam.height, x, y)) return;
    Ray ray;
    Hit hit;
    const hiprz_gather_sample g = view_walk(s, cam, map, x, y, ray, hit);
    v3 rgb = V3(0.0f, 0.0f, 0.0f);
    uint32_t kind = HIPRZ_VIEW_NONE, count = 0u;
    if (g.id == HIPRZ_GATHER_MISS || g.id == HIPRZ_GATHER_INVALID_RAY) {
        kind = HIPRZ_VIEW_SKY, rgb = V3(sky.x, sky.y, sky.z);
    } else if (g.id == HIPRZ_GATHER_BACK) {
        kind = HIPRZ_VIEW_BACK;
    } else if (g.id == HIPRZ_GATHER_UNMAPPED) {
        if (field.probes) count = view_field(s, field, ray, hit, rgb);
        if (count) kind = HIPRZ_VIEW_FIELD;
    } else {
        count = view_atlas(map, g, source, W, H, filter, rgb);
        if (count) kind = HIPRZ_VIEW_ATLAS;
    }
    if (kind == HIPRZ_VIEW_NONE) rgb = V3(0.0f, 0.0f, 0.0f);
    const size_t i = size_t(y) * cam.width + x;
    if (pixels) pixels[i] = make_float4(rgb.x, rgb.y, rgb.z, __uint_as_float((kind << HIPRZ_VIEW_KIND_SHIFT) | count));
    if (image) image[i] = make_float4(rgb.x, rgb.y, rgb.z, 1.0f);
}

// one thread per pixel: the record view_walk makes for it
__global__ void __launch_bounds__(RZ_VIEW_WG) rz_view_samples_kernel(const DScene s, const DCamera cam, const ViewMap map, float4* __restrict__ samples) {
    uint32_t x, y;
    if (!view_pixel_of(cam.width, cam.height, x, y)) return;
    Ray ray;
    Hit hit;
    const hiprz_gather_sample g = view_walk(s, cam, map, x, y, ray, hit);
    samples[size_t(y) * cam.width + x] = make_float4(__uint_as_float(g.id), g.bx, g.by, g.t);
}

}  // namespace hiprz

using namespace hiprz;

static_assert(sizeof(hiprz_view_pixel) == 16 && sizeof(hiprz_gather_sample) == 16 && sizeof(hiprz_gather_chart) == 32 && sizeof(hiprz_bake_point) == 32 &&
                  sizeof(hiprz_probe_sh) == 144 && sizeof(hiprz_field_vis) == 528 && offsetof(hiprz_field_vis, words) == 512,
              "one 16-byte store per pixel and sample, two 16-byte loads per chart and probe, nine per record, 33 per visibility record");

struct hiprz_view : Session {
    std::vector<uint32_t> base;  // the chart map as set
    std::vector<hiprz_gather_chart> uv;
    bool has_charts = false, charts_stale = false;
    uint32_t* base_dev = nullptr;  // its device copy, made by the first call after set_charts
    float4* uv_dev = nullptr;
    float4* source_dev = nullptr;  // the device copy of a host source, source_capacity records
    size_t source_capacity = 0;
    void* held = nullptr;          // the device copy of a host field: probes, records and visibility records behind one another
    size_t held_bytes = 0;
};

namespace {

// what every call refuses before a view is asked for
int refuse(hiprz_view* h, bool any_null, uint32_t W, uint32_t H, const hiprz_view_params* params, const hiprz_view_field* field, const char* what) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null view");
    int code;
    if (const char* why = view_refusal(any_null, h->has_charts, W, H, params, field, &code)) return fail(h, code, std::string(what) + ": " + why);
    return HIPRZ_OK;
}

// the view of the call with its camera, held against the most pixels a call takes and the chart map's number of instances
int view_and_map(hiprz_view* h, const char* what, DScene& s, DCamera& cam) {
    if (const int rc = view(h, what, s, &cam); rc != HIPRZ_OK) return rc;
    if (const char* why = view_pixels_refusal(cam.width, cam.height)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
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

// the chart map a set_charts left on the host goes to the device before the call's kernel; the stream is waited for, since the host arrays
// are pageable and may be replaced
int place_charts(hiprz_view* h, hipStream_t stream, const char* what) {
    if (!h->charts_stale) return HIPRZ_OK;
    if (const hipError_t e = replace(h->base_dev, h->base.data(), h->base.size() * sizeof(uint32_t), stream); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = replace(h->uv_dev, h->uv.data(), h->uv.size() * sizeof(hiprz_gather_chart), stream); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return fail_hip(h, what, e);
    h->charts_stale = false;
    return HIPRZ_OK;
}

ViewMap map_of(const hiprz_view* h) { return ViewMap{h->base_dev, h->uv_dev, uint32_t(h->uv.size())}; }

// the field of a call with its arrays on the device; null: none
ViewField field_of(const hiprz_view_field* field, const void* probes, const void* sh, const void* vis) {
    ViewField a{};
    if (!field) return a;
    a.grid = *field->grid;
    a.probes = static_cast<const float4*>(probes), a.sh = static_cast<const float4*>(sh), a.vis = static_cast<const float4*>(vis);
    if (field->params) a.bias = field->params->bias, a.max_back = field->params->max_back;
    return a;
}

// the view of the frame on the device view the call has fetched
int launch_view(hiprz_view* h, const DScene& s, const DCamera& cam, const void* source, uint32_t W, uint32_t H, const ViewField& field, const float sky[3],
                const hiprz_view_params* params, void* pixels, void* image, hipStream_t stream, const char* what) {
    if (const int rc = place_charts(h, stream, what); rc != HIPRZ_OK) return rc;
    hipLaunchKernelGGL(rz_view_kernel, dim3(view_groups(cam.width, cam.height, RZ_VIEW_ROWS_BUILD != 0)), dim3(RZ_VIEW_WG), 0, stream, s, cam, map_of(h), field,
                       static_cast<const float4*>(source), W, H, params ? params->filter : HIPRZ_VIEW_NEAREST, make_float4(sky[0], sky[1], sky[2], 0.0f),
                       static_cast<float4*>(pixels), static_cast<float4*>(image));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

}  // namespace

extern "C" {

int hiprz_view_create(hiprz_view** out, hiprz_ctx* ctx) { return create(out, ctx, "view_create"); }

int hiprz_view_destroy(hiprz_view* h) {
    return destroy(h, h && (h->base_dev || h->uv_dev || h->source_dev || h->held), [h] {
        for (void* p : {static_cast<void*>(h->base_dev), static_cast<void*>(h->uv_dev), static_cast<void*>(h->source_dev), h->held})
            if (p) (void)hipFree(p);
    });
}

const char* hiprz_view_last_error(const hiprz_view* h) { return last_error(h); }

int hiprz_view_set_charts(hiprz_view* h, const uint32_t* base_host, uint32_t n_instances, const hiprz_gather_chart* uv_host, uint32_t n_charts) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, "view_set_charts: null view");
    if (const char* why = view_charts_refusal(base_host, n_instances, uv_host, n_charts)) return fail(h, HIPRZ_ERR_INVALID, std::string("view_set_charts: ") + why);
    // the map that is already set, byte for byte: nothing to place again (a caller that passes its map with every frame pays one comparison)
    if (h->has_charts && h->base.size() == n_instances && h->uv.size() == n_charts &&
        (n_instances == 0u || std::memcmp(h->base.data(), base_host, n_instances * sizeof(uint32_t)) == 0) &&
        (n_charts == 0u || std::memcmp(h->uv.data(), uv_host, n_charts * sizeof(hiprz_gather_chart)) == 0))
        return HIPRZ_OK;
    h->base.assign(base_host, base_host + n_instances);
    h->uv.assign(uv_host, uv_host + n_charts);
    h->has_charts = h->charts_stale = true;
    return HIPRZ_OK;
}

int hiprz_view_pixels(hiprz_view* h, const void* source16_device, uint32_t W, uint32_t H, const hiprz_view_field* field, const float sky[3],
                      const hiprz_view_params* params, hiprz_view_pixel* pixels_out_device, void* image_out_device, void* stream) {
    const char* what = "view_pixels";
    if (const int rc = refuse(h, !source16_device || !sky || (!pixels_out_device && !image_out_device), W, H, params, field, what); rc != HIPRZ_OK) return rc;
    DScene s;
    DCamera cam;
    if (const int rc = view_and_map(h, what, s, cam); rc != HIPRZ_OK) return rc;
    if (cam.width == 0u || cam.height == 0u) return HIPRZ_OK;
    return launch_view(h, s, cam, source16_device, W, H, field_of(field, field ? field->probes : nullptr, field ? field->sh : nullptr, field ? field->vis : nullptr), sky, params,
                       pixels_out_device, image_out_device, stream_of(h, stream), what);
}

int hiprz_view_samples(hiprz_view* h, hiprz_gather_sample* samples_out_device, void* stream) {
    const char* what = "view_samples";
    if (const int rc = refuse(h, !samples_out_device, 1u, 1u, nullptr, nullptr, what); rc != HIPRZ_OK) return rc;
    DScene s;
    DCamera cam;
    if (const int rc = view_and_map(h, what, s, cam); rc != HIPRZ_OK) return rc;
    if (cam.width == 0u || cam.height == 0u) return HIPRZ_OK;
    hipStream_t st = stream_of(h, stream);
    if (const int rc = place_charts(h, st, what); rc != HIPRZ_OK) return rc;
    hipLaunchKernelGGL(rz_view_samples_kernel, dim3(view_groups(cam.width, cam.height, RZ_VIEW_ROWS_BUILD != 0)), dim3(RZ_VIEW_WG), 0, st, s, cam, map_of(h),
                       reinterpret_cast<float4*>(samples_out_device));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

int hiprz_view_pixels_host(hiprz_view* h, const void* source16, uint32_t W, uint32_t H, const hiprz_view_field* field, const float sky[3], const hiprz_view_params* params,
                           hiprz_view_pixel* pixels_out, void* image_out) {
    const char* what = "view_pixels_host";
    if (const int rc = refuse(h, !source16 || !sky || (!pixels_out && !image_out), W, H, params, field, what); rc != HIPRZ_OK) return rc;
    DScene s;
    DCamera cam;
    if (const int rc = view_and_map(h, what, s, cam); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the buffers
    const size_t n = size_t(cam.width) * cam.height;
    if (n == 0u) return HIPRZ_OK;
    // the staging's two sides both carry results here: the records come back through its out side, the image through its in side
    if (const int rc = grow_staging(h, what, n, 16u, sizeof(hiprz_view_pixel), view_capacity); rc != HIPRZ_OK) return rc;
    hipStream_t st = stream_of(h, nullptr);
    const size_t texels = size_t(W) * H;
    if (texels > h->source_capacity) {
        if (h->source_dev) (void)hipFree(h->source_dev);
        h->source_dev = nullptr, h->source_capacity = 0;
        if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->source_dev), texels * 16u); e != hipSuccess) return fail_hip(h, what, e);
        h->source_capacity = texels;
    }
    if (const hipError_t e = hipMemcpyAsync(h->source_dev, source16, texels * 16u, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
    // the field: the probes, their records and their visibility records behind one another in one device buffer (each a multiple of 16 bytes)
    char* dev = nullptr;
    size_t probe_bytes = 0, sh_bytes = 0;
    if (field) {
        probe_bytes = field->n_probes * sizeof(hiprz_bake_point), sh_bytes = field->n_probes * sizeof(hiprz_probe_sh);
        const size_t vis_bytes = field->vis ? field->n_probes * sizeof(hiprz_field_vis) : 0u;
        const size_t bytes = probe_bytes + sh_bytes + vis_bytes;
        if (bytes > h->held_bytes) {
            if (h->held) (void)hipFree(h->held);  // (hipFree waits for whatever still reads the buffer)
            h->held = nullptr, h->held_bytes = 0;
            if (const hipError_t e = hipMalloc(&h->held, bytes); e != hipSuccess) return fail_hip(h, what, e);
            h->held_bytes = bytes;
        }
        dev = static_cast<char*>(h->held);
        if (const hipError_t e = hipMemcpyAsync(dev, field->probes, probe_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
        if (const hipError_t e = hipMemcpyAsync(dev + probe_bytes, field->sh, sh_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
        if (field->vis)
            if (const hipError_t e = hipMemcpyAsync(dev + probe_bytes + sh_bytes, field->vis, vis_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
    }
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(h, what, e);  // the source and the field are pageable and the caller's
    const Staging& g = h->staging;
    const ViewField on_device = field_of(field, dev, dev + probe_bytes, field && field->vis ? dev + probe_bytes + sh_bytes : nullptr);
    if (const int rc = launch_view(h, s, cam, h->source_dev, W, H, on_device, sky, params, pixels_out ? g.dev_out : nullptr, image_out ? g.dev_in : nullptr, st, what); rc != HIPRZ_OK)
        return rc;
    if (pixels_out)
        if (const hipError_t e = hipMemcpyAsync(g.pinned_out, g.dev_out, n * sizeof(hiprz_view_pixel), hipMemcpyDeviceToHost, st); e != hipSuccess) return fail_hip(h, what, e);
    if (image_out)
        if (const hipError_t e = hipMemcpyAsync(g.pinned_in, g.dev_in, n * 16u, hipMemcpyDeviceToHost, st); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(h, what, e);
    if (pixels_out) std::memcpy(pixels_out, g.pinned_out, n * sizeof(hiprz_view_pixel));
    if (image_out) std::memcpy(image_out, g.pinned_in, n * 16u);
    return HIPRZ_OK;
}

}  // extern "C"
