// hiprz_probe.hip — probe baking (include/hiprz_probe.h): the K rays of a probe are made from a table of directions over the whole sphere,
// walked to their closest hits by the query's closest-hit walk, looked up in an atlas that holds light through the caller's chart map and
// projected onto nine spherical-harmonic basis functions per colour, summed across the wave in a fixed order, 144 bytes out per probe; a
// second kernel adds the scene's own lights with their shadows.  A library of its own (libhiprz_probe.so) beside the eight whose kernels
// and ABI are pinned; the ray rule and the walks are the query's device functions (query/hiprz_query_device.hpp, no __global__), so a
// ray's t, instance, triangle and verdict are hiprz_query_closest's and hiprz_query_occluded's.  The frame and the ray of hiprz_bake.h,
// the walk and the lookup of hiprz_gather.h and the sampling of hiprz_light.h are restated here.  The context is read through
// hiprz_device_view on every call.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hiprz_probe.h"
#include "hiprz_probe_host.hpp"
#include "query/hiprz_query_device.hpp"
#include "query/hiprz_session.hpp"  // the handle, its errors, the view, the staging and its round trip

// threads per workgroup: one wave — the ballots and the butterfly span exactly the workgroup
#define RZ_PROBE_WG 64
// the running sums of a lane: 9 coefficients x 3 colours
#define RZ_PROBE_SUMS 27

// Where a lane's 27 running sums live, per kernel: 1 = LDS, acc[b * 3 + c][lane], a column per lane (no barrier: no lane reads another's),
// 0 = registers; and the waves per SIMD the kernel is bounded for.  The arithmetic and every output byte are the same.  Shipped is what
// was faster on the MI355X (DESIGN.md §6 "Probe baking" has the resource usage and the timings of all four): the gather keeps its sums in
// LDS at five waves, the light term in registers at four.
// make PROBE_DEFS="-DRZ_PROBE_GATHER_IN_LDS=0 -DRZ_PROBE_GATHER_WAVES=4 -DRZ_PROBE_LIGHT_IN_LDS=1 -DRZ_PROBE_LIGHT_WAVES=5" builds the other two.
#ifndef RZ_PROBE_GATHER_IN_LDS
#define RZ_PROBE_GATHER_IN_LDS 1
#endif
#ifndef RZ_PROBE_GATHER_WAVES
#define RZ_PROBE_GATHER_WAVES 5
#endif
#ifndef RZ_PROBE_LIGHT_IN_LDS
#define RZ_PROBE_LIGHT_IN_LDS 0
#endif
#ifndef RZ_PROBE_LIGHT_WAVES
#define RZ_PROBE_LIGHT_WAVES 4
#endif

namespace hiprz {

// what a probe gives every one of its rays: the two words of the probe, whether it is valid, its set and its frame
struct ProbePoint {
    float4 p0, p1;  // position, near_ | normal as given, far_
    v3 n, t, bt;    // include/hiprz_probe.h "THE FRAME" of the normalised normal (read on a valid probe only)
    uint32_t set;
    bool valid;
};

RZ_DEV ProbePoint probe_point(const float4* __restrict__ probes, uint32_t i, uint32_t seed, uint32_t S) {
    ProbePoint p;
    p.p0 = probes[2 * size_t(i)], p.p1 = probes[2 * size_t(i) + 1];
    Ray along;
    p.valid = take_ray(p.p0, p.p1, HIPRZ_QUERY_NORMALIZE, along);  // valid: along.d = normalized(normal)
    p.set = probe_hash(i ^ seed) % S;
    const v3 n = along.d;
    const float s = copysignf(1.0f, n.z);
    const float a = -1.0f / (s + n.z);
    const float b = (n.x * n.y) * a;
    p.n = n;
    p.t = V3(1.0f + ((s * n.x) * n.x) * a, s * b, (-s) * n.x);
    p.bt = V3(b, s + (n.y * n.y) * a, -n.y);
    return p;
}

// the ray of (probe, direction k) as the two float4 of a hiprz_ray.  An invalid probe: direction +0, which the ray rule refuses.
RZ_DEV void probe_ray(const ProbePoint& p, const float4* __restrict__ dirs, uint32_t K, uint32_t k, float4& r0, float4& r1) {
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
struct ProbeMap {
    const uint32_t* base;
    const float4* uv;  // (u1, v1, u2, v2) (u3, v3, 0, 0)
    uint32_t n_charts;
};

// include/hiprz_probe.h "THE SAMPLES": the walk of one ray and the chart under its hit, hiprz_gather.h's restated.  No material, texture or
// normal is fetched, only the hit triangle's second word for its source index.
RZ_DEV hiprz_gather_sample probe_walk(const DScene& s, const ProbeMap& map, const float4 r0, const float4 r1) {
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

// include/hiprz_probe.h "THE LOOKUP": true and the texel's RGB when the sample lies on a chart and its texel has a value
RZ_DEV bool probe_lookup(const ProbeMap& map, const hiprz_gather_sample& g, const float4* __restrict__ source, uint32_t W, uint32_t H, v3& rgb) {
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
    if (__float_as_uint(texel.w) == HIPRZ_PROBE_INVALID) return false;
    rgb = xyz(texel);
    return true;
}

// A lane's running sums.  In LDS: column threadIdx.x of the workgroup's array, stride 64 floats, volatile — every step reads and writes
// its column where it stands; without it the compiler finds that no lane reads another's column, turns the array into 27 registers per
// lane and the build into the other one.  In registers: an array of the lane's own, stride 1.
template <bool IN_LDS>
struct ProbeSums;
template <>
struct ProbeSums<true> {
    volatile float* at;
    RZ_DEV explicit ProbeSums(volatile float* columns) : at(columns + threadIdx.x) {}
    RZ_DEV volatile float& operator[](int i) const { return at[i * RZ_PROBE_WG]; }
};
template <>
struct ProbeSums<false> {
    float v[RZ_PROBE_SUMS];
    RZ_DEV explicit ProbeSums(volatile float*) {}
    RZ_DEV float& operator[](int i) { return v[i]; }
    RZ_DEV const float& operator[](int i) const { return v[i]; }
};
#define RZ_PROBE_DECLARE_SUMS(name, in_lds)                                             \
    __shared__ volatile float name##_columns[(in_lds) ? RZ_PROBE_SUMS * RZ_PROBE_WG : 1]; \
    ProbeSums<(in_lds) != 0> name(name##_columns)

// include/hiprz_probe.h "THE BASIS" on d, and one step of a lane's 27 running sums: acc[b].c = acc[b].c + (L.c * B_b)
template <typename Sums>
RZ_DEV void probe_add(Sums& acc, const v3 L, const v3 d) {
    const float B[9] = {1.0f, d.y, d.z, d.x, d.x * d.y, d.y * d.z, (3.0f * (d.z * d.z)) - 1.0f, d.x * d.z, (d.x * d.x) - (d.y * d.y)};
#pragma unroll
    for (int b = 0; b < 9; ++b) {
        acc[3 * b] = acc[3 * b] + (L.x * B[b]);
        acc[3 * b + 1] = acc[3 * b + 1] + (L.y * B[b]);
        acc[3 * b + 2] = acc[3 * b + 2] + (L.z * B[b]);
    }
}

template <typename Sums>
RZ_DEV void probe_clear(Sums& acc) {
#pragma unroll
    for (int i = 0; i < RZ_PROBE_SUMS; ++i) acc[i] = 0.0f;
}

// coefficient b of a lane's sums after the butterfly over the `seg` lanes of its probe, times rcp: every lane calls it
template <typename Sums>
RZ_DEV v3 probe_mean(const Sums& acc, int b, uint32_t seg, float rcp) {
    v3 v = V3(acc[3 * b], acc[3 * b + 1], acc[3 * b + 2]);
    for (uint32_t off = 1u; off < seg; off <<= 1) {
        v.x = v.x + __shfl_xor(v.x, int(off));
        v.y = v.y + __shfl_xor(v.y, int(off));
        v.z = v.z + __shfl_xor(v.z, int(off));
    }
    return V3(v.x * rcp, v.y * rcp, v.z * rcp);
}

RZ_DEV void probe_store_invalid(float4* __restrict__ record) {
    record[0] = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(HIPRZ_PROBE_INVALID));
#pragma unroll
    for (int b = 1; b < 9; ++b) record[b] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

// One wave per workgroup.  K >= 64: the wave gathers probe blockIdx.x in K / 64 rounds, lane l walks rays l, 64 + l, ...  K < 64: it gathers
// the 64 / K probes from blockIdx.x * (64 / K) on, lane l walks ray l % K of probe l / K.  A lane whose probe is >= n or invalid walks
// nothing and contributes +0, but takes part in every ballot and shuffle: nothing returns before them.
__global__ void __launch_bounds__(RZ_PROBE_WG, RZ_PROBE_GATHER_WAVES) rz_probe_gather_kernel(const DScene s, const float4* __restrict__ probes, uint32_t n,
                                                                                    const float4* __restrict__ dirs, uint32_t K, uint32_t S, uint32_t seed,
                                                                                    const ProbeMap map, const float4* __restrict__ source, uint32_t W, uint32_t H,
                                                                                    const float4 sky, float4* __restrict__ out) {
    RZ_PROBE_DECLARE_SUMS(acc, RZ_PROBE_GATHER_IN_LDS);
    const uint32_t lane = threadIdx.x;
    const uint32_t seg = K < 64u ? K : 64u;      // lanes per probe, a power of two
    const uint32_t first = lane & ~(seg - 1u);  // the first lane of this lane's probe
    const uint32_t probe = blockIdx.x * (64u / seg) + lane / seg;
    const bool inside = probe < n;
    ProbePoint p;
    p.valid = false;
    if (inside) p = probe_point(probes, probe, seed, S);
    const bool walks = inside && p.valid;
    const unsigned long long segment = (seg == 64u ? ~0ull : (1ull << seg) - 1ull) << first;
    uint32_t n_read = 0u, n_missed = 0u;
    probe_clear(acc);
    const uint32_t rounds = K < 64u ? 1u : K / 64u;  // of a kernel argument alone: the same trip count on every lane
    for (uint32_t r = 0u; r < rounds; ++r) {
        const uint32_t k = 64u * r + (lane - first);
        bool read = false, missed = false;
        v3 c = V3(0.0f, 0.0f, 0.0f), d = V3(0.0f, 0.0f, 0.0f);
        if (walks) {
            float4 r0, r1;
            probe_ray(p, dirs, K, k, r0, r1);
            d = xyz(r1);
            const hiprz_gather_sample g = probe_walk(s, map, r0, r1);
            missed = g.id == HIPRZ_GATHER_MISS || g.id == HIPRZ_GATHER_INVALID_RAY;
            if (missed) c = V3(sky.x, sky.y, sky.z);
            else read = probe_lookup(map, g, source, W, H, c);
        }
        n_read += uint32_t(__popcll(__ballot(read) & segment));
        n_missed += uint32_t(__popcll(__ballot(missed) & segment));
        probe_add(acc, c, d);
    }
    const float rcp = 1.0f / float(K);
    const bool writes = inside && lane == first;
    float4* record = out + 9 * size_t(writes ? probe : 0u);
    if (writes && !p.valid) probe_store_invalid(record);
#pragma unroll
    for (int b = 0; b < 9; ++b) {
        const v3 m = probe_mean(acc, b, seg, rcp);
        if (writes && p.valid) record[b] = make_float4(m.x, m.y, m.z, b == 0 ? __uint_as_float(n_read | (n_missed << 16)) : 0.0f);
    }
}

// thread i: sample i = (probe i / K, direction i % K), the record the gather makes for that pair
__global__ void __launch_bounds__(RZ_PROBE_WG) rz_probe_samples_kernel(const DScene s, const float4* __restrict__ probes, uint32_t n_rays,
                                                                     const float4* __restrict__ dirs, uint32_t K, uint32_t S, uint32_t seed, const ProbeMap map,
                                                                     float4* __restrict__ samples) {
    const uint32_t i = blockIdx.x * RZ_PROBE_WG + threadIdx.x;
    if (i >= n_rays) return;
    const ProbePoint p = probe_point(probes, i / K, seed, S);
    float4 r0, r1;
    probe_ray(p, dirs, K, i % K, r0, r1);
    const hiprz_gather_sample g = probe_walk(s, map, r0, r1);
    samples[i] = make_float4(__uint_as_float(g.id), g.bx, g.by, g.t);
}

// include/hiprz_light.h "THE FRAME", restated
RZ_DEV void probe_light_frame(const v3 a, v3& t, v3& bt) {
    const float s = copysignf(1.0f, a.z);
    const float e = -1.0f / (s + a.z);
    const float b = (a.x * a.y) * e;
    t = V3(1.0f + ((s * a.x) * a.x) * e, s * b, (-s) * a.x);
    bt = V3(b, s + (a.y * a.y) * e, -a.y);
}

RZ_DEV bool probe_all_finite(const v3 a, float b, float c) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z) && isfinite(b) && isfinite(c); }

// The sample (x, y) of light l of the span (spot lights first) seen from the probe, include/hiprz_probe.h "THE LIGHT TERM": its weight w
// without a cosine, +0 for a skipped sample, the shadow ray as the two float4 of a hiprz_ray (direction +0 when skipped or the probe
// invalid) and the light's colour * emission.  l comes from a loop counter, so the record is loaded once per wave.
RZ_DEV float probe_light_sample(const DScene& s, const ProbeSpan span, uint32_t l, const float4 p0, const float4 p1, bool valid, const float2 xy, float4& r0, float4& r1,
                                v3& ce) {
    const bool spot = l < span.spots;
    const v3 position = xyz(p0);
    float w = 0.0f, far_ = p1.w, emission;
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
        probe_light_frame(a, t, bt);
        const v3 q = V3(lpos.x + ((t.x * xy.x + bt.x * xy.y) * size), lpos.y + ((t.y * xy.x + bt.y * xy.y) * size), lpos.z + ((t.z * xy.x + bt.z * xy.y) * size));
        const v3 vPL = q - position;
        const float dPL = magnitude(vPL);
        w3 = normalized(vPL);
        const float A = (size * size) * RZ_PI_F;
        const float d1 = dPL + 1.0f;
        const bool inside = cos_angle < similarity(-vPL, ldir);
        if (inside) w = A / (d1 * d1);
        far_ = dPL;
    } else {
        const uint32_t li = span.direct_first + (l - span.spots);
        const float4 l0 = s.direct_lights[2 * li], l1 = s.direct_lights[2 * li + 1];
        const float ca = l1.z;
        emission = l0.w, rgba = __float_as_uint(l1.x);
        const v3 a = -xyz(l0);
        v3 t, bt;
        probe_light_frame(a, t, bt);
        const float r2 = xy.x * xy.x + xy.y * xy.y;
        const float z = 1.0f - r2 * (1.0f - ca);
        const float h = sqrtf(fmaxf(0.0f, 1.0f - z * z));
        const float g = r2 > 0.0f ? h / sqrtf(r2) : 0.0f;
        const float xg = xy.x * g, yg = xy.y * g;
        const v3 d = V3((t.x * xg + bt.x * yg) + a.x * z, (t.y * xg + bt.y * yg) + a.y * z, (t.z * xg + bt.z * yg) + a.z * z);
        w3 = normalized(d);
        w = (2.0f * RZ_PI_F) * (1.0f - ca);
    }
    const col4 colour = from_u8(rgba);
    ce = V3(colour.r * emission, colour.g * emission, colour.b * emission);
    const bool kept = valid && w > 0.0f && emission > 0.0f && probe_all_finite(w3, far_, w);
    if (!kept) w = 0.0f, w3 = V3(0.0f, 0.0f, 0.0f), far_ = p1.w;
    r0 = p0;
    r1 = make_float4(w3.x, w3.y, w3.z, far_);
    return w;
}

// One wave per workgroup, the shape of the gather kernel above over the K samples of the light's table, per light of the span.  A lane
// whose probe is >= n or invalid, or whose sample is skipped, walks nothing and adds +0, but takes part in every ballot and shuffle.
// `base` may be null and `out` may be `base`: the lane that writes a record reads the base's words before it writes them.
__global__ void __launch_bounds__(RZ_PROBE_WG, RZ_PROBE_LIGHT_WAVES) rz_probe_light_kernel(const DScene s, const float4* __restrict__ probes, uint32_t n,
                                                                                   const float2* __restrict__ samples, uint32_t K, uint32_t S, uint32_t seed,
                                                                                   const ProbeSpan span, const float4* base, float4* out) {
    RZ_PROBE_DECLARE_SUMS(acc, RZ_PROBE_LIGHT_IN_LDS);
    const uint32_t lane = threadIdx.x;
    const uint32_t seg = K < 64u ? K : 64u;      // lanes per probe, a power of two
    const uint32_t first = lane & ~(seg - 1u);  // the first lane of this lane's probe
    const uint32_t probe = blockIdx.x * (64u / seg) + lane / seg;
    const bool inside = probe < n;
    float4 p0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), p1 = p0;
    bool valid = false;
    uint32_t set = 0u;
    if (inside) {
        p0 = probes[2 * size_t(probe)], p1 = probes[2 * size_t(probe) + 1];
        Ray along;
        valid = take_ray(p0, p1, HIPRZ_QUERY_NORMALIZE, along);
        set = probe_hash(probe ^ seed) % S;
    }
    const unsigned long long segment = (seg == 64u ? ~0ull : (1ull << seg) - 1ull) << first;
    uint32_t count = 0u;
    probe_clear(acc);
    const uint32_t lights = span.spots + span.directs;  // of kernel arguments alone: the same trip counts on every lane
    const uint32_t rounds = K < 64u ? 1u : K / 64u;
    for (uint32_t l = 0u; l < lights; ++l) {
        for (uint32_t r = 0u; r < rounds; ++r) {
            const uint32_t k = 64u * r + (lane - first);
            const float2 xy = samples[size_t(set) * K + k];  // (set 0 on a lane without a probe: inside the table)
            float4 r0, r1;
            v3 ce;
            const float w = probe_light_sample(s, span, l, p0, p1, valid, xy, r0, r1, ce);
            uint32_t occluded = 0u;
            if (w > 0.0f) occluded = occluded_word(s, r0, r1, 0u);
            count += uint32_t(__popcll(__ballot(occluded != 0u) & segment));
            const bool adds = w > 0.0f && !occluded;
            const v3 P = adds ? V3((ce.x * w) * 0.25f, (ce.y * w) * 0.25f, (ce.z * w) * 0.25f) : V3(0.0f, 0.0f, 0.0f);
            probe_add(acc, P, xyz(r1));
        }
    }
    const float rcp = 1.0f / float(K);
    const bool writes = inside && lane == first;
    const float4* below = base ? base + 9 * size_t(writes ? probe : 0u) : nullptr;
    float4* record = out + 9 * size_t(writes ? probe : 0u);
    uint32_t word = 0u;
    if (writes && below) word = __float_as_uint(below[0].w);
    const bool whole = valid && word != HIPRZ_PROBE_INVALID;
    if (writes && !whole) probe_store_invalid(record);
#pragma unroll
    for (int b = 0; b < 9; ++b) {
        const v3 m = probe_mean(acc, b, seg, rcp);
        if (writes && whole) {
            const float4 under = below ? below[b] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            record[b] = make_float4(under.x + m.x, under.y + m.y, under.z + m.z, b == 0 ? __uint_as_float(word) : (b == 1 ? __uint_as_float(count) : 0.0f));
        }
    }
}

}  // namespace hiprz

using namespace hiprz;

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_probe_sh) == 144 && sizeof(hiprz_gather_sample) == 16 && sizeof(hiprz_gather_chart) == 32,
              "two 16-byte loads per probe and chart, nine 16-byte stores per record, one per sample");
static_assert(sizeof(ProbeSpan) == sizeof(hiprz_light_range), "four words either way");

struct hiprz_probe : Session {
    std::vector<float> table;  // the directions as set, S*K float4 with w = 0; K == 0: none yet
    uint32_t K = 0, S = 0;
    float4* dirs = nullptr;    // the device copy, made by the first call after set_directions (`stale`)
    bool stale = false;
    std::vector<float> disk;   // the light's samples as set, LS*LK float2; LK == 0: none yet
    uint32_t LK = 0, LS = 0;
    float2* disk_dev = nullptr;
    bool disk_stale = false;
    std::vector<uint32_t> base;            // the chart map as set
    std::vector<hiprz_gather_chart> uv;
    bool has_charts = false, charts_stale = false;
    uint32_t* base_dev = nullptr;          // its device copy, made by the first call after set_charts
    float4* uv_dev = nullptr;
    float4* source_dev = nullptr;          // the device copy of a host source, source_capacity records
    size_t source_capacity = 0;
};

namespace {
// what a gather or samples call refuses before a view is asked for; *empty: nothing to do (n == 0 is HIPRZ_OK without a view or a launch)
int refuse_gather(hiprz_probe* h, bool any_null, size_t n, const char* what, bool* empty) {
    *empty = false;
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null probe");
    int code;
    if (const char* why = probe_gather_refusal(any_null, n, h->K, h->has_charts, &code)) return fail(h, code, std::string(what) + ": " + why);
    *empty = n == 0u;
    return HIPRZ_OK;
}

int refuse_light(hiprz_probe* h, bool any_null, size_t n, const char* what, bool* empty) {
    *empty = false;
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null probe");
    int code;
    if (const char* why = probe_light_refusal(any_null, n, h->LK, &code)) return fail(h, code, std::string(what) + ": " + why);
    *empty = n == 0u;
    return HIPRZ_OK;
}

// the view of the call, held against the chart map's number of instances
int view_and_map(hiprz_probe* h, const char* what, DScene& s) {
    if (const int rc = view(h, what, s); rc != HIPRZ_OK) return rc;
    if (s.n_instances != h->base.size()) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": the chart map is for another number of instances than the scene has");
    return HIPRZ_OK;
}

// the view of the call and the lights of it that `range` selects
int view_and_span(hiprz_probe* h, const hiprz_light_range* range, const char* what, DScene& s, ProbeSpan& span) {
    if (const int rc = view(h, what, s); rc != HIPRZ_OK) return rc;
    if (const char* why = probe_range_refusal(range, s.n_spot_lights, s.n_direct_lights, &span)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
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

// the directions and the chart map a set_* left on the host go to the device before the call's kernel; the stream is waited for, since the
// host arrays are pageable and may be replaced
int place_tables(hiprz_probe* h, hipStream_t stream, const char* what) {
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

// the same for the light term's samples
int place_disk(hiprz_probe* h, hipStream_t stream, const char* what) {
    if (!h->disk_stale) return HIPRZ_OK;
    if (const hipError_t e = replace(h->disk_dev, h->disk.data(), h->disk.size() * sizeof(float), stream); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return fail_hip(h, what, e);
    h->disk_stale = false;
    return HIPRZ_OK;
}

ProbeMap map_of(const hiprz_probe* h) { return ProbeMap{h->base_dev, h->uv_dev, uint32_t(h->uv.size())}; }

// the gather of n device probes on the view the call has fetched
int launch_gather(hiprz_probe* h, const DScene& s, const hiprz_bake_point* probes, size_t n, uint32_t seed, const void* source, uint32_t W, uint32_t H, const float sky[3],
                  hiprz_probe_sh* out, hipStream_t stream, const char* what) {
    if (const int rc = place_tables(h, stream, what); rc != HIPRZ_OK) return rc;
    const uint32_t per_wave = h->K < 64u ? 64u / h->K : 1u;
    const uint32_t grid = uint32_t((n + per_wave - 1u) / per_wave);
    hipLaunchKernelGGL(rz_probe_gather_kernel, dim3(grid), dim3(RZ_PROBE_WG), 0, stream, s, reinterpret_cast<const float4*>(probes), uint32_t(n), h->dirs, h->K, h->S, seed,
                       map_of(h), static_cast<const float4*>(source), W, H, make_float4(sky[0], sky[1], sky[2], 0.0f), reinterpret_cast<float4*>(out));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

// the light term of n device probes on the view and the span the call has fetched
int launch_light(hiprz_probe* h, const DScene& s, const ProbeSpan& span, const hiprz_bake_point* probes, size_t n, uint32_t seed, const hiprz_probe_sh* base,
                 hiprz_probe_sh* out, hipStream_t stream, const char* what) {
    if (const int rc = place_disk(h, stream, what); rc != HIPRZ_OK) return rc;
    const uint32_t per_wave = h->LK < 64u ? 64u / h->LK : 1u;
    const uint32_t grid = uint32_t((n + per_wave - 1u) / per_wave);
    hipLaunchKernelGGL(rz_probe_light_kernel, dim3(grid), dim3(RZ_PROBE_WG), 0, stream, s, reinterpret_cast<const float4*>(probes), uint32_t(n), h->disk_dev, h->LK, h->LS,
                       seed, span, reinterpret_cast<const float4*>(base), reinterpret_cast<float4*>(out));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}
}  // namespace

extern "C" {

int hiprz_probe_create(hiprz_probe** out, hiprz_ctx* ctx) { return create(out, ctx, "probe_create"); }

int hiprz_probe_destroy(hiprz_probe* h) {
    return destroy(h, h && (h->dirs || h->disk_dev || h->base_dev || h->uv_dev || h->source_dev), [h] {
        for (void* p : {static_cast<void*>(h->dirs), static_cast<void*>(h->disk_dev), static_cast<void*>(h->base_dev), static_cast<void*>(h->uv_dev),
                        static_cast<void*>(h->source_dev)})
            if (p) (void)hipFree(p);
    });
}

const char* hiprz_probe_last_error(const hiprz_probe* h) { return last_error(h); }

int hiprz_probe_set_directions(hiprz_probe* h, const float* xyz0_host, uint32_t K, uint32_t S) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, "probe_set_directions: null probe");
    if (const char* why = probe_table_refusal(xyz0_host, K, S)) return fail(h, HIPRZ_ERR_INVALID, std::string("probe_set_directions: ") + why);
    h->table.assign(xyz0_host, xyz0_host + 4 * size_t(K) * S);
    for (size_t i = 3; i < h->table.size(); i += 4) h->table[i] = 0.0f;
    h->K = K, h->S = S, h->stale = true;
    return HIPRZ_OK;
}

int hiprz_probe_set_samples(hiprz_probe* h, const float* xy_host, uint32_t K, uint32_t S) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, "probe_set_samples: null probe");
    if (const char* why = probe_samples_refusal(xy_host, K, S)) return fail(h, HIPRZ_ERR_INVALID, std::string("probe_set_samples: ") + why);
    h->disk.assign(xy_host, xy_host + 2 * size_t(K) * S);
    h->LK = K, h->LS = S, h->disk_stale = true;
    return HIPRZ_OK;
}

int hiprz_probe_set_charts(hiprz_probe* h, const uint32_t* base_host, uint32_t n_instances, const hiprz_gather_chart* uv_host, uint32_t n_charts) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, "probe_set_charts: null probe");
    if (const char* why = probe_charts_refusal(base_host, n_instances, uv_host, n_charts)) return fail(h, HIPRZ_ERR_INVALID, std::string("probe_set_charts: ") + why);
    h->base.assign(base_host, base_host + n_instances);
    h->uv.assign(uv_host, uv_host + n_charts);
    h->has_charts = h->charts_stale = true;
    return HIPRZ_OK;
}

int hiprz_probe_gather(hiprz_probe* h, const hiprz_bake_point* probes_device, size_t n, uint32_t seed, const void* source16_device, uint32_t W, uint32_t H,
                       const float sky[3], hiprz_probe_sh* out_device, void* stream) {
    const char* what = "probe_gather";
    bool empty;
    if (const int rc = refuse_gather(h, !probes_device || !source16_device || !sky || !out_device, n, what, &empty); rc != HIPRZ_OK) return rc;
    if (const char* why = probe_size_refusal(W, H)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    if (empty) return HIPRZ_OK;
    DScene s;
    if (const int rc = view_and_map(h, what, s); rc != HIPRZ_OK) return rc;
    return launch_gather(h, s, probes_device, n, seed, source16_device, W, H, sky, out_device, stream_of(h, stream), what);
}

int hiprz_probe_samples(hiprz_probe* h, const hiprz_bake_point* probes_device, size_t n, uint32_t seed, hiprz_gather_sample* samples_out_device, void* stream) {
    const char* what = "probe_samples";
    bool empty;
    if (const int rc = refuse_gather(h, !probes_device || !samples_out_device, n, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view_and_map(h, what, s); rc != HIPRZ_OK) return rc;
    hipStream_t st = stream_of(h, stream);
    if (const int rc = place_tables(h, st, what); rc != HIPRZ_OK) return rc;
    const uint32_t n_rays = uint32_t(n * h->K);  // < 2^31
    hipLaunchKernelGGL(rz_probe_samples_kernel, dim3((n_rays + RZ_PROBE_WG - 1u) / RZ_PROBE_WG), dim3(RZ_PROBE_WG), 0, st, s, reinterpret_cast<const float4*>(probes_device),
                       n_rays, h->dirs, h->K, h->S, seed, map_of(h), reinterpret_cast<float4*>(samples_out_device));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

int hiprz_probe_light(hiprz_probe* h, const hiprz_bake_point* probes_device, size_t n, uint32_t seed, const hiprz_light_range* range, const hiprz_probe_sh* base_device,
                      hiprz_probe_sh* out_device, void* stream) {
    const char* what = "probe_light";
    bool empty;
    if (const int rc = refuse_light(h, !probes_device || !out_device, n, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    ProbeSpan span;
    if (const int rc = view_and_span(h, range, what, s, span); rc != HIPRZ_OK) return rc;
    return launch_light(h, s, span, probes_device, n, seed, base_device, out_device, stream_of(h, stream), what);
}

int hiprz_probe_gather_host(hiprz_probe* h, const hiprz_bake_point* probes, size_t n, uint32_t seed, const void* source16, uint32_t W, uint32_t H, const float sky[3],
                            hiprz_probe_sh* out) {
    const char* what = "probe_gather_host";
    bool empty;
    if (const int rc = refuse_gather(h, !probes || !source16 || !sky || !out, n, what, &empty); rc != HIPRZ_OK) return rc;
    if (const char* why = probe_size_refusal(W, H)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    if (empty) return HIPRZ_OK;
    DScene s;
    if (const int rc = view_and_map(h, what, s); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the buffers
    if (const int rc = grow_staging(h, what, n, sizeof(hiprz_bake_point), sizeof(hiprz_probe_sh), probe_capacity); rc != HIPRZ_OK) return rc;
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
    return round_trip(h, what, probes, n, sizeof(hiprz_bake_point), out, sizeof(hiprz_probe_sh), [&](void* dev_probes, void* dev_out, hipStream_t stream) {
        return launch_gather(h, s, static_cast<const hiprz_bake_point*>(dev_probes), n, seed, h->source_dev, W, H, sky, static_cast<hiprz_probe_sh*>(dev_out), stream, what);
    });
}

int hiprz_probe_light_host(hiprz_probe* h, const hiprz_bake_point* probes, size_t n, uint32_t seed, const hiprz_light_range* range, const hiprz_probe_sh* base,
                           hiprz_probe_sh* out) {
    const char* what = "probe_light_host";
    bool empty;
    if (const int rc = refuse_light(h, !probes || !out, n, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    ProbeSpan span;
    if (const int rc = view_and_span(h, range, what, s, span); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the staging
    if (const int rc = grow_staging(h, what, n, sizeof(hiprz_bake_point), sizeof(hiprz_probe_sh), probe_capacity); rc != HIPRZ_OK) return rc;
    return round_trip(h, what, probes, n, sizeof(hiprz_bake_point), out, sizeof(hiprz_probe_sh), [&](void* dev_probes, void* dev_out, hipStream_t stream) {
        if (base) {  // the base goes where the records will stand: the kernel reads a record before it writes it
            if (const hipError_t e = hipMemcpyAsync(dev_out, base, n * sizeof(hiprz_probe_sh), hipMemcpyHostToDevice, stream); e != hipSuccess) return fail_hip(h, what, e);
            if (const hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return fail_hip(h, what, e);  // the base is pageable and the caller's
        }
        return launch_light(h, s, span, static_cast<const hiprz_bake_point*>(dev_probes), n, seed, base ? static_cast<const hiprz_probe_sh*>(dev_out) : nullptr,
                            static_cast<hiprz_probe_sh*>(dev_out), stream, what);
    });
}

}  // extern "C"
