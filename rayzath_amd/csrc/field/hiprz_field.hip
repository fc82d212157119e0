// hiprz_field.hip — probe fields (include/hiprz_field.h): a visibility map per probe — the K rays of a probe are made as the probe library
// makes them, walked to their closest hits by the query's closest-hit walk and summed, per texel of an 8 x 8 octahedral map, into the
// first two moments of the distance seen — and the lookup of a grid of probes for shaded points, each probe weighted by a Chebyshev test
// against its map.  A library of its own (libhiprz_field.so) beside the ten whose kernels and ABI are pinned; the ray rule and the walk
// are the query's device functions (query/hiprz_query_device.hpp, no __global__), so a ray's t and side are hiprz_query_closest's.  The
// frame, the hash and the ray of hiprz_probe.h are restated here.  The bake reads the context through hiprz_device_view on every call; the
// lookup takes no view: the context gives its stream, the stream its device.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hiprz_field.h"
#include "hiprz_field_host.hpp"
#include "query/hiprz_query_device.hpp"
#include "query/hiprz_session.hpp"  // the handle, its errors, the view, the staging and its round trip

// threads per workgroup of the bake: one wave — a lane per ray of a round, then a lane per texel; the ballots span exactly the workgroup
#define RZ_FIELD_WG 64

namespace hiprz {

// what a probe gives every one of its rays: the two words of the probe, whether it is valid, its set and its frame
struct FieldProbe {
    float4 p0, p1;  // position, near_ | normal as given, far_
    v3 n, t, bt;    // include/hiprz_probe.h "THE FRAME" of the normalised normal (read on a valid probe only)
    uint32_t set;
    bool valid;
};

RZ_DEV FieldProbe field_probe(const float4* __restrict__ probes, uint32_t i, uint32_t seed, uint32_t S) {
    FieldProbe p;
    p.p0 = probes[2 * size_t(i)], p.p1 = probes[2 * size_t(i) + 1];
    Ray along;
    p.valid = take_ray(p.p0, p.p1, HIPRZ_QUERY_NORMALIZE, along);  // valid: along.d = normalized(normal)
    p.set = field_hash(i ^ seed) % S;
    const v3 n = along.d;
    const float s = copysignf(1.0f, n.z);
    const float a = -1.0f / (s + n.z);
    const float b = (n.x * n.y) * a;
    p.n = n;
    p.t = V3(1.0f + ((s * n.x) * n.x) * a, s * b, (-s) * n.x);
    p.bt = V3(b, s + (n.y * n.y) * a, -n.y);
    return p;
}

// the ray of (valid probe, direction k) as the two float4 of a hiprz_ray
RZ_DEV void field_ray(const FieldProbe& p, const float4* __restrict__ dirs, uint32_t K, uint32_t k, float4& r0, float4& r1) {
    const float4 l = dirs[size_t(p.set) * K + k];
    v3 d;
    d.x = (p.t.x * l.x + p.bt.x * l.y) + p.n.x * l.z;
    d.y = (p.t.y * l.x + p.bt.y * l.y) + p.n.y * l.z;
    d.z = (p.t.z * l.x + p.bt.z * l.y) + p.n.z * l.z;
    r0 = p.p0;
    r1 = make_float4(d.x, d.y, d.z, p.p1.w);
}

// include/hiprz_field.h "THE WALK": 0 = MISSED (an invalid ray included), 1 = FRONT, 2 = BACK; t is read for a hit only
RZ_DEV uint32_t field_walk(const DScene& s, const float4 r0, const float4 r1, float& t) {
    Ray ray;
    if (!take_ray(r0, r1, 0u, ray)) return 0u;
    Hit hit;
    hit.instance = -1, hit.triangle = 0u, hit.bx = hit.by = 0.0f, hit.external = true;
    Counters cnt;
    int found = 0;
    if (s.n_instances != 0u) found = closest_hit_skip<false, false, true>(s, TopCache{nullptr, nullptr, 0u}, ray, hit, cnt);
    if (found != 2) return 0u;
    t = ray.far_;
    return hit.external ? 1u : 2u;
}

// One wave per workgroup, probe blockIdx.x, K / 64 rounds.  In a round lane l walks ray 64 r + l and puts (d, r) into row l of LDS; behind
// the barrier every lane, as texel l, runs over the 64 rows in order (every lane reads the same address: a broadcast).  A lane whose probe
// is >= n or invalid walks nothing, but takes part in every ballot and barrier: nothing returns before them.
__global__ void __launch_bounds__(RZ_FIELD_WG) rz_field_visibility_kernel(const DScene s, const float4* __restrict__ probes, uint32_t n, const float4* __restrict__ dirs,
                                                                         uint32_t K, uint32_t S, uint32_t seed, float reach, const float4* __restrict__ texels,
                                                                         float* __restrict__ out) {
    __shared__ float4 rows[RZ_FIELD_WG];
    const uint32_t lane = threadIdx.x;
    const uint32_t probe = blockIdx.x;
    const bool inside = probe < n;
    FieldProbe p;
    p.valid = false;
    if (inside) p = field_probe(probes, probe, seed, S);
    const bool walks = inside && p.valid;
    const float4 o = texels[lane];
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    uint32_t n_front = 0u, n_back = 0u, n_missed = 0u;
    const uint32_t rounds = K / 64u;  // of a kernel argument alone: the same trip count on every lane
    for (uint32_t r = 0u; r < rounds; ++r) {
        float4 row = make_float4(0.0f, 0.0f, 0.0f, reach);
        uint32_t side = 3u;  // none
        if (walks) {
            float4 r0, r1;
            field_ray(p, dirs, K, 64u * r + lane, r0, r1);
            float t = reach;
            side = field_walk(s, r0, r1, t);
            row = make_float4(r1.x, r1.y, r1.z, side == 0u ? reach : fminf(t, reach));
        }
        rows[lane] = row;
        n_front += uint32_t(__popcll(__ballot(side == 1u)));
        n_back += uint32_t(__popcll(__ballot(side == 2u)));
        n_missed += uint32_t(__popcll(__ballot(side == 0u)));
        __syncthreads();
        for (uint32_t j = 0u; j < RZ_FIELD_WG; ++j) {
            const float4 q = rows[j];
            const float c = fmaxf(0.0f, (o.x * q.x + o.y * q.y) + o.z * q.z);
            float w = c * c;
            w = w * w;
            w = w * w;
            w = w * w;
            w = w * w;
            sw = sw + w;
            s1 = s1 + (w * q.w);
            s2 = s2 + (w * (q.w * q.w));
        }
        __syncthreads();
    }
    if (!inside) return;
    float* record = out + size_t(probe) * (sizeof(hiprz_field_vis) / sizeof(float));
    float2 m = make_float2(0.0f, 0.0f);
    if (p.valid) m = sw > 0.0f ? make_float2(s1 / sw, s2 / sw) : make_float2(reach, reach * reach);
    reinterpret_cast<float2*>(record)[lane] = m;
    if (lane == 0u)
        *reinterpret_cast<uint4*>(record + 2u * HIPRZ_FIELD_TEXELS) = p.valid ? make_uint4(n_front, n_back, n_missed, K) : make_uint4(0u, 0u, 0u, HIPRZ_FIELD_INVALID);
}

// the field of a lookup: the grid by value, the three arrays of its probes (vis may be null) and the params
struct FieldLookup {
    hiprz_field_grid grid;
    const float4* probes;  // two float4 per probe
    const float4* sh;      // nine per probe
    const float4* vis;     // 33 per probe, or null
    float bias;
    uint32_t max_back;
};

// include/hiprz_probe.h "THE EVALUATION" of the record at `sh` for the normal n
RZ_DEV v3 field_irradiance(const float4* __restrict__ sh, const v3 n) {
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
RZ_DEV float field_visible(const float4* __restrict__ vis, const v3 P, const v3 p, const v3 n, float bias) {
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

// thread i: point i
__global__ void __launch_bounds__(RZ_FIELD_LOOKUP_WG) rz_field_lookup_kernel(const FieldLookup a, const float4* __restrict__ points, uint32_t m, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * RZ_FIELD_LOOKUP_WG + threadIdx.x;
    if (i >= m) return;
    const float4 q0 = points[2 * size_t(i)], q1 = points[2 * size_t(i) + 1];
    const v3 p = xyz(q0), n = xyz(q1);
    const float4 invalid = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(HIPRZ_FIELD_INVALID));
    const float sq = (n.x * n.x + n.y * n.y) + n.z * n.z;
    const bool valid = isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(n.x) && isfinite(n.y) && isfinite(n.z) && sq >= 0.99f && sq <= 1.01f;
    if (!valid) {
        out[i] = invalid;
        return;
    }
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
            if (!left_out) w = field_visible(map, xyz(a.probes[2u * index]), p, n, a.bias) * tri;
        }
        if (left_out) continue;
        const v3 E = field_irradiance(record, n);
        acc.x = acc.x + (w * E.x);
        acc.y = acc.y + (w * E.y);
        acc.z = acc.z + (w * E.z);
        sw = sw + w;
        if (w > 0.0f) ++counted;
    }
    out[i] = sw > 0.0f ? make_float4(acc.x / sw, acc.y / sw, acc.z / sw, __uint_as_float(counted)) : invalid;
}

}  // namespace hiprz

using namespace hiprz;

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_probe_sh) == 144 && sizeof(hiprz_field_vis) == 528 && sizeof(hiprz_field_result) == 16 &&
                  offsetof(hiprz_field_vis, words) == 512,
              "two 16-byte loads per point, nine per record, 33 per visibility record, one 16-byte store per result");
static_assert(RZ_FIELD_LOOKUP_WG == 64 || RZ_FIELD_LOOKUP_WG == 256, "the two workgroup sizes that were measured");

struct hiprz_field : Session {
    std::vector<float> table;  // the directions as set, S*K float4 with w = 0; K == 0: none yet
    uint32_t K = 0, S = 0;
    float4* dirs = nullptr;    // the device copy, made by the first bake after set_directions (`stale`)
    bool stale = false;
    float4* texels = nullptr;  // THE TEXEL DIRECTIONS on the device, uploaded once
    void* held = nullptr;      // the device copy of a host field: probes, records and visibility records behind one another
    size_t held_bytes = 0;
};

namespace {

// the context's head device — the device of its stream — made current for a lookup's buffers and launch (a bake takes a view, which does it)
int enter(hiprz_field* h, const char* what) {
    if (h->device < 0) {
        hipDevice_t device = 0;
        if (const hipError_t e = hipStreamGetDevice(static_cast<hipStream_t>(hiprz_stream(h->ctx)), &device); e != hipSuccess) return fail_hip(h, what, e);
        h->device = int(device);
    }
    if (const hipError_t e = hipSetDevice(h->device); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

int refuse_visibility(hiprz_field* h, bool any_null, size_t n, float reach, const char* what, bool* empty) {
    *empty = false;
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null field");
    int code;
    if (const char* why = field_visibility_refusal(any_null, n, h->K, reach, &code)) return fail(h, code, std::string(what) + ": " + why);
    *empty = n == 0u;
    return HIPRZ_OK;
}

int refuse_lookup(hiprz_field* h, bool any_null, const hiprz_field_grid* grid, size_t n_probes, const hiprz_field_params* params, size_t m, const char* what, bool* empty) {
    *empty = false;
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null field");
    if (const char* why = field_lookup_refusal(any_null, grid, n_probes, params, m)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    *empty = m == 0u;
    return HIPRZ_OK;
}

// the directions a set_directions left on the host and, once, the texel directions go to the device before the bake's kernel; the stream
// is waited for, since the host arrays are pageable and may be replaced
int place_tables(hiprz_field* h, hipStream_t stream, const char* what) {
    if (!h->stale && h->texels) return HIPRZ_OK;
    float octahedron[64][4];
    if (!h->texels) {
        (void)hiprz_field_texel_directions(octahedron);
        if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->texels), sizeof octahedron); e != hipSuccess) return fail_hip(h, what, e);
        if (const hipError_t e = hipMemcpyAsync(h->texels, octahedron, sizeof octahedron, hipMemcpyHostToDevice, stream); e != hipSuccess) return fail_hip(h, what, e);
    }
    if (h->stale) {
        if (h->dirs) (void)hipFree(h->dirs);  // (hipFree waits for whatever still reads the old table)
        h->dirs = nullptr;
        const size_t bytes = h->table.size() * sizeof(float);
        if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->dirs), bytes); e != hipSuccess) return fail_hip(h, what, e);
        if (const hipError_t e = hipMemcpyAsync(h->dirs, h->table.data(), bytes, hipMemcpyHostToDevice, stream); e != hipSuccess) return fail_hip(h, what, e);
    }
    if (const hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return fail_hip(h, what, e);
    h->stale = false;
    return HIPRZ_OK;
}

// the bake of n device probes on the view the call has fetched
int launch_visibility(hiprz_field* h, const DScene& s, const hiprz_bake_point* probes, size_t n, uint32_t seed, float reach, hiprz_field_vis* out, hipStream_t stream,
                      const char* what) {
    if (const int rc = place_tables(h, stream, what); rc != HIPRZ_OK) return rc;
    hipLaunchKernelGGL(rz_field_visibility_kernel, dim3(uint32_t(n)), dim3(RZ_FIELD_WG), 0, stream, s, reinterpret_cast<const float4*>(probes), uint32_t(n), h->dirs, h->K, h->S,
                       seed, reach, h->texels, reinterpret_cast<float*>(out));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

// the lookup of m device points in a device field
int launch_lookup(hiprz_field* h, const hiprz_field_grid& grid, const void* probes, const void* sh, const void* vis, const hiprz_field_params& params, const void* points,
                  size_t m, void* out, hipStream_t stream, const char* what) {
    FieldLookup a;
    a.grid = grid, a.probes = static_cast<const float4*>(probes), a.sh = static_cast<const float4*>(sh), a.vis = static_cast<const float4*>(vis);
    a.bias = params.bias, a.max_back = params.max_back;
    const uint32_t groups = uint32_t((m + RZ_FIELD_LOOKUP_WG - 1u) / RZ_FIELD_LOOKUP_WG);
    hipLaunchKernelGGL(rz_field_lookup_kernel, dim3(groups), dim3(RZ_FIELD_LOOKUP_WG), 0, stream, a, static_cast<const float4*>(points), uint32_t(m), static_cast<float4*>(out));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

}  // namespace

extern "C" {

int hiprz_field_create(hiprz_field** out, hiprz_ctx* ctx) { return create(out, ctx, "field_create"); }

int hiprz_field_destroy(hiprz_field* h) {
    return destroy(h, h && (h->dirs || h->texels || h->held), [h] {
        for (void* p : {static_cast<void*>(h->dirs), static_cast<void*>(h->texels), h->held})
            if (p) (void)hipFree(p);
    });
}

const char* hiprz_field_last_error(const hiprz_field* h) { return last_error(h); }

int hiprz_field_set_directions(hiprz_field* h, const float* xyz0_host, uint32_t K, uint32_t S) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, "field_set_directions: null field");
    if (const char* why = field_table_refusal(xyz0_host, K, S)) return fail(h, HIPRZ_ERR_INVALID, std::string("field_set_directions: ") + why);
    h->table.assign(xyz0_host, xyz0_host + 4 * size_t(K) * S);
    for (size_t i = 3; i < h->table.size(); i += 4) h->table[i] = 0.0f;
    h->K = K, h->S = S, h->stale = true;
    return HIPRZ_OK;
}

int hiprz_field_visibility(hiprz_field* h, const hiprz_bake_point* probes_device, size_t n, uint32_t seed, float reach, hiprz_field_vis* out_device, void* stream) {
    const char* what = "field_visibility";
    bool empty;
    if (const int rc = refuse_visibility(h, !probes_device || !out_device, n, reach, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(h, what, s); rc != HIPRZ_OK) return rc;
    return launch_visibility(h, s, probes_device, n, seed, reach, out_device, stream_of(h, stream), what);
}

int hiprz_field_visibility_host(hiprz_field* h, const hiprz_bake_point* probes, size_t n, uint32_t seed, float reach, hiprz_field_vis* out) {
    const char* what = "field_visibility_host";
    bool empty;
    if (const int rc = refuse_visibility(h, !probes || !out, n, reach, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(h, what, s); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the staging
    if (const int rc = grow_staging(h, what, n, sizeof(hiprz_bake_point), sizeof(hiprz_field_vis), field_capacity); rc != HIPRZ_OK) return rc;
    return round_trip(h, what, probes, n, sizeof(hiprz_bake_point), out, sizeof(hiprz_field_vis), [&](void* dev_probes, void* dev_out, hipStream_t stream) {
        return launch_visibility(h, s, static_cast<const hiprz_bake_point*>(dev_probes), n, seed, reach, static_cast<hiprz_field_vis*>(dev_out), stream, what);
    });
}

int hiprz_field_lookup(hiprz_field* h, const hiprz_field_grid* grid, const hiprz_bake_point* probes_device, const hiprz_probe_sh* sh_device, const hiprz_field_vis* vis_device,
                       size_t n_probes, const hiprz_field_params* params, const hiprz_bake_point* points_device, size_t m, hiprz_field_result* out_device, void* stream) {
    const char* what = "field_lookup";
    bool empty;
    if (const int rc = refuse_lookup(h, !grid || !probes_device || !sh_device || !params || !points_device || !out_device, grid, n_probes, params, m, what, &empty);
        rc != HIPRZ_OK || empty)
        return rc;
    if (const int rc = enter(h, what); rc != HIPRZ_OK) return rc;
    return launch_lookup(h, *grid, probes_device, sh_device, vis_device, *params, points_device, m, out_device, stream_of(h, stream), what);
}

int hiprz_field_lookup_host(hiprz_field* h, const hiprz_field_grid* grid, const hiprz_bake_point* probes, const hiprz_probe_sh* sh, const hiprz_field_vis* vis, size_t n_probes,
                            const hiprz_field_params* params, const hiprz_bake_point* points, size_t m, hiprz_field_result* out) {
    const char* what = "field_lookup_host";
    bool empty;
    if (const int rc = refuse_lookup(h, !grid || !probes || !sh || !params || !points || !out, grid, n_probes, params, m, what, &empty); rc != HIPRZ_OK || empty) return rc;
    if (const int rc = enter(h, what); rc != HIPRZ_OK) return rc;
    if (const int rc = grow_staging(h, what, m, sizeof(hiprz_bake_point), sizeof(hiprz_field_result), field_capacity); rc != HIPRZ_OK) return rc;
    // the field: the probes, their records and their visibility records behind one another in one device buffer (each a multiple of 16 bytes)
    const size_t probe_bytes = n_probes * sizeof(hiprz_bake_point), sh_bytes = n_probes * sizeof(hiprz_probe_sh), vis_bytes = vis ? n_probes * sizeof(hiprz_field_vis) : 0u;
    const size_t bytes = probe_bytes + sh_bytes + vis_bytes;
    if (bytes > h->held_bytes) {
        if (h->held) (void)hipFree(h->held);  // (hipFree waits for whatever still reads the buffer)
        h->held = nullptr, h->held_bytes = 0;
        if (const hipError_t e = hipMalloc(&h->held, bytes); e != hipSuccess) return fail_hip(h, what, e);
        h->held_bytes = bytes;
    }
    char* dev = static_cast<char*>(h->held);
    hipStream_t st = stream_of(h, nullptr);
    if (const hipError_t e = hipMemcpyAsync(dev, probes, probe_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipMemcpyAsync(dev + probe_bytes, sh, sh_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
    if (vis)
        if (const hipError_t e = hipMemcpyAsync(dev + probe_bytes + sh_bytes, vis, vis_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(h, what, e);  // the field is pageable and the caller's
    return round_trip(h, what, points, m, sizeof(hiprz_bake_point), out, sizeof(hiprz_field_result), [&](void* dev_points, void* dev_out, hipStream_t stream) {
        return launch_lookup(h, *grid, dev, dev + probe_bytes, vis ? dev + probe_bytes + sh_bytes : nullptr, *params, dev_points, m, dev_out, stream, what);
    });
}

}  // extern "C"
