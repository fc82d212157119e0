// hiprz_place.hip — probe placement (include/hiprz_place.h): every probe of a grid is evaluated by its K rays — made as the probe library
// makes them, walked to their closest hits by the query's closest-hit walk — and moved, up to `iterations` times, through the nearest back
// face when it sits inside geometry and towards its most open direction when a front face is nearer than a margin; the loop runs inside
// the kernel.  A library of its own (libhiprz_place.so) beside the eleven whose kernels and ABI are pinned; the ray rule and the walk are
// the query's device functions (query/hiprz_query_device.hpp, no __global__), so a ray's t and side are hiprz_query_closest's.  The
// frame, the hash and the ray of hiprz_probe.h are restated here.  The context is read through hiprz_device_view on every call.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "hiprz_place.h"
#include "hiprz_place_host.hpp"
#include "query/hiprz_query_device.hpp"
#include "query/hiprz_session.hpp"  // the handle, its errors, the view, the staging

// threads per workgroup: one wave — a lane per ray of a round; the ballots and the butterfly span exactly the workgroup
#define RZ_PLACE_WG 64

namespace hiprz {

// what a probe gives every one of its rays: the two words of the probe, whether it is valid, its set and its frame
struct PlaceProbe {
    float4 p0, p1;  // position, near_ | normal as given, far_
    v3 n, t, bt;    // include/hiprz_probe.h "THE FRAME" of the normalised normal (read on a valid probe only)
    uint32_t set;
    bool valid;
};

RZ_DEV PlaceProbe place_probe(const float4* __restrict__ probes, uint32_t i, uint32_t seed, uint32_t S) {
    PlaceProbe p;
    p.p0 = probes[2 * size_t(i)], p.p1 = probes[2 * size_t(i) + 1];
    Ray along;
    p.valid = take_ray(p.p0, p.p1, HIPRZ_QUERY_NORMALIZE, along);  // valid: along.d = normalized(normal)
    p.set = place_hash(i ^ seed) % S;
    const v3 n = along.d;
    const float s = copysignf(1.0f, n.z);
    const float a = -1.0f / (s + n.z);
    const float b = (n.x * n.y) * a;
    p.n = n;
    p.t = V3(1.0f + ((s * n.x) * n.x) * a, s * b, (-s) * n.x);
    p.bt = V3(b, s + (n.y * n.y) * a, -n.y);
    return p;
}

// the direction of ray k of a valid probe, as made: it does not depend on where the probe is
RZ_DEV v3 place_direction(const PlaceProbe& p, const float4* __restrict__ dirs, uint32_t K, uint32_t k) {
    const float4 l = dirs[size_t(p.set) * K + k];
    v3 d;
    d.x = (p.t.x * l.x + p.bt.x * l.y) + p.n.x * l.z;
    d.y = (p.t.y * l.x + p.bt.y * l.y) + p.n.y * l.z;
    d.z = (p.t.z * l.x + p.bt.z * l.y) + p.n.z * l.z;
    return d;
}

// include/hiprz_field.h "THE WALK": 0 = OPEN (an invalid ray included), 1 = FRONT, 2 = BACK; t is read for a hit only
RZ_DEV uint32_t place_walk(const DScene& s, const float4 r0, const float4 r1, float& t) {
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

constexpr uint64_t kPlaceNone = ~uint64_t(0);

// a value every lane of the wave holds alike, moved to a scalar register: the same bits, and no vector register held across the walk
RZ_DEV float place_uniform(float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); }
RZ_DEV v3 place_uniform(const v3 a) { return V3(place_uniform(a.x), place_uniform(a.y), place_uniform(a.z)); }

// the least key of the wave, in every lane and then in scalar registers: a minimum is exact and does not depend on the order
RZ_DEV uint64_t place_least(uint64_t key) {
#pragma unroll
    for (int off = 1; off < RZ_PLACE_WG; off <<= 1) {
        const uint64_t other = __shfl_xor(key, off, RZ_PLACE_WG);
        key = other < key ? other : key;
    }
    const uint32_t lo = __builtin_amdgcn_readfirstlane(uint32_t(key)), hi = __builtin_amdgcn_readfirstlane(uint32_t(key >> 32));
    return (uint64_t(hi) << 32) | lo;
}

// One wave per workgroup, probe blockIdx.x, K / 64 rounds per evaluation, up to iterations + 1 evaluations.  Everything the loop branches
// on is a kernel argument, a word of the wave's one probe or a value reduced over the wave and read into scalar registers: every branch is
// taken by the whole wave, and nothing returns before the last ballot and shuffle.
__global__ void __launch_bounds__(RZ_PLACE_WG) rz_place_kernel(const DScene s, const float4* __restrict__ probes, uint32_t n, const float4* __restrict__ dirs, uint32_t K,
                                                               uint32_t S, uint32_t seed, const hiprz_place_params a, float4* __restrict__ out_probes,
                                                               float4* __restrict__ out_records) {
    const uint32_t lane = threadIdx.x;
    const uint32_t probe = blockIdx.x;
    const bool inside = probe < n;
    PlaceProbe p;
    p.valid = false, p.p0 = p.p1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (inside) p = place_probe(probes, probe, seed, S);
    p.n = place_uniform(p.n), p.t = place_uniform(p.t), p.bt = place_uniform(p.bt);  // (one probe per wave: its frame is the wave's)
    const bool walks = inside && p.valid;
    const v3 H = xyz(p.p0);
    v3 P = H, o = V3(0.0f, 0.0f, 0.0f);
    uint32_t moves = 0u, state = HIPRZ_PLACE_CLEAR, stuck = 0u, n_back = 0u, n_front = 0u;
    float front = a.reach, back = a.reach;
    const uint32_t rounds = K / 64u;  // of a kernel argument alone: the same trip count on every lane
    for (;;) {
        // --- one evaluation at P ---
        uint64_t kb = kPlaceNone, kf = kPlaceNone, ko = kPlaceNone;
        n_back = n_front = 0u;
        for (uint32_t r = 0u; r < rounds; ++r) {
            const uint32_t k = 64u * r + lane;
            uint32_t side = 3u;  // none
            float dist = a.reach;
            if (walks) {
                const v3 d = place_direction(p, dirs, K, k);
                float t = a.reach;
                side = place_walk(s, make_float4(P.x, P.y, P.z, p.p0.w), make_float4(d.x, d.y, d.z, p.p1.w), t);
                dist = side == 0u ? a.reach : fminf(t, a.reach);
            }
            const uint64_t key = (uint64_t(__float_as_uint(dist)) << 32) | k, open_key = (uint64_t(~__float_as_uint(dist)) << 32) | k;
            if (side == 2u && key < kb) kb = key;
            if (side == 1u && key < kf) kf = key;
            if (side <= 1u && open_key < ko) ko = open_key;
            n_front += uint32_t(__popcll(__ballot(side == 1u)));
            n_back += uint32_t(__popcll(__ballot(side == 2u)));
        }
        kb = place_least(kb), kf = place_least(kf), ko = place_least(ko);
        const float r_b = __uint_as_float(uint32_t(kb >> 32)), r_f = __uint_as_float(uint32_t(kf >> 32)), r_o = __uint_as_float(~uint32_t(ko >> 32));
        front = kf != kPlaceNone ? r_f : a.reach;
        back = kb != kPlaceNone ? r_b : a.reach;
        state = n_back > a.max_back ? HIPRZ_PLACE_INSIDE : (kf != kPlaceNone && r_f < a.min_front) ? HIPRZ_PLACE_NEAR : HIPRZ_PLACE_CLEAR;
        // --- the move ---
        if (moves == a.iterations || state == HIPRZ_PLACE_CLEAR) break;
        v3 m;
        if (state == HIPRZ_PLACE_INSIDE) {  // (n_back > max_back >= 0: B exists, its k < K)
            const v3 d = place_direction(p, dirs, K, uint32_t(kb));
            const float step = r_b + (0.5f * a.min_front);
            m = V3(d.x * step, d.y * step, d.z * step);
        } else {
            bool open = ko != kPlaceNone;
            v3 d_o = V3(0.0f, 0.0f, 0.0f);
            if (open) {
                d_o = place_direction(p, dirs, K, uint32_t(ko));
                const v3 d_f = place_direction(p, dirs, K, uint32_t(kf));
                open = (d_o.x * d_f.x + d_o.y * d_f.y) + d_o.z * d_f.z <= 0.5f;
            }
            if (__builtin_amdgcn_readfirstlane(uint32_t(open)) == 0u) {  // (every lane holds the same: the branch is the wave's)
                stuck = HIPRZ_PLACE_STUCK;
                break;
            }
            const float step = fminf(a.min_front - r_f, 0.5f * r_o);
            m = V3(d_o.x * step, d_o.y * step, d_o.z * step);
        }
        const v3 to = V3(o.x + m.x, o.y + m.y, o.z + m.z);
        const bool beyond = fabsf(to.x) > a.max_offset[0] || fabsf(to.y) > a.max_offset[1] || fabsf(to.z) > a.max_offset[2];
        if (__builtin_amdgcn_readfirstlane(uint32_t(beyond)) != 0u) {
            stuck = HIPRZ_PLACE_STUCK;
            break;
        }
        o = place_uniform(to);
        P = place_uniform(V3(H.x + o.x, H.y + o.y, H.z + o.z));
        ++moves;
    }
    if (!inside || lane != 0u) return;
    out_probes[2 * size_t(probe)] = p.valid ? make_float4(P.x, P.y, P.z, p.p0.w) : p.p0;
    out_probes[2 * size_t(probe) + 1] = p.p1;
    if (!out_records) return;
    float4 w0 = make_float4(0.0f, 0.0f, 0.0f, __uint_as_float(HIPRZ_PLACE_INVALID)), w1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (p.valid) {
        w0 = make_float4(o.x, o.y, o.z, __uint_as_float(state | stuck | (moves << 16)));
        w1 = make_float4(front, back, __uint_as_float(n_back), __uint_as_float(n_front));
    }
    out_records[2 * size_t(probe)] = w0;
    out_records[2 * size_t(probe) + 1] = w1;
}

}  // namespace hiprz

using namespace hiprz;

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_place_params) == 32 && sizeof(hiprz_place_record) == 32 && offsetof(hiprz_place_record, word) == 12 &&
                  offsetof(hiprz_place_record, front) == 16,
              "two 16-byte loads and stores per probe, two 16-byte stores per record");

struct hiprz_place : Session {
    std::vector<float> table;  // the directions as set, S*K float4 with w = 0; K == 0: none yet
    uint32_t K = 0, S = 0;
    float4* dirs = nullptr;  // the device copy, made by the first placement after set_directions (`stale`)
    bool stale = false;
};

namespace {

int refuse(hiprz_place* h, bool any_null, size_t n, const hiprz_place_params* params, const char* what, bool* empty) {
    *empty = false;
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null place");
    int code;
    if (const char* why = place_probes_refusal(any_null, n, h->K, params, &code)) return fail(h, code, std::string(what) + ": " + why);
    *empty = n == 0u;
    return HIPRZ_OK;
}

// the directions a set_directions left on the host go to the device before the kernel; the stream is waited for, since the host array is
// pageable and may be replaced
int place_table(hiprz_place* h, hipStream_t stream, const char* what) {
    if (!h->stale) return HIPRZ_OK;
    if (h->dirs) (void)hipFree(h->dirs);  // (hipFree waits for whatever still reads the old table)
    h->dirs = nullptr;
    const size_t bytes = h->table.size() * sizeof(float);
    if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->dirs), bytes); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipMemcpyAsync(h->dirs, h->table.data(), bytes, hipMemcpyHostToDevice, stream); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipStreamSynchronize(stream); e != hipSuccess) return fail_hip(h, what, e);
    h->stale = false;
    return HIPRZ_OK;
}

// the placement of n device probes on the view the call has fetched
int launch(hiprz_place* h, const DScene& s, const void* probes, size_t n, uint32_t seed, const hiprz_place_params& params, void* out_probes, void* out_records,
           hipStream_t stream, const char* what) {
    if (const int rc = place_table(h, stream, what); rc != HIPRZ_OK) return rc;
    hipLaunchKernelGGL(rz_place_kernel, dim3(uint32_t(n)), dim3(RZ_PLACE_WG), 0, stream, s, static_cast<const float4*>(probes), uint32_t(n), h->dirs, h->K, h->S, seed, params,
                       static_cast<float4*>(out_probes), static_cast<float4*>(out_records));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

}  // namespace

extern "C" {

int hiprz_place_create(hiprz_place** out, hiprz_ctx* ctx) { return create(out, ctx, "place_create"); }

int hiprz_place_destroy(hiprz_place* h) {
    return destroy(h, h && h->dirs, [h] {
        if (h->dirs) (void)hipFree(h->dirs);
    });
}

const char* hiprz_place_last_error(const hiprz_place* h) { return last_error(h); }

int hiprz_place_set_directions(hiprz_place* h, const float* xyz0_host, uint32_t K, uint32_t S) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, "place_set_directions: null place");
    if (const char* why = place_table_refusal(xyz0_host, K, S)) return fail(h, HIPRZ_ERR_INVALID, std::string("place_set_directions: ") + why);
    h->table.assign(xyz0_host, xyz0_host + 4 * size_t(K) * S);
    for (size_t i = 3; i < h->table.size(); i += 4) h->table[i] = 0.0f;
    h->K = K, h->S = S, h->stale = true;
    return HIPRZ_OK;
}

int hiprz_place_probes(hiprz_place* h, const hiprz_bake_point* probes_device, size_t n, uint32_t seed, const hiprz_place_params* params, hiprz_bake_point* out_probes_device,
                       hiprz_place_record* out_records_device, void* stream) {
    const char* what = "place_probes";
    bool empty;
    if (const int rc = refuse(h, !probes_device || !params || !out_probes_device, n, params, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(h, what, s); rc != HIPRZ_OK) return rc;
    return launch(h, s, probes_device, n, seed, *params, out_probes_device, out_records_device, stream_of(h, stream), what);
}

int hiprz_place_probes_host(hiprz_place* h, const hiprz_bake_point* probes, size_t n, uint32_t seed, const hiprz_place_params* params, hiprz_bake_point* out_probes,
                            hiprz_place_record* out_records) {
    const char* what = "place_probes_host";
    bool empty;
    if (const int rc = refuse(h, !probes || !params || !out_probes, n, params, what, &empty); rc != HIPRZ_OK || empty) return rc;
    DScene s;
    if (const int rc = view(h, what, s); rc != HIPRZ_OK) return rc;  // refuses first, and makes the head device current for the staging
    // a staging record out is a moved probe and its record: the n probes first, the n records behind them
    constexpr size_t in_bytes = sizeof(hiprz_bake_point), out_bytes = sizeof(hiprz_bake_point) + sizeof(hiprz_place_record);
    if (const int rc = grow_staging(h, what, n, in_bytes, out_bytes, place_capacity); rc != HIPRZ_OK) return rc;
    const Staging& g = h->staging;
    hipStream_t st = stream_of(h, nullptr);
    char* dev_records = static_cast<char*>(g.dev_out) + n * sizeof(hiprz_bake_point);
    std::memcpy(g.pinned_in, probes, n * in_bytes);
    if (const hipError_t e = hipMemcpyAsync(g.dev_in, g.pinned_in, n * in_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
    if (const int rc = launch(h, s, g.dev_in, n, seed, *params, g.dev_out, dev_records, st, what); rc != HIPRZ_OK) return rc;
    if (const hipError_t e = hipMemcpyAsync(g.pinned_out, g.dev_out, n * out_bytes, hipMemcpyDeviceToHost, st); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(h, what, e);
    std::memcpy(out_probes, g.pinned_out, n * sizeof(hiprz_bake_point));
    if (out_records) std::memcpy(out_records, static_cast<const char*>(g.pinned_out) + n * sizeof(hiprz_bake_point), n * sizeof(hiprz_place_record));
    return HIPRZ_OK;
}

}  // extern "C"
