// hiprz_smooth.hip — lightmap smoothing (include/hiprz_smooth.h): an a-trous filter over the 16-byte records of an atlas whose stops are
// made of the surface point under each texel, one launch of rz_smooth_kernel per iteration, ping-ponging through scratch the handle owns.
// A library of its own (libhiprz_smooth.so) beside the nine whose kernels and ABI are pinned.  It takes no device view: the context gives
// its stream, and the stream its device.  The kernel has two forms that write the same bytes — the taps of a texel are one device
// function, called in the header's order from LDS or from global memory.
#include <hip/hip_runtime.h>

#include <string>

#include "hiprz_smooth.h"
#include "hiprz_smooth_host.hpp"
#include "query/hiprz_session.hpp"  // the handle, its errors and the staging

#define RZ_SMOOTH_WG (kSmoothBlock * kSmoothBlock)
#define RZ_SMOOTH_HALO_TEXELS (kSmoothHalo * kSmoothHalo)

namespace hiprz {

// one iteration: what it reads, what it writes, which stops are on and the squares they divide by
struct SmoothPass {
    const float4* points;   // W*H hiprz_bake_point, two float4 each
    const float4* in;       // this iteration's input: the caller's records (first) or scratch, whose word is 1 on a texel that takes part, else 0
    const float4* words;    // the call's input, read for its word by the last iteration
    float4* out;
    uint32_t W, H, step;
    uint32_t per_x, per_y;  // staged: blocks per residue along each axis
    uint32_t first, last;
    uint32_t stops;         // bit 0: the radius stop is on (radius != 0), bit 1: the plane stop, bit 2: the colour stop
    float rr, pp, cc;       // radius*radius, plane*plane, sc*sc with sc = sigma_colour / float(step)
};

// what a tap needs of a texel
struct SmoothTexel {
    float px, py, pz, nx, ny, nz, r, g, b;
    bool on;  // takes part
};

// include/hiprz_smooth.h "A texel TAKES PART", decided on the call's input by the first iteration and carried in the word after it
RZ_DEV SmoothTexel smooth_texel(const float4 p0, const float4 p1, const float4 rec, bool first) {
    SmoothTexel t;
    t.px = p0.x, t.py = p0.y, t.pz = p0.z, t.nx = p1.x, t.ny = p1.y, t.nz = p1.z, t.r = rec.x, t.g = rec.y, t.b = rec.z;
    const uint32_t word = __float_as_uint(rec.w);
    if (first) {
        const bool flat = p1.x == 0.0f && p1.y == 0.0f && p1.z == 0.0f;
        t.on = word != HIPRZ_SMOOTH_INVALID && !flat && isfinite(rec.x) && isfinite(rec.y) && isfinite(rec.z);
    } else {
        t.on = word != 0u;
    }
    return t;
}

// include/hiprz_smooth.h "One iteration": tap q of texel p with the kernel weight h
RZ_DEV void smooth_tap(const SmoothPass& a, const SmoothTexel& p, const SmoothTexel& q, float h, float& nr, float& ng, float& nb, float& den) {
    if (!q.on) return;
    const float d = (p.nx * q.nx + p.ny * q.ny) + p.nz * q.nz;
    const float c = fmaxf(0.0f, d);
    const float c2 = c * c;
    float w = h * (c2 * c2);
    const float vx = q.px - p.px, vy = q.py - p.py, vz = q.pz - p.pz;
    if (a.stops & 1u) {
        const float r2 = (vx * vx + vy * vy) + vz * vz;
        w = w * fmaxf(0.0f, 1.0f - r2 / a.rr);
    }
    if (a.stops & 2u) {
        const float e = (p.nx * vx + p.ny * vy) + p.nz * vz;
        w = w * fmaxf(0.0f, 1.0f - (e * e) / a.pp);
    }
    if (a.stops & 4u) {
        const float gx = q.r - p.r, gy = q.g - p.g, gz = q.b - p.b;
        const float g2 = (gx * gx + gy * gy) + gz * gz;
        w = w * fmaxf(0.0f, 1.0f - g2 / a.cc);
    }
    if (w > 0.0f) {
        nr = nr + w * q.r, ng = ng + w * q.g, nb = nb + w * q.b;
        den = den + w;
    }
}

// what texel p at index i writes once its sums stand: the mean when it takes part and den > 0, else its value; the word is the call's
// input word on the last iteration and the take-part flag before it
RZ_DEV void smooth_store(const SmoothPass& a, size_t i, const SmoothTexel& p, float nr, float ng, float nb, float den) {
    float4 o = make_float4(p.r, p.g, p.b, __uint_as_float(p.on ? 1u : 0u));
    if (p.on && den > 0.0f) o.x = nr / den, o.y = ng / den, o.z = nb / den;
    if (a.last) o.w = a.words[i].w;
    a.out[i] = o;
}

RZ_DEV float smooth_b3(int k) { return k == 0 ? 6.0f : ((k == 1 || k == -1) ? 4.0f : 1.0f); }

// STAGED: the workgroup takes the 16 x 16 block (bx, by) of the sub-lattice (x0, y0) of step s: texel (x0 + s * lx, y0 + s * ly) for the
// lattice point (lx, ly) = (16 bx + tx, 16 by + ty).  Its 20 x 20 halo goes to LDS once, ten planes of 400 floats, entry e of a plane
// written by thread e % 256: consecutive lanes, consecutive banks.  A halo entry outside the atlas reads as a texel that does not take
// part.  DIRECT: one thread per texel (16 bx + tx, 16 by + ty), every tap from global memory.
template <bool STAGED>
__global__ void __launch_bounds__(RZ_SMOOTH_WG) rz_smooth_kernel(const SmoothPass a) {
    const int tx = int(threadIdx.x % kSmoothBlock);
    const int s = int(a.step);
    if constexpr (STAGED) {
        // The 32 lanes an LDS read serves in one cycle hold rows r and r + 4 of the block, not r and r + 1: with the halo's pitch of 20
        // floats their 16 banks each are 80 = 16 (mod 32) apart and never the same (rows r and r + 1, 20 apart, shared four banks and
        // doubled the LDS cycles of every tap, as SQ_LDS_BANK_CONFLICT showed).  Group g = thread / 32 takes rows (g % 4) + 8 (g / 4) + {0, 4}.
        const int group = int(threadIdx.x / 32u), ty = (group & 3) + 8 * (group >> 2) + 4 * int((threadIdx.x / kSmoothBlock) & 1u);
        __shared__ float plane[kSmoothPlanes][RZ_SMOOTH_HALO_TEXELS];
        const int x0 = int(blockIdx.x / a.per_x), y0 = int(blockIdx.y / a.per_y);
        const int lx0 = int(blockIdx.x % a.per_x) * int(kSmoothBlock), ly0 = int(blockIdx.y % a.per_y) * int(kSmoothBlock);
        for (uint32_t e = threadIdx.x; e < RZ_SMOOTH_HALO_TEXELS; e += RZ_SMOOTH_WG) {
            const int x = x0 + s * (lx0 + int(e % kSmoothHalo) - 2), y = y0 + s * (ly0 + int(e / kSmoothHalo) - 2);
            SmoothTexel t;
            t.px = t.py = t.pz = t.nx = t.ny = t.nz = t.r = t.g = t.b = 0.0f, t.on = false;
            if (x >= 0 && y >= 0 && x < int(a.W) && y < int(a.H)) {
                const size_t i = size_t(y) * a.W + size_t(x);
                t = smooth_texel(a.points[2 * i], a.points[2 * i + 1], a.in[i], a.first != 0u);
            }
            plane[0][e] = t.px, plane[1][e] = t.py, plane[2][e] = t.pz, plane[3][e] = t.nx, plane[4][e] = t.ny, plane[5][e] = t.nz;
            plane[6][e] = t.r, plane[7][e] = t.g, plane[8][e] = t.b, plane[9][e] = t.on ? 1.0f : 0.0f;
        }
        __syncthreads();
        const int x = x0 + s * (lx0 + tx), y = y0 + s * (ly0 + ty);
        if (x >= int(a.W) || y >= int(a.H)) return;
        const auto staged = [&](int e) {
            SmoothTexel t;
            t.px = plane[0][e], t.py = plane[1][e], t.pz = plane[2][e], t.nx = plane[3][e], t.ny = plane[4][e], t.nz = plane[5][e];
            t.r = plane[6][e], t.g = plane[7][e], t.b = plane[8][e], t.on = plane[9][e] != 0.0f;
            return t;
        };
        const int centre = (ty + 2) * int(kSmoothHalo) + tx + 2;
        const SmoothTexel p = staged(centre);
        float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
        if (p.on) {
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) smooth_tap(a, p, staged(centre + dy * int(kSmoothHalo) + dx), smooth_b3(dx) * smooth_b3(dy), nr, ng, nb, den);
        }
        smooth_store(a, size_t(y) * a.W + size_t(x), p, nr, ng, nb, den);
    } else {
        const int ty = int(threadIdx.x / kSmoothBlock);
        const int x = int(blockIdx.x * kSmoothBlock) + tx, y = int(blockIdx.y * kSmoothBlock) + ty;
        if (x >= int(a.W) || y >= int(a.H)) return;
        const size_t i = size_t(y) * a.W + size_t(x);
        const SmoothTexel p = smooth_texel(a.points[2 * i], a.points[2 * i + 1], a.in[i], a.first != 0u);
        float nr = 0.0f, ng = 0.0f, nb = 0.0f, den = 0.0f;
        if (p.on) {
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy)
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const int qx = x + s * dx, qy = y + s * dy;
                    if (qx < 0 || qy < 0 || qx >= int(a.W) || qy >= int(a.H)) continue;
                    const size_t j = size_t(qy) * a.W + size_t(qx);
                    smooth_tap(a, p, smooth_texel(a.points[2 * j], a.points[2 * j + 1], a.in[j], a.first != 0u), smooth_b3(dx) * smooth_b3(dy), nr, ng, nb, den);
                }
        }
        smooth_store(a, i, p, nr, ng, nb, den);
    }
}

}  // namespace hiprz

using namespace hiprz;

static_assert(sizeof(hiprz_bake_point) == 32 && sizeof(hiprz_smooth_params) == 16, "two 16-byte loads per point, one 16-byte argument");
static_assert(kSmoothPlanes * RZ_SMOOTH_HALO_TEXELS * sizeof(float) == 16000, "the staged form's LDS");

struct hiprz_smooth : Session {
    // [0], [1]: the ping and the pong of the iterations; [2]: the copy of an input that `out` overlaps.  Each grown on demand.
    float4* scratch[3] = {nullptr, nullptr, nullptr};
    size_t capacity[3] = {0, 0, 0};
};

namespace {

// the context's head device — the device of its stream — made current for the call's buffers and launches
int enter(hiprz_smooth* h, const char* what) {
    if (h->device < 0) {
        hipDevice_t device = 0;
        if (const hipError_t e = hipStreamGetDevice(static_cast<hipStream_t>(hiprz_stream(h->ctx)), &device); e != hipSuccess) return fail_hip(h, what, e);
        h->device = int(device);
    }
    if (const hipError_t e = hipSetDevice(h->device); e != hipSuccess) return fail_hip(h, what, e);
    return HIPRZ_OK;
}

int grow_scratch(hiprz_smooth* h, int k, size_t texels, const char* what) {
    if (texels <= h->capacity[k]) return HIPRZ_OK;
    const size_t cap = smooth_capacity(h->capacity[k], texels);
    if (h->scratch[k]) (void)hipFree(h->scratch[k]);  // (hipFree waits for whatever still uses the buffer)
    h->scratch[k] = nullptr, h->capacity[k] = 0;
    if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(&h->scratch[k]), cap * sizeof(float4)); e != hipSuccess) return fail_hip(h, what, e);
    h->capacity[k] = cap;
    return HIPRZ_OK;
}

// the iterations of a call whose refusals are behind it, on device arrays
int launch_iterations(hiprz_smooth* h, const hiprz_bake_point* points, const void* records, uint32_t W, uint32_t H, const hiprz_smooth_params& p, void* out,
                      hipStream_t stream, const char* what) {
    const size_t texels = size_t(W) * H;
    const float4* input = static_cast<const float4*>(records);
    if (p.iterations >= 2u)
        if (const int rc = grow_scratch(h, 0, texels, what); rc != HIPRZ_OK) return rc;
    if (p.iterations >= 3u)
        if (const int rc = grow_scratch(h, 1, texels, what); rc != HIPRZ_OK) return rc;
    if (smooth_overlap(records, out, texels * sizeof(float4))) {  // the last iteration would write what its neighbours still read
        if (const int rc = grow_scratch(h, 2, texels, what); rc != HIPRZ_OK) return rc;
        if (const hipError_t e = hipMemcpyAsync(h->scratch[2], records, texels * sizeof(float4), hipMemcpyDeviceToDevice, stream); e != hipSuccess)
            return fail_hip(h, what, e);
        input = h->scratch[2];
    }
    SmoothPass a;
    a.points = reinterpret_cast<const float4*>(points), a.words = input, a.W = W, a.H = H;
    a.rr = p.radius * p.radius, a.pp = p.plane * p.plane;
    a.stops = (p.radius != 0.0f ? 1u : 0u) | (p.plane != 0.0f ? 2u : 0u) | (p.sigma_colour != 0.0f ? 4u : 0u);
    const float4* src = input;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        a.step = 1u << i, a.first = i == 0u, a.last = i + 1u == p.iterations;
        const float sc = p.sigma_colour / float(a.step);
        a.cc = sc * sc;
        a.in = src, a.out = a.last ? static_cast<float4*>(out) : h->scratch[i & 1u];
        const bool staged = smooth_staged(a.step);
        const SmoothGrid g = smooth_grid(W, H, a.step, staged);
        a.per_x = g.per_x, a.per_y = g.per_y;
        if (staged) hipLaunchKernelGGL(rz_smooth_kernel<true>, dim3(g.x, g.y), dim3(RZ_SMOOTH_WG), 0, stream, a);
        else hipLaunchKernelGGL(rz_smooth_kernel<false>, dim3(g.x, g.y), dim3(RZ_SMOOTH_WG), 0, stream, a);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(h, what, e);
        src = a.out;
    }
    return HIPRZ_OK;
}

int refuse(hiprz_smooth* h, bool any_null, const hiprz_smooth_params* params, uint32_t W, uint32_t H, const char* what) {
    if (!h) return fail(nullptr, HIPRZ_ERR_INVALID, std::string(what) + ": null smooth");
    if (const char* why = smooth_refusal(any_null, params, W, H)) return fail(h, HIPRZ_ERR_INVALID, std::string(what) + ": " + why);
    return HIPRZ_OK;
}

}  // namespace

extern "C" {

int hiprz_smooth_create(hiprz_smooth** out, hiprz_ctx* ctx) { return create(out, ctx, "smooth_create"); }

int hiprz_smooth_destroy(hiprz_smooth* h) {
    return destroy(h, h && (h->scratch[0] || h->scratch[1] || h->scratch[2]), [h] {
        for (float4* p : h->scratch)
            if (p) (void)hipFree(p);
    });
}

const char* hiprz_smooth_last_error(const hiprz_smooth* h) { return last_error(h); }

int hiprz_smooth_texels(hiprz_smooth* h, const hiprz_bake_point* points_device, const void* records16_device, uint32_t W, uint32_t H, const hiprz_smooth_params* params,
                        void* out16_device, void* stream) {
    const char* what = "smooth_texels";
    if (const int rc = refuse(h, !points_device || !records16_device || !params || !out16_device, params, W, H, what); rc != HIPRZ_OK) return rc;
    if (const int rc = enter(h, what); rc != HIPRZ_OK) return rc;
    return launch_iterations(h, points_device, records16_device, W, H, *params, out16_device, stream_of(h, stream), what);
}

int hiprz_smooth_texels_host(hiprz_smooth* h, const hiprz_bake_point* points, const void* records16, uint32_t W, uint32_t H, const hiprz_smooth_params* params,
                             void* out16) {
    const char* what = "smooth_texels_host";
    if (const int rc = refuse(h, !points || !records16 || !params || !out16, params, W, H, what); rc != HIPRZ_OK) return rc;
    if (const int rc = enter(h, what); rc != HIPRZ_OK) return rc;
    const size_t n = size_t(W) * H, point_bytes = n * sizeof(hiprz_bake_point), record_bytes = n * 16u;
    // one staging record holds a point and a record: the n points first, the n records behind them
    if (const int rc = grow_staging(h, what, n, sizeof(hiprz_bake_point) + 16u, 16u, smooth_capacity); rc != HIPRZ_OK) return rc;
    const Staging& g = h->staging;
    hipStream_t st = stream_of(h, nullptr);
    std::memcpy(g.pinned_in, points, point_bytes);
    std::memcpy(static_cast<char*>(g.pinned_in) + point_bytes, records16, record_bytes);
    if (const hipError_t e = hipMemcpyAsync(g.dev_in, g.pinned_in, point_bytes + record_bytes, hipMemcpyHostToDevice, st); e != hipSuccess) return fail_hip(h, what, e);
    if (const int rc = launch_iterations(h, static_cast<const hiprz_bake_point*>(g.dev_in), static_cast<const char*>(g.dev_in) + point_bytes, W, H, *params, g.dev_out, st, what);
        rc != HIPRZ_OK)
        return rc;
    if (const hipError_t e = hipMemcpyAsync(g.pinned_out, g.dev_out, record_bytes, hipMemcpyDeviceToHost, st); e != hipSuccess) return fail_hip(h, what, e);
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(h, what, e);
    std::memcpy(out16, g.pinned_out, record_bytes);
    return HIPRZ_OK;
}

}  // extern "C"
