// hiprz_noise.hip — the noise meter's kernel and C-ABI (include/hiprz_noise.h): a W*H accumulator image and its variance estimate in, one
// float4 record per 32x8 tile out.  A library of its own (libhiprz_noise.so): libhiprz.so's kernel set is pinned (tests/test_launch_plan.py),
// and a caller that never measures runs none of this.  The summary is pure host code (hiprz_noise_host.cpp).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "hiprz_noise.h"

#define RZ_NOISE_PI_F 3.14159265358979323846f

// One workgroup per tile; thread l is lane l of the tile: pixel (l % 32, l / 32), so a wave holds two rows of the tile and 32 consecutive
// lanes read 512 contiguous bytes of each image.  The four reductions run down the wave by __shfl_down (v[l] += v[l + s], s = 32 .. 1: lane
// 0 ends with the specified association), the four wave results meet in LDS as (w0 + w1) + (w2 + w3).
__global__ void __launch_bounds__(256) rz_noise_tiles_kernel(const float4* __restrict__ accum, const float4* __restrict__ variance,
                                                             float4* __restrict__ tiles, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                             float k, float threshold, float min_batches) {
    __shared__ float4 wave_part[4];
    const uint32_t l = threadIdx.x;
    const uint32_t tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const uint32_t x = tx * 32u + (l & 31u), y = ty * 8u + (l >> 5);
    float sum = 0.0f, peak = 0.0f;
    uint32_t counts = 0u;  // n_estimated | n_above << 16 (at most 256 each)
    if (x < width && y < height) {
        const size_t i = size_t(y) * width + x;
        const float4 c = accum[i], v = variance[i];
        const float a = c.w == 0.0f ? 1.0f : c.w;
        const float dr = k * (c.x / a) + 1.0f, dg = k * (c.y / a) + 1.0f, db = k * (c.z / a) + 1.0f;
        const float sr = sqrtf(v.x) * (k / (dr * dr)), sg = sqrtf(v.y) * (k / (dg * dg)), sb = sqrtf(v.z) * (k / (db * db));
        const float e = (0.2126f * sr + 0.7152f * sg) + 0.0722f * sb;
        if (v.w >= min_batches && isfinite(e)) {
            sum = e * e, peak = e;
            counts = 1u | (e > threshold ? 0x10000u : 0u);
        }
    }
    for (int s = 32; s >= 1; s >>= 1) {
        sum += __shfl_down(sum, s);
        peak = fmaxf(peak, __shfl_down(peak, s));
        counts += __shfl_down(counts, s);
    }
    if ((l & 63u) == 0u) wave_part[l >> 6] = make_float4(sum, peak, float(counts & 0xFFFFu), float(counts >> 16));
    __syncthreads();
    if (l == 0u) {
        const float4 p0 = wave_part[0], p1 = wave_part[1], p2 = wave_part[2], p3 = wave_part[3];
        tiles[blockIdx.x] = make_float4((p0.x + p1.x) + (p2.x + p3.x), fmaxf(fmaxf(p0.y, p1.y), fmaxf(p2.y, p3.y)), (p0.z + p1.z) + (p2.z + p3.z),
                                        (p0.w + p1.w) + (p2.w + p3.w));
    }
}

struct hiprz_noise_meter {
    int device = 0;
    float4* tiles = nullptr;   // device: the tile records of hiprz_noise_measure
    float4* pinned = nullptr;  // ... and their pinned twin
    size_t capacity = 0;       // of both, in records
    std::string error;
};

namespace {
thread_local std::string g_error;  // of calls without a meter

int fail(hiprz_noise_meter* m, int code, const std::string& message) {
    (m ? m->error : g_error) = message;
    return code;
}
int fail_hip(hiprz_noise_meter* m, const char* what, hipError_t e) { return fail(m, HIPRZ_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e)); }

bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}
bool plausible(float v) { return std::isfinite(v) && v >= 0.0f; }

// everything refused is refused here, before anything is launched
int launch(hiprz_noise_meter* m, const void* accum, const void* variance, uint32_t width, uint32_t height, const hiprz_noise_params* p, float4* tiles_out,
           hipStream_t stream, const char* what) {
    const std::string who = what;
    if (!accum || !variance) return fail(m, HIPRZ_ERR_INVALID, who + ": null image");
    if (!tiles_out) return fail(m, HIPRZ_ERR_INVALID, who + ": null output");
    if (!p) return fail(m, HIPRZ_ERR_INVALID, who + ": null params");
    if (!width || !height) return fail(m, HIPRZ_ERR_INVALID, who + ": zero width or height");
    if (p->min_batches < 2u) return fail(m, HIPRZ_ERR_INVALID, who + ": min_batches must be at least 2");
    if (!plausible(p->threshold) || !plausible(p->aperture) || !plausible(p->exposure_time))
        return fail(m, HIPRZ_ERR_INVALID, who + ": threshold, aperture and exposure_time must be finite and not negative");
    const uint64_t tiles_x = (width - 1u) / HIPRZ_NOISE_TILE_W + 1u, tiles_y = (height - 1u) / HIPRZ_NOISE_TILE_H + 1u;
    if (tiles_x * tiles_y > 0x7FFFFFFFull) return fail(m, HIPRZ_ERR_INVALID, who + ": more tiles than one grid holds");
    const size_t image_bytes = size_t(width) * height * sizeof(float4), out_bytes = size_t(tiles_x * tiles_y) * sizeof(float4);
    if (overlaps(accum, image_bytes, tiles_out, out_bytes) || overlaps(variance, image_bytes, tiles_out, out_bytes))
        return fail(m, HIPRZ_ERR_INVALID, who + ": an image aliases the output");
    const float k = ((p->aperture * p->aperture * RZ_NOISE_PI_F) * p->exposure_time) * 1.0e5f;
    hipLaunchKernelGGL(rz_noise_tiles_kernel, dim3(uint32_t(tiles_x * tiles_y)), dim3(256), 0, stream, static_cast<const float4*>(accum),
                       static_cast<const float4*>(variance), tiles_out, width, height, uint32_t(tiles_x), k, p->threshold, float(p->min_batches));
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return fail_hip(m, what, e);
    return HIPRZ_OK;
}
}  // namespace

extern "C" {

int hiprz_noise_create(hiprz_noise_meter** out, int device_id) {
    if (!out) return fail(nullptr, HIPRZ_ERR_INVALID, "noise_create: null output");
    *out = nullptr;
    int n = 0;
    if (const hipError_t e = hipGetDeviceCount(&n); e != hipSuccess || n <= 0)
        return fail(nullptr, HIPRZ_ERR_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(nullptr, HIPRZ_ERR_DEVICE, "noise_create: no HIP device " + std::to_string(device_id));
    hiprz_noise_meter* m = new hiprz_noise_meter;
    m->device = device_id;
    *out = m;
    return HIPRZ_OK;
}

int hiprz_noise_destroy(hiprz_noise_meter* m) {
    if (!m) return HIPRZ_ERR_INVALID;
    (void)hipSetDevice(m->device);
    if (m->tiles) (void)hipFree(m->tiles);
    if (m->pinned) (void)hipHostFree(m->pinned);
    delete m;
    return HIPRZ_OK;
}

const char* hiprz_noise_last_error(const hiprz_noise_meter* m) { return m ? m->error.c_str() : g_error.c_str(); }

int hiprz_noise_tiles(hiprz_noise_meter* m, const void* accum, const void* variance, uint32_t width, uint32_t height, const hiprz_noise_params* p,
                      void* tiles_out_device, void* stream) {
    if (!m) return fail(nullptr, HIPRZ_ERR_INVALID, "noise_tiles: null meter");
    if (const hipError_t e = hipSetDevice(m->device); e != hipSuccess) return fail_hip(m, "noise_tiles", e);
    return launch(m, accum, variance, width, height, p, static_cast<float4*>(tiles_out_device), static_cast<hipStream_t>(stream), "noise_tiles");
}

int hiprz_noise_measure(hiprz_noise_meter* m, const void* accum, const void* variance, uint32_t width, uint32_t height, const hiprz_noise_params* p,
                        void* stream, hiprz_noise_summary* out, float* tiles_out_host) {
    if (!m) return fail(nullptr, HIPRZ_ERR_INVALID, "noise_measure: null meter");
    if (!out) return fail(m, HIPRZ_ERR_INVALID, "noise_measure: null summary");
    if (!width || !height) return fail(m, HIPRZ_ERR_INVALID, "noise_measure: zero width or height");
    if (const hipError_t e = hipSetDevice(m->device); e != hipSuccess) return fail_hip(m, "noise_measure", e);
    const uint64_t tiles_x = (width - 1u) / HIPRZ_NOISE_TILE_W + 1u, tiles_y = (height - 1u) / HIPRZ_NOISE_TILE_H + 1u;
    if (tiles_x * tiles_y > 0x7FFFFFFFull) return fail(m, HIPRZ_ERR_INVALID, "noise_measure: more tiles than one grid holds");
    const size_t n = size_t(tiles_x * tiles_y);
    if (n > m->capacity) {  // (hipFree waits for whatever still reads the old buffer)
        if (m->tiles) (void)hipFree(m->tiles);
        if (m->pinned) (void)hipHostFree(m->pinned);
        m->tiles = m->pinned = nullptr, m->capacity = 0;
        if (const hipError_t e = hipMalloc(reinterpret_cast<void**>(&m->tiles), n * sizeof(float4)); e != hipSuccess) return fail_hip(m, "noise_measure: tile buffer", e);
        if (const hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&m->pinned), n * sizeof(float4), hipHostMallocDefault); e != hipSuccess)
            return fail_hip(m, "noise_measure: pinned staging", e);
        m->capacity = n;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (const int rc = launch(m, accum, variance, width, height, p, m->tiles, st, "noise_measure"); rc != HIPRZ_OK) return rc;
    if (const hipError_t e = hipMemcpyAsync(m->pinned, m->tiles, n * sizeof(float4), hipMemcpyDeviceToHost, st); e != hipSuccess) return fail_hip(m, "noise_measure: copy", e);
    if (const hipError_t e = hipStreamSynchronize(st); e != hipSuccess) return fail_hip(m, "noise_measure", e);
    if (tiles_out_host) std::memcpy(tiles_out_host, m->pinned, n * sizeof(float4));
    if (hiprz_noise_summarise(reinterpret_cast<const float*>(m->pinned), uint32_t(tiles_x), uint32_t(tiles_y), width, height, out) != HIPRZ_OK)
        return fail(m, HIPRZ_ERR_INVALID, "noise_measure: summary refused the tile grid");
    return HIPRZ_OK;
}

}  // extern "C"
