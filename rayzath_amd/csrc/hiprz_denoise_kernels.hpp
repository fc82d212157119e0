// hiprz_denoise_kernels.hpp — the edge-avoiding a-trous filter of include/hiprz.h ("THE FILTER": the formulas there are the specification;
// this file follows their order of operations, and tests/denoise_reference.py restates them in numpy).
//
// One iteration with step s reads, per pixel, 25 taps s pixels apart: a colour (16 B) and a guide (32 B) each.  The taps of neighbouring
// pixels of the SAME residue class (x mod s, y mod s) overlap, those of different classes never do — on the sub-lattice of one class the
// filter is a dense 5x5 again.  So a workgroup takes a 32x8 tile of ONE sub-lattice, stages the tile plus its 2-pixel halo (36x12 records
// of 48 B: colour + instance, normal + depth, tone-curved colour + validity = 20.3 KiB of LDS, seven workgroups per CU) with 16-byte loads,
// and every tap is three ds_read_b128.  Per staged pixel the demodulation (first iteration) and the tone curve t(c) are evaluated once
// instead of once per tap.  For s = 1 the sub-lattice is the image itself.  Workgroups of the s*s classes over the same image region are
// neighbours in the grid (blockIdx = tile * s + class), so the cache lines they share — a class uses every s-th record of a line — are
// fetched while hot.  The first iteration divides by the sample count and the albedo on the way in, the last multiplies the albedo back
// and tone-maps on the way out: neither costs a pass over the image.
//
// HIPRZ_DENOISE_VARIANCE (include/hiprz.h "THE VARIANCE-GUIDED FILTER") is a third instantiation axis on the same scheme and the same
// record: the tone-curved colour is unused there, so its slot carries lum(c_i) and v_i; the intermediate iterates' alpha, constant 1 and
// never read otherwise, carries v_i from one iteration to the next.  g_i, the weights and both sums come from the taps already staged —
// a first sweep over the 25 records' third quarter for g_i, then the sweep of the plain filter.
#pragma once
#include <hip/hip_runtime.h>

#include "hiprz.h"
#include "hiprz_device.hpp"

namespace hiprz {

struct DenoiseArgs {
    const float4* src;     // iteration 0: the accumulator image (alpha = finished paths); later: the previous iterate
    const float4* guides;  // two float4 per pixel: (normal, depth), (albedo, bits(instance))
    float4* dst;
    uint32_t* rgba8;       // last iteration: the tone map of dst, or nullptr
    uint32_t width, height;
    uint32_t shift;        // step s = 1 << shift
    float sigma_normal, sigma_depth;
    float color_scale2;    // (sigma_color * 2^-i)^2, 0 = no colour term
    float tone_k;          // pi * aperture^2 * exposure_time * 1e5
    uint32_t demodulate;
    float aperture, exposure_time;
    const float4* variance;  // VARIANCE, iteration 0: (V_r, V_g, V_b, K) per pixel (hiprz_read_variance)
    float sigma_lum;         // VARIANCE: sigma_color, in standard deviations
};

struct DenoiseTap {
    float4 c;  // current iterate rgb, bits(instance)
    float4 n;  // normal, depth
    float4 t;  // tone curve of c per channel, 1 = the tap lies in the frame; VARIANCE: (lum(c), v, 0, 1)
};

RZ_DEV float denoise_tone(float k, float c) {
    const float kc = k * c;
    return kc / (kc + 1.0f);
}
RZ_DEV float denoise_albedo(float a) { return fmaxf(a, 0.01f); }
RZ_DEV float denoise_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }

// the record of pixel (x, y), which lies in the frame
template <bool FIRST, bool VARIANCE>
RZ_DEV DenoiseTap denoise_load(const DenoiseArgs& a, uint32_t x, uint32_t y) {
    const size_t i = size_t(y) * a.width + x;
    const float4 v = a.src[i], g0 = a.guides[2u * i], g1 = a.guides[2u * i + 1u];
    float r = v.x, g = v.y, b = v.z;
    if constexpr (FIRST) {
        const float n = v.w == 0.0f ? 1.0f : v.w;
        r = r / n, g = g / n, b = b / n;
        if (a.demodulate) r = r / denoise_albedo(g1.x), g = g / denoise_albedo(g1.y), b = b / denoise_albedo(g1.z);
    }
    DenoiseTap tap;
    tap.c = make_float4(r, g, b, g1.w);
    tap.n = g0;
    if constexpr (VARIANCE) {
        float var = v.w;  // the previous iteration left v_i in the alpha channel
        if constexpr (FIRST) {
            const float4 V = a.variance[i];
            var = -1.0f;
            if (V.w >= 2.0f) {
                float sr = sqrtf(V.x), sg = sqrtf(V.y), sb = sqrtf(V.z);
                if (a.demodulate) sr = sr / denoise_albedo(g1.x), sg = sg / denoise_albedo(g1.y), sb = sb / denoise_albedo(g1.z);
                const float sd = denoise_lum(sr, sg, sb);
                var = sd * sd;
            }
        }
        tap.t = make_float4(denoise_lum(r, g, b), var, 0.0f, 1.0f);
    } else {
        tap.t = make_float4(denoise_tone(a.tone_k, r), denoise_tone(a.tone_k, g), denoise_tone(a.tone_k, b), 1.0f);
    }
    return tap;
}

struct DenoiseSum {
    float r, g, b, w;
};
// w(p, q) c(q) of one tap that is not the centre (include/hiprz.h, in its order of operations)
RZ_DEV void denoise_accumulate(const DenoiseArgs& a, const DenoiseTap& p, float depth_scale, const DenoiseTap& q, float spline, DenoiseSum& sum) {
    const uint32_t instance = __float_as_uint(p.c.w);
    if (q.t.w == 0.0f || __float_as_uint(q.c.w) != instance) return;
    float w = spline;
    if (instance != HIPRZ_GUIDE_MISS) {  // between two misses w_n = w_z = 1: no normal, and the depth is the far plane (inf - inf otherwise)
        w = w * RZ_POWF(fmaxf(0.0f, p.n.x * q.n.x + p.n.y * q.n.y + p.n.z * q.n.z), a.sigma_normal);
        w = w * RZ_EXPF(-(fabsf(p.n.w - q.n.w) / depth_scale));
    }
    if (a.color_scale2 > 0.0f) {
        const float dr = p.t.x - q.t.x, dg = p.t.y - q.t.y, db = p.t.z - q.t.z;
        w = w * RZ_EXPF(-((dr * dr + dg * dg + db * db) / a.color_scale2));
    }
    sum.r = sum.r + w * q.c.x, sum.g = sum.g + w * q.c.y, sum.b = sum.b + w * q.c.z, sum.w = sum.w + w;
}
// the same under HIPRZ_DENOISE_VARIANCE: w_l in the place of w_c, and sum w^2 v beside the sums
RZ_DEV void denoise_accumulate_variance(const DenoiseArgs& a, const DenoiseTap& p, float depth_scale, float lum_scale, const DenoiseTap& q, float spline, DenoiseSum& sum,
                                        float& sum_v) {
    const uint32_t instance = __float_as_uint(p.c.w);
    if (q.t.w == 0.0f || __float_as_uint(q.c.w) != instance) return;
    float w = spline;
    if (instance != HIPRZ_GUIDE_MISS) {
        w = w * RZ_POWF(fmaxf(0.0f, p.n.x * q.n.x + p.n.y * q.n.y + p.n.z * q.n.z), a.sigma_normal);
        w = w * RZ_EXPF(-(fabsf(p.n.w - q.n.w) / depth_scale));
    }
    if (p.t.y >= 0.0f) w = w * RZ_EXPF(-(fabsf(p.t.x - q.t.x) / lum_scale));
    sum.r = sum.r + w * q.c.x, sum.g = sum.g + w * q.c.y, sum.b = sum.b + w * q.c.z, sum.w = sum.w + w;
    sum_v = sum_v + (w * w) * fmaxf(q.t.y, 0.0f);
}
RZ_DEV float denoise_spline(int d) { return d == 0 ? 0.375f : (d == 1 || d == -1) ? 0.25f : 0.0625f; }

// alpha: 1, or under HIPRZ_DENOISE_VARIANCE the next iteration's v
template <bool LAST>
RZ_DEV void denoise_store(const DenoiseArgs& a, uint32_t x, uint32_t y, const DenoiseSum& sum, float alpha = 1.0f) {
    const size_t i = size_t(y) * a.width + x;
    float r = sum.r / sum.w, g = sum.g / sum.w, b = sum.b / sum.w;
    if constexpr (LAST) {
        if (a.demodulate) {
            const float4 g1 = a.guides[2u * i + 1u];
            r = r * denoise_albedo(g1.x), g = g * denoise_albedo(g1.y), b = b * denoise_albedo(g1.z);
        }
        if (a.rgba8) a.rgba8[i] = tonemap(col4{r, g, b, 1.0f}, a.aperture, a.exposure_time);
    }
    a.dst[i] = make_float4(r, g, b, LAST ? 1.0f : alpha);
}

constexpr uint32_t kDenoiseTileW = 32u, kDenoiseTileH = 8u, kDenoiseHalo = 2u;
constexpr uint32_t kDenoiseLdsW = kDenoiseTileW + 2u * kDenoiseHalo, kDenoiseLdsH = kDenoiseTileH + 2u * kDenoiseHalo;
constexpr uint32_t kDenoiseLdsRecords = kDenoiseLdsW * kDenoiseLdsH;

// grid: (tiles_x << shift, tiles_y << shift) with tiles over the sub-lattice of ceil(W / s) x ceil(H / s) pixels
template <bool FIRST, bool LAST, bool VARIANCE>
__global__ void __launch_bounds__(256) rz_atrous_kernel(const DenoiseArgs a) {
    __shared__ float4 lds_c[kDenoiseLdsRecords], lds_n[kDenoiseLdsRecords], lds_t[kDenoiseLdsRecords];
    const uint32_t s_mask = (1u << a.shift) - 1u;
    const uint32_t ox = blockIdx.x & s_mask, oy = blockIdx.y & s_mask;  // the residue class
    const int sx0 = int((blockIdx.x >> a.shift) * kDenoiseTileW) - int(kDenoiseHalo), sy0 = int((blockIdx.y >> a.shift) * kDenoiseTileH) - int(kDenoiseHalo);
    for (uint32_t i = threadIdx.x; i < kDenoiseLdsRecords; i += 256u) {
        const int sx = sx0 + int(i % kDenoiseLdsW), sy = sy0 + int(i / kDenoiseLdsW);
        DenoiseTap tap;
        tap.c = tap.n = tap.t = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (sx >= 0 && sy >= 0) {
            const uint32_t x = ox + (uint32_t(sx) << a.shift), y = oy + (uint32_t(sy) << a.shift);
            if (x < a.width && y < a.height) tap = denoise_load<FIRST, VARIANCE>(a, x, y);
        }
        lds_c[i] = tap.c, lds_n[i] = tap.n, lds_t[i] = tap.t;
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & 31u, ly = threadIdx.x >> 5;
    const uint32_t x = ox + (((blockIdx.x >> a.shift) * kDenoiseTileW + lx) << a.shift), y = oy + (((blockIdx.y >> a.shift) * kDenoiseTileH + ly) << a.shift);
    if (x >= a.width || y >= a.height) return;
    const uint32_t centre = (ly + kDenoiseHalo) * kDenoiseLdsW + lx + kDenoiseHalo;
    const DenoiseTap p{lds_c[centre], lds_n[centre], lds_t[centre]};
    const float depth_scale = a.sigma_depth * p.n.w + 1.0e-6f;
    DenoiseSum sum{0.0f, 0.0f, 0.0f, 0.0f};
    if constexpr (VARIANCE) {
        float lum_scale = 1.0f, sum_v = 0.0f;
        if (p.t.y >= 0.0f) {  // g_i(p): the spline average of v_i over the taps that have an estimate (the centre is one of them)
            const uint32_t instance = __float_as_uint(p.c.w);
            float gv = 0.0f, gk = 0.0f;
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    const uint32_t j = uint32_t(int(centre) + dy * int(kDenoiseLdsW) + dx);
                    const float4 t = lds_t[j];
                    if (t.w == 0.0f || !(t.y >= 0.0f) || __float_as_uint(lds_c[j].w) != instance) continue;
                    const float spline = denoise_spline(dx) * denoise_spline(dy);
                    gv = gv + spline * t.y, gk = gk + spline;
                }
            }
            lum_scale = a.sigma_lum * sqrtf(gv / gk) + 1.0e-10f;
        }
#pragma unroll
        for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
            for (int dx = -2; dx <= 2; ++dx) {
                const float spline = denoise_spline(dx) * denoise_spline(dy);
                if (dx == 0 && dy == 0) {
                    sum.r = sum.r + spline * p.c.x, sum.g = sum.g + spline * p.c.y, sum.b = sum.b + spline * p.c.z, sum.w = sum.w + spline;
                    sum_v = sum_v + (spline * spline) * fmaxf(p.t.y, 0.0f);
                    continue;
                }
                const uint32_t j = uint32_t(int(centre) + dy * int(kDenoiseLdsW) + dx);
                const DenoiseTap q{lds_c[j], lds_n[j], lds_t[j]};
                denoise_accumulate_variance(a, p, depth_scale, lum_scale, q, spline, sum, sum_v);
            }
        }
        denoise_store<LAST>(a, x, y, sum, p.t.y >= 0.0f ? sum_v / (sum.w * sum.w) : -1.0f);
        return;
    }
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float spline = denoise_spline(dx) * denoise_spline(dy);
            if (dx == 0 && dy == 0) {
                sum.r = sum.r + spline * p.c.x, sum.g = sum.g + spline * p.c.y, sum.b = sum.b + spline * p.c.z, sum.w = sum.w + spline;
                continue;
            }
            const uint32_t j = uint32_t(int(centre) + dy * int(kDenoiseLdsW) + dx);
            const DenoiseTap q{lds_c[j], lds_n[j], lds_t[j]};
            denoise_accumulate(a, p, depth_scale, q, spline, sum);
        }
    }
    denoise_store<LAST>(a, x, y, sum);
}

}  // namespace hiprz
