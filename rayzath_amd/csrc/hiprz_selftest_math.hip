// hiprz_selftest_math.hip — hiprz_selftest_math (include/hiprz.h): the shading arithmetic of hiprz_device.hpp evaluated one function call
// per case, so that a test can hold every result to a float64 reference (tests/test_device_math_gpu.py).  The kernel calls the RZ_* macros
// and the RZ_DEV functions themselves — what the render kernels inline — and is compiled with the flags of every other unit.  Nothing here
// is on a render path.
#include <hip/hip_runtime.h>

#include <string>

#include "hiprz.h"
#include "hiprz_ctx.hpp"
#include "hiprz_device.hpp"

using namespace hiprz;

namespace {

struct Widths {
    uint32_t in, out;
};
// row widths per op, in the order of the HIPRZ_MATH_* values
constexpr Widths kWidths[HIPRZ_MATH_OP_COUNT] = {
    {1, 1}, {1, 1}, {1, 2}, {1, 1}, {1, 1}, {2, 1}, {2, 1}, {1, 1}, {1, 1}, {1, 1}, {2, 1}, {1, 1},  // library calls
    {3, 6}, {5, 3}, {5, 3}, {5, 3}, {6, 3}, {10, 3}, {7, 1}, {2, 1}, {6, 3}, {6, 3}, {2, 4},          // composed primitives
    {22, 21},                                                                                         // sample_direction
};

RZ_DEV void st3(float* o, v3 v) { o[0] = v.x, o[1] = v.y, o[2] = v.z; }

// The reference's sampleDirection (cpu_engine_kernel.cpp:596-687) with every formula spelled by the separate function the reference calls:
// sample_sphere; the refraction; reflect_vector; cosine_sample_hemisphere; sample_hemisphere then reflect_vector.  sample_direction merges
// the last two by hand; this is what it has to equal, draw for draw.  `path`: which of them ran, plus 8 where the direction was flipped.
RZ_DEV v3 sample_direction_parts(v3 ray_d, uint32_t& ray_material, Surface& sf, Rng& rng, uint32_t& path) {
    if (sf.color.a > 0.0f) {
        if (sf.surface_scattering > 0.0f) {
            const float u1 = rng.unsignedUniform();
            const float u2 = rng.unsignedUniform();
            const v3 vO = sample_sphere(u1, u2, ray_d);
            sf.tint_factor = sf.metalness;
            path = 0u;
            return vO;
        }
        if (sf.fresnel < rng.unsignedUniform()) {
            const v3 vO = ray_d * sf.refr_x + sf.mapped_normal * sf.refr_y;
            ray_material = sf.behind_material;
            sf.normal = -sf.normal;
            sf.tint_factor = 1.0f;
            path = 1u;
            return vO;
        }
        v3 vO = reflect_vector(ray_d, sf.mapped_normal);
        const float d = dot(vO, sf.normal);
        path = 2u;
        if (d < 0.0f) vO = vO + (sf.normal * -2.0f) * d, path |= 8u;
        sf.tint_factor = sf.metalness;
        return vO;
    }
    if (rng.unsignedUniform() > sf.reflectance) {
        const float u1 = rng.unsignedUniform();
        const float u2 = rng.unsignedUniform();
        v3 vO = cosine_sample_hemisphere(u1, u2, sf.mapped_normal);
        const float d = similarity(vO, sf.normal);
        path = 3u;
        if (d < 0.0f) vO = vO + (sf.normal * -2.0f) * d, path |= 8u;
        sf.tint_factor = 1.0f;
        return vO;
    }
    const float u1 = rng.unsignedUniform();
    const float u2 = rng.unsignedUniform();
    const v3 vH = sample_hemisphere(u1, 1.0f - RZ_POWF(u2 + 1.0e-5f, sf.roughness), sf.mapped_normal);
    v3 vO = reflect_vector(ray_d, vH);
    const float d = similarity(vO, sf.normal);
    path = 4u;
    if (d < 0.0f) vO = vO + (sf.normal * -2.0f) * d, path |= 8u;
    sf.tint_factor = sf.metalness;
    return vO;
}

}  // namespace

// one thread per case: row i of `in` -> row i of `out`; `op` is uniform over the launch
__global__ void __launch_bounds__(256) rz_selftest_math_kernel(uint32_t op, const float* in, uint32_t w_in, uint32_t n, float* out, uint32_t w_out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float* a = in + size_t(i) * w_in;
    float* o = out + size_t(i) * w_out;
    switch (op) {
    case HIPRZ_MATH_SINF: o[0] = RZ_SINF(a[0]); break;
    case HIPRZ_MATH_COSF: o[0] = RZ_COSF(a[0]); break;
    case HIPRZ_MATH_SINCOSF: {
        float s, c;
        RZ_SINCOSF(a[0], s, c);
        o[0] = s, o[1] = c;
        break;
    }
    case HIPRZ_MATH_ACOSF: o[0] = RZ_ACOSF(a[0]); break;
    case HIPRZ_MATH_ASINF: o[0] = RZ_ASINF(a[0]); break;
    case HIPRZ_MATH_ATAN2F: o[0] = RZ_ATAN2F(a[0], a[1]); break;
    case HIPRZ_MATH_POWF: o[0] = RZ_POWF(a[0], a[1]); break;
    case HIPRZ_MATH_EXPF: o[0] = RZ_EXPF(a[0]); break;
    case HIPRZ_MATH_LOGF: o[0] = RZ_LOGF(a[0]); break;
    case HIPRZ_MATH_SQRTF: o[0] = sqrtf(a[0]); break;
    case HIPRZ_MATH_DIV: o[0] = a[0] / a[1]; break;
    case HIPRZ_MATH_WRAP: o[0] = fmodf(fmodf(a[0], 1.0f) + 1.0f, 1.0f); break;  // texel_offset
    case HIPRZ_MATH_LOCAL_COORDINATE: {
        v3 vX, vY;
        local_coordinate(ld3(a), vX, vY);
        st3(o, vX), st3(o + 3, vY);
        break;
    }
    case HIPRZ_MATH_COSINE_SAMPLE_HEMISPHERE: st3(o, cosine_sample_hemisphere(a[0], a[1], ld3(a + 2))); break;
    case HIPRZ_MATH_SAMPLE_SPHERE: st3(o, sample_sphere(a[0], a[1], ld3(a + 2))); break;
    case HIPRZ_MATH_SAMPLE_HEMISPHERE: st3(o, sample_hemisphere(a[0], a[1], ld3(a + 2))); break;
    case HIPRZ_MATH_SAMPLE_DISK: st3(o, sample_disk(a[0], a[1], ld3(a + 2), a[5])); break;
    case HIPRZ_MATH_FRESNEL: {
        float fx = a[8], fy = a[9];
        o[0] = fresnel_specular_ratio(ld3(a), ld3(a + 3), a[6], a[7], fx, fy);
        o[1] = fx, o[2] = fy;
        break;
    }
    case HIPRZ_MATH_NDF: o[0] = ndf(ld3(a), ld3(a + 3), a[6]); break;
    case HIPRZ_MATH_ATTENUATION: o[0] = attenuation(a[0], a[1]); break;
    case HIPRZ_MATH_REFLECT_VECTOR: st3(o, reflect_vector(ld3(a), ld3(a + 3))); break;
    case HIPRZ_MATH_HALFWAY_VECTOR: st3(o, halfway_vector(ld3(a), ld3(a + 3))); break;
    case HIPRZ_MATH_GLOSSY_LOBE: {
        // the general sequence, as sampleGlossyDirection reaches it through sample_hemisphere and sample_sphere ...
        const float theta = RZ_ACOSF(1.0f - 2.0f * ((1.0f - RZ_POWF(a[0] + 1.0e-5f, a[1])) * 0.5f));
        float s, c;
        RZ_SINCOSF(theta, s, c);
        o[0] = s, o[1] = c;
        // ... and what sample_direction takes at this roughness
        glossy_lobe(a[0], a[1], s, c);
        o[2] = s, o[3] = c;
        break;
    }
    case HIPRZ_MATH_SAMPLE_DIRECTION: {
        Surface sf;
        sf.surface_material = 0u, sf.behind_material = __float_as_uint(a[21]);
        sf.u = 0.0f, sf.v = 0.0f, sf.emission = 0.0f;
        sf.color = col4{1.0f, 1.0f, 1.0f, a[3]};
        sf.surface_scattering = a[4], sf.fresnel = a[5], sf.reflectance = a[6], sf.metalness = a[7], sf.roughness = a[8];
        sf.normal = ld3(a + 9), sf.mapped_normal = ld3(a + 12);
        sf.refr_x = a[15], sf.refr_y = a[16];
        sf.tint_factor = -1.0f;
        const v3 ray_d = ld3(a + 17);
        Surface parts = sf;
        Rng rng(a[0], a[1], a[2]), rng_parts(a[0], a[1], a[2]);
        uint32_t material = __float_as_uint(a[20]), material_parts = material, path = 0u;
        st3(o, sample_direction(ray_d, material, sf, rng));
        o[3] = sf.tint_factor, o[4] = __uint_as_float(material);
        st3(o + 5, sf.normal);
        o[8] = rng.a, o[9] = rng.b;
        st3(o + 10, sample_direction_parts(ray_d, material_parts, parts, rng_parts, path));
        o[13] = parts.tint_factor, o[14] = __uint_as_float(material_parts);
        st3(o + 15, parts.normal);
        o[18] = rng_parts.a, o[19] = rng_parts.b;
        o[20] = __uint_as_float(path);
        break;
    }
    default: break;  // (the host refuses an unknown op before it launches)
    }
}

int hiprz_selftest_math_widths(uint32_t op, uint32_t* floats_per_case_in, uint32_t* floats_per_case_out) {
    if (op >= HIPRZ_MATH_OP_COUNT || !floats_per_case_in || !floats_per_case_out) return HIPRZ_ERR_INVALID;
    *floats_per_case_in = kWidths[op].in, *floats_per_case_out = kWidths[op].out;
    return HIPRZ_OK;
}

int hiprz_selftest_math(hiprz_ctx* c, uint32_t op, const float* in, uint32_t floats_per_case_in, uint32_t n_cases, float* out,
                        uint32_t floats_per_case_out) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!in || !out) return fail(c, HIPRZ_ERR_INVALID, "selftest_math: null pointer");
    if (op >= HIPRZ_MATH_OP_COUNT) return fail(c, HIPRZ_ERR_INVALID, "selftest_math: unknown op " + std::to_string(op));
    if (floats_per_case_in != kWidths[op].in || floats_per_case_out != kWidths[op].out)
        return fail(c, HIPRZ_ERR_INVALID, "selftest_math: op " + std::to_string(op) + " takes rows of " + std::to_string(kWidths[op].in) +
                                              " floats and returns rows of " + std::to_string(kWidths[op].out));
    if (n_cases > (1u << 24)) return fail(c, HIPRZ_ERR_INVALID, "selftest_math: more than 2^24 cases");
    if (n_cases == 0u) return HIPRZ_OK;
    (void)hipSetDevice(c->device);
    struct Work {
        DeviceArray<float> in, out;
        ~Work() { in.release(), out.release(); }
    } w;
    const size_t n_in = size_t(n_cases) * floats_per_case_in, n_out = size_t(n_cases) * floats_per_case_out;
    RZ_HIP(c, w.out.resize(n_out));
    RZ_HIP(c, w.in.assign(in, n_in, c->stream));
    RZ_LAUNCH(rz_selftest_math_kernel, dim3((n_cases + 255u) / 256u), dim3(256), 0, c->stream, op, w.in.ptr, floats_per_case_in, n_cases, w.out.ptr,
              floats_per_case_out);
    RZ_HIP(c, hipGetLastError());
    RZ_HIP(c, hipMemcpyAsync(out, w.out.ptr, sizeof(float) * n_out, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return HIPRZ_OK;
}
