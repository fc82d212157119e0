// hiprz_denoise.hip — the denoiser's host side: parameter checks, the launch sequence of the a-trous iterations (hiprz_denoise_kernels.hpp)
// and the entry points of include/hiprz.h that run the filter and read its result.  No counterpart in the reference.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "hiprz_ctx.hpp"
#include "hiprz_denoise_kernels.hpp"

using namespace hiprz;

namespace {

// Defaults: the paper's 5 iterations and normal exponent; depth and colour tolerances from the error measurements of DESIGN.md "Denoising".
constexpr hiprz_denoise_params kDefaultParams{5u, 128.0f, 0.1f, 0.7f, HIPRZ_DENOISE_DEMODULATE};

int check_params(hiprz_ctx* c, const hiprz_denoise_params& p) {
    if (p.iterations < 1u || p.iterations > 6u) return fail(c, HIPRZ_ERR_INVALID, "denoise: iterations must be 1..6");
    if (!(p.sigma_normal >= 0.0f) || !(p.sigma_depth >= 0.0f) || !(p.sigma_color >= 0.0f) || std::isinf(p.sigma_normal) || std::isinf(p.sigma_depth) ||
        std::isinf(p.sigma_color))
        return fail(c, HIPRZ_ERR_INVALID, "denoise: the sigmas must be finite and not negative");
    if (p.flags & ~(HIPRZ_DENOISE_DEMODULATE | HIPRZ_DENOISE_VARIANCE)) return fail(c, HIPRZ_ERR_INVALID, "denoise: unknown flag");
    return HIPRZ_OK;
}

template <bool FIRST, bool LAST, bool VARIANCE>
void launch_iteration(const DenoiseArgs& a, hipStream_t stream) {
    const uint32_t s = 1u << a.shift;
    const uint32_t sub_w = (a.width + s - 1u) / s, sub_h = (a.height + s - 1u) / s;
    const dim3 grid(((sub_w + kDenoiseTileW - 1u) / kDenoiseTileW) << a.shift, ((sub_h + kDenoiseTileH - 1u) / kDenoiseTileH) << a.shift);
    RZ_LAUNCH((rz_atrous_kernel<FIRST, LAST, VARIANCE>), grid, dim3(256), 0, stream, a);
}

template <bool VARIANCE>
void launch_iteration(const DenoiseArgs& a, bool first, bool last, hipStream_t stream) {
    if (first && last) launch_iteration<true, true, VARIANCE>(a, stream);
    else if (first) launch_iteration<true, false, VARIANCE>(a, stream);
    else if (last) launch_iteration<false, true, VARIANCE>(a, stream);
    else launch_iteration<false, false, VARIANCE>(a, stream);
}

// the filter: src (accumulator image) -> dst (+ its tone map into rgba8 when given), guides as given, on `stream`; `variance`: the
// estimate's image under HIPRZ_DENOISE_VARIANCE
int run_filter(hiprz_ctx* c, const float4* src, const float4* guides, const float4* variance, const hiprz_denoise_params& p, float4* dst, uint32_t* rgba8,
               hipStream_t stream) {
    if (const int rc = check_params(c, p); rc != HIPRZ_OK) return rc;
    const bool guided = (p.flags & HIPRZ_DENOISE_VARIANCE) != 0u;
    if (guided != (variance != nullptr)) return fail(c, HIPRZ_ERR_INVALID, "denoise: HIPRZ_DENOISE_VARIANCE and the variance image go together");
    const uint32_t W = c->camera.width, H = c->camera.height;
    const size_t n = size_t(W) * H;
    for (uint32_t k = 0; k + 1u < p.iterations && k < 2u; ++k) RZ_HIP(c, c->dn_tmp[k].resize(n));
    DenoiseArgs a{};
    a.guides = guides, a.width = W, a.height = H;
    a.sigma_normal = p.sigma_normal, a.sigma_depth = p.sigma_depth;
    a.tone_k = ((c->camera.aperture * c->camera.aperture * RZ_PI_F) * c->camera.exposure_time) * 1.0e5f;
    a.demodulate = (p.flags & HIPRZ_DENOISE_DEMODULATE) ? 1u : 0u;
    a.aperture = c->camera.aperture, a.exposure_time = c->camera.exposure_time;
    a.variance = variance, a.sigma_lum = p.sigma_color;
    for (uint32_t i = 0; i < p.iterations; ++i) {
        const bool first = i == 0u, last = i + 1u == p.iterations;
        a.src = first ? src : c->dn_tmp[(i - 1u) & 1u].ptr;
        a.dst = last ? dst : c->dn_tmp[i & 1u].ptr;
        a.rgba8 = last ? rgba8 : nullptr;
        a.shift = i;
        const float scale = p.sigma_color / float(1u << i);
        a.color_scale2 = scale * scale;
        if (guided) launch_iteration<true>(a, first, last, stream);
        else launch_iteration<false>(a, first, last, stream);
    }
    RZ_HIP(c, hipGetLastError());
    return HIPRZ_OK;
}

int check_frame_holder(hiprz_ctx* c, const char* what) {
    if (c->is_peer) return fail(c, HIPRZ_ERR_STATE, std::string(what) + " on a part of a multi-device context");
    if (!c->have_scene || !c->have_camera) return fail(c, HIPRZ_ERR_STATE, std::string(what) + " before scene and camera upload");
    return HIPRZ_OK;
}

}  // namespace

namespace hiprz {

int denoise_frame(hiprz_ctx* c, const hiprz_denoise_params* params, uint32_t* rgba8_out) {
    if (const int rc = check_frame_holder(c, "denoise"); rc != HIPRZ_OK) return rc;
    if (c->user_world > 1u)
        return fail(c, HIPRZ_ERR_STATE, "denoise: this context renders shard " + std::to_string(c->user_rank) + " of " + std::to_string(c->user_world) +
                                            " and does not hold the frame (gather it, then hiprz_denoise_image)");
    const hiprz_denoise_params p = params ? *params : kDefaultParams;
    if (const int rc = check_params(c, p); rc != HIPRZ_OK) return rc;
    const bool guided = (p.flags & HIPRZ_DENOISE_VARIANCE) != 0u;
    if (guided && !c->variance_on) return fail(c, HIPRZ_ERR_STATE, "denoise: HIPRZ_DENOISE_VARIANCE needs the estimate of hiprz_set_variance, which is off");
    if (const int rc = ensure_guides(c); rc != HIPRZ_OK) return rc;
    if (guided)
        if (const int rc = assemble_variance_image(c); rc != HIPRZ_OK) return rc;
    if (const int rc = assemble_accum_image(c); rc != HIPRZ_OK) return rc;
    (void)hipSetDevice(c->device);
    const size_t n = size_t(c->camera.width) * c->camera.height;
    RZ_HIP(c, c->dn_out.resize(n));
    RZ_HIP(c, c->dn_rgba8.resize(n));
    if (const int rc = run_filter(c, c->image_f4.ptr, c->guides.ptr, guided ? c->var_image.ptr : nullptr, p, c->dn_out.ptr, c->dn_rgba8.ptr, c->stream); rc != HIPRZ_OK) return rc;
    if (rgba8_out) RZ_HIP(c, hipMemcpyAsync(rgba8_out, c->dn_rgba8.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c->stream));
    c->dn_valid = true;
    return HIPRZ_OK;
}

}  // namespace hiprz

extern "C" {

void hiprz_denoise_default_params(hiprz_denoise_params* out) {
    if (out) *out = kDefaultParams;
}

int hiprz_denoise(hiprz_ctx* c, const hiprz_denoise_params* params) {
    if (!c) return HIPRZ_ERR_INVALID;
    return denoise_frame(c, params, nullptr);
}

namespace {
int denoise_image(hiprz_ctx* c, const void* accum_image, const void* guides, const void* variance, bool guided, const hiprz_denoise_params* params, void* dst,
                  void* stream) {
    if (const int rc = check_frame_holder(c, "denoise_image"); rc != HIPRZ_OK) return rc;
    if (!accum_image || !dst || accum_image == dst) return fail(c, HIPRZ_ERR_INVALID, "denoise_image: null or aliased image");
    if (guided && (!variance || variance == dst)) return fail(c, HIPRZ_ERR_INVALID, "denoise_image_variance: null or aliased variance image");
    {
        const hiprz_denoise_params q = params ? *params : kDefaultParams;
        if (const int rc = check_params(c, q); rc != HIPRZ_OK) return rc;
        if (guided && !(q.flags & HIPRZ_DENOISE_VARIANCE)) return fail(c, HIPRZ_ERR_INVALID, "denoise_image_variance: HIPRZ_DENOISE_VARIANCE is not set");
        if (!guided && (q.flags & HIPRZ_DENOISE_VARIANCE)) return fail(c, HIPRZ_ERR_INVALID, "denoise_image: HIPRZ_DENOISE_VARIANCE takes hiprz_denoise_image_variance");
    }
    if (!guides) {
        if (const int rc = ensure_guides(c); rc != HIPRZ_OK) return rc;
        guides = c->guides.ptr;
    }
    (void)hipSetDevice(c->device);
    hipStream_t on = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (on != c->stream && (guides == c->guides.ptr || (variance && variance == c->var_image.ptr))) {  // the context's guides (its estimate) were enqueued on its own stream
        hipEvent_t e = nullptr;
        RZ_HIP(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        RZ_HIP(c, hipEventRecord(e, c->stream));
        RZ_HIP(c, hipStreamWaitEvent(on, e, 0));
        RZ_HIP(c, hipEventDestroy(e));
    }
    const hiprz_denoise_params p = params ? *params : kDefaultParams;
    return run_filter(c, static_cast<const float4*>(accum_image), static_cast<const float4*>(guides), static_cast<const float4*>(variance), p,
                      static_cast<float4*>(dst), nullptr, on);
}
}  // namespace

int hiprz_denoise_image(hiprz_ctx* c, const void* accum_image, const void* guides, const hiprz_denoise_params* params, void* dst, void* stream) {
    if (!c) return HIPRZ_ERR_INVALID;
    return denoise_image(c, accum_image, guides, nullptr, false, params, dst, stream);
}

int hiprz_denoise_image_variance(hiprz_ctx* c, const void* accum_image, const void* guides, const void* variance_image, const hiprz_denoise_params* params,
                                 void* dst, void* stream) {
    if (!c) return HIPRZ_ERR_INVALID;
    return denoise_image(c, accum_image, guides, variance_image, true, params, dst, stream);
}

int hiprz_read_denoised(hiprz_ctx* c, float* dst, size_t bytes) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!c->have_camera || !c->dn_valid) return fail(c, HIPRZ_ERR_STATE, "read_denoised: no hiprz_denoise on this camera at its size");
    if (!dst || bytes != size_t(c->camera.width) * c->camera.height * sizeof(float4)) return fail(c, HIPRZ_ERR_INVALID, "read_denoised: destination size mismatch");
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipMemcpyAsync(dst, c->dn_out.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return HIPRZ_OK;
}

int hiprz_read_denoised_rgba8(hiprz_ctx* c, uint8_t* dst, size_t bytes) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!c->have_camera || !c->dn_valid) return fail(c, HIPRZ_ERR_STATE, "read_denoised_rgba8: no hiprz_denoise on this camera at its size");
    if (!dst || bytes != size_t(c->camera.width) * c->camera.height * sizeof(uint32_t)) return fail(c, HIPRZ_ERR_INVALID, "read_denoised_rgba8: destination size mismatch");
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipMemcpyAsync(dst, c->dn_rgba8.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return HIPRZ_OK;
}

int hiprz_set_denoise(hiprz_ctx* c, const hiprz_denoise_params* params) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (params) {
        if (const int rc = check_params(c, *params); rc != HIPRZ_OK) return rc;
        c->denoise_params = *params;
    }
    c->denoise_on = params != nullptr;
    return HIPRZ_OK;
}

void hiprz_denoise_layout(uint32_t out[4]) {
    out[0] = sizeof(hiprz_guide), out[1] = sizeof(hiprz_denoise_params), out[2] = offsetof(hiprz_guide, albedo), out[3] = offsetof(hiprz_guide, instance);
}

}  // extern "C"
