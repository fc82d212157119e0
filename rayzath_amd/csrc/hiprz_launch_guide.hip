// hiprz_launch_guide.hip — first-hit guide buffers of the denoiser (include/hiprz.h: hiprz_guide): rz_guide_kernel, its launch and the
// three entry points that hand the guides out.  No counterpart in the reference.
#include <hip/hip_runtime.h>

#include "hiprz_ctx.hpp"
#include "hiprz_kernels.hpp"

namespace hiprz {

// One thread per pixel of the WHOLE frame, row-major (no tiles, no shards): the first pass's pixel-centre ray, the skip-link walk on the
// trees the context holds (ties ranked by the reference's order, so every tree gives the reference's triangle), then analyze_intersection
// and fetch_color_emission, the very functions shade_segment fills the Surface with.  Nothing else is read or written: no random numbers, no frame state, no
// counters.  A record is two 16-byte stores.
__global__ void __launch_bounds__(256) rz_guide_kernel(const DScene s, const DCamera cam, const DConfig cfg, float4* guides) {
    const uint32_t x = blockIdx.x * 32u + (threadIdx.x & 31u), y = blockIdx.y * 8u + (threadIdx.x >> 5);
    if (x >= cam.width || y >= cam.height) return;
    Ray ray;
    generate_simple_ray(cam, ray, x, y);
    Hit hit;
    hit.instance = -1, hit.triangle = 0u, hit.bx = hit.by = 0.0f, hit.external = true;
    Counters cnt;
    int found = 0;
    if (s.n_instances != 0u) found = closest_hit_skip<false, false, true>(s, TopCache{nullptr, nullptr, 0u}, ray, hit, cnt);
    v3 normal = V3(0.0f, 0.0f, 0.0f);
    col4 albedo = splat(1.0f);
    uint32_t instance = HIPRZ_GUIDE_MISS;
    if (found == 2) {
        const bool compat = (cfg.flags & kIntegratorFlags) != 0u;  // the passes run rz_compat_pass_kernel: its fetches
        const bool filtering = compat && (cfg.flags & HIPRZ_COMPAT_FILTERING) != 0u;
        Surface sf;
        sf.u = sf.v = 0.0f;
        Material m;
        analyze_intersection<false, true>(s, hit, sf, m, cnt, filtering);
        if (compat) fetch_color_emission<false, true, true>(s, m, cfg.flags, filtering, sf, cnt);
        else fetch_color_emission<false, true, false>(s, m, cfg.flags, filtering, sf, cnt);
        normal = sf.mapped_normal;
        if (!(sf.emission > 0.0f)) albedo = sf.color;
        instance = uint32_t(hit.instance);
    }
    float4* g = guides + 2u * (size_t(y) * cam.width + x);
    g[0] = make_float4(normal.x, normal.y, normal.z, ray.far_);
    g[1] = make_float4(albedo.r, albedo.g, albedo.b, __uint_as_float(instance));
}

int ensure_guides(hiprz_ctx* c) {
    if (!c->have_scene || !c->have_camera) return fail(c, HIPRZ_ERR_STATE, "guides before scene and camera upload");
    if (c->is_peer) return fail(c, HIPRZ_ERR_STATE, "guides on a part of a multi-device context");
    (void)hipSetDevice(c->device);
    const uint32_t W = c->camera.width, H = c->camera.height;
    if (c->guides_valid && c->guides.ptr && c->guides.count >= 2u * size_t(W) * H) return HIPRZ_OK;
    RZ_HIP(c, c->guides.resize(2u * size_t(W) * H));
    RZ_LAUNCH(rz_guide_kernel, dim3((W + 31u) / 32u, (H + 7u) / 8u), dim3(256), 0, c->stream, c->dscene, c->dcamera, make_config(c), c->guides.ptr);
    RZ_HIP(c, hipGetLastError());
    c->guides_valid = true;
    return HIPRZ_OK;
}

}  // namespace hiprz

using namespace hiprz;

extern "C" {

int hiprz_render_guides(hiprz_ctx* c) {
    if (!c) return HIPRZ_ERR_INVALID;
    c->guides_valid = false;
    return ensure_guides(c);
}

int hiprz_read_guides(hiprz_ctx* c, hiprz_guide* dst, size_t bytes) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (c->have_camera && (!dst || bytes != size_t(c->camera.width) * c->camera.height * sizeof(hiprz_guide)))
        return fail(c, HIPRZ_ERR_INVALID, "read guides: destination size mismatch");
    if (const int rc = ensure_guides(c); rc != HIPRZ_OK) return rc;
    RZ_HIP(c, hipMemcpyAsync(dst, c->guides.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return HIPRZ_OK;
}

int hiprz_guides_device(hiprz_ctx* c, const void** out) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!out) return fail(c, HIPRZ_ERR_INVALID, "guides_device: null output");
    if (const int rc = ensure_guides(c); rc != HIPRZ_OK) return rc;
    *out = c->guides.ptr;
    return HIPRZ_OK;
}

}  // extern "C"
