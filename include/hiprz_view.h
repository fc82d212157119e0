/* hiprz_view.h — baked view: a frame of the selected camera shaded from a lit atlas and a probe field (libhiprz_view.so).
 *
 * The bake libraries end in arrays: a lit atlas (include/hiprz_light.h, hiprz_gather.h, hiprz_atlas.h) and a grid of probes
 * (include/hiprz_probe.h, hiprz_field.h, hiprz_place.h).  This library is their consumer.  One thread per pixel casts the pixel-centre ray,
 * walks it to its closest hit, finds the atlas texel under a hit on a mapped object through the gather's chart map — or, for an object that
 * is not in the atlas, looks the probe field up at the hit and multiplies by the surface colour — and writes 16 bytes per pixel, a float4
 * image, or both.  Neither the ray (32 bytes) nor its hit (48 bytes) exists in memory.  A library of its own for the reasons the other
 * twelve are: their kernel sets and exports are pinned, and a caller that never views runs no code of this library.  It links against
 * libhiprz.so alone.  It reads the context through hiprz_device_view (include/hiprz.h) on EVERY call that walks and caches nothing an
 * upload could make stale: a view after hiprz_update_instances sees the change.  What it needs of the gather's lookup and of the field's
 * lookup it restates.
 *
 * Every rule below is plain float32, one rounding per operation (no fused multiply-add), true division and square root; the device
 * evaluates no power, exponential or trigonometric function.
 *
 * THE PIXEL AND ITS RAY: pixel (x, y) of the selected camera's W_c x H_c frame, record y * W_c + x, casts the ray hiprz_query_pixel_rays
 * writes for it, bit for bit (the first pass's pixel-centre ray).  It is walked WITHOUT HIPRZ_QUERY_NORMALIZE by the closest-hit walk of
 * hiprz_query_closest (the same device function, ties included), so t, the instance, the triangle and the side are that call's on the same
 * ray by construction, the invalid-ray rule included.
 *
 * THE CHART MAP AND THE SOURCE are hiprz_gather.h's: one uint32_t `base` per instance, HIPRZ_GATHER_NONE for an instance outside the
 * atlas; one hiprz_gather_chart per id; a hit on instance I and mesh triangle T has id base[I] + T (64-bit sum), unmapped when it is
 * >= n_charts.  The source is W x H 16-byte records, row-major, RGB and a word: what a texel sends on,
 * albedo x (direct + indirect) + emission, composed and dilated as hiprz_gather_compose and hiprz_atlas_dilate leave it.  A texel HAS A
 * VALUE when its word is not 0x80000000.  1 <= W, H <= 16384.
 *
 * A FRONT-FACE HIT ON A MAPPED ID, with the walk's bx and by:
 *     b1 = (1.0f - bx) - by
 *     u  = (u1 * b1 + u2 * bx) + u3 * by          v = (v1 * b1 + v2 * bx) + v3 * by
 * A u or v that is not finite reads kind NONE.  Then the params decide.
 *   HIPRZ_VIEW_NEAREST (0): the gather's texel by the gather's formula,
 *     x = clamp(int(floorf(u * float(W))), 0, W - 1)          y = clamp(int(floorf(v * float(H))), 0, H - 1)
 *   (the clamp taken on the float): a view pixel equals what a gather ray hitting the same place reads.  One tap.
 *   HIPRZ_VIEW_BILINEAR (1): the atlas library's texel space, texel centres at half-integers,
 *     gx = u * float(W) - 0.5f          x0 = int(floorf(gx))          fx = gx - floorf(gx)          (gy, y0, fy likewise with H)
 *   the conversion taken on floorf(gx) clamped to [-1, W].  Four taps in the order (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1), with
 *     w = wx * wy          wx = 1.0f - fx for x0 and fx for x0 + 1          wy likewise
 *   A tap outside the atlas or without a value is LEFT OUT; for the others, in that order,
 *     acc.c = acc.c + (w * rgb.c)          sw = sw + w
 *   and the result is acc.c / sw when sw > 0.
 * The kind is ATLAS and the word's low bits count the taps used (1 for nearest); when no tap has a value — or sw is not > 0 — the kind is
 * NONE and the RGB +0.  A hit on a mapped id fetches no material.
 *
 * A FRONT-FACE HIT ON AN UNMAPPED INSTANCE OR ID is kind FIELD when a field is given (hiprz_view_field: the grid, probes, records,
 * optional visibility records and params of hiprz_field.h).
 *     p.c = o.c + (t * d.c)          n = the hit's Surface::mapped_normal facing the ray — the bytes of hiprz_hit::normal
 *   E and the probe count are what hiprz_field_lookup writes for the point (p, n), byte for byte (include/hiprz_field.h §2, restated in
 *   this library: the cell, the corners 0 .. 7, the probes left out, the Chebyshev weights and hiprz_probe.h's evaluation).
 *   The surface is the renderer's: analyze_intersection with textures and the reference's colour rule — the material's colour bytes / 255,
 *   or its texture's texel at the hit's texture coordinates; emission the material's, or its emission map's texel.  Then
 *     rgb.c = color.c * E.c          where emission > 0:  rgb.c = (color.c * E.c) + (color.c * emission)
 *   (the term the first pass adds for an emitting hit).  The word's low bits are the probes counted.  The kind is NONE, RGB +0, when
 *   there is no field, when the lookup is invalid or when no probe is counted.
 *
 * EVERYTHING ELSE: a miss, an empty world or an invalid ray reads the call's sky[3], kind SKY; a back-face hit reads +0, kind BACK.
 * There are no invalid pixels other than through the ray rule.
 *
 * THE OUTPUTS, two W_c x H_c device arrays of which at least one is not null: hiprz_view_pixel, 16 bytes — the RGB and
 * word = kind << 28 | count — and a float4 image (r, g, b, 1.0f), the layout hiprz_tonemap_image turns into RGBA8 and hiprz_denoise_image
 * takes as an accumulator.  This library has no tone map of its own.
 *
 * THE SAMPLES: hiprz_view_samples writes what the view walks, one hiprz_gather_sample {id, bx, by, t} per pixel with the gather's codes
 * (HIPRZ_GATHER_MISS, _UNMAPPED, _BACK, _INVALID_RAY), from the device function the view kernel itself calls.
 *
 * Left out on purpose:
 *   - supersampling and depth of field: one pixel-centre ray per pixel;
 *   - glossy, transmissive and scattering appearance: every surface is shown as a diffuse one, a hit ends the ray;
 *   - shadows cast by unmapped objects onto the atlas: the atlas holds what was baked;
 *   - mip-mapping of the atlas;
 *   - a headless task key.
 *
 * THE KERNELS, no LDS, no atomics, 64 threads per workgroup (one wave).  rz_view_kernel: one thread per pixel; a wave shades an 8 x 8
 * block of pixels, as the renderer's tiles do — lane l is pixel (8 bx + l % 8, 8 by + l / 8), blocks row-major, partial at the right and
 * bottom edges.  make VIEW_DEFS=-DRZ_VIEW_ROWS builds the row-major form of the query's kernels (thread i is pixel i), which writes the
 * same bytes.  rz_view_samples_kernel: one thread per pixel, the same mapping.
 *
 * MEASURED on an MI355X (tools/view_time.py, configs D and E at 1920 x 1080, a 1024 x 1024 source; DESIGN.md §6 "Baked view" and
 * profiles/r34 have the conditions), stated as measured, not as a promise: the atlas-only view takes 0.98 - 1.00 (D) and 0.85 (E) of
 * hiprz_query_closest over the same pixel rays already on the device, 1.00 (D) and 0.90 (E) with a quarter of the instances read from a
 * 16^3 field; the row-major build takes 1.00 - 1.06 and 1.03 - 1.11 of the query, so the 8 x 8 block ships.  rz_view_kernel: 93 VGPRs,
 * 44 bytes of scratch per lane, five waves per SIMD (four waves: the same time on D, 3 - 5 % later on E).  The numpy route through the host
 * takes 201 and 231 ms for the same frame. */
#ifndef HIPRZ_VIEW_H
#define HIPRZ_VIEW_H

#include <stddef.h>
#include <stdint.h>

#include "hiprz_field.h"  /* hiprz_field_grid, _vis, _params; hiprz_probe.h: hiprz_probe_sh; hiprz_bake.h: hiprz_bake_point */
#include "hiprz_gather.h" /* hiprz_gather_chart, hiprz_gather_sample and the codes */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiprz_view_pixel {
    float rgb[3];
    uint32_t word; /* kind << 28 | count */
} hiprz_view_pixel; /* 16 B */

typedef struct hiprz_view_params {
    uint32_t filter; /* HIPRZ_VIEW_NEAREST or HIPRZ_VIEW_BILINEAR */
    uint32_t reserved[3]; /* 0 */
} hiprz_view_params; /* 16 B */

/* the field of a call: `grid` and `params` are host pointers in both calls (params null: bias 0, max_back 0); probes, sh and vis (which may
 * be null) are device pointers for hiprz_view_pixels and host pointers for hiprz_view_pixels_host */
typedef struct hiprz_view_field {
    const hiprz_field_grid* grid;
    const hiprz_bake_point* probes;
    const hiprz_probe_sh* sh;
    const hiprz_field_vis* vis;
    size_t n_probes;
    const hiprz_field_params* params;
} hiprz_view_field; /* 48 B */

#define HIPRZ_VIEW_NEAREST 0u
#define HIPRZ_VIEW_BILINEAR 1u
#define HIPRZ_VIEW_NONE 0u
#define HIPRZ_VIEW_ATLAS 1u
#define HIPRZ_VIEW_FIELD 2u
#define HIPRZ_VIEW_SKY 3u
#define HIPRZ_VIEW_BACK 4u
#define HIPRZ_VIEW_KIND_SHIFT 28u
#define HIPRZ_VIEW_COUNT_MASK 0x0FFFFFFFu

/* Bound to one context and answering on its head device.  It owns the chart map, the device copies of a host source and a host field and
 * the pinned staging of the host-pointer call, grown on demand.  One call at a time per handle.  HIPRZ_ERR_DEVICE without a HIP device.
 * Destroy it before its context. */
typedef struct hiprz_view hiprz_view;
int hiprz_view_create(hiprz_view** out, hiprz_ctx* ctx);
int hiprz_view_destroy(hiprz_view* view);
const char* hiprz_view_last_error(const hiprz_view* view); /* NULL: the last error of a call without a handle, on this thread */

/* THE CHART MAP from the host, the arguments and the checks of hiprz_gather_set_charts: refused with HIPRZ_ERR_INVALID, the map before
 * stays, are a null handle or pointer, n_charts > HIPRZ_GATHER_MAX_CHARTS, a UV that is not finite.  It reaches the device with the next
 * call below, on that call's stream, which that one call waits for.  A map equal in every byte to the one already set is not placed again:
 * setting the same map before every frame costs a comparison on the host, no allocation and no wait. */
int hiprz_view_set_charts(hiprz_view* view, const uint32_t* base_host, uint32_t n_instances, const hiprz_gather_chart* uv_host, uint32_t n_charts);

/* Host only, pure: HIPRZ_OK when a view takes the params (a known filter, reserved 0), else HIPRZ_ERR_INVALID */
int hiprz_view_check_params(const hiprz_view_params* params);

/* Every call that takes a `stream` (a hipStream_t) only enqueues; NULL = hiprz_stream(ctx).  Device arrays are 16-byte aligned.  `field`
 * may be null (no field), `params` may be null (HIPRZ_VIEW_NEAREST), one of `pixels_out_device` and `image_out_device` may be null.
 * Refused before anything is launched or copied, in this order: a null handle or pointer — the source, the sky, both outputs, a field
 * without grid, probes or records — (HIPRZ_ERR_INVALID), no chart map set (HIPRZ_ERR_STATE), a W or H outside 1 .. HIPRZ_GATHER_MAX_SIZE
 * (HIPRZ_ERR_INVALID), params hiprz_view_check_params refuses, a grid hiprz_field_check_grid refuses, field params
 * hiprz_field_check_params refuses (HIPRZ_ERR_INVALID), whatever hiprz_device_view refuses (a context without a scene or without a camera:
 * HIPRZ_ERR_STATE), more than 2^31 - 1 pixels (HIPRZ_ERR_INVALID; the camera is known from the view on), a chart map for another number
 * of instances than the view's (HIPRZ_ERR_INVALID).  A camera of no pixels is HIPRZ_OK without a launch.  hiprz_view_samples skips what
 * it has no argument for. */
int hiprz_view_pixels(hiprz_view* view, const void* source16_device, uint32_t W, uint32_t H, const hiprz_view_field* field, const float sky[3],
                      const hiprz_view_params* params, hiprz_view_pixel* pixels_out_device, void* image_out_device, void* stream);
int hiprz_view_samples(hiprz_view* view, hiprz_gather_sample* samples_out_device, void* stream);

/* The view for host pointers (the C++ Engine): the source and the field go to device copies the handle owns, the results come back through
 * its pinned staging on the context's stream, which is waited for.  Either output may be null, not both. */
int hiprz_view_pixels_host(hiprz_view* view, const void* source16, uint32_t W, uint32_t H, const hiprz_view_field* field, const float sky[3],
                           const hiprz_view_params* params, hiprz_view_pixel* pixels_out, void* image_out);

/* sizeof(hiprz_view_pixel), sizeof(hiprz_view_params), sizeof(hiprz_view_field), sizeof(hiprz_gather_sample), sizeof(hiprz_gather_chart),
 * the offset of hiprz_view_pixel::word, HIPRZ_VIEW_KIND_SHIFT, and 1 when this library was compiled with RZ_VIEW_ROWS, else 0 */
void hiprz_view_layout(uint32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
