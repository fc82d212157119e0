/* hiprz_light.h — light baking: the shadowed direct light of the scene's own lights per surface point, sampled, walked and summed on the
 * device (libhiprz_light.so).
 *
 * An occlusion bake (include/hiprz_bake.h) answers how much of the hemisphere a point sees.  A lightmap also needs the direct light of the
 * spot and direct lights of the scene with their shadows.  Those lights are on the device already (hiprz_device_view); this library reads
 * 32 bytes per POINT, makes K shadow rays per (point, light) from a table of disk samples, walks them with the query's occlusion walk
 * and writes 16 bytes per point: the light that arrives and how many rays were shadowed.  A library of its own for the reasons the other
 * six are: their kernel sets and exports are pinned, and a caller that never bakes light runs no code of this library.  It links against
 * libhiprz.so alone.  It reads the context through hiprz_device_view (include/hiprz.h) on EVERY call and caches nothing an upload could
 * make stale: a bake after hiprz_update_shading or hiprz_update_instances sees the change.
 *
 * Every rule below is plain float32, one rounding per operation (no fused multiply-add), true division and square root; the device
 * evaluates no sine, cosine, arc cosine or exponential.  dot(a, b) = (a.x*b.x + a.y*b.y) + a.z*b.z, magnitude(a) = sqrtf(dot(a, a)),
 * normalized(a) = a * (1.0f / magnitude(a)), similarity(a, b) = dot(a, b) * ((1.0f / magnitude(a)) * (1.0f / magnitude(b))): the device
 * functions of the renderer.  pi_f = 3.14159265358979323846f.
 *
 * THE POINT: a hiprz_bake_point, 32 bytes, the layout and the validity rule of hiprz_bake.h — position, near_, normal, far_; INVALID exactly
 * when the ray (position, near_, normal, far_) is invalid under HIPRZ_QUERY_NORMALIZE (the query's own device function decides).  n is
 * the normalised normal.  An invalid point walks no ray and affects no other point.
 *
 * THE SAMPLES: S sets (1 <= S <= 64) of K points (x, y) of the unit disk, set-major, S*K float2.  K is a power of two in 1 .. 1024; K = 1
 * gives hard shadows.  Every value must be finite and (x*x + y*y) <= 1.0f in float32.
 *
 * THE SET OF A POINT: point i uses set hiprz_bake_hash(i ^ seed) % S, on uint32_t
 *     x ^= x >> 16;  x *= 0x7feb352du;  x ^= x >> 15;  x *= 0x846ca68bu;  x ^= x >> 16;
 * (hiprz_light_set_of is the same on the host).
 *
 * THE LIGHTS are taken in this order: the selected spot lights by index, then the selected direct lights by index; L of them.  The fields
 * are the device records' as the renderer's direct_illumination reads them: the colour per component u8 / 255.0f, emission, size,
 * cos_angle, cos_angular_size.  A hiprz_light_range selects a sub-range of either kind: NULL selects every light, a count of
 * HIPRZ_LIGHT_TO_END (0xFFFFFFFF) means "to the end", first > the number of lights or first + count > it is HIPRZ_ERR_INVALID.  Per-light
 * maps for switchable lights are one call per range.
 *
 * THE FRAME of a unit vector a (Duff et al.), with the parenthesisation of hiprz_bake.h:
 *     s = copysignf(1, a.z);   e = -1.0f / (s + a.z);   b = (a.x * a.y) * e;
 *     t  = ( 1.0f + ((s * a.x) * a.x) * e,   s * b,                   (-s) * a.x );
 *     bt = ( b,                              s + (a.y * a.y) * e,     -a.y       );
 *
 * A SPOT LIGHT (lpos, ldir, size, cos_angle), sample (x, y), per component c where a vector is built:
 *     vOP = lpos - position;   a = normalized(vOP);   (t, bt) the frame of a
 *     q.c = lpos.c + ((t.c * x + bt.c * y) * size);   vPL = q - position;   dPL = magnitude(vPL);   w3 = normalized(vPL)   ("omega")
 *     c = dot(n, w3);   A = (size * size) * pi_f;   d1 = dPL + 1.0f
 *     inside = cos_angle < similarity(-vPL, ldir)
 *     w = c * (A / (d1 * d1))  when c > 0 and inside, else +0
 * the disk the reference's spotLightSampleDirection samples, with the reference's SolidAngle and BeamIllumination; the table supplies
 * (r cos phi, r sin phi).  The shadow ray: origin = position, near_ = the point's, direction = w3, far_ = dPL.
 *
 * A DIRECT LIGHT (ldir, cos_angular_size = ca), sample (x, y):
 *     a = -ldir;   (t, bt) the frame of a;   r2 = x * x + y * y;   z = 1.0f - r2 * (1.0f - ca)
 *     h = sqrtf(fmaxf(0.0f, 1.0f - z * z));   g = r2 > 0 ? h / sqrtf(r2) : 0
 *     d.c = (t.c * (x * g) + bt.c * (y * g)) + a.c * z;   w3 = normalized(d);   c = dot(n, w3)
 *     w = c * ((2.0f * pi_f) * (1.0f - ca))  when c > 0, else +0
 * a uniform disk gives a direction uniform on the cap: the distribution of the reference's sample_sphere(u1, u2 * 0.5 * (1 - cos)).  The
 * shadow ray: origin = position, near_ and far_ = the point's, direction = w3.
 *
 * For either kind w is +0 as well — the sample is SKIPPED — when a component of w3, the ray's far_ or w itself is not finite (a light at
 * the point), when w is not greater than 0 (size 0, angular size 0), or when the light's emission is not greater than 0.  A skipped
 * sample walks nothing, adds +0 and is never counted.  Every other ray is walked WITHOUT HIPRZ_QUERY_NORMALIZE by the query's occlusion
 * (the same device function), so its verdict is hiprz_query_occluded's on the same ray by construction, the invalid-ray rule included:
 * a ray with an empty range, near_ >= dPL for one, counts as not occluded.
 *
 * THE RESULT, 16 bytes, one store.  Per lane and colour component: lane j = k % 64 starts at +0; the lights run in order and, within a
 * light, the rounds r = 0, 1, ... of sample k = 64 r + j in order; each step is
 *     acc = acc + (skipped or occluded ? 0.0f : ((colour.c * emission) * w))
 * then for off = 1, 2, 4, ..., min(K, 64) / 2 every lane does v = v + v[lane ^ off], then light.c = v * (1.0f / float(K)).  `shadowed`
 * is the exact number of walked rays found occluded.  An invalid point reads light = +0 and shadowed = HIPRZ_LIGHT_INVALID.  With no
 * selected light light is +0 and shadowed 0; in an empty world light is the unshadowed sum and shadowed 0.
 *
 * THE MEANING: for a surface of reflectance 0 and opacity 0 (the brdf is then max(dot(n, w3), 0)), surface colour x light is the
 * reference's light-sampled next-event term Le with Lw = 1, summed over all selected lights where the reference picks one at random and
 * divides by the probability.  Left out on purpose:
 *   - the reference's `radiance < 1e-4` cut-off: a bake keeps dim light;
 *   - the world material's scattering factor: it is an expf, and a bake is of surfaces in a clear medium;
 *   - the coloured shadow mask of the CUDA-compatible mode: a shadow is 0 or 1;
 *   - the BRDF-sampled term Se (a path that happens to run into the light): a bake samples lights only.
 * Rendered frames are no yardstick for this quantity: the reference weights its two strategies with an unnormalised pdf.
 *
 * THE KERNELS, 64 threads per workgroup (one wave), no LDS, no atomics.  rz_light_bake_kernel: for K >= 64 one wave bakes one point in
 * K / 64 rounds per light; for K < 64 one wave bakes 64 / K consecutive points, one sample per lane and light.  The light loop's trip
 * count comes from kernel arguments alone and a light's record is a wave-uniform load; lanes that are out of range, invalid or skipped
 * take part in every ballot and shuffle.  rz_light_rays_kernel: one thread per (point, light, sample) writes ray (i * L + l) * K + k as
 * a hiprz_ray — the ray the bake walks — and w into a float array; the ray of an invalid point or a skipped sample is (position, near_,
 * direction +0, the point's far_), which the query flags invalid, with w = +0. */
#ifndef HIPRZ_LIGHT_H
#define HIPRZ_LIGHT_H

#include <stddef.h>
#include <stdint.h>

#include "hiprz_bake.h" /* hiprz_bake_point; hiprz_query.h: hiprz_ray; hiprz.h: hiprz_ctx, the return codes */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiprz_light_texel {
    float light[3];
    uint32_t shadowed;
} hiprz_light_texel; /* 16 B */

typedef struct hiprz_light_range {
    uint32_t spot_first, spot_count;
    uint32_t direct_first, direct_count;
} hiprz_light_range; /* 16 B */

#define HIPRZ_LIGHT_INVALID 0x80000000u
#define HIPRZ_LIGHT_TO_END 0xFFFFFFFFu

/* Bound to one context and answering on its head device.  It owns the sample table and the pinned staging of the host-pointer call, grown
 * on demand.  One call at a time per handle.  HIPRZ_ERR_DEVICE without a HIP device.  Destroy it before its context. */
typedef struct hiprz_light hiprz_light;
int hiprz_light_create(hiprz_light** out, hiprz_ctx* ctx);
int hiprz_light_destroy(hiprz_light* light);
const char* hiprz_light_last_error(const hiprz_light* light); /* NULL: the last error of a call without a handle, on this thread */

/* S*K float2 (x, y) from the host, checked against THE SAMPLES above (HIPRZ_ERR_INVALID, the table before stays).  The handle keeps the
 * table; it reaches the device with the next call below, on that call's stream, once the context's device is known from a view.  That one
 * call waits for its stream (the copy reads pageable memory); every later call with the same table only enqueues. */
int hiprz_light_set_samples(hiprz_light* light, const float* xy_host, uint32_t K, uint32_t S);

/* Host only, pure.  The set of point i: hiprz_bake_hash(i ^ seed) % S; 0 when S == 0. */
uint32_t hiprz_light_set_of(uint32_t i, uint32_t seed, uint32_t S);

/* Host only, pure, computed in double: S*K float2.  For set s and sample k: r = sqrt((k + 0.5) / K),
 * phi = 2 pi (frac(k * 0.6180339887498949) + s / S), (x, y) = (r cos phi, r sin phi) rounded to float (r*r <= 1 - 1/2048: the
 * rounding leaves no sample outside the disk).  HIPRZ_ERR_INVALID on a K or S that hiprz_light_set_samples refuses, or a null pointer. */
int hiprz_light_disk_samples(uint32_t K, uint32_t S, float* xy_out);

/* Every call that takes a `stream` (a hipStream_t) only enqueues; NULL = hiprz_stream(ctx).  Device arrays are 16-byte aligned (the
 * weights 4-byte).  Entries past n (past n*L*K for the rays and weights) are never written; n == 0 is HIPRZ_OK without a view or a
 * launch.  Refused before anything is launched or copied, in this order: a null handle or pointer (HIPRZ_ERR_INVALID; `range` may be
 * null), no sample table set (HIPRZ_ERR_STATE), n*K >= 2^31 (HIPRZ_ERR_INVALID), whatever hiprz_device_view refuses (a context without
 * a scene: HIPRZ_ERR_STATE), a range outside the view's lights (HIPRZ_ERR_INVALID) and, for the rays, whose L is known only from the
 * view, n*L*K >= 2^31 (HIPRZ_ERR_INVALID). */
int hiprz_light_bake(hiprz_light* light, const hiprz_bake_point* points_device, size_t n, uint32_t seed, const hiprz_light_range* range,
                     hiprz_light_texel* out_device, void* stream);
int hiprz_light_rays(hiprz_light* light, const hiprz_bake_point* points_device, size_t n, uint32_t seed, const hiprz_light_range* range,
                     hiprz_ray* rays_out_device, float* weights_out_device, void* stream);

/* The bake for host pointers: copied through the handle's pinned staging on the context's stream, which is waited for once. */
int hiprz_light_bake_host(hiprz_light* light, const hiprz_bake_point* points, size_t n, uint32_t seed, const hiprz_light_range* range,
                          hiprz_light_texel* out);

/* The lights a call with `range` would work on now: *spots spot lights, then *directs direct lights (L is their sum), from the context's
 * device view of this call.  No table is needed.  HIPRZ_ERR_INVALID on a null handle or output, whatever hiprz_device_view refuses, then
 * HIPRZ_ERR_INVALID on a range outside the view's lights.  The way to size the arrays of hiprz_light_rays. */
int hiprz_light_count(hiprz_light* light, const hiprz_light_range* range, uint32_t* spots, uint32_t* directs);

/* sizeof(hiprz_bake_point), sizeof(hiprz_light_texel), sizeof(hiprz_light_range) and the offsets of hiprz_light_texel::light,
 * ::shadowed and hiprz_light_range::direct_first as this library was compiled */
void hiprz_light_layout(uint32_t out[6]);

#ifdef __cplusplus
}
#endif
#endif
