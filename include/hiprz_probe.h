/* hiprz_probe.h — probe baking: the light that arrives at a point of free space from all directions, gathered on the device into nine
 * spherical-harmonic (SH) coefficients per colour (libhiprz_probe.so).
 *
 * The bake pipeline (include/hiprz_atlas.h, hiprz_bake.h, hiprz_light.h, hiprz_gather.h) lights surfaces that are in an atlas.  A moving
 * object, a character or a mesh too small to unwrap has nothing to read there.  A light PROBE fills that gap: a point in free space that
 * stores the light arriving from all directions as nine SH coefficients per colour, evaluated by a shader or a host for any normal.  This
 * library reads 32 bytes per PROBE, makes the probe's K rays from a table of directions over the whole sphere, walks each to its CLOSEST
 * hit, finds the atlas texel under the hit through a chart map the caller has set, and writes 144 bytes per probe; a second call adds the
 * scene's own lights with their shadows.  Neither the rays nor their hits exist in memory.  A library of its own for the reasons the other
 * eight are: their kernel sets and exports are pinned, and a caller that never bakes probes runs no code of this library.  It links against
 * libhiprz.so alone.  It reads the context through hiprz_device_view (include/hiprz.h) on EVERY call and caches nothing an upload could
 * make stale: a bake after hiprz_update_instances sees the change.  What it needs of the gather's walk and lookup and of the light's
 * sampling it restates.
 *
 * Every rule below is plain float32, one rounding per operation (no fused multiply-add), true division and square root; the device
 * evaluates no sine, cosine, arc cosine or exponential.  dot, magnitude, normalized, similarity and pi_f are those of hiprz_light.h.
 *
 * THE PROBE: a hiprz_bake_point, 32 bytes, the layout and the validity rule of hiprz_bake.h — position, near_, normal, far_; INVALID exactly
 * when the ray (position, near_, normal, far_) is invalid under HIPRZ_QUERY_NORMALIZE.  `position` is where the probe sits.  `normal` is
 * only the axis of the probe's frame: with the per-probe set it decorrelates neighbouring probes.  near_ and far_ are the rays' range.
 * An invalid probe walks no ray and affects no other probe.
 *
 * THE DIRECTIONS, THE SET OF A PROBE, THE FRAME and THE RAY are those of hiprz_bake.h, restated as hiprz_gather.h restates them: S sets
 * (1 <= S <= 64) of K unit directions in the local frame, S*K float4 (x, y, z, ignored), set-major; K is one of 16, 32, 64, 128, 256,
 * 512, 1024; every component finite and the float32 squared length (x*x + y*y) + z*z in [0.999, 1.001] — z may be negative, the table
 * rule never asked otherwise.  Probe i uses set hiprz_bake_hash(i ^ seed) % S, on uint32_t
 *     x ^= x >> 16;  x *= 0x7feb352du;  x ^= x >> 15;  x *= 0x846ca68bu;  x ^= x >> 16;
 * The frame of the normalised normal n (Duff et al.):
 *     s = copysignf(1, n.z);   a = -1.0f / (s + n.z);   b = (n.x * n.y) * a;
 *     t  = ( 1.0f + ((s * n.x) * n.x) * a,   s * b,                   (-s) * n.x );
 *     bt = ( b,                              s + (n.y * n.y) * a,     -n.y       );
 * and the world direction of the table's l, per component c:
 *     d.c = (t.c * l.x + bt.c * l.y) + n.c * l.z
 * The ray of (probe i, direction k) is origin = position, near_, direction = d, far_: the ray hiprz_bake_rays and hiprz_gather_samples
 * make for the same table and seed, bit for bit.  hiprz_probe_sphere_directions is the intended table, uniform on the whole sphere.
 *
 * THE BASIS, evaluated on a direction d as made, not renormalised:
 *     B0 = 1          B1 = d.y          B2 = d.z          B3 = d.x          B4 = d.x*d.y          B5 = d.y*d.z
 *     B6 = (3.0f*(d.z*d.z)) - 1.0f      B7 = d.x*d.z      B8 = (d.x*d.x) - (d.y*d.y)
 * the real SH functions up to band 2 without their normalisation constants: those live in THE EVALUATION, so the stored numbers are
 * plain means.
 *
 * THE GATHERED TERM (hiprz_probe_gather) takes hiprz_gather.h's chart map (hiprz_gather_chart, one uint32_t base per instance,
 * HIPRZ_GATHER_NONE for an instance outside the atlas), its W x H source of 16-byte records (a texel HAS A VALUE when its word is not
 * 0x80000000) and sky[3].  The walk is the closest-hit walk of hiprz_query_closest WITHOUT HIPRZ_QUERY_NORMALIZE; the chart id of a hit on
 * instance I and mesh triangle T is base[I] + T (on 64 bits; an id >= n_charts is unmapped); THE LOOKUP of a front-face hit is
 *     b1 = (1.0f - bx) - by
 *     u  = (u1 * b1 + u2 * bx) + u3 * by          v = (v1 * b1 + v2 * bx) + v3 * by
 *     x  = clamp(int(floorf(u * float(W))), 0, W - 1)          y = clamp(int(floorf(v * float(H))), 0, H - 1)
 * (the clamp taken on the float; a u or v that is not finite is unmapped).  Ray k contributes L by the gather's rule, byte for byte: sky
 * for a miss or an invalid ray (MISSED), the texel's RGB for a front-face hit whose texel has a value (READ), +0 otherwise (counted
 * nowhere).  Per lane j = k % 64, per coefficient b and colour c, from +0, for rounds r = 0, 1, ... of ray k = 64 r + j:
 *     acc[b].c = acc[b].c + (L.c * B_b)
 * then for off = 1, 2, 4, ..., min(K, 64) / 2 every lane does v = v + v[lane ^ off] (the order hiprz_bake.h fixes for `bent`), then
 * m[b].c = v * (1.0f / float(K)).  The order does not depend on where the running sums are held.
 *
 * THE RECORD, hiprz_probe_sh, 144 bytes: float4 sh[9], written as nine 16-byte stores.  .xyz holds m[b].  sh[0].w holds the gather's count
 * word: READ in bits 0 - 15, MISSED in bits 16 - 30.  sh[1].w holds the light term's count of shadowed rays (0 from the gather).  The
 * other seven .w words are 0.  An invalid probe reads all +0 with sh[0].w = HIPRZ_PROBE_INVALID (0x80000000).
 *
 * THE LIGHT TERM (hiprz_probe_light) has hiprz_light.h's sample table (S sets of K points of the unit disk, K a power of two in 1 .. 1024,
 * set hiprz_bake_hash(i ^ seed) % S of that table's S), its light order (the selected spot lights by index, then the direct lights) and
 * its hiprz_light_range.  Per (light, sample) the rules of hiprz_light.h give q, vPL, dPL, w3, the beam test and the shadow ray, with the
 * cosine taken out:
 *     w = A / (d1 * d1)                      for a spot light when inside the beam, else +0   (A = (size * size) * pi_f, d1 = dPL + 1.0f)
 *     w = (2.0f * pi_f) * (1.0f - ca)        for a direct light
 * the `c > 0` test is dropped; every other skip rule holds as written: a sample is SKIPPED when a component of w3, the ray's far_ or w is
 * not finite, when w is not greater than 0 or when the light's emission is not greater than 0.  The shadow ray (origin = position, the
 * probe's near_, direction = w3, far_ = dPL for a spot light and the probe's far_ for a direct light) is walked WITHOUT
 * HIPRZ_QUERY_NORMALIZE by the query's occlusion function.  An unskipped, unoccluded sample adds
 *     acc[b].c = acc[b].c + (P.c * B_b(w3))          P.c = ((colour.c * emission) * w) * 0.25f
 * with the lights in order and, within a light, the rounds in order (the light bake's order), then the butterfly, then
 * light[b].c = v * (1.0f / float(K)).  The call takes a nullable `base` array of records:
 *     out.sh[b].c = base.sh[b].c + light[b].c          out.sh[0].w = base.sh[0].w          out.sh[1].w = the number of shadowed rays
 * without `base` the sum is +0 + light[b].c and sh[0].w is 0.  `out` may be `base`.  An invalid probe, or a `base` record that is
 * invalid (sh[0].w == HIPRZ_PROBE_INVALID), writes the invalid record.  With `base` a probe is complete in two launches and never
 * visits the host.
 *
 * THE MEANING and THE EVALUATION.  hiprz_probe_irradiance evaluates, per colour c and for a unit normal n,
 *     E.c(n) = sum over b of w_b * sh[b].c * B_b(n)          w = {1, 2, 2, 2, 15/4, 15/4, 5/16, 15/4, 15/16}
 * in float32 as e = +0; for b = 0 .. 8 in order: e = e + ((w_b * sh[b].c) * B_b(n)), the weights the float32 constants 1.0f, 2.0f, 3.75f,
 * 0.3125f, 0.9375f.  For a probe with both terms E(n) approximates hiprz_light_texel::light + hiprz_gather_texel::mean of a surface point
 * at the probe's position with normal n: the quantity a lightmap texel holds, so a dynamic object beside a baked wall is lit in the same
 * units.  The weights are the clamped-cosine band factors (pi, 2 pi / 3, pi / 4) times the squared SH constants times 4 (4 pi because a
 * stored number is a mean over the sphere and not an integral, over the pi of the irradiance convention); the 0.25f
 * of the light term makes a delta light fit the same weights.  A band-limited radiance reproduces (1 / pi) * integral of L max(0, n.w) dw;
 * a delta light along n reads 1.0625 of its true value, the known overshoot of the band-2 clamped cosine.
 *
 * THE SAMPLES: hiprz_probe_samples writes what the gather walks, one hiprz_gather_sample {id, bx, by, t} per (probe i, direction k) at
 * i * K + k, made by the device function the gather call itself uses, with the codes of hiprz_gather.h.
 *
 * Left out on purpose:
 *   - bands above 2;
 *   - ringing windowing: the coefficients are the plain projection;
 *   - probe placement and visibility: a probe inside geometry sees back faces (+0), a probe behind a wall leaks through a plain
 *     interpolation — include/hiprz_field.h bakes a visibility map per probe and weights the blend by it, include/hiprz_place.h moves
 *     probes out of geometry before either bake;
 *   - glossy transport, transmission and the scattering medium, as the gather leaves them out;
 *   - a device-side evaluation kernel: the evaluation is nine multiply-adds a shader writes itself; the lookup of a whole grid of
 *     probes for shaded points on the device is include/hiprz_field.h's.
 *
 * THE KERNELS, 64 threads per workgroup (one wave), no atomics.  rz_probe_gather_kernel and rz_probe_light_kernel have the shapes of
 * rz_gather_kernel and rz_light_bake_kernel: for K >= 64 one wave takes one probe in K / 64 rounds (per light); for K < 64 one wave takes
 * 64 / K consecutive probes; lanes that are out of range, invalid or skipped take part in every ballot and shuffle.  A lane carries 27
 * running sums.  The gather kernel holds them in LDS, acc[b * 3 + c][lane], 6 912 bytes per wave: each lane touches its own column only,
 * so no barrier is needed and no two lanes share a bank; the light kernel, whose walk is the lighter occlusion walk, holds them in
 * registers.  Either kernel can be built the other way (-DRZ_PROBE_GATHER_IN_LDS=0, -DRZ_PROBE_LIGHT_IN_LDS=1) and then writes the same
 * bytes.  rz_probe_samples_kernel: one thread per (probe, k). */
#ifndef HIPRZ_PROBE_H
#define HIPRZ_PROBE_H

#include <stddef.h>
#include <stdint.h>

#include "hiprz_gather.h" /* hiprz_gather_chart, hiprz_gather_sample, the codes; hiprz_bake.h: hiprz_bake_point */
#include "hiprz_light.h"  /* hiprz_light_range */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiprz_probe_sh {
    float sh[9][4]; /* [b]: m[b].rgb and a word; [0][3]: READ | MISSED << 16 or HIPRZ_PROBE_INVALID, [1][3]: shadowed rays, else 0 */
} hiprz_probe_sh; /* 144 B */

#define HIPRZ_PROBE_INVALID 0x80000000u
#define HIPRZ_PROBE_MAX_SIZE 16384u

/* Bound to one context and answering on its head device.  It owns the two tables, the chart map, the device copies of a host source and
 * the pinned staging of the host-pointer calls, grown on demand.  One call at a time per handle.  HIPRZ_ERR_DEVICE without a HIP device.
 * Destroy it before its context. */
typedef struct hiprz_probe hiprz_probe;
int hiprz_probe_create(hiprz_probe** out, hiprz_ctx* ctx);
int hiprz_probe_destroy(hiprz_probe* probe);
const char* hiprz_probe_last_error(const hiprz_probe* probe); /* NULL: the last error of a call without a handle, on this thread */

/* S*K float4 (x, y, z, ignored) from the host, checked as hiprz_bake_set_directions checks them; S*K float2 checked as
 * hiprz_light_set_samples checks them; the chart map checked as hiprz_gather_set_charts checks it (HIPRZ_ERR_INVALID, what was set before
 * stays).  The handle keeps them; they reach the device with the next call that needs them, on that call's stream, which that one call
 * waits for. */
int hiprz_probe_set_directions(hiprz_probe* probe, const float* xyz0_host, uint32_t K, uint32_t S);
int hiprz_probe_set_samples(hiprz_probe* probe, const float* xy_host, uint32_t K, uint32_t S);
int hiprz_probe_set_charts(hiprz_probe* probe, const uint32_t* base_host, uint32_t n_instances, const hiprz_gather_chart* uv_host, uint32_t n_charts);

/* Host only, pure, computed in double and rounded to float: S*K float4 (x, y, z, 0) uniform on the whole sphere.  For set s and
 * direction k: z = 1 - 2 (k + 0.5) / K, phi = 2 pi (frac(k * 0.6180339887498949) + s / S), (r cos phi, r sin phi, z) with
 * r = sqrt(1 - z * z).  HIPRZ_ERR_INVALID on a K or S that hiprz_probe_set_directions refuses, or a null pointer. */
int hiprz_probe_sphere_directions(uint32_t K, uint32_t S, float* xyz0_out);

/* Host only, pure float32: THE EVALUATION of one record for the unit normal n.  An invalid record or a null pointer writes nothing that
 * is not +0 (out, when not null, reads +0). */
void hiprz_probe_irradiance(const hiprz_probe_sh* sh, const float n[3], float out[3]);

/* Every call that takes a `stream` (a hipStream_t) only enqueues; NULL = hiprz_stream(ctx).  Device arrays are 16-byte aligned.  Entries
 * past n (past n*K for the samples) are never written; n == 0 is HIPRZ_OK without a view or a launch.  Refused before anything is
 * launched or copied, in this order: a null handle or pointer (HIPRZ_ERR_INVALID; `base` and `range` may be null), no direction table or
 * no chart map set — for the light term no sample table set — (HIPRZ_ERR_STATE), n*K >= 2^31 (HIPRZ_ERR_INVALID), for the gather a W or
 * H outside 1 .. HIPRZ_PROBE_MAX_SIZE (HIPRZ_ERR_INVALID), whatever hiprz_device_view refuses (a context without a scene:
 * HIPRZ_ERR_STATE), a chart map for another number of instances than the view's or a range outside the view's lights
 * (HIPRZ_ERR_INVALID). */
int hiprz_probe_gather(hiprz_probe* probe, const hiprz_bake_point* probes_device, size_t n, uint32_t seed, const void* source16_device, uint32_t W, uint32_t H,
                       const float sky[3], hiprz_probe_sh* out_device, void* stream);
int hiprz_probe_samples(hiprz_probe* probe, const hiprz_bake_point* probes_device, size_t n, uint32_t seed, hiprz_gather_sample* samples_out_device,
                        void* stream);
int hiprz_probe_light(hiprz_probe* probe, const hiprz_bake_point* probes_device, size_t n, uint32_t seed, const hiprz_light_range* range,
                      const hiprz_probe_sh* base_device, hiprz_probe_sh* out_device, void* stream);

/* The two terms for host pointers, the source and the base included: the probes and records go through the handle's pinned staging on the
 * context's stream, which is waited for; the source goes to a device copy the handle owns.  `out` may be `base`. */
int hiprz_probe_gather_host(hiprz_probe* probe, const hiprz_bake_point* probes, size_t n, uint32_t seed, const void* source16, uint32_t W, uint32_t H,
                            const float sky[3], hiprz_probe_sh* out);
int hiprz_probe_light_host(hiprz_probe* probe, const hiprz_bake_point* probes, size_t n, uint32_t seed, const hiprz_light_range* range,
                           const hiprz_probe_sh* base, hiprz_probe_sh* out);

/* sizeof(hiprz_bake_point), sizeof(hiprz_probe_sh), sizeof(hiprz_gather_sample), sizeof(hiprz_gather_chart) and the offsets of
 * hiprz_probe_sh::sh[0][3] and ::sh[1][3] as this library was compiled */
void hiprz_probe_layout(uint32_t out[6]);

#ifdef __cplusplus
}
#endif
#endif
