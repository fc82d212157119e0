/* hiprz_field.h — probe fields: what makes a grid of baked probes usable (libhiprz_field.so).  Two things: a VISIBILITY MAP per probe — an
 * 8 x 8 octahedral map of the first two moments of the distance to the nearest surface, so that a probe records how far it can see in each
 * direction — and a LOOKUP on the device that blends the eight probes around a shaded point and weights each by a Chebyshev test of the
 * point's distance against that probe's map, so that a probe behind a wall does not leak through the interpolation (the scheme of the
 * dynamic-diffuse-global-illumination papers in PAPERS.md's lineage).
 *
 * include/hiprz_probe.h writes 144 bytes of band-2 spherical harmonics per probe and leaves the blend to the host (probe.Field.blend:
 * trilinear, straight through geometry).  This library adds the missing step.  It is a library of its own for the reasons the other nine
 * are: their kernel sets and exports are pinned, and a caller that never looks a field up runs no code of this library.  It links against
 * libhiprz.so alone.  The visibility bake reads the context through hiprz_device_view (include/hiprz.h) on EVERY call and caches nothing
 * an upload could make stale; the lookup needs no scene and takes no device view.  What it needs of the probe's frame, hash and ray it
 * restates.
 *
 * Every rule below is plain float32, one rounding per operation (no fused multiply-add), true division and square root; the device
 * evaluates no power, exponential or trigonometric function.
 *
 * ---------------------------------------------------------------------------------------------------------------------------------
 * 1. THE VISIBILITY BAKE (hiprz_field_visibility)
 *
 * THE PROBE is a hiprz_bake_point with the validity rule of hiprz_probe.h: INVALID exactly when the ray (position, near_, normal, far_)
 * is invalid under HIPRZ_QUERY_NORMALIZE.  THE DIRECTIONS, THE SET OF A PROBE, THE FRAME and THE RAY are those of hiprz_probe.h: S sets
 * (1 <= S <= 64) of K unit directions, probe i uses set hiprz_bake_hash(i ^ seed) % S, the frame is Duff et al.'s of the normalised
 * normal, d.c = (t.c * l.x + bt.c * l.y) + n.c * l.z.  The ray of (probe i, direction k) is hiprz_probe_samples's and hiprz_bake_rays's,
 * bit for bit.  K is one of 64, 128, 256, 512, 1024: a 64-texel map from 16 rays means nothing, K < 64 is HIPRZ_ERR_INVALID.
 *
 * THE WALK is the closest-hit walk of hiprz_query_closest WITHOUT HIPRZ_QUERY_NORMALIZE; no chart map is involved.  With `reach` finite
 * and > 0:
 *     r = min(t, reach)     for a hit, from either side (FRONT when the face looks at the ray's origin, else BACK)
 *     r = reach             for a miss or an invalid ray (MISSED)
 *
 * THE TEXEL DIRECTIONS (hiprz_field_texel_directions): texel j = 8 * iy + ix has e = ((ix + 0.5) / 4 - 1, (iy + 0.5) / 4 - 1),
 * z = 1 - |e.x| - |e.y|; for z < 0 (x, y) = ((1 - |e.y|) sgn e.x, (1 - |e.x|) sgn e.y), otherwise (x, y) = e; then (x, y, z) is
 * normalised.  Computed in double and rounded to float.  The directions are in WORLD axes, not the probe's frame: the lookup needs no
 * frame.
 *
 * THE MOMENTS, per texel j with direction o, from +0, for k = 0 .. K - 1 in ascending order, d the direction of ray k as made:
 *     c  = max(0, (o.x*d.x + o.y*d.y) + o.z*d.z)          w = c^32 by five squarings: w = c*c; w = w*w; w = w*w; w = w*w; w = w*w
 *     sw = sw + w
 *     s1 = s1 + (w * r)
 *     s2 = s2 + (w * (r * r))
 * then mean = s1 / sw and mean2 = s2 / sw when sw > 0, else (reach, reach * reach).
 *
 * THE RECORD, hiprz_field_vis, 528 bytes: float moments[64][2] = (mean, mean2) per texel, uint32_t words[4] = {FRONT, BACK, MISSED
 * (invalid rays included), K}.  An invalid probe writes +0 everywhere and words[3] = HIPRZ_FIELD_INVALID (0x80000000).
 *
 * ---------------------------------------------------------------------------------------------------------------------------------
 * 2. THE LOOKUP (hiprz_field_lookup)
 *
 * THE GRID, hiprz_field_grid {lo[3], step[3], n[3], reserved}: probe (i, j, k) has index (i * n[1] + j) * n[2] + k — the C order of
 * probe.grid's shape — and its position is read from the probes array, never recomputed.  Refused (HIPRZ_ERR_INVALID) unless every
 * n[a] >= 1, the product equals the probe count passed (and is below 2^31), lo is finite and step[a] is finite and > 0 where n[a] > 1.
 * THE PARAMS, hiprz_field_params {bias, max_back, reserved[2]}: bias finite and >= 0.
 *
 * A POINT is a hiprz_bake_point: position p and unit normal n; near_ and far_ are ignored.  It is INVALID when a component of p or n is
 * not finite or when (n.x*n.x + n.y*n.y) + n.z*n.z lies outside [0.99, 1.01]: the output is then RGB +0 and the word HIPRZ_FIELD_INVALID.
 *
 * THE CELL AND THE FRACTIONS, per axis a:
 *     g = (p.a - lo.a) / step.a   (g = 0 when n[a] == 1), clamped: g = min(max(g, 0), float(n[a] - 1))
 *     i = min(int(floorf(g)), n[a] - 2), or 0 when n[a] == 1          f = g - float(i)
 *
 * THE CORNERS c = 0 .. 7 in order; bit a of c selects "up" on axis a.  The index on axis a is min(i + up, n[a] - 1), and
 *     tri = (wx * wy) * wz          w_a = up ? f : 1.0f - f
 * A probe is LEFT OUT (weight +0, not counted) when its sh[0].w is HIPRZ_PROBE_INVALID, or — with visibility records — when its words[3]
 * is HIPRZ_FIELD_INVALID or its words[1] > max_back (the probe sits inside geometry).
 * Without visibility records w = tri.  With them, for the probe at position P:
 *     q = p + bias * n                 q.c = p.c + (bias * n.c)
 *     v = q - P                        dist = sqrtf((v.x*v.x + v.y*v.y) + v.z*v.z)          dir = v / dist per component
 *   when dist == 0: wb = 1 and ch = 1.  Otherwise
 *   wrap shading:
 *     u = P - p                        len = sqrtf((u.x*u.x + u.y*u.y) + u.z*u.z)           uh = u / len per component
 *     b = (((uh.x*n.x + uh.y*n.y) + uh.z*n.z) + 1.0f) * 0.5f          wb = (b * b) + 0.2f          (len == 0: wb = 1)
 *   the texel of dir = (x, y, z):
 *     s = (|x| + |y|) + |z|            ex = x / s          ey = y / s
 *     z < 0:  fx = (1.0f - |ey|) * copysignf(1, ex)        fy = (1.0f - |ex|) * copysignf(1, ey)          else fx = ex, fy = ey
 *     tx = int(min(max(floorf((fx * 0.5f + 0.5f) * 8.0f), 0), 7))          ty likewise          j = 8 * ty + tx
 *   (the clamp taken on the float, a NaN reading 0; the nearest texel, no bilinear tap)
 *   Chebyshev, with (mean, mean2) = moments[j]:
 *     dist > mean:  var = fabsf(mean2 - mean*mean)     dd = dist - mean     ch = var / (var + dd*dd)     ch = (ch*ch)*ch          else ch = 1
 *   then
 *     w = max(wb * ch, 1e-6f)          if w < 0.2f: w = w * ((w*w) * 25.0f)          w = w * tri
 * E is hiprz_probe_irradiance's rule on the probe's record for n (include/hiprz_probe.h "THE EVALUATION"), and
 *     acc.c = acc.c + (w * E.c)        sw = sw + w          the probe is COUNTED when w > 0
 * THE RESULT, hiprz_field_result, 16 bytes: rgb = acc / sw and the word is the count when sw > 0; otherwise the INVALID record.  The RGB
 * is irradiance in the units of a lightmap texel.
 *
 * Left out on purpose:
 *   - probe placement: moving probes out of geometry is include/hiprz_place.h's, whose moved probes this lookup takes as they are; a
 *     probe that still sits inside geometry is only left out (max_back);
 *   - a bilinear tap of the visibility map and maps larger than 8 x 8;
 *   - an irregular or sparse grid, and a grid streamed in parts;
 *   - blending the coefficients: the lookup evaluates each probe for the point's normal and blends irradiance.
 *
 * THE KERNELS, no atomics.  rz_field_visibility_kernel: 64 threads per workgroup (one wave), one wave per probe, K / 64 rounds.  In a
 * round lane l walks ray 64 r + l and puts (d, r) as one float4 into its row of LDS (1 KB per wave); after a workgroup barrier — one
 * wave: it costs a wait for the LDS counter — every lane, as texel l, runs over the 64 rows in order; all lanes read the same address, a
 * broadcast without a bank conflict; a second barrier keeps the next round's rows from overwriting them.  The counts come from __ballot;
 * lanes of an invalid or out-of-range probe take part in every ballot and barrier.  Lane l stores its float2, 512 coalesced bytes; lane 0
 * stores the words.  rz_field_lookup_kernel: one thread per point, nothing shared, no LDS; workgroups of 64
 * (FIELD_DEFS="-DRZ_FIELD_LOOKUP_WG=256" builds the other size, same bytes).
 *
 * MEASURED on an MI355X (tools/field_time.py, one scene, K = 256; DESIGN.md §6 "Probe fields" and profiles/r32 have the conditions),
 * stated as measured, not as a promise: the bake takes 1.32 times hiprz_probe_samples over the same rays at 4 096 probes (3.22 against
 * 2.43 ms) and 1.14 times at 32 768 (14.61 against 12.78 ms) — not the "near 1" that was expected; a wave per probe makes a quarter of
 * the baseline's waves, each four times as long.  The lookup does 4.8e9 points per second without and 5.0e9 with visibility records
 * (2^20 points in 0.219 and 0.211 ms), 4.7 % and 4.9 % of the device-to-device copy rate at 48 bytes per point: it is bound by its
 * gathers and arithmetic, not by HBM; numpy's probe.Field.irradiance takes 931 ms for the same points.  Workgroups of 64 and of 256
 * time the same within their spread (0.2186 against 0.2192 ms). */
#ifndef HIPRZ_FIELD_H
#define HIPRZ_FIELD_H

#include <stddef.h>
#include <stdint.h>

#include "hiprz_probe.h" /* hiprz_probe_sh, HIPRZ_PROBE_INVALID; hiprz_bake.h: hiprz_bake_point */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiprz_field_vis {
    float moments[64][2]; /* [j]: (mean, mean2) of the distance seen through texel j */
    uint32_t words[4];    /* FRONT, BACK, MISSED, K — or 0, 0, 0, HIPRZ_FIELD_INVALID */
} hiprz_field_vis; /* 528 B */

typedef struct hiprz_field_grid {
    float lo[3];
    float step[3];
    uint32_t n[3];
    uint32_t reserved; /* 0 */
} hiprz_field_grid; /* 40 B */

typedef struct hiprz_field_params {
    float bias;        /* the shaded point is moved this far along its normal before it is held against a visibility map */
    uint32_t max_back; /* a probe more of whose rays hit back faces is left out */
    uint32_t reserved[2];
} hiprz_field_params; /* 16 B */

typedef struct hiprz_field_result {
    float rgb[3];
    uint32_t word; /* the probes counted, or HIPRZ_FIELD_INVALID */
} hiprz_field_result; /* 16 B */

#define HIPRZ_FIELD_INVALID 0x80000000u
#define HIPRZ_FIELD_TEXELS 64u

/* Bound to one context and answering on its head device.  It owns the direction table, the texel directions' device copy, the device
 * copies of a host field and the pinned staging of the host-pointer calls, grown on demand.  One call at a time per handle.
 * HIPRZ_ERR_DEVICE without a HIP device.  Destroy it before its context. */
typedef struct hiprz_field hiprz_field;
int hiprz_field_create(hiprz_field** out, hiprz_ctx* ctx);
int hiprz_field_destroy(hiprz_field* field);
const char* hiprz_field_last_error(const hiprz_field* field); /* NULL: the last error of a call without a handle, on this thread */

/* S*K float4 (x, y, z, ignored) from the host, checked as hiprz_probe_set_directions checks them, K >= 64 (HIPRZ_ERR_INVALID, what was
 * set before stays).  The handle keeps them; they reach the device with the next bake, on that call's stream, which that one call waits
 * for. */
int hiprz_field_set_directions(hiprz_field* field, const float* xyz0_host, uint32_t K, uint32_t S);

/* Host only, pure, computed in double and rounded to float: THE TEXEL DIRECTIONS, 64 float4 (x, y, z, 0).  HIPRZ_ERR_INVALID on null. */
int hiprz_field_texel_directions(float out[64][4]);

/* Host only, pure: HIPRZ_OK when the lookup takes the grid for n_probes probes / the params, else HIPRZ_ERR_INVALID */
int hiprz_field_check_grid(const hiprz_field_grid* grid, size_t n_probes);
int hiprz_field_check_params(const hiprz_field_params* params);

/* Every call that takes a `stream` (a hipStream_t) only enqueues; NULL = hiprz_stream(ctx).  Device arrays are 16-byte aligned.  Records
 * past n are never written; n == 0 is HIPRZ_OK without a view or a launch.  Refused before anything is launched or copied, in this order:
 * a null handle or pointer (HIPRZ_ERR_INVALID), no direction table set (HIPRZ_ERR_STATE), n*K >= 2^31 (HIPRZ_ERR_INVALID), a reach that
 * is not finite or not > 0 (HIPRZ_ERR_INVALID), whatever hiprz_device_view refuses (a context without a scene: HIPRZ_ERR_STATE). */
int hiprz_field_visibility(hiprz_field* field, const hiprz_bake_point* probes_device, size_t n, uint32_t seed, float reach, hiprz_field_vis* out_device,
                           void* stream);
/* the same for host pointers, through the handle's pinned staging on the context's stream, which is waited for */
int hiprz_field_visibility_host(hiprz_field* field, const hiprz_bake_point* probes, size_t n, uint32_t seed, float reach, hiprz_field_vis* out);

/* m points against the n_probes probes of `grid`, their records `sh` and — unless null — their visibility records `vis`; 16 bytes out per
 * point, entries past m never written; m == 0 is HIPRZ_OK without a launch.  No scene is needed.  Refused in this order, all
 * HIPRZ_ERR_INVALID: a null handle or pointer (`vis` may be null), a grid hiprz_field_check_grid refuses, params hiprz_field_check_params
 * refuses, m >= 2^31. */
int hiprz_field_lookup(hiprz_field* field, const hiprz_field_grid* grid, const hiprz_bake_point* probes_device, const hiprz_probe_sh* sh_device,
                       const hiprz_field_vis* vis_device, size_t n_probes, const hiprz_field_params* params, const hiprz_bake_point* points_device, size_t m,
                       hiprz_field_result* out_device, void* stream);
/* the same for host pointers: the field goes to device copies the handle owns, the points and results through its pinned staging */
int hiprz_field_lookup_host(hiprz_field* field, const hiprz_field_grid* grid, const hiprz_bake_point* probes, const hiprz_probe_sh* sh, const hiprz_field_vis* vis,
                            size_t n_probes, const hiprz_field_params* params, const hiprz_bake_point* points, size_t m, hiprz_field_result* out);

/* sizeof(hiprz_bake_point), sizeof(hiprz_probe_sh), sizeof(hiprz_field_vis), sizeof(hiprz_field_grid), sizeof(hiprz_field_params),
 * sizeof(hiprz_field_result), the offset of hiprz_field_vis::words and the lookup kernel's workgroup size as this library was compiled */
void hiprz_field_layout(uint32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
