/* hiprz_smooth.h — lightmap smoothing: an edge-stopping filter in texel space for what the bake pipeline leaves per texel, guided by the
 * surface point under the texel (libhiprz_smooth.so).
 *
 * Every number the bake pipeline makes (include/hiprz_light.h, hiprz_gather.h, hiprz_bake.h) is a Monte-Carlo mean over K rays: a penumbra
 * or a bounce texel takes about K + 1 distinct values and the map is grainy.  This library reads the W x H surface points the atlas
 * library left on the device (hiprz_atlas_points_device: position and normal per texel) and W x H 16-byte records, and writes W x H
 * records in which every texel is a weighted mean of its neighbours ON THE SAME SURFACE: an a-trous scheme (Dammertz et al. 2010), the
 * frame denoiser's (include/hiprz.h, hiprz_denoise), with stops made of the world position and normal instead of a camera's guides.  It
 * belongs between a bake and its dilation, so that the gutters take smoothed values.  A library of its own for the reasons the other nine
 * are: their kernel sets and exports are pinned, and a caller that never smooths runs no code of this library.  It links against
 * libhiprz.so alone and needs no device view: it uses the context only for its head device and its stream.
 *
 * Every rule below is plain float32, one rounding per operation (no fused multiply-add), true division; there is no exponential, power or
 * square root, so a numpy restatement (tests/smooth_reference.py) matches every byte.  fmaxf(0, x) is 0 for a NaN x.
 *
 * INPUT AND OUTPUT.  W x H hiprz_bake_point (32 bytes: position, near_, normal, far_; a texel no chart covers is 32 zero bytes; near_
 * and far_ are not read) and W x H 16-byte records: float rgb[3] and one 32-bit word, texel (x, y) at index y * W + x, 1 <= W, H <= 16384.
 * A texel TAKES PART when its word is not 0x80000000 (HIPRZ_SMOOTH_INVALID, the invalid mark of every bake), its point's normal is not all
 * +-0 and its three RGB floats are finite.  The output's word is always the input's word; a texel that does not take part keeps its 16
 * bytes.  Which texels take part is decided once, on the input.
 *
 * THE PARAMETERS, hiprz_smooth_params, 16 bytes: iterations in 1 .. 8 and three floats, each finite and >= 0, 0 switching that stop off:
 * `radius` (world units: no tap further from the texel's point), `plane` (world units: no tap further from the texel's tangent plane) and
 * `sigma_colour` (the units of the records: no tap whose colour differs by more; halved with every iteration as the frame filter halves
 * its sigma_color).
 *
 * THE ITERATIONS.  Iteration i = 0 .. iterations - 1 has the step s = 1 << i and reads the result of the iteration before it (the first
 * the input).  One iteration, per texel p that takes part: num = (+0, +0, +0), den = +0, then the 25 taps q = p + s * (dx, dy) in the
 * order dy = -2 .. 2 outer, dx = -2 .. 2 inner.  A tap outside the atlas or one that does not take part adds nothing.  For the others,
 * with x the position, n the normal AS GIVEN (not normalised) and rgb this iteration's input:
 *     h  = B[dx+2] * B[dy+2]                                   B = {1, 4, 6, 4, 1}
 *     d  = (n_p.x*n_q.x + n_p.y*n_q.y) + n_p.z*n_q.z ;   c = fmaxf(0, d) ;   c2 = c*c ;   wn = c2*c2
 *     v  = x_q - x_p
 *     r2 = (v.x*v.x + v.y*v.y) + v.z*v.z ;               wr = fmaxf(0, 1.0f - r2 / (radius*radius))
 *     e  = (n_p.x*v.x + n_p.y*v.y) + n_p.z*v.z ;         wd = fmaxf(0, 1.0f - (e*e) / (plane*plane))
 *     g  = rgb_q - rgb_p
 *     g2 = (g.x*g.x + g.y*g.y) + g.z*g.z ;   sc = sigma_colour / float(s) ;   wc = fmaxf(0, 1.0f - g2 / (sc*sc))
 *     w  = (((h * wn) * wr) * wd) * wc                         a stop that is off is left out of the product
 * A tap contributes only when w > 0 — a NaN fails that test, so a point whose position is not finite contributes nothing — and then does
 *     num.c = num.c + w * rgb_q.c          den = den + w
 * After the 25 taps out.c = num.c / den when den > 0; otherwise the texel keeps its value.  A texel never blends with a neighbour of the
 * atlas that is not its neighbour on the surface: a gutter or an invalid texel does not take part, the other side of a crease has
 * wn = 0 for a right angle or more, a parallel face a step away has wd = 0 once the step reaches `plane`, and another chart far away in
 * the world has wr = 0.
 *
 * Left out on purpose:
 *   - filtering across UV seams: two charts that meet on the surface but not in the atlas do not see each other;
 *   - a stop guided by variance: no bake of the pipeline estimates one;
 *   - the occlusion bake's integer count: a caller that wants smoothed occlusion writes 1 - occluded / K into the float channels first;
 *     the bent normal (three floats and a word, hiprz_bake.h) filters as it is.
 *
 * THE KERNEL, rz_smooth_kernel, one launch per iteration, no atomics; the iterations ping-pong through scratch the handle owns and only
 * the last one writes `out`.  Two forms write the same bytes, since the tap order above is the only summation order.  DIRECT: one thread
 * per texel, the taps read from global memory.  STAGED: at step s a workgroup of 256 threads takes a 16 x 16 block of ONE sub-lattice
 * (x = x0, y = y0 mod s), stages the block's 20 x 20 halo once into LDS as ten planes of floats (position, normal, RGB and the take-part
 * flag: 40 bytes x 400 = 16 000 bytes) and does its 25 taps from there — the arrangement of the frame filter's kernel per sub-lattice.
 * Which form is shipped for s = 1 and for s > 1 is a build choice (make SMOOTH_DEFS="-DRZ_SMOOTH_STAGED_S1=.. -DRZ_SMOOTH_STAGED_SN=.."). */
#ifndef HIPRZ_SMOOTH_H
#define HIPRZ_SMOOTH_H

#include <stddef.h>
#include <stdint.h>

#include "hiprz_bake.h" /* hiprz_bake_point; hiprz.h: hiprz_ctx, the return codes */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiprz_smooth_params {
    uint32_t iterations; /* 1 .. 8: the steps 1, 2, 4, ... */
    float radius;        /* world units; 0: no radius stop */
    float plane;         /* world units; 0: no plane stop */
    float sigma_colour;  /* the records' units at iteration 0; 0: no colour stop */
} hiprz_smooth_params; /* 16 B */

#define HIPRZ_SMOOTH_INVALID 0x80000000u
#define HIPRZ_SMOOTH_MAX_SIZE 16384u
#define HIPRZ_SMOOTH_MAX_ITERATIONS 8u

/* Bound to one context and answering on its head device.  It owns the scratch of the iterations and the pinned staging of the
 * host-pointer call, grown on demand.  One call at a time per handle.  HIPRZ_ERR_DEVICE without a HIP device.  Destroy it before its
 * context. */
typedef struct hiprz_smooth hiprz_smooth;
int hiprz_smooth_create(hiprz_smooth** out, hiprz_ctx* ctx);
int hiprz_smooth_destroy(hiprz_smooth* smooth);
const char* hiprz_smooth_last_error(const hiprz_smooth* smooth); /* NULL: the last error of a call without a handle, on this thread */

/* Host only, pure: HIPRZ_OK when `params` is what a call takes, else HIPRZ_ERR_INVALID (null, iterations outside 1 .. 8, a float that is
 * NaN, infinite or negative; -0 is 0). */
int hiprz_smooth_check_params(const hiprz_smooth_params* params);

/* Enqueues only; stream: a hipStream_t, NULL = hiprz_stream(ctx).  Device arrays are 16-byte aligned.  `out16_device` may be
 * `records16_device` (or overlap it: the input is then copied to scratch on the stream first).  Refused before anything is launched,
 * copied or allocated, in this order: a null handle or pointer, params that hiprz_smooth_check_params refuses, a W or H outside
 * 1 .. HIPRZ_SMOOTH_MAX_SIZE (all HIPRZ_ERR_INVALID). */
int hiprz_smooth_texels(hiprz_smooth* smooth, const hiprz_bake_point* points_device, const void* records16_device, uint32_t W, uint32_t H,
                        const hiprz_smooth_params* params, void* out16_device, void* stream);

/* The same for host pointers: points and records go through the handle's pinned staging on the context's stream, which is waited for.
 * `out16` may be `records16`. */
int hiprz_smooth_texels_host(hiprz_smooth* smooth, const hiprz_bake_point* points, const void* records16, uint32_t W, uint32_t H,
                             const hiprz_smooth_params* params, void* out16);

/* sizeof(hiprz_bake_point), the size of a record (16), sizeof(hiprz_smooth_params), the offset of a record's word (12), the offsets of
 * hiprz_smooth_params::radius and ::sigma_colour, and which form this library runs at s = 1 and at s > 1 (0 direct, 1 staged) */
void hiprz_smooth_layout(uint32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
