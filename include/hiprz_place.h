/* hiprz_place.h — probe placement: the probes of a grid moved out of geometry and away from the surface they hug, on the device
 * (libhiprz_place.so).  A regular grid laid over a scene puts probes inside walls and objects and a hair in front of surfaces.
 * include/hiprz_field.h only leaves the first kind out of its lookup (max_back) and keeps the second with half of its visibility map a wall
 * at distance 0.  This library is the relocation step of the dynamic-diffuse-global-illumination lineage in PAPERS.md: every probe is
 * nudged, within a box around where it was put, through the nearest back face when it sits inside geometry and towards the most open
 * direction when a surface is nearer than a margin.  hiprz_field_lookup reads each probe's position from the probes array, so the moved
 * probes are used as they are.
 *
 * A library of its own for the reasons the other eleven are: their kernel sets and exports are pinned, and a caller that never places
 * probes runs no code of this library.  It links against libhiprz.so alone, reads the context through hiprz_device_view (include/hiprz.h)
 * on EVERY call and caches nothing an upload could make stale.  What it needs of the probe's frame, hash and ray it restates.
 *
 * Every rule below is plain float32, one rounding per operation (no fused multiply-add); the device evaluates no division, square root,
 * power, exponential or trigonometric function of its own (the ray rule's are hiprz_query.h's).
 *
 * THE PROBE is a hiprz_bake_point with the validity rule of hiprz_probe.h: INVALID exactly when the ray (position, near_, normal, far_) is
 * invalid under HIPRZ_QUERY_NORMALIZE.  THE DIRECTIONS, THE SET OF A PROBE, THE FRAME and THE RAY are hiprz_field_visibility's: S sets
 * (1 <= S <= 64) of K unit directions, K one of 64, 128, 256, 512, 1024; probe i uses set hiprz_bake_hash(i ^ seed) % S; the frame is Duff
 * et al.'s of the normalised normal; d.c = (t.c * l.x + bt.c * l.y) + n.c * l.z.  The direction d of ray k depends on the probe's normal
 * alone and stays what it is while the probe moves.  The ray of direction k from the probe's CURRENT position P is origin = P, the probe's
 * near_, direction = d, the probe's far_: what hiprz_probe_samples / hiprz_bake_rays make for a probe at P with the same near_, normal and
 * far_, bit for bit.  THE WALK is the closest-hit walk of hiprz_query_closest WITHOUT HIPRZ_QUERY_NORMALIZE.
 *
 * THE PARAMS, hiprz_place_params, 32 bytes: min_front (the margin kept to a front face), reach (what a ray that hits nothing sees, and the
 * cap of every distance), max_offset[3] (the box, per axis, that the offset stays in), iterations (the most moves made), max_back (a probe
 * more of whose rays hit back faces is INSIDE) and reserved.  Refused (HIPRZ_ERR_INVALID) unless min_front and reach are finite and > 0,
 * every max_offset[a] is finite and >= 0, iterations <= 16 and reserved is 0.
 *
 * ONE EVALUATION AT P walks the K rays.
 *     r = min(t, reach)     for a hit, FRONT when the face looks at the ray's origin, else BACK
 *     r = reach             for a miss or an invalid ray (OPEN; a probe moved to where its rays are invalid sees only OPEN rays)
 * n_back and n_front are the exact counts.  Three selections, each an exact extremum that does not depend on the order the rays are
 * looked at, ties going to the LOWEST k:
 *     B   the BACK ray of least r
 *     F   the FRONT ray of least r
 *     O   the ray of greatest r among the FRONT and the OPEN rays
 * front = r_F, or reach when there is no FRONT ray; back = r_B, or reach when there is no BACK ray.  THE STATE is
 *     INSIDE (2)   when n_back > max_back
 *     NEAR (1)     otherwise, when F exists and r_F < min_front
 *     CLEAR (0)    otherwise
 *
 * THE LOOP.  H is the probe's position as given, P = H (its bytes), o = (+0, +0, +0), moves = 0.
 *     1. evaluate at P
 *     2. stop when moves == iterations, or when the state is CLEAR
 *     3. INSIDE:  s = r_B + (0.5f * min_front)                         m.a = d_B.a * s
 *                 (through the nearest back face and half a margin beyond; n_back > max_back >= 0, so B exists)
 *        NEAR:    when O exists and (d_O.x*d_F.x + d_O.y*d_F.y) + d_O.z*d_F.z <= 0.5f:
 *                     s = min(min_front - r_F, 0.5f * r_O)             m.a = d_O.a * s
 *                 otherwise stop with STUCK (the most open direction points at the surface that is too near)
 *     4. o'.a = o.a + m.a; when |o'.a| > max_offset[a] on any axis stop with STUCK: the probe stays where it is
 *     5. o = o', P.a = H.a + o.a, moves = moves + 1, go to 1
 * d is the ray's direction as made, not renormalised.  The state, the counts, front and back that are reported are those of the LAST
 * evaluation, which was made at the final position: at most iterations + 1 evaluations; iterations = 0 only classifies.
 *
 * THE RECORD, hiprz_place_record, 32 bytes: offset[3] = o, word = state | HIPRZ_PLACE_STUCK (0x100) when the loop stopped so |
 * moves << 16, front, back, n_back, n_front.  An INVALID probe writes word = HIPRZ_PLACE_INVALID (0x80000000) and +0 everywhere else.
 * THE MOVED PROBE is a hiprz_bake_point: the position P — the bytes of H when no move was made, else H.a + o.a — and the other 20 bytes
 * unchanged.  An invalid probe is copied unchanged.
 *
 * Left out on purpose:
 *   - a search over several directions per step, or a line search along one: a step follows one ray;
 *   - moving a probe across cells: max_offset is the caller's, Python's params_for takes 0.45 of the grid's step;
 *   - re-baking: the caller bakes SH and visibility at the moved positions (Context.bake_probe_field(place=) does);
 *   - probes classified "off" to save rays, as the DDGI papers also do: every probe is kept.
 *
 * THE KERNEL, rz_place_kernel, no atomics, no LDS: 64 threads per workgroup (one wave), one wave per probe, K / 64 rounds per evaluation,
 * the loop inside the kernel with P and o in registers.  In a round lane l walks ray 64 r + l.  Each selection is the minimum of 64-bit
 * keys — (bits of r << 32) | k for B and F, (~bits of r << 32) | k for O; r >= 0, so the bit patterns order as the floats do; all ones
 * means "none" — kept per lane over the rounds and then reduced across the wave by a __shfl_xor butterfly; the counts come from
 * __ballot.  The winner's direction is recomputed from k.  Every branch of the loop depends on reduced values only, the same in every
 * lane; lanes of an invalid probe walk nothing but take part in every ballot and shuffle.  Lane 0 stores the probe and the record.
 *
 * The wave-uniform frame, P and offset sit in scalar registers: 104 VGPRs, no scratch, 4 waves per SIMD (the gather walk alone: 96 and 5).
 *
 * MEASURED on an MI355X (tools/place_time.py, one scene, K = 256, iterations 4; DESIGN.md §6 "Probe placement" and profiles/r33 have the
 * conditions), stated as measured, not as a promise: the placement takes 1.99 times hiprz_probe_samples over the same rays — launched
 * once per evaluation the placement made — at 4 096 probes (13.72 against 6.88 ms) and 1.33 times at 32 768 (26.05 against 19.51 ms): a
 * wave runs up to five evaluations of four rounds in sequence, and the few probes that use every move are a long tail.  The host loop it
 * replaces (numpy rays, a round trip of rays and hits per evaluation) takes 175 and 2 066 ms: 12.8 and 79 times as long. */
#ifndef HIPRZ_PLACE_H
#define HIPRZ_PLACE_H

#include <stddef.h>
#include <stdint.h>

#include "hiprz_bake.h" /* hiprz_bake_point; hiprz.h: hiprz_ctx, the return codes */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiprz_place_params {
    float min_front;     /* a front face nearer than this makes a probe NEAR */
    float reach;         /* what a ray that hits nothing sees, and the cap of every distance */
    float max_offset[3]; /* |offset| per axis never exceeds this */
    uint32_t iterations; /* the most moves made, <= 16 */
    uint32_t max_back;   /* a probe more of whose rays hit back faces is INSIDE */
    uint32_t reserved;   /* 0 */
} hiprz_place_params; /* 32 B */

typedef struct hiprz_place_record {
    float offset[3]; /* the final position is the given one + offset, per component */
    uint32_t word;   /* state | HIPRZ_PLACE_STUCK | moves << 16, or HIPRZ_PLACE_INVALID */
    float front;     /* the nearest front face at the final position, reach when none */
    float back;      /* the nearest back face at the final position, reach when none */
    uint32_t n_back;
    uint32_t n_front;
} hiprz_place_record; /* 32 B */

#define HIPRZ_PLACE_CLEAR 0u
#define HIPRZ_PLACE_NEAR 1u
#define HIPRZ_PLACE_INSIDE 2u
#define HIPRZ_PLACE_STATE_MASK 0xffu
#define HIPRZ_PLACE_STUCK 0x100u
#define HIPRZ_PLACE_INVALID 0x80000000u
#define HIPRZ_PLACE_MAX_ITERATIONS 16u

/* Bound to one context and answering on its head device.  It owns the direction table and the pinned staging of the host-pointer call,
 * grown on demand.  One call at a time per handle.  HIPRZ_ERR_DEVICE without a HIP device.  Destroy it before its context. */
typedef struct hiprz_place hiprz_place;
int hiprz_place_create(hiprz_place** out, hiprz_ctx* ctx);
int hiprz_place_destroy(hiprz_place* place);
const char* hiprz_place_last_error(const hiprz_place* place); /* NULL: the last error of a call without a handle, on this thread */

/* S*K float4 (x, y, z, ignored) from the host, checked as hiprz_field_set_directions checks them, K >= 64 (HIPRZ_ERR_INVALID, what was
 * set before stays).  The handle keeps them; they reach the device with the next placement, on that call's stream, which that one call
 * waits for. */
int hiprz_place_set_directions(hiprz_place* place, const float* xyz0_host, uint32_t K, uint32_t S);

/* Host only, pure: HIPRZ_OK when a placement takes the params, else HIPRZ_ERR_INVALID (null included) */
int hiprz_place_check_params(const hiprz_place_params* params);

/* n probes at probes_device -> n moved probes at out_probes_device (which may be probes_device) and, unless out_records_device is null,
 * n records.  `stream` (a hipStream_t) NULL = hiprz_stream(ctx); the call only enqueues.  Device arrays are 16-byte aligned.  Entries past
 * n are never written; n == 0 is HIPRZ_OK without a view or a launch.  Refused before anything is launched or copied, in this order: a
 * null handle or pointer (HIPRZ_ERR_INVALID; out_records_device may be null), no direction table set (HIPRZ_ERR_STATE), n*K >= 2^31
 * (HIPRZ_ERR_INVALID), params that hiprz_place_check_params refuses (HIPRZ_ERR_INVALID), whatever hiprz_device_view refuses (a context
 * without a scene: HIPRZ_ERR_STATE). */
int hiprz_place_probes(hiprz_place* place, const hiprz_bake_point* probes_device, size_t n, uint32_t seed, const hiprz_place_params* params,
                       hiprz_bake_point* out_probes_device, hiprz_place_record* out_records_device, void* stream);
/* the same for host pointers, through the handle's pinned staging on the context's stream, which is waited for; out_probes may be probes,
 * out_records may be null */
int hiprz_place_probes_host(hiprz_place* place, const hiprz_bake_point* probes, size_t n, uint32_t seed, const hiprz_place_params* params,
                            hiprz_bake_point* out_probes, hiprz_place_record* out_records);

/* sizeof(hiprz_bake_point), sizeof(hiprz_place_params), sizeof(hiprz_place_record), the offsets of hiprz_place_params::max_offset,
 * ::iterations and ::max_back, and of hiprz_place_record::word and ::front, as this library was compiled */
void hiprz_place_layout(uint32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
