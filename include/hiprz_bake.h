/* hiprz_bake.h — occlusion baking: K hemisphere rays per surface point, made, walked and counted on the device (libhiprz_bake.so).
 *
 * A ray query (include/hiprz_query.h) answers rays the caller has written out: ambient occlusion for n points with K rays each costs n*K
 * 32-byte rays in and n*K words out, to obtain n answers.  A bake reads 32 bytes per POINT, makes the point's K rays on the device from a
 * table of directions, walks them with the query's occlusion walk and writes 16 bytes per point: how many of the K rays are occluded and
 * the sum of the directions that are not (the bent normal).  A library of its own for the reasons the query and order libraries are: their
 * kernel sets and libhiprz.so's are pinned, and a caller that never bakes runs no code of this library.  It reads the context through
 * hiprz_device_view (include/hiprz.h) on EVERY call and caches nothing an upload could make stale.
 *
 * THE POINT, 32 bytes, two 16-byte loads, in the layout of hiprz_ray: position, near_, normal, far_ — a point IS the ray along its normal.
 * The normal is always passed through the device's normalized() first, n = normal * (1 / sqrt((x*x + y*y) + z*z)), every operation rounded
 * separately.  A point is INVALID exactly when the ray (position, near_, normal, far_) is invalid under HIPRZ_QUERY_NORMALIZE
 * (hiprz_query.h "AN INVALID RAY"; the same device function decides).  An invalid point walks no ray and affects no other point.
 *
 * THE DIRECTIONS: S sets of K unit directions in the local frame, z along the normal; S*K float4 (x, y, z, 0), set-major.  K is one of 16,
 * 32, 64, 128, 256, 512, 1024 and 1 <= S <= 64.  Every component must be finite and the squared length (x*x + y*y) + z*z in float32 must
 * lie in [0.999, 1.001]: a direction rotated by a frame that is orthonormal to a few ulp then stays inside the query's own [0.99, 1.01].
 * No sign of z is required: a caller may bake over a sphere.  The fourth component is not read; the device copy holds 0 there.
 *
 * THE SET OF A POINT: point i uses set hiprz_bake_hash(i ^ seed) % S, on uint32_t
 *     x ^= x >> 16;  x *= 0x7feb352du;  x ^= x >> 15;  x *= 0x846ca68bu;  x ^= x >> 16;
 * (hiprz_bake_set_of is the same on the host).
 *
 * THE FRAME (Duff et al., "Building an Orthonormal Basis, Revisited"), plain float32, one rounding per operation, n the normalised normal:
 *     s = copysignf(1, n.z);   a = -1.0f / (s + n.z);   b = (n.x * n.y) * a;
 *     t  = ( 1.0f + ((s * n.x) * n.x) * a,   s * b,                   (-s) * n.x );
 *     bt = ( b,                              s + (n.y * n.y) * a,     -n.y       );
 * and the world direction of the table's l, per component c:
 *     d.c = (t.c * l.x + bt.c * l.y) + n.c * l.z
 * The ray of (point i, direction k) is origin = position, near_, direction = d, far_.  It is walked WITHOUT HIPRZ_QUERY_NORMALIZE by the
 * query's occlusion (the same device function), so its verdict is hiprz_query_occluded's on the same ray by construction — the invalid-ray
 * rule included: a d whose squared length leaves [0.99, 1.01] counts as not occluded.
 *
 * THE RESULT, 16 bytes, one store.  `occluded` is the number of the K rays that are occluded, an exact integer; ambient visibility is
 * 1 - occluded / K.  `bent` is the unnormalised sum of the world directions d of the UNOCCLUDED rays, per component in this fixed order:
 * lane l = k % 64 starts at +0 and for rounds r = 0, 1, ... adds ray k = 64 r + l — its direction if unoccluded, +0 otherwise — then for
 * off = 1, 2, 4, ..., min(K, 64) / 2 every lane does v = v + v[lane ^ off].  An invalid point reads bent = +0 and occluded =
 * HIPRZ_BAKE_INVALID.  An empty world reads occluded = 0 and bent = the sum of all K directions.
 *
 * THE KERNELS, 64 threads per workgroup (one wave), no LDS, no atomics.  rz_bake_occlusion_kernel: for K >= 64 one wave bakes one point in
 * K / 64 rounds; for K < 64 one wave bakes 64 / K consecutive points, one ray per lane.  The count is a 64-bit ballot and a population count
 * of the point's K-bit segment, bent the butterfly above.  The rays of a wave share an origin (or 64 / K neighbouring ones): the coherence
 * the order library buys with a sort, so none is done.  rz_bake_rays_kernel: one thread per (point, direction) writes ray i*K + k as a
 * hiprz_ray, by the device function that makes it in the bake — the way to closest-hit distances for the same rays (distance-weighted
 * occlusion).  An invalid point's rays carry its position, near_ and far_ and the direction +0, which hiprz_query flags invalid. */
#ifndef HIPRZ_BAKE_H
#define HIPRZ_BAKE_H

#include <stddef.h>
#include <stdint.h>

#include "hiprz_query.h" /* hiprz_ray; hiprz.h: hiprz_ctx, the return codes */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiprz_bake_point {
    float position[3];
    float near_;
    float normal[3];
    float far_;
} hiprz_bake_point; /* 32 B */

typedef struct hiprz_bake_texel {
    float bent[3];
    uint32_t occluded;
} hiprz_bake_texel; /* 16 B */

#define HIPRZ_BAKE_INVALID 0x80000000u

/* Bound to one context and answering on its head device.  It owns the direction table and the pinned staging of the host-pointer call,
 * grown on demand.  One call at a time per handle.  HIPRZ_ERR_DEVICE without a HIP device.  Destroy it before its context. */
typedef struct hiprz_bake hiprz_bake;
int hiprz_bake_create(hiprz_bake** out, hiprz_ctx* ctx);
int hiprz_bake_destroy(hiprz_bake* bake);
const char* hiprz_bake_last_error(const hiprz_bake* bake); /* NULL: the last error of a call without a handle, on this thread */

/* S*K float4 (x, y, z, ignored) from the host, checked against THE DIRECTIONS above (HIPRZ_ERR_INVALID, the table before stays).  The
 * handle keeps the table; it reaches the device with the next call below, on that call's stream, once the context's device is known from
 * a view — so a table may be set before a scene is uploaded.  That one call waits for its stream (the copy reads pageable memory); every
 * later call with the same table only enqueues. */
int hiprz_bake_set_directions(hiprz_bake* bake, const float* xyz0_host, uint32_t K, uint32_t S);

/* Host only, pure.  The set of point i: hiprz_bake_hash(i ^ seed) % S; 0 when S == 0. */
uint32_t hiprz_bake_set_of(uint32_t i, uint32_t seed, uint32_t S);

/* Host only, pure, computed in double: a cosine-weighted Fibonacci table, S*K float4.  For set s and sample k: u = (k + 0.5) / K,
 * r = sqrt(u), phi = 2 pi (frac(k * 0.6180339887498949) + s / S), (x, y, z) = (r cos phi, r sin phi, sqrt(1 - u)) rounded to float.
 * HIPRZ_ERR_INVALID on a K or S that hiprz_bake_set_directions refuses, or a null pointer. */
int hiprz_bake_cosine_directions(uint32_t K, uint32_t S, float* xyz0_out);

/* Every call that takes a `stream` (a hipStream_t) only enqueues; NULL = hiprz_stream(ctx), the stream scene uploads, refits and rebuilds
 * are ordered on.  Device arrays are 16-byte aligned.  Entries past n (past n*K for the rays) are never written; n == 0 is HIPRZ_OK
 * without a view or a launch.  Refused before anything is launched or copied: a null handle or pointer (HIPRZ_ERR_INVALID), no direction
 * table set (HIPRZ_ERR_STATE), n*K >= 2^31 (HIPRZ_ERR_INVALID), a context without a scene (HIPRZ_ERR_STATE), whatever else
 * hiprz_device_view refuses. */
int hiprz_bake_occlusion(hiprz_bake* bake, const hiprz_bake_point* points_device, size_t n, uint32_t seed, hiprz_bake_texel* out_device, void* stream);
int hiprz_bake_rays(hiprz_bake* bake, const hiprz_bake_point* points_device, size_t n, uint32_t seed, hiprz_ray* rays_out_device, void* stream);

/* The bake for host pointers: copied through the handle's pinned staging on the context's stream, which is waited for once. */
int hiprz_bake_occlusion_host(hiprz_bake* bake, const hiprz_bake_point* points, size_t n, uint32_t seed, hiprz_bake_texel* out);

/* sizeof(hiprz_bake_point), sizeof(hiprz_bake_texel) and the offsets of hiprz_bake_point::normal, ::far_, hiprz_bake_texel::bent and
 * ::occluded as this library was compiled */
void hiprz_bake_layout(uint32_t out[6]);

#ifdef __cplusplus
}
#endif
#endif
