/* hiprz_query.h — ray queries: closest hit and occlusion for rays the CALLER supplies (libhiprz_query.so).
 *
 * The renderer intersects only the rays it generates; hiprz_ray_cast answers for one pixel of the current frame per host round trip.  A
 * query walks a batch of caller rays through the world a hiprz_ctx holds — the trees, the walks and the exact tests the passes use — and
 * writes one record per ray.  No counterpart in the reference beyond Kernel::rayCast.  A library of its own: libhiprz.so's kernel set is
 * pinned, and a caller that never queries runs no code of this library.  It reads the context through hiprz_device_view (include/hiprz.h)
 * on EVERY call and caches nothing an upload could make stale.
 *
 * THE RAY, 32 bytes, two 16-byte loads:  origin, near_, direction, far_ — the segment origin + t * direction, near_ < t < far_, in world
 * space.  Without HIPRZ_QUERY_NORMALIZE the direction is walked as given and must be of unit length (squared length in [0.99, 1.01]); with
 * it the device's normalized() — d * (1 / sqrt(d.d)), every operation rounded separately — is applied first and t counts along the
 * normalised direction.
 *
 * AN INVALID RAY is decided per ray on the device, before any walk (the host cannot see device rays).  A ray is invalid when
 *   - a component of origin or direction, near_ or far_ is not finite;
 *   - near_ < 0;
 *   - far_ <= near_;
 *   - without NORMALIZE: the direction's squared length (x*x + y*y) + z*z lies outside [0.99, 1.01];
 *   - with NORMALIZE: the direction's length sqrt((x*x + y*y) + z*z) is zero or not finite, or its reciprocal is not finite.
 * It reads flags = HIPRZ_HIT_INVALID, the miss fields, t = far_ (the input's bits) and occlusion 0; no other ray is affected.  Why: every
 * walk terminates (the skip links of finite trees are proven on the host), but a NaN passes every slab test, so one such ray would visit
 * every node and triangle of the world.
 *
 * THE HIT, 48 bytes, three 16-byte stores (fields below).  The walk is closest_hit_skip with ties ranked in the reference's order, so the
 * trees the context holds (hiprz_set_tree) do not change the answer; the surface is analyze_intersection under the CPU engine's fetches
 * (mode 0: hiprz_set_mode does not change a query).  A miss — an empty world included — reads t = far_, u = v = +0, flags 0, instance =
 * material_slot = material = -1, triangle 0, normal +0, scene_triangle -1.
 *
 * OCCLUSION: one uint32_t per ray, 1 = some triangle lies in (near_, far_), the CPU engine's anyIntersection for opaque surfaces
 * (any_hit_skip).  It equals "closest found" on the same ray.
 *
 * THE KERNELS (rz_query_closest_kernel, rz_query_occluded_kernel, rz_query_pixel_rays_kernel): one thread per ray in caller order, 64
 * threads per workgroup (DESIGN.md "Ray queries" has the measurement against 256), no LDS, no counters. */
#ifndef HIPRZ_QUERY_H
#define HIPRZ_QUERY_H

#include <stddef.h>
#include <stdint.h>

#include "hiprz.h" /* hiprz_ctx, the return codes */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiprz_ray {
    float origin[3];
    float near_;
    float direction[3];
    float far_;
} hiprz_ray; /* 32 B */

#define HIPRZ_HIT_FOUND 1u
#define HIPRZ_HIT_EXTERNAL 2u /* the triangle was met from its front */
#define HIPRZ_HIT_INVALID 4u

typedef struct hiprz_hit {
    float t;                /* ray.far_ after the walk: the hit's distance along the direction walked; the ray's far_ on a miss */
    float u, v;             /* Surface::texcrd at the hit, 0 on a miss (and where the triangle has no texcrds) */
    uint32_t flags;         /* HIPRZ_HIT_* */
    int32_t instance;       /* the four fields of hiprz_raycast, -1 / -1 / -1 / 0 on a miss */
    int32_t material_slot;
    int32_t material;
    uint32_t triangle;      /* hiprz_tri::source_index: the triangle's index within its mesh */
    float normal[3];        /* Surface::mapped_normal facing the ray, under the CPU engine's fetches (mode 0); +0 on a miss */
    int32_t scene_triangle; /* index into hiprz_scene::tris as uploaded, -1 on a miss */
} hiprz_hit; /* 48 B */

#define HIPRZ_QUERY_NORMALIZE 1u /* `flags` of the calls below */

/* Bound to one context and answering on its head device; pinned staging for the host-pointer calls, grown on demand.  One call at a time
 * per query.  HIPRZ_ERR_DEVICE without a HIP device.  The query must be destroyed before its context. */
typedef struct hiprz_query hiprz_query;
int hiprz_query_create(hiprz_query** out, hiprz_ctx* ctx);
int hiprz_query_destroy(hiprz_query* query);
const char* hiprz_query_last_error(const hiprz_query* query); /* NULL: the last error of a call without a query, on this thread */

/* Every call that takes a `stream` (a hipStream_t) only enqueues; NULL = hiprz_stream(ctx), the stream scene uploads, refits and rebuilds
 * are ordered on, so a query after an update sees the update.  Device arrays are 16-byte aligned (whatever hipMalloc returns is).  Entries
 * past n are never written; n == 0 is HIPRZ_OK without a launch.
 * Refused before anything is launched or copied: a null query or pointer, a flag other than HIPRZ_QUERY_NORMALIZE, n >= 2^31
 * (HIPRZ_ERR_INVALID); a context without a scene (HIPRZ_ERR_STATE); a libhiprz.so compiled from other device views (HIPRZ_ERR_INVALID from
 * hiprz_device_view).  hiprz_device_view also refuses a part of a multi-device context, so a query bound to one would fail at its first
 * call; no call of include/hiprz.h hands a part's handle out today, so that refusal cannot be reached (or tested) from outside. */
int hiprz_query_closest(hiprz_query* query, const hiprz_ray* rays_device, size_t n, uint32_t flags, hiprz_hit* hits_out_device, void* stream);
int hiprz_query_occluded(hiprz_query* query, const hiprz_ray* rays_device, size_t n, uint32_t flags, uint32_t* out_device, void* stream);

/* The same for host pointers: copied through the query's pinned staging on the context's stream, which is waited for once. */
int hiprz_query_closest_host(hiprz_query* query, const hiprz_ray* rays, size_t n, uint32_t flags, hiprz_hit* hits_out);
int hiprz_query_occluded_host(hiprz_query* query, const hiprz_ray* rays, size_t n, uint32_t flags, uint32_t* out);

/* The W*H pixel-centre rays of the selected camera, row-major, by generate_simple_ray: the rays the first pass, the guides and
 * hiprz_ray_cast walk (unit directions: feed them back without NORMALIZE).  HIPRZ_ERR_STATE before a camera. */
int hiprz_query_pixel_rays(hiprz_query* query, hiprz_ray* rays_out_device, void* stream);

/* sizeof(hiprz_ray), sizeof(hiprz_hit) and the offsets of hiprz_ray::direction, hiprz_hit::flags, ::instance, ::normal and
 * ::scene_triangle as this library was compiled */
void hiprz_query_layout(uint32_t out[7]);

#ifdef __cplusplus
}
#endif
#endif
