/* hiprz_atlas.h — bake atlases: UV charts rasterised on the device into one surface point per texel, and the dilation that fills the
 * gutters of what was baked per texel (libhiprz_atlas.so).
 *
 * hiprz_bake.h bakes surface points the caller supplies.  This library makes them in texture space: the caller's triangles carry, per
 * vertex, a position and a normal in the mesh's own space and a UV in atlas units; every texel of a W x H atlas whose centre a triangle
 * covers becomes the hiprz_bake_point of that place on the instance as the context holds it NOW, the array goes straight to
 * hiprz_bake_occlusion, and hiprz_atlas_dilate then spreads the baked texels over the gutters between the charts.  The charts are the
 * caller's, not the scene's device copy: lightmap UVs are a second unwrap the scene does not carry, and the device's triangle order is no
 * interface.  A library of its own for the reasons the query, order and bake libraries are; it reads the context through
 * hiprz_device_view (include/hiprz.h) on EVERY add and caches nothing an upload could make stale.
 *
 * Every rule is plain float32 with one rounding per operation (-ffp-contract=off, true divisions and square roots).
 *
 * THE TRIANGLE, 96 bytes, six 16-byte loads: (p1.xyz, u1) (p2.xyz, u2) (p3.xyz, u3) (n1.xyz, v1) (n2.xyz, v2) (n3.xyz, v3).  (u, v) are
 * in atlas units: [0, 1]^2 is the atlas, nothing wraps.  A triangle whose nine normal components are all +-0 uses its face normal
 * normalize(cross(p2 - p3, p2 - p1)), the formula of hiprz_tri_attr::face_normal.
 *
 * TEXEL SPACE: vertex i lies at a_i = (u_i * float(W) - 0.5f, v_i * float(H) - 0.5f); texel (x, y) is the point (float(x), float(y)).
 *
 * THE EDGE VALUE: order the two endpoints of an edge so that the one with the smaller x comes first, ties broken by the smaller y: A, B.
 *     e(p) = (B.x - A.x) * (p.y - A.y) - (B.y - A.y) * (p.x - A.x)
 * A triangle that walks the edge from A to B uses e, one that walks it from B to A uses -e: the two triangles on either side of a shared
 * edge see exact negatives of one float, so no texel is refused by both.
 *
 * ORIENTATION: area = the oriented value of edge 1->2 at a_3.  A triangle is DEGENERATE when any of its 24 floats is not finite or area
 * is zero or not finite; it covers nothing.  Otherwise s = +1 or -1 by the sign of area: mirrored charts are valid.
 *
 * COVERAGE: with w1, w2, w3 the oriented values at (x, y) of the edges 2->3, 3->1 and 1->2, texel (x, y) is covered when
 *     s*w1 >= 0 and s*w2 >= 0 and s*w3 >= 0,   0 <= x < W,  0 <= y < H,
 *     min(a_1.x, a_2.x, a_3.x) <= float(x) <= max(a_1.x, a_2.x, a_3.x)   and the same in y
 * (the last line is what every point of the triangle satisfies exactly; it makes the bounding box the kernel steps through part of the
 * rule instead of an assumption about rounding).  The test is inclusive on every edge; of several triangles covering a texel the one with
 * the LOWEST ID owns it.
 *
 * THE SAMPLE, 16 bytes, one store: the owner's id, bx = (s*w2) / (s*area) and by = (s*w3) / (s*area) — the weights of vertices 2 and 3 —
 * and a zero word.  A texel nothing covers: HIPRZ_ATLAS_NONE, 0, 0, 0.
 *
 * THE POINT, a hiprz_bake_point.  b1 = (1.0f - bx) - by.  With position, scale and the axes xa, ya, za of the instance record:
 *     p = (p1 * b1 + p2 * bx) + p3 * by          q = p * scale          position_out = ((xa * q.x + ya * q.y) + za * q.z) + position
 *     n = (n1 * b1 + n2 * bx) + n3 * by   (or the face normal)
 *     normal_out = normalized(transform_forward(xa, ya, za, normalized(n) / scale))
 * with normalized(v) = v * (1.0f / sqrtf((x*x + y*y) + z*z)) and transform_forward(v) = (xa * v.x + ya * v.y) + za * v.z: the inverse of
 * the renderer's to_local and the normal steps of its analyze_intersection.  near_ and far_ are the call's.  A normal that comes out
 * zero or not finite is written as +0, which the bake flags HIPRZ_BAKE_INVALID by its own rule; an uncovered texel is 32 zero bytes,
 * which the bake treats the same.
 *
 * DILATION works in place on any array of W*H 16-byte records.  A texel HAS A VALUE when its sample's triangle is not HIPRZ_ATLAS_NONE.
 * For ring r = 1 ... rings, reading the state before that ring: a texel without a value takes the 16 bytes of the first of its
 * neighbours (x-1, y) (x+1, y) (x, y-1) (x, y+1) (x-1, y-1) (x+1, y-1) (x-1, y+1) (x+1, y+1) that lies in the atlas and has one, and
 * then has a value.  The ring map reads 0 for a covered texel, r for one filled in ring r, HIPRZ_ATLAS_NONE otherwise.
 *
 * THE KERNELS, 64 threads per workgroup (one wave), no LDS, vector atomics only.  rz_atlas_clear_kernel: the owner map to NONE.
 * rz_atlas_cover_kernel: grid.x over the triangles, grid.y a fixed number of helpers; a wave is an 8x8 block of texels and helper h takes
 * the blocks h, h + grid.y, ... of the triangle's clipped bounding box; atomicMin(&owner[texel], id), so the map does not depend on the
 * launch shape.  rz_atlas_points_kernel: one thread per texel, two 16-byte stores for the point and one for the sample.
 * rz_atlas_dilate_kernel: one thread per texel and ring, records and ring map ping-ponged through the handle's scratch. */
#ifndef HIPRZ_ATLAS_H
#define HIPRZ_ATLAS_H

#include <stddef.h>
#include <stdint.h>

#include "hiprz_bake.h" /* hiprz_bake_point; hiprz.h: hiprz_ctx, the return codes */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiprz_atlas_tri {
    float p1[3], u1;
    float p2[3], u2;
    float p3[3], u3;
    float n1[3], v1;
    float n2[3], v2;
    float n3[3], v3;
} hiprz_atlas_tri; /* 96 B */

typedef struct hiprz_atlas_sample {
    uint32_t triangle; /* the owner's id or HIPRZ_ATLAS_NONE */
    float bx, by;      /* the weights of vertices 2 and 3 */
    uint32_t zero;
} hiprz_atlas_sample; /* 16 B */

#define HIPRZ_ATLAS_NONE 0xFFFFFFFFu
#define HIPRZ_ATLAS_MAX_SIZE 16384u
#define HIPRZ_ATLAS_MAX_RINGS 64u

/* Bound to one context and working on its head device.  It owns the owner map (uint32_t per texel), the point array, the sample array,
 * a record array of 16 bytes per texel for what the caller bakes, the dilation scratch and the pinned staging of the host-pointer calls,
 * all allocated on demand and kept while a later begin asks for no more texels.  One call at a time per handle.  HIPRZ_ERR_DEVICE without
 * a HIP device.  Destroy it before its context. */
typedef struct hiprz_atlas hiprz_atlas;
int hiprz_atlas_create(hiprz_atlas** out, hiprz_ctx* ctx);
int hiprz_atlas_destroy(hiprz_atlas* atlas);
const char* hiprz_atlas_last_error(const hiprz_atlas* atlas); /* NULL: the last error of a call without a handle, on this thread */

/* sizeof(hiprz_atlas_tri), sizeof(hiprz_atlas_sample), sizeof(hiprz_bake_point) and the offsets of hiprz_atlas_tri::n1, ::v3,
 * hiprz_atlas_sample::bx, ::by and ::zero as this library was compiled */
void hiprz_atlas_layout(uint32_t out[8]);

/* Host only: a new atlas of width x height texels, 1 <= width, height <= HIPRZ_ATLAS_MAX_SIZE (else HIPRZ_ERR_INVALID and the atlas
 * before stays).  The next add clears the owner map; what the device arrays held is forgotten. */
int hiprz_atlas_begin(hiprz_atlas* atlas, uint32_t width, uint32_t height);

/* Every call that takes a `stream` (a hipStream_t) only enqueues; NULL = hiprz_stream(ctx).  Device arrays are 16-byte aligned.
 *
 * n triangles, triangle i with the id triangle_base + i, placed as instance `instance` is in the device view fetched in THIS call.  The
 * first add after a begin writes every texel, uncovered ones as zeros (n == 0 included); a later add writes only the texels whose owner
 * lies in its own id range.  After any sequence of adds with disjoint id ranges the atlas is what one add of all the triangles would
 * give, whatever the order.  Refused before anything is launched or copied: a null handle or pointer (HIPRZ_ERR_INVALID; the pointer
 * may be null when n == 0), no begin (HIPRZ_ERR_STATE), triangle_base + n >= 0xFFFFFFFF (HIPRZ_ERR_INVALID), a near_ or far_ that makes
 * every point invalid — either not finite, near_ < 0 or far_ <= near_ (HIPRZ_ERR_INVALID), a context without a scene (HIPRZ_ERR_STATE)
 * and whatever else hiprz_device_view refuses, instance >= the view's n_instances (HIPRZ_ERR_INVALID). */
int hiprz_atlas_add(hiprz_atlas* atlas, const hiprz_atlas_tri* tris_device, size_t n, uint32_t triangle_base, uint32_t instance, float near_, float far_,
                    void* stream);
/* The same for host triangles: copied through the handle's pinned staging on the context's stream, which is waited for once. */
int hiprz_atlas_add_host(hiprz_atlas* atlas, const hiprz_atlas_tri* tris, size_t n, uint32_t triangle_base, uint32_t instance, float near_, float far_);

/* The device arrays of width*height entries, row-major (texel (x, y) at y * width + x), valid until the next begin or destroy; NULL
 * before the first add after a begin.  The points can be handed straight to hiprz_bake_occlusion on the same stream. */
const hiprz_bake_point* hiprz_atlas_points_device(const hiprz_atlas* atlas);
const hiprz_atlas_sample* hiprz_atlas_samples_device(const hiprz_atlas* atlas);

/* Either or both arrays to the host (either pointer may be null, not both); waits for the context's stream.  HIPRZ_ERR_STATE before the
 * first add after a begin. */
int hiprz_atlas_read_host(hiprz_atlas* atlas, hiprz_bake_point* points_out, hiprz_atlas_sample* samples_out);

/* A device array of width*height 16-byte records that the handle owns, for what is baked per texel: the out array of hiprz_bake_occlusion
 * over the points and the array hiprz_atlas_dilate then works on, so that a host without a device allocator of its own (the C++ Engine)
 * bakes an atlas without the points ever visiting it.  The library itself never writes it.  Valid as the arrays above; NULL before the
 * first add after a begin. */
void* hiprz_atlas_records_device(const hiprz_atlas* atlas);
/* That array and / or the ring map of the last hiprz_atlas_dilate since the begin to the host (either pointer may be null, not both);
 * waits for the context's stream.  HIPRZ_ERR_STATE before the first add after a begin, and for a ring map before a dilation. */
int hiprz_atlas_read_records_host(hiprz_atlas* atlas, void* records16_out, uint32_t* ring_out);

/* DILATION above, in place on width*height 16-byte records on the device (bake texels, or anything else baked per texel); ring_out_device,
 * which may be null, receives the ring map.  rings <= HIPRZ_ATLAS_MAX_RINGS; rings == 0 writes only the ring map.  HIPRZ_ERR_STATE
 * before the first add after a begin: the samples say which texels have a value. */
int hiprz_atlas_dilate(hiprz_atlas* atlas, void* records16_device, uint32_t rings, uint32_t* ring_out_device, void* stream);
/* The same for host arrays, through the pinned staging on the context's stream, which is waited for once. */
int hiprz_atlas_dilate_host(hiprz_atlas* atlas, void* records16, uint32_t rings, uint32_t* ring_out);

#ifdef __cplusplus
}
#endif
#endif
