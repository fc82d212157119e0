/* hiprz_gather.h — bounce baking: the light that reaches a surface point after one bounce, gathered on the device from an atlas that
 * already holds light (libhiprz_gather.so).
 *
 * An occlusion bake (include/hiprz_bake.h) answers how much of the hemisphere a point sees, a light bake (include/hiprz_light.h) how much
 * light reaches it straight from the scene's lights.  A lightmap also needs what arrives after a bounce: the red of the wall beside a
 * white one, the light of an emissive surface.  This library reads 32 bytes per POINT, makes the point's K hemisphere rays from a table of
 * directions, walks each to its CLOSEST hit, finds the atlas texel under the hit through a chart map the caller has set, and writes 16
 * bytes per point: the mean of what the atlas holds there.  Neither the K rays (32 bytes each) nor their hits (48 bytes each) exist in
 * memory.  A library of its own for the reasons the other seven are: their kernel sets and exports are pinned, and a caller that never
 * gathers runs no code of this library.  It links against libhiprz.so alone.  It reads the context through hiprz_device_view
 * (include/hiprz.h) on EVERY call and caches nothing an upload could make stale: a gather after hiprz_update_instances sees the change.
 *
 * Every rule below is plain float32, one rounding per operation (no fused multiply-add), true division and square root.
 *
 * THE POINT: a hiprz_bake_point, 32 bytes, the layout and the validity rule of hiprz_bake.h — position, near_, normal, far_; INVALID exactly
 * when the ray (position, near_, normal, far_) is invalid under HIPRZ_QUERY_NORMALIZE (the query's own device function decides).  n is
 * the normalised normal.  An invalid point walks no ray and affects no other point.
 *
 * THE DIRECTIONS, THE SET OF A POINT, THE FRAME and THE RAY are those of hiprz_bake.h, restated here: S sets (1 <= S <= 64) of K unit
 * directions in the local frame, z along the normal, S*K float4 (x, y, z, ignored), set-major; K is one of 16, 32, 64, 128, 256, 512,
 * 1024; every component finite and the float32 squared length (x*x + y*y) + z*z in [0.999, 1.001].  Point i uses set
 * hiprz_bake_hash(i ^ seed) % S, on uint32_t
 *     x ^= x >> 16;  x *= 0x7feb352du;  x ^= x >> 15;  x *= 0x846ca68bu;  x ^= x >> 16;
 * The frame of the normalised normal n (Duff et al.):
 *     s = copysignf(1, n.z);   a = -1.0f / (s + n.z);   b = (n.x * n.y) * a;
 *     t  = ( 1.0f + ((s * n.x) * n.x) * a,   s * b,                   (-s) * n.x );
 *     bt = ( b,                              s + (n.y * n.y) * a,     -n.y       );
 * and the world direction of the table's l, per component c:
 *     d.c = (t.c * l.x + bt.c * l.y) + n.c * l.z
 * The ray of (point i, direction k) is origin = position, near_, direction = d, far_: the ray hiprz_bake_rays emits for the same table and
 * seed, bit for bit.  hiprz_bake_cosine_directions is the intended table: with cosine-weighted directions the plain mean below is the
 * cosine-weighted integral over the hemisphere divided by pi.  The ray is walked WITHOUT HIPRZ_QUERY_NORMALIZE by the closest-hit walk of
 * hiprz_query_closest (the same device function, ties between equally distant triangles included), so t, the instance and the triangle
 * are that call's on the same ray by construction, the invalid-ray rule included.
 *
 * THE CHART MAP says which atlas triangle a hit lies on.  One uint32_t `base` per instance of the scene, HIPRZ_GATHER_NONE for an instance
 * that is not in the atlas; one 32-byte hiprz_gather_chart per chart id, (u1, v1, u2, v2, u3, v3, 0, 0) in atlas units — the UVs of the
 * hiprz_atlas_tri with that id (include/hiprz_atlas.h).  A hit on instance I and mesh triangle T has chart id base[I] + T, with T =
 * hiprz_tri::source_index of the triangle hit: the position of the triangle in its mesh as uploaded.  An id >= n_charts (the sum is
 * taken on 64 bits) is unmapped.  Charts made from a mesh in its own triangle order and atlas parts numbered through in list order are
 * therefore mapped by base = the running sum of the parts' triangle counts.
 *
 * THE SOURCE: W x H 16-byte records on the device, row-major (texel (x, y) at y * W + x): RGB float and one word.  A texel HAS A VALUE
 * when its word is not 0x80000000 (HIPRZ_GATHER_INVALID = HIPRZ_LIGHT_INVALID = HIPRZ_BAKE_INVALID): light texels, after the atlas's
 * dilation, can be fed in as they are.  1 <= W, H <= 16384.
 *
 * THE LOOKUP of a front-face hit (the walk's `external`) with the walk's bx and by, the weights of vertices 2 and 3:
 *     b1 = (1.0f - bx) - by
 *     u  = (u1 * b1 + u2 * bx) + u3 * by          v = (v1 * b1 + v2 * bx) + v3 * by
 *     x  = clamp(int(floorf(u * float(W))), 0, W - 1)          y = clamp(int(floorf(v * float(H))), 0, H - 1)
 * (the clamp is taken on the float before the conversion: a product beyond the integers clamps like any other).  A u or v that is not
 * finite is unmapped.
 *
 * A RAY'S CONTRIBUTION: a ray without a hit — a miss, an empty world, an invalid ray (a d whose squared length leaves [0.99, 1.01])
 * — contributes the call's sky[3] and counts as MISSED.  A front-face hit whose texel has a value contributes the texel's RGB and counts
 * as READ.  Everything else contributes +0 and is counted nowhere: a back-face hit, a hit on an instance or an id that is unmapped, a
 * texel without a value.
 *
 * THE RESULT, 16 bytes, one store.  Per colour component: lane j = k % 64 starts at +0 and for rounds r = 0, 1, ... adds the contribution
 * of ray k = 64 r + j; then for off = 1, 2, 4, ..., min(K, 64) / 2 every lane does v = v + v[lane ^ off] (the order hiprz_bake.h fixes
 * for `bent`); then mean.c = v * (1.0f / float(K)).  `counts`: bits 0 - 15 the exact number of rays READ, bits 16 - 30 the exact number
 * MISSED.  An invalid point reads mean = +0 and counts = HIPRZ_GATHER_INVALID.
 *
 * THE SAMPLES: hiprz_gather_samples writes what the gather walks, one 16-byte record per (point i, direction k) at i * K + k:
 * {id, bx, by, t}.  id is the chart id of a front-face hit, or HIPRZ_GATHER_MISS (no hit), HIPRZ_GATHER_UNMAPPED (a front-face hit on an
 * instance or id outside the chart map), HIPRZ_GATHER_BACK (a back-face hit) or HIPRZ_GATHER_INVALID_RAY (the ray is invalid: an invalid
 * point, whose ray has the direction +0, or a d outside the length rule).  bx and by are the walk's for any hit and +0 otherwise; t is the
 * walk's ray.far_: the distance of a hit, the ray's own far_ otherwise.  The gather calls the device function that makes this record.
 *
 * COMPOSE, one radiosity step per texel on the device, all arrays W*H 16-byte records:
 *     out.c = (albedo.c * (direct.c + indirect.c)) + emission.c          out.word = direct.word
 * `indirect` and `emission` may be null, which reads +0 for every component.  `out` may be `indirect` (a thread reads before it writes).
 *
 * THE MEANING: in the renderer's convention (a diffuse surface returns its colour times what arrives), light + gathered is a texel's
 * irradiance in that convention when the source holds albedo x (light + gathered of the bounce before) + emission: hiprz_light_texel::light for the
 * scene's lights plus hiprz_gather_texel::mean for everything a diffuse surface sends on.  Left out on purpose:
 *   - glossy transport: every surface bounces as a diffuse one (roughness is not read);
 *   - transmission: a hit ends the ray whatever the opacity of the material (no material is fetched);
 *   - the scattering medium of the world material: a bake is of surfaces in a clear medium.
 *
 * THE KERNELS, no LDS, no atomics.  rz_gather_kernel, 64 threads per workgroup (one wave): for K >= 64 one wave gathers one point in
 * K / 64 rounds; for K < 64 one wave gathers 64 / K consecutive points, one ray per lane.  Lanes that are out of range or invalid take
 * part in every ballot and shuffle.  The walk fetches no material, texture or normal: the instance, the triangle's source index, bx, by
 * and the side are all it needs.  rz_gather_samples_kernel: one thread per (point, k).  rz_gather_compose_kernel: one thread per texel. */
#ifndef HIPRZ_GATHER_H
#define HIPRZ_GATHER_H

#include <stddef.h>
#include <stdint.h>

#include "hiprz_bake.h" /* hiprz_bake_point; hiprz.h: hiprz_ctx, the return codes */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hiprz_gather_texel {
    float mean[3];
    uint32_t counts; /* bits 0 - 15: rays that read a texel value; bits 16 - 30: rays that missed; HIPRZ_GATHER_INVALID */
} hiprz_gather_texel; /* 16 B */

typedef struct hiprz_gather_sample {
    uint32_t id; /* a chart id or one of the four codes */
    float bx, by;
    float t;
} hiprz_gather_sample; /* 16 B */

typedef struct hiprz_gather_chart {
    float u1, v1, u2, v2, u3, v3;
    float zero[2];
} hiprz_gather_chart; /* 32 B */

#define HIPRZ_GATHER_INVALID 0x80000000u
#define HIPRZ_GATHER_NONE 0xFFFFFFFFu
#define HIPRZ_GATHER_MISS 0xFFFFFFFFu
#define HIPRZ_GATHER_UNMAPPED 0xFFFFFFFEu
#define HIPRZ_GATHER_BACK 0xFFFFFFFDu
#define HIPRZ_GATHER_INVALID_RAY 0xFFFFFFFCu
#define HIPRZ_GATHER_MAX_CHARTS 0xFFFFFFFCu /* chart ids lie below the codes */
#define HIPRZ_GATHER_MAX_SIZE 16384u

/* Bound to one context and answering on its head device.  It owns the direction table, the chart map, the device copy of a host source and
 * the pinned staging of the host-pointer call, grown on demand.  One call at a time per handle.  HIPRZ_ERR_DEVICE without a HIP device.
 * Destroy it before its context. */
typedef struct hiprz_gather hiprz_gather;
int hiprz_gather_create(hiprz_gather** out, hiprz_ctx* ctx);
int hiprz_gather_destroy(hiprz_gather* gather);
const char* hiprz_gather_last_error(const hiprz_gather* gather); /* NULL: the last error of a call without a handle, on this thread */

/* S*K float4 (x, y, z, ignored) from the host, checked as hiprz_bake_set_directions checks them (HIPRZ_ERR_INVALID, the table before
 * stays).  The handle keeps the table; it reaches the device with the next call below, on that call's stream.  That one call waits for
 * its stream (the copy reads pageable memory); every later call with the same table only enqueues. */
int hiprz_gather_set_directions(hiprz_gather* gather, const float* xyz0_host, uint32_t K, uint32_t S);

/* THE CHART MAP from the host: n_instances bases and n_charts charts (either array may be null when its count is 0).  Refused with
 * HIPRZ_ERR_INVALID, the map before stays: a null handle or pointer, n_charts > HIPRZ_GATHER_MAX_CHARTS, a UV that is not finite.  It
 * reaches the device as the table does.  The number of instances is held against the view's at every call that walks. */
int hiprz_gather_set_charts(hiprz_gather* gather, const uint32_t* base_host, uint32_t n_instances, const hiprz_gather_chart* uv_host, uint32_t n_charts);

/* Every call that takes a `stream` (a hipStream_t) only enqueues; NULL = hiprz_stream(ctx).  Device arrays are 16-byte aligned.  Entries
 * past n (past n*K for the samples) are never written; n == 0 is HIPRZ_OK without a view or a launch.  Refused before anything is
 * launched or copied, in this order: a null handle or pointer (HIPRZ_ERR_INVALID), no direction table or no chart map set
 * (HIPRZ_ERR_STATE), n*K >= 2^31 (HIPRZ_ERR_INVALID), for the gather a W or H outside 1 .. HIPRZ_GATHER_MAX_SIZE (HIPRZ_ERR_INVALID),
 * whatever hiprz_device_view refuses (a context without a scene: HIPRZ_ERR_STATE), a chart map for another number of instances than the
 * view's (HIPRZ_ERR_INVALID). */
int hiprz_gather_texels(hiprz_gather* gather, const hiprz_bake_point* points_device, size_t n, uint32_t seed, const void* source16_device, uint32_t W,
                        uint32_t H, const float sky[3], hiprz_gather_texel* out_device, void* stream);
int hiprz_gather_samples(hiprz_gather* gather, const hiprz_bake_point* points_device, size_t n, uint32_t seed, hiprz_gather_sample* samples_out_device,
                         void* stream);

/* The gather for host pointers, the source included: the points and texels go through the handle's pinned staging on the context's stream,
 * which is waited for once; the source goes to a device copy the handle owns. */
int hiprz_gather_texels_host(hiprz_gather* gather, const hiprz_bake_point* points, size_t n, uint32_t seed, const void* source16, uint32_t W, uint32_t H,
                             const float sky[3], hiprz_gather_texel* out);

/* COMPOSE over n_texels records on the device; `indirect` and `emission` may be null.  No table, map or scene is needed: refused are a
 * null handle, a null direct, albedo or out (HIPRZ_ERR_INVALID) and n_texels >= 2^31 (HIPRZ_ERR_INVALID); n_texels == 0 is HIPRZ_OK. */
int hiprz_gather_compose(hiprz_gather* gather, const void* direct16_device, const void* indirect16_device, const void* albedo16_device,
                         const void* emission16_device, void* out16_device, size_t n_texels, void* stream);

/* COMPOSE for host arrays (a host without a device allocator of its own, the C++ Engine): copied through device buffers of the call on
 * the context's stream, which is waited for.  The refusals of hiprz_gather_compose, then whatever hiprz_device_view refuses (a context
 * without a scene: HIPRZ_ERR_STATE) — the view is what makes the context's device the current one. */
int hiprz_gather_compose_host(hiprz_gather* gather, const void* direct16, const void* indirect16, const void* albedo16, const void* emission16, void* out16,
                              size_t n_texels);

/* sizeof(hiprz_bake_point), sizeof(hiprz_gather_texel), sizeof(hiprz_gather_sample), sizeof(hiprz_gather_chart) and the offsets of
 * hiprz_gather_texel::counts, hiprz_gather_sample::bx, ::t and hiprz_gather_chart::u3 as this library was compiled */
void hiprz_gather_layout(uint32_t out[8]);

#ifdef __cplusplus
}
#endif
#endif
