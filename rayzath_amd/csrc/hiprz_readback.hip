// hiprz_readback.hip — from the parts' tile-major buffers to frames: tone map, frame assembly and the reads (hiprz_read_*), the sums of
// HIPRZ_SHARD_SAMPLES, the variance estimate, the history of a restarted frame, tile export (hiprz_export_*_tiles, hiprz_untile_*), the ray
// cast, and pipelined delivery (hiprz_present / hiprz_read_frame): the readback of cuda_engine_core.cu, the tone map of
// cuda_postprocess_kernel.cu.  A multi-part head (hiprz_create_multi) collects its peers' buffers through the two stagings of
// hiprz_ctx.hpp (PartStaging: push_part, mark_consumed, part_geometry); no code here touches a staging's event itself.
#include <hip/hip_runtime.h>

#include <string>

#include "hiprz.h"
#include "hiprz_ctx.hpp"
#include "hiprz_device.hpp"

using namespace hiprz;

// ---- kernels: tone map, sums of parts, variance, tile <-> image, picking, present ----
// toneMap (cuda_postprocess_kernel.cu:38-93; CPU: cpu_engine_renderer.cpp:224-235)
__global__ void __launch_bounds__(256) rz_tonemap_tiles_kernel(const float4* accum, uint32_t* rgba8, uint32_t n, float aperture,
                                                               float exposure_time) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 a = accum[i];
    rgba8[i] = tonemap(col4{a.x, a.y, a.z, a.w}, aperture, exposure_time);
}
__global__ void __launch_bounds__(256) rz_tonemap_image_kernel(const float4* image, uint32_t* rgba8, uint32_t n, float aperture,
                                                               float exposure_time) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 a = image[i];
    rgba8[i] = tonemap(col4{a.x, a.y, a.z, a.w}, aperture, exposure_time);
}

// HIPRZ_SHARD_SAMPLES: the parts of a context rendered the same pixels on different seed streams; what leaves the context is the sum of
// their accumulators (colour sums and finished-path counts), taken in part order — own + staged[0] + staged[1] + ... — so that the
// result does not depend on when a part finished
__global__ void __launch_bounds__(256) rz_sum_parts_kernel(const float4* own, const float4* staged, size_t stride, uint32_t n_staged, float4* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    float4 a = own[i];
    for (uint32_t r = 0; r < n_staged; ++r) {
        const float4 b = staged[size_t(r) * stride + i];
        a.x += b.x, a.y += b.y, a.z += b.z, a.w += b.w;
    }
    out[i] = a;
}

// the estimate of hiprz_read_variance from the accumulator and the moments, per local pixel
RZ_DEV float variance_of(float R, float A, float S2, float S1, float SA, float K) {
    const float r = R / A;
    const float E = fmaxf(0.0f, (S2 - (2.0f * r) * S1) + (r * r) * SA);
    return (E * (K / (K - 1.0f))) / (A * A);
}
__global__ void __launch_bounds__(256) rz_variance_kernel(const float4* accum, const float4* m0, const float4* m1, float4* out, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 a = accum[i], u = m0[i], v = m1[i];
    float4 o = make_float4(0.0f, 0.0f, 0.0f, v.w);
    if (v.w >= 2.0f) o.x = variance_of(a.x, a.w, u.x, v.x, u.w, v.w), o.y = variance_of(a.y, a.w, u.y, v.y, u.w, v.w), o.z = variance_of(a.z, a.w, u.z, v.z, u.w, v.w);
    out[i] = o;
}

// tile-major (owned tiles of shard rank/world) -> row-major full frame
template <typename T>
__global__ void __launch_bounds__(256) rz_untile_kernel(const T* tiles, T* image, uint32_t width, uint32_t height,
                                                        uint32_t tiles_x, uint32_t rank, uint32_t world) {
    uint32_t tx, ty;
    shard_tile(blockIdx.x, tiles_x, rank, world, tx, ty);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = tx * 32u + wave * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
    if (x < width && y < height) image[size_t(y) * width + x] = tiles[size_t(blockIdx.x) * 256u + threadIdx.x];
}
// the gathered tiles of ALL shards (shard r at tiles + r * part_stride elements) -> row-major full frame, one launch
// (slice blockIdx.y holds shard rank0 + blockIdx.y of `world`)
template <typename T>
__global__ void __launch_bounds__(256) rz_untile_gathered_kernel(const T* tiles, size_t part_stride, T* image, uint32_t width, uint32_t height,
                                                                 uint32_t tiles_x, uint32_t n_tiles, uint32_t world, uint32_t rank0) {
    const uint32_t part = blockIdx.y;
    if (blockIdx.x * world + rank0 + part >= n_tiles) return;  // the higher shards own one tile less
    uint32_t tx, ty;
    shard_tile(blockIdx.x, tiles_x, rank0 + part, world, tx, ty);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = tx * 32u + wave * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
    if (x < width && y < height) image[size_t(y) * width + x] = tiles[part * part_stride + size_t(blockIdx.x) * 256u + threadIdx.x];
}
__global__ void __launch_bounds__(256) rz_untile_state_kernel(const float4* st0, const float4* st1, const float2* st2, float* ray9,
                                                              uint32_t* md2, uint32_t width, uint32_t height, uint32_t tiles_x,
                                                              uint32_t rank, uint32_t world) {
    uint32_t tx, ty;
    shard_tile(blockIdx.x, tiles_x, rank, world, tx, ty);
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    const uint32_t x = tx * 32u + wave * 8u + (lane & 7u), y = ty * 8u + (lane >> 3);
    if (x >= width || y >= height) return;
    const size_t i = size_t(blockIdx.x) * 256u + threadIdx.x, o = size_t(y) * width + x;
    const float4 a = st0[i], b = st1[i];
    const float2 c = st2[i];
    float* r = ray9 + 9 * o;
    r[0] = a.x, r[1] = a.y, r[2] = a.z, r[3] = a.w, r[4] = b.x, r[5] = b.y, r[6] = b.z, r[7] = b.w, r[8] = c.x;
    const uint32_t bits = __float_as_uint(c.y);
    md2[2 * o] = bits & 0xFFFFu;
    md2[2 * o + 1] = (bits >> 16) & 0xFFu;
}

// Kernel::rayCast (cpu_engine_kernel.cpp:102-111, 483-501): one thread.
__device__ inline void pick_at(const DScene& s, const DCamera& cam, uint32_t x, uint32_t y, float depth, int32_t* out4) {
    Ray ray;
    generate_simple_ray(cam, ray, x, y);
    ray.near_ = depth * 0.99f;
    ray.far_ = depth * 1.01f;
    Hit hit;
    hit.instance = -1, hit.triangle = 0u, hit.bx = hit.by = 0.0f, hit.external = true;
    Counters cnt;
    out4[0] = out4[1] = out4[2] = -1, out4[3] = 0;
    if (s.n_instances != 0u && closest_hit_skip<false, false, true>(s, TopCache{nullptr, nullptr, 0u}, ray, hit, cnt) == 2) {
        const uint32_t inst = uint32_t(hit.instance);
        const uint32_t material_base = __float_as_uint(s.instances[7 * inst + 1].w);
        const uint32_t material_count = __float_as_uint(s.instances[7 * inst + 2].w);
        uint32_t slot = __float_as_uint(s.tris[3 * hit.triangle].w) & HIPRZ_TRI_MATERIAL_MASK;
        if (slot > 63u) slot = 63u;
        out4[0] = hit.instance;
        out4[1] = int32_t(slot);
        out4[2] = slot < material_count ? s.inst_materials[material_base + slot] : -1;
        out4[3] = int32_t(__float_as_uint(s.tris[3 * hit.triangle + 1].w));  // hiprz_tri::source_index
    }
}
__global__ void rz_pick_kernel(const DScene s, const DCamera cam, uint32_t x, uint32_t y, float depth, int32_t* out4) {
    pick_at(s, cam, x, y, depth, out4);
}
// hiprz_present: the same ray cast with the depth taken from the assembled row-major frame on the device (no host round trip).  `owned`: a
// part of this context rendered pixel (x, y) — hiprz_ray_cast answers "nothing met" for pixels of shards rendered elsewhere.
__global__ void rz_pick_slot_kernel(const DScene s, const DCamera cam, uint32_t x, uint32_t y, uint32_t owned, const float* depth, int32_t* out4) {
    if (!owned) {
        out4[0] = out4[1] = out4[2] = -1, out4[3] = 0;
        return;
    }
    pick_at(s, cam, x, y, depth[size_t(y) * cam.width + x], out4);
}

// hiprz_present: tile-major rgba8 + depth -> the row-major frame slot, both images in one launch.  One workgroup per 32x8 tile of shard
// rank0 + blockIdx.y of `world`; thread t moves pixel (t % 32, t / 32) of its tile, so that every 32 lanes store one row of the tile as 128
// contiguous bytes per image (the reads gather 4 runs of 8 pixels: the in-tile order is ((x%32)/8)*64 + (y%8)*8 + x%8).
// Gathered = false: the context's own tiles (blockIdx.y = 0).  Gathered = true: slice 0 is the head's own, slice r >= 1 the tiles peer r
// pushed into the head's present_gather (`parts_* + (r - 1) * stride`).
template <bool Gathered>
__global__ void __launch_bounds__(256) rz_present_kernel(const uint32_t* own_rgba8, const float* own_depth, const uint32_t* parts_rgba8,
                                                         const float* parts_depth, size_t stride, uint32_t* rgba8, float* depth, uint32_t width,
                                                         uint32_t height, uint32_t tiles_x, uint32_t n_tiles, uint32_t world, uint32_t rank0) {
    const uint32_t part = Gathered ? blockIdx.y : 0u;
    if (blockIdx.x * world + rank0 + part >= n_tiles) return;  // the higher shards own one tile less
    uint32_t tx, ty;
    shard_tile(blockIdx.x, tiles_x, rank0 + part, world, tx, ty);
    const uint32_t xr = threadIdx.x & 31u, yr = threadIdx.x >> 5;
    const uint32_t x = tx * 32u + xr, y = ty * 8u + yr;
    if (x >= width || y >= height) return;
    const size_t src = size_t(blockIdx.x) * 256u + (xr >> 3) * 64u + yr * 8u + (xr & 7u);
    uint32_t c;
    float d;
    if (Gathered && part != 0u) {
        c = parts_rgba8[(part - 1u) * stride + src];
        d = parts_depth[(part - 1u) * stride + src];
    } else {
        c = own_rgba8[src];
        d = own_depth[src];
    }
    const size_t o = size_t(y) * width + x;
    rgba8[o] = c;
    depth[o] = d;
}

namespace {
// the row-major full frame of a tile-major per-pixel quantity in c->image_f4, on the context's stream: own tiles, or all parts' gathered
// (or in `image`: the variance estimate has staging of its own, image_f4 holds the accumulator image the filter reads beside it)
template <typename T, typename PeerTiles>
int assemble_untiled(hiprz_ctx* c, const T* tiles, PeerTiles peer_tiles_of, T* image = nullptr) {
    const size_t bytes = size_t(c->camera.width) * c->camera.height * sizeof(T);
    if (!image) image = reinterpret_cast<T*>(c->image_f4.ptr);
    // the shards of this context cover the whole frame unless the caller split it further (hiprz_set_shard): only then are there
    // pixels nobody writes, and only then is the image cleared first
    if (c->user_world > 1u) RZ_HIP(c, hipMemsetAsync(image, 0, bytes, c->stream));
    if (c->peers.empty() || c->shard_mode == HIPRZ_SHARD_SAMPLES) {  // (sample mode: `tiles` is the head's own / the summed buffer of the whole share)
        if (c->n_local_tiles)
            RZ_LAUNCH((rz_untile_kernel<T>), dim3(c->n_local_tiles), dim3(256), 0, c->stream, tiles, image,
                               c->camera.width, c->camera.height, c->tiles_x, c->rank, c->world);
    } else {
        // multi-device head: every part's tiles land in a slice of their own of `gather` — the copies of different peers cross their xGMI
        // links side by side — and one launch on the head's stream untiles every slice (shard rank0 + r of `world` in slice r)
        const auto [n_parts, stride, cap] = part_geometry(c);
        RZ_HIP(c, c->gather.buf.resize(stride * n_parts * sizeof(T)));
        T* parts = reinterpret_cast<T*>(c->gather.buf.ptr);
        if (c->n_local_tiles) RZ_HIP(c, hipMemcpyAsync(parts, tiles, stride * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
        // (the previous assembly may only be enqueued — hiprz_denoise, hiprz_present with hiprz_set_denoise: the push waits for its untile kernel)
        for (uint32_t r = 1; r < n_parts; ++r) {
            hiprz_ctx* p = c->peers[r - 1u];
            if (const int rc = push_part(c, p, &c->gather, {{parts + stride * r, peer_tiles_of(p), size_t(p->n_local_tiles) * 256u * sizeof(T)}}); rc != HIPRZ_OK) return rc;
        }
        if (c->n_local_tiles)
            RZ_LAUNCH((rz_untile_gathered_kernel<T>), dim3(c->n_local_tiles, n_parts), dim3(256), 0, c->stream, parts, stride, image, c->camera.width,
                               c->camera.height, c->tiles_x, c->tiles_x * c->tiles_y, c->world, c->rank);
        return mark_consumed(c, c->gather);
    }
    return HIPRZ_OK;
}
// a synchronous read of the image `assemble` leaves in c->image_f4
template <typename T, typename Assemble>
int read_image(hiprz_ctx* c, T* dst, size_t bytes, const char* what, Assemble assemble) {
    (void)hipSetDevice(c->device);
    if (!c->have_camera) return fail(c, HIPRZ_ERR_STATE, "readback before camera upload");
    const size_t n = size_t(c->camera.width) * c->camera.height;
    if (!dst || bytes != n * sizeof(T)) return fail(c, HIPRZ_ERR_INVALID, std::string(what) + ": destination size mismatch");
    StageTimer timer;
    if (const int rc = assemble(); rc != HIPRZ_OK) return rc;
    RZ_HIP(c, hipMemcpyAsync(dst, c->image_f4.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    c->timings.set(what, timer.ms());
    return HIPRZ_OK;
}

bool samples_head(const hiprz_ctx* c) { return c->shard_mode == HIPRZ_SHARD_SAMPLES && !c->peers.empty(); }
// HIPRZ_SHARD_SAMPLES head: out = the sum of the parts' accumulators over the context's share (tile-major, n_local_tiles * 256 pixels).
// Every peer pushes its accumulators into its slice of `gather` (push_part) and one launch adds them up in part order.
template <typename Buffer>
int sum_parts_of(hiprz_ctx* c, float4* out, Buffer buffer_of) {
    const size_t n = part_geometry(c).stride;
    if (!n) return HIPRZ_OK;
    (void)hipSetDevice(c->device);
    const uint32_t n_staged = uint32_t(c->peers.size());
    RZ_HIP(c, c->gather.buf.resize(n * n_staged * sizeof(float4)));
    float4* staged = reinterpret_cast<float4*>(c->gather.buf.ptr);
    for (uint32_t r = 0; r < n_staged; ++r) {
        hiprz_ctx* p = c->peers[r];
        if (p->n_local_tiles != c->n_local_tiles || !buffer_of(p)) return fail(c, HIPRZ_ERR_STATE, "sample sharding: a part's share differs from the head's");
        if (const int rc = push_part(c, p, &c->gather, {{staged + n * r, buffer_of(p), n * sizeof(float4)}}); rc != HIPRZ_OK) return rc;
    }
    RZ_LAUNCH(rz_sum_parts_kernel, dim3(c->n_local_tiles), dim3(256), 0, c->stream, buffer_of(c), staged, n, n_staged, out, uint32_t(n));
    RZ_HIP(c, hipGetLastError());
    return mark_consumed(c, c->gather);
}
int sum_parts(hiprz_ctx* c, float4* out) {
    return sum_parts_of(c, out, [](hiprz_ctx* p) { return (const float4*)p->accum.ptr; });
}
int sum_accum(hiprz_ctx* c) {  // ... into c->sum_accum
    RZ_HIP(c, c->sum_accum.resize(part_geometry(c).stride));
    return sum_parts(c, c->sum_accum.ptr);
}
// Tile-major hand-off of a context's share.  One device / one stream: the owned tiles of shard (rank, world), in order.  A context over
// several devices or streams (n parts) hands out n slices of equal capacity — slice r holds sub-shard rank * n + r of world * n, what
// that device rendered — so the slices of all the ranks of a job, laid end to end, are the sub-shards 0 .. world * n - 1 in order:
// hiprz_untile_gathered with world * n parts of that capacity assembles the frame.
template <typename T, typename Tiles>
int export_tiles(hiprz_ctx* c, void* dst_device, size_t bytes, const char* what, Tiles tiles_of) {
    const bool one_slice = c->shard_mode == HIPRZ_SHARD_SAMPLES;  // the head's buffer of the whole share (the caller summed / tone-mapped the parts into it)
    const auto [n_parts, own, cap] = part_geometry(c);
    if (!dst_device || bytes < (one_slice ? own : cap * n_parts) * sizeof(T)) return fail(c, HIPRZ_ERR_INVALID, std::string(what) + ": destination too small");
    (void)hipSetDevice(c->device);
    T* dst = static_cast<T*>(dst_device);
    if (own) RZ_HIP(c, hipMemcpyAsync(dst, tiles_of(c), own * sizeof(T), hipMemcpyDeviceToDevice, c->stream));
    for (uint32_t r = 1; !one_slice && r < n_parts; ++r) {  // every peer pushes its slice on its own stream; the head's stream waits for all of them
        hiprz_ctx* p = c->peers[r - 1u];
        if (const int rc = push_part(c, p, nullptr, {{dst + cap * r, tiles_of(p), size_t(p->n_local_tiles) * 256u * sizeof(T)}}); rc != HIPRZ_OK) return rc;
    }
    return HIPRZ_OK;
}
// hiprz_untile_rgba8 / hiprz_untile_accum: the tiles of one shard into the frame
template <typename T>
int untile_shard(hiprz_ctx* c, const void* src_tiles, uint32_t rank, uint32_t world, void* dst_image, const char* what) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!c->have_camera) return fail(c, HIPRZ_ERR_STATE, "untile before camera upload");
    if (!src_tiles || !dst_image || world == 0 || rank >= world) return fail(c, HIPRZ_ERR_INVALID, std::string(what) + ": bad arguments");
    (void)hipSetDevice(c->device);
    const uint32_t n_local = shard_local_tiles(c->tiles_x, c->tiles_y, rank, world);
    if (n_local)
        RZ_LAUNCH((rz_untile_kernel<T>), dim3(n_local), dim3(256), 0, c->stream, static_cast<const T*>(src_tiles), static_cast<T*>(dst_image), c->camera.width,
                  c->camera.height, c->tiles_x, rank, world);
    RZ_HIP(c, hipGetLastError());
    return HIPRZ_OK;
}
int check_variance(hiprz_ctx* c, const char* what) {
    if (c->is_peer) return fail(c, HIPRZ_ERR_STATE, std::string(what) + " on a part of a multi-device context");
    if (!c->variance_on) return fail(c, HIPRZ_ERR_STATE, std::string(what) + ": hiprz_set_variance is off");
    if (!c->have_scene || !c->have_camera) return fail(c, HIPRZ_ERR_STATE, std::string(what) + " before scene and camera upload");
    return HIPRZ_OK;
}
}  // namespace

namespace hiprz {

// Called where a first pass is about to run.  Returns whether the finished first pass is to be followed by reproject_after_first_pass.
// The frame a restart replaces is kept as row-major images of the whole frame (accumulator, first-hit depth).  A multi-device head has
// assembled them from all its devices before the call fanned out (assemble_history, history_ready); a single context untiles its own
// shard — pixels of shards rendered elsewhere (hiprz_set_shard by the caller: another process) stay zero and carry no history.
bool keep_history(hiprz_ctx* c) {
    const bool reproject = (c->mode_flags & HIPRZ_COMPAT_REPROJECTION) && c->frame_started && c->n_local_tiles != 0u;
    if (reproject && !c->history_ready) {
        const size_t n = size_t(c->camera.width) * c->camera.height;
        if (c->prev_accum.resize(n) != hipSuccess || c->prev_depth.resize(n) != hipSuccess) return false;
        if (c->world > 1u) {
            (void)hipMemsetAsync(c->prev_accum.ptr, 0, n * sizeof(float4), c->stream);
            (void)hipMemsetAsync(c->prev_depth.ptr, 0, n * sizeof(float), c->stream);
        }
        RZ_LAUNCH((rz_untile_kernel<float4>), dim3(c->n_local_tiles), dim3(256), 0, c->stream, c->accum.ptr, c->prev_accum.ptr, c->camera.width,
                           c->camera.height, c->tiles_x, c->rank, c->world);
        RZ_LAUNCH((rz_untile_kernel<float>), dim3(c->n_local_tiles), dim3(256), 0, c->stream, c->depth.ptr, c->prev_depth.ptr, c->camera.width,
                           c->camera.height, c->tiles_x, c->rank, c->world);
    }
    c->history_ready = false;
    return reproject;
}
// Multi-device head, before a render call fans out to devices that are about to restart their frames: the whole previous frame —
// every device's tiles over the peer-to-peer path of the readbacks — as row-major images on the head, then a copy to every peer.
int assemble_history(hiprz_ctx* c) {
    if (c->peers.empty() || !(c->mode_flags & HIPRZ_COMPAT_REPROJECTION) || !c->reset_pending || !c->frame_started || !c->have_camera) return HIPRZ_OK;
    if (c->shard_mode == HIPRZ_SHARD_SAMPLES) return HIPRZ_OK;  // every part holds the context's whole share: each keeps its own history (keep_history)
    (void)hipSetDevice(c->device);
    const size_t n = size_t(c->camera.width) * c->camera.height;
    RZ_HIP(c, c->prev_accum.resize(n));
    RZ_HIP(c, c->prev_depth.resize(n));
    if (c->user_world > 1u) {
        RZ_HIP(c, hipMemsetAsync(c->prev_accum.ptr, 0, n * sizeof(float4), c->stream));
        RZ_HIP(c, hipMemsetAsync(c->prev_depth.ptr, 0, n * sizeof(float), c->stream));
    }
    const auto [n_parts, stride, cap] = part_geometry(c);
    RZ_HIP(c, c->gather.buf.resize(stride * n_parts * (sizeof(float4) + sizeof(float))));
    float4* parts_a = reinterpret_cast<float4*>(c->gather.buf.ptr);
    float* parts_d = reinterpret_cast<float*>(parts_a + stride * n_parts);
    if (c->n_local_tiles) {
        RZ_HIP(c, hipMemcpyAsync(parts_a, c->accum.ptr, stride * sizeof(float4), hipMemcpyDeviceToDevice, c->stream));
        RZ_HIP(c, hipMemcpyAsync(parts_d, c->depth.ptr, stride * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    }
    for (uint32_t r = 1; r < n_parts; ++r) {
        hiprz_ctx* p = c->peers[r - 1u];
        const size_t local = size_t(p->n_local_tiles) * 256u;
        const int rc = push_part(c, p, &c->gather, {{parts_a + stride * r, p->accum.ptr, local * sizeof(float4)}, {parts_d + stride * r, p->depth.ptr, local * sizeof(float)}});
        if (rc != HIPRZ_OK) return rc;
    }
    if (c->n_local_tiles) {
        RZ_LAUNCH((rz_untile_gathered_kernel<float4>), dim3(c->n_local_tiles, n_parts), dim3(256), 0, c->stream, parts_a, stride, c->prev_accum.ptr,
                           c->camera.width, c->camera.height, c->tiles_x, c->tiles_x * c->tiles_y, c->world, c->rank);
        RZ_LAUNCH((rz_untile_gathered_kernel<float>), dim3(c->n_local_tiles, n_parts), dim3(256), 0, c->stream, parts_d, stride, c->prev_depth.ptr,
                           c->camera.width, c->camera.height, c->tiles_x, c->tiles_x * c->tiles_y, c->world, c->rank);
    }
    if (const int rc = mark_consumed(c, c->gather); rc != HIPRZ_OK) return rc;
    c->history_ready = true;
    // every peer gets the same images; its stream waits for the copy before its first pass runs
    if (!c->history_done) RZ_HIP(c, hipEventCreateWithFlags(&c->history_done, hipEventDisableTiming));
    for (hiprz_ctx* p : c->peers) {
        (void)hipSetDevice(p->device);
        RZ_HIP(c, p->prev_accum.resize(n));
        RZ_HIP(c, p->prev_depth.resize(n));
        (void)hipSetDevice(c->device);
        RZ_HIP(c, hipMemcpyPeerAsync(p->prev_accum.ptr, p->device, c->prev_accum.ptr, c->device, n * sizeof(float4), c->stream));
        RZ_HIP(c, hipMemcpyPeerAsync(p->prev_depth.ptr, p->device, c->prev_depth.ptr, c->device, n * sizeof(float), c->stream));
        p->history_ready = true;
    }
    RZ_HIP(c, hipEventRecord(c->history_done, c->stream));
    for (hiprz_ctx* p : c->peers) {
        (void)hipSetDevice(p->device);
        RZ_HIP(c, hipStreamWaitEvent(p->stream, c->history_done, 0));
    }
    (void)hipSetDevice(c->device);
    return HIPRZ_OK;
}

// hiprz_present's frame slots of one camera: freed only after the copy stream has finished with them
void release_present(hiprz_ctx* c, hiprz_frame_state* f) {
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    for (auto& s : f->frame_slot) {
        s.dev.release();
        if (s.host) (void)hipHostFree(s.host);
        if (s.ready) (void)hipEventDestroy(s.ready);
        if (s.copied) (void)hipEventDestroy(s.copied);
        s = hiprz_frame_state::FrameSlot{};
    }
    f->presented = 0u;
}
// the multi-part head's staging of its peers' tiles for a present: (parts - 1) slices of rgba8 then as many of depth
int size_present_gather(hiprz_ctx* c) {
    if (c->peers.empty() || c->shard_mode == HIPRZ_SHARD_SAMPLES || !c->have_camera) return HIPRZ_OK;
    RZ_HIP(c, c->present_gather.buf.resize(part_geometry(c).stride * c->peers.size() * (sizeof(uint32_t) + sizeof(float))));
    return HIPRZ_OK;
}
// the selected camera's frame slots for its (new) size; the sequence restarts
int allocate_present(hiprz_ctx* c) {
    if (c->is_peer) return HIPRZ_OK;
    release_present(c, c);
    if (!c->copy_stream) RZ_HIP(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    const size_t bytes = size_t(c->camera.width) * c->camera.height * (sizeof(uint32_t) + sizeof(float)) + 4u * sizeof(int32_t);
    for (auto& s : c->frame_slot) {
        RZ_HIP(c, s.dev.resize(bytes));
        RZ_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&s.host), bytes, hipHostMallocDefault));
        RZ_HIP(c, hipEventCreateWithFlags(&s.ready, hipEventDisableTiming));
        RZ_HIP(c, hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
    }
    return size_present_gather(c);
}

int assemble_accum_image(hiprz_ctx* c) {
    (void)hipSetDevice(c->device);
    const float4* tiles = c->accum.ptr;
    if (samples_head(c) && c->n_local_tiles) {
        if (const int rc = sum_accum(c); rc != HIPRZ_OK) return rc;
        tiles = c->sum_accum.ptr;
    }
    return assemble_untiled<float4>(c, tiles, [](hiprz_ctx* p) { return (const float4*)p->accum.ptr; });
}
// Tile mode: every part turns its own pixels' moments into the estimate on its stream and the tiles are assembled as the accumulator's
// are.  Sample mode: the parts' batches are just more batches — accumulator and moments are summed in part order (K included) and the
// formula runs on the sums.  Before the first render call after a restart there is no estimate: zeros.
int assemble_variance_image(hiprz_ctx* c) {
    (void)hipSetDevice(c->device);
    const size_t pixels = size_t(c->camera.width) * c->camera.height, n = size_t(c->n_local_tiles) * 256u;
    RZ_HIP(c, c->var_image.resize(pixels));
    if (c->reset_pending || !c->var_m0.ptr || c->var_m0.count < n || !n) {
        RZ_HIP(c, hipMemsetAsync(c->var_image.ptr, 0, pixels * sizeof(float4), c->stream));
        return HIPRZ_OK;
    }
    const auto var_tiles_of = [](hiprz_ctx* p) { return (const float4*)p->var_tiles.ptr; };
    RZ_HIP(c, c->var_tiles.resize(n));
    if (samples_head(c)) {
        RZ_HIP(c, c->sum_m0.resize(n));
        RZ_HIP(c, c->sum_m1.resize(n));
        if (const int rc = sum_accum(c); rc != HIPRZ_OK) return rc;
        if (const int rc = sum_parts_of(c, c->sum_m0.ptr, [](hiprz_ctx* p) { return (const float4*)p->var_m0.ptr; }); rc != HIPRZ_OK) return rc;
        if (const int rc = sum_parts_of(c, c->sum_m1.ptr, [](hiprz_ctx* p) { return (const float4*)p->var_m1.ptr; }); rc != HIPRZ_OK) return rc;
        RZ_LAUNCH(rz_variance_kernel, dim3(c->n_local_tiles), dim3(256), 0, c->stream, c->sum_accum.ptr, c->sum_m0.ptr, c->sum_m1.ptr, c->var_tiles.ptr, uint32_t(n));
        RZ_HIP(c, hipGetLastError());
        return assemble_untiled<float4>(c, c->var_tiles.ptr, var_tiles_of, c->var_image.ptr);
    }
    RZ_LAUNCH(rz_variance_kernel, dim3(c->n_local_tiles), dim3(256), 0, c->stream, c->accum.ptr, c->var_m0.ptr, c->var_m1.ptr, c->var_tiles.ptr, uint32_t(n));
    for (hiprz_ctx* p : c->peers) {
        const size_t local = size_t(p->n_local_tiles) * 256u;
        if (!local) continue;
        if (!p->var_m0.ptr || p->var_m0.count < local) return fail(c, HIPRZ_ERR_STATE, "variance: a part holds no moments");
        (void)hipSetDevice(p->device);
        RZ_HIP(c, p->var_tiles.resize(local));
        RZ_LAUNCH(rz_variance_kernel, dim3(p->n_local_tiles), dim3(256), 0, p->stream, p->accum.ptr, p->var_m0.ptr, p->var_m1.ptr, p->var_tiles.ptr, uint32_t(local));
    }
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipGetLastError());
    return assemble_untiled<float4>(c, c->var_tiles.ptr, var_tiles_of, c->var_image.ptr);
}
}  // namespace hiprz

extern "C" {

int hiprz_tonemap(hiprz_ctx* c) {
    if (!c) return HIPRZ_ERR_INVALID;
    const bool summed = samples_head(c);  // the tone map of the SUM of the parts' accumulators, into the head's pixels
    if (!summed) RZ_FANOUT(c, hiprz_tonemap(p));
    if (!c->have_camera) return fail(c, HIPRZ_ERR_STATE, "tonemap before camera upload");
    (void)hipSetDevice(c->device);
    if (!summed && c->rgba8_valid && !c->reset_pending) return HIPRZ_OK;  // the resident kernel already wrote this frame's pixels
    const uint32_t n = c->n_local_tiles * 256u;
    if (summed && n)
        if (const int rc = sum_accum(c); rc != HIPRZ_OK) return rc;
    if (n)
        RZ_LAUNCH(rz_tonemap_tiles_kernel, dim3(c->n_local_tiles), dim3(256), 0, c->stream, summed ? c->sum_accum.ptr : c->accum.ptr, c->rgba8.ptr, n,
                  c->camera.aperture, c->camera.exposure_time);
    RZ_HIP(c, hipGetLastError());
    return HIPRZ_OK;
}

int hiprz_read_rgba8(hiprz_ctx* c, uint8_t* dst, size_t bytes) {
    if (!c) return HIPRZ_ERR_INVALID;
    return read_image(c, reinterpret_cast<uint32_t*>(dst), bytes, "read rgba8",
                      [c] { return assemble_untiled<uint32_t>(c, c->rgba8.ptr, [](hiprz_ctx* p) { return (const uint32_t*)p->rgba8.ptr; }); });
}
int hiprz_read_depth(hiprz_ctx* c, float* dst, size_t bytes) {
    if (!c) return HIPRZ_ERR_INVALID;
    return read_image(c, dst, bytes, "read depth", [c] { return assemble_untiled<float>(c, c->depth.ptr, [](hiprz_ctx* p) { return (const float*)p->depth.ptr; }); });
}
int hiprz_read_accum(hiprz_ctx* c, float* dst, size_t bytes) {
    if (!c) return HIPRZ_ERR_INVALID;
    return read_image(c, reinterpret_cast<float4*>(dst), bytes, "read accum", [c] { return assemble_accum_image(c); });
}

int hiprz_accum_device(hiprz_ctx* c, const void** out) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!out) return fail(c, HIPRZ_ERR_INVALID, "accum_device: null output");
    if (c->is_peer) return fail(c, HIPRZ_ERR_STATE, "accum_device on a part of a multi-device context");
    if (!c->have_scene || !c->have_camera) return fail(c, HIPRZ_ERR_STATE, "accum_device before scene and camera upload");
    if (const int rc = assemble_accum_image(c); rc != HIPRZ_OK) return rc;
    *out = c->image_f4.ptr;
    return HIPRZ_OK;
}

int hiprz_read_state(hiprz_ctx* c, float* ray9, uint32_t* md2, size_t n_pixels) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!c->have_camera) return fail(c, HIPRZ_ERR_STATE, "readback before camera upload");
    const size_t n = size_t(c->camera.width) * c->camera.height;
    if (!ray9 || !md2 || n_pixels != n) return fail(c, HIPRZ_ERR_INVALID, "read_state: destination size mismatch");
    (void)hipSetDevice(c->device);
    RZ_HIP(c, c->state_ray.resize(9 * n));
    RZ_HIP(c, c->state_md.resize(2 * n));
    RZ_HIP(c, hipMemsetAsync(c->state_ray.ptr, 0, 9 * n * sizeof(float), c->stream));
    RZ_HIP(c, hipMemsetAsync(c->state_md.ptr, 0, 2 * n * sizeof(uint32_t), c->stream));
    if (c->n_local_tiles)
        RZ_LAUNCH(rz_untile_state_kernel, dim3(c->n_local_tiles), dim3(256), 0, c->stream, c->st0.ptr, c->st1.ptr,
                           c->st2.ptr, c->state_ray.ptr, c->state_md.ptr, c->camera.width, c->camera.height, c->tiles_x, c->rank,
                           c->world);
    // multi-device head: the peers' path state, one peer at a time through `gather`.  The head PULLS here, on its own stream, behind
    // whatever read the staging before; only the peers' later pushes have to be told when the last kernel below is done (mark_consumed)
    for (hiprz_ctx* p : c->peers) {
        const size_t n_local = size_t(p->n_local_tiles) * 256u;
        if (!n_local || c->shard_mode == HIPRZ_SHARD_SAMPLES) continue;  // (sample mode: the parts walk different paths through the same pixels — part 0 answers)
        RZ_HIP(c, c->gather.buf.resize(n_local * 40u));
        float4* g0 = reinterpret_cast<float4*>(c->gather.buf.ptr);
        float4* g1 = g0 + n_local;
        float2* g2 = reinterpret_cast<float2*>(g1 + n_local);
        (void)hipSetDevice(p->device);
        RZ_HIP(c, hipEventRecord(p->peer_done, p->stream));
        (void)hipSetDevice(c->device);
        RZ_HIP(c, hipStreamWaitEvent(c->stream, p->peer_done, 0));
        RZ_HIP(c, hipMemcpyPeerAsync(g0, c->device, p->st0.ptr, p->device, n_local * 16u, c->stream));
        RZ_HIP(c, hipMemcpyPeerAsync(g1, c->device, p->st1.ptr, p->device, n_local * 16u, c->stream));
        RZ_HIP(c, hipMemcpyPeerAsync(g2, c->device, p->st2.ptr, p->device, n_local * 8u, c->stream));
        RZ_LAUNCH(rz_untile_state_kernel, dim3(p->n_local_tiles), dim3(256), 0, c->stream, g0, g1, g2, c->state_ray.ptr, c->state_md.ptr,
                           c->camera.width, c->camera.height, c->tiles_x, p->rank, p->world);
    }
    if (!c->peers.empty())
        if (const int rc = mark_consumed(c, c->gather); rc != HIPRZ_OK) return rc;
    RZ_HIP(c, hipMemcpyAsync(ray9, c->state_ray.ptr, 9 * n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipMemcpyAsync(md2, c->state_md.ptr, 2 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return HIPRZ_OK;
}

int hiprz_read_variance(hiprz_ctx* c, float* dst, size_t bytes) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (const int rc = check_variance(c, "read_variance"); rc != HIPRZ_OK) return rc;
    if (!dst || bytes != size_t(c->camera.width) * c->camera.height * sizeof(float4)) return fail(c, HIPRZ_ERR_INVALID, "read_variance: destination size mismatch");
    if (const int rc = assemble_variance_image(c); rc != HIPRZ_OK) return rc;
    RZ_HIP(c, hipMemcpyAsync(dst, c->var_image.ptr, bytes, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return HIPRZ_OK;
}

int hiprz_variance_device(hiprz_ctx* c, const void** out) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!out) return fail(c, HIPRZ_ERR_INVALID, "variance_device: null output");
    if (const int rc = check_variance(c, "variance_device"); rc != HIPRZ_OK) return rc;
    if (const int rc = assemble_variance_image(c); rc != HIPRZ_OK) return rc;
    *out = c->var_image.ptr;
    return HIPRZ_OK;
}

int hiprz_local_pixel_capacity(hiprz_ctx* c, size_t* out) {
    if (!c || !out) return HIPRZ_ERR_INVALID;
    const PartGeometry g = part_geometry(c);
    *out = c->shard_mode == HIPRZ_SHARD_SAMPLES ? g.stride : g.capacity * g.n_parts;
    return HIPRZ_OK;
}
int hiprz_export_accum_tiles(hiprz_ctx* c, void* dst_device, size_t bytes) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (samples_head(c)) {  // the parts' sum, straight into the caller's buffer
        if (!dst_device || bytes < size_t(c->n_local_tiles) * 256u * sizeof(float4)) return fail(c, HIPRZ_ERR_INVALID, "export_accum_tiles: destination too small");
        return sum_parts(c, static_cast<float4*>(dst_device));
    }
    return export_tiles<float4>(c, dst_device, bytes, "export_accum_tiles", [](hiprz_ctx* x) { return (const float4*)x->accum.ptr; });
}
int hiprz_export_rgba8_tiles(hiprz_ctx* c, void* dst_device, size_t bytes) {
    if (!c) return HIPRZ_ERR_INVALID;
    return export_tiles<uint32_t>(c, dst_device, bytes, "export_rgba8_tiles", [](hiprz_ctx* x) { return (const uint32_t*)x->rgba8.ptr; });
}
int hiprz_untile_rgba8(hiprz_ctx* c, const void* src_tiles, uint32_t rank, uint32_t world, void* dst_image) {
    return untile_shard<uint32_t>(c, src_tiles, rank, world, dst_image, "untile_rgba8");
}
int hiprz_untile_accum(hiprz_ctx* c, const void* src_tiles, uint32_t rank, uint32_t world, void* dst_image) {
    return untile_shard<float4>(c, src_tiles, rank, world, dst_image, "untile_accum");
}
int hiprz_untile_gathered(hiprz_ctx* c, const void* src_parts, uint32_t world, size_t part_stride_bytes, uint32_t element_bytes,
                          void* dst_image, void* stream) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!c->have_camera) return fail(c, HIPRZ_ERR_STATE, "untile before camera upload");
    if (!src_parts || !dst_image || world == 0 || world > 65535u || (element_bytes != 4u && element_bytes != 16u) || part_stride_bytes % element_bytes)
        return fail(c, HIPRZ_ERR_INVALID, "untile_gathered: bad arguments");
    (void)hipSetDevice(c->device);
    const uint32_t n_tiles = c->tiles_x * c->tiles_y;
    const uint32_t per_rank = shard_local_tiles(c->tiles_x, c->tiles_y, 0u, world);
    if (part_stride_bytes < size_t(per_rank) * 256u * element_bytes) return fail(c, HIPRZ_ERR_INVALID, "untile_gathered: part stride smaller than a shard");
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    if (n_tiles) {
        const dim3 grid(per_rank, world);
        if (element_bytes == 4u)
            RZ_LAUNCH((rz_untile_gathered_kernel<uint32_t>), grid, dim3(256), 0, st, reinterpret_cast<const uint32_t*>(src_parts),
                               part_stride_bytes / 4u, reinterpret_cast<uint32_t*>(dst_image), c->camera.width, c->camera.height, c->tiles_x, n_tiles, world, 0u);
        else
            RZ_LAUNCH((rz_untile_gathered_kernel<float4>), grid, dim3(256), 0, st, reinterpret_cast<const float4*>(src_parts),
                               part_stride_bytes / 16u, reinterpret_cast<float4*>(dst_image), c->camera.width, c->camera.height, c->tiles_x, n_tiles, world, 0u);
    }
    RZ_HIP(c, hipGetLastError());
    return HIPRZ_OK;
}
int hiprz_tonemap_image(hiprz_ctx* c, const void* src_image, void* dst_rgba8) { return hiprz_tonemap_image_on(c, src_image, dst_rgba8, nullptr); }
int hiprz_tonemap_image_on(hiprz_ctx* c, const void* src_image, void* dst_rgba8, void* stream) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!c->have_camera) return fail(c, HIPRZ_ERR_STATE, "tonemap before camera upload");
    if (!src_image || !dst_rgba8) return fail(c, HIPRZ_ERR_INVALID, "tonemap_image: null pointer");
    (void)hipSetDevice(c->device);
    const uint32_t n = c->camera.width * c->camera.height;
    RZ_LAUNCH(rz_tonemap_image_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream ? static_cast<hipStream_t>(stream) : c->stream,
                       reinterpret_cast<const float4*>(src_image), reinterpret_cast<uint32_t*>(dst_rgba8), n, c->camera.aperture,
                       c->camera.exposure_time);
    RZ_HIP(c, hipGetLastError());
    return HIPRZ_OK;
}

int hiprz_ray_cast(hiprz_ctx* c, uint32_t x, uint32_t y, hiprz_raycast* out) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!c->have_scene || !c->have_camera) return fail(c, HIPRZ_ERR_STATE, "ray cast before scene and camera upload");
    if (!out) return fail(c, HIPRZ_ERR_INVALID, "ray cast: null output");
    // Camera::rayCastPixel clamps (camera.cpp:159-165)
    if (x >= c->camera.width) x = c->camera.width - 1;
    if (y >= c->camera.height) y = c->camera.height - 1;
    (void)hipSetDevice(c->device);
    // depth of the pixel: only the shard that owns it can answer
    uint32_t owner, lt;
    shard_of_tile(x / 32u, y / 8u, c->tiles_x, c->world, owner, lt);
    *out = hiprz_raycast{-1, -1, -1, 0u};
    if (owner != c->rank) {
        for (hiprz_ctx* p : c->peers)
            if (p->world == c->world && owner == p->rank) {
                const int rc = hiprz_ray_cast(p, x, y, out);
                return rc == HIPRZ_OK ? rc : fail(c, rc, "device " + std::to_string(p->device) + ": " + p->error);
            }
        return HIPRZ_OK;
    }
    const uint32_t in_tile = ((x % 32u) / 8u) * 64u + (y % 8u) * 8u + (x % 8u);
    float depth = 0.0f;
    RZ_HIP(c, hipMemcpyAsync(&depth, c->depth.ptr + size_t(lt) * 256u + in_tile, sizeof(float), hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    RZ_LAUNCH(rz_pick_kernel, dim3(1), dim3(1), 0, c->stream, c->dscene, c->dcamera, x, y, depth, c->pick_dev.ptr);
    int32_t out4[4] = {-1, -1, -1, 0};
    RZ_HIP(c, hipMemcpyAsync(out4, c->pick_dev.ptr, sizeof out4, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    out->instance = out4[0], out->material_slot = out4[1], out->material = out4[2], out->triangle = uint32_t(out4[3]);
    return HIPRZ_OK;
}

int hiprz_pick(hiprz_ctx* c, uint32_t x, uint32_t y, int32_t* instance_out, int32_t* material_out) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!instance_out || !material_out) return fail(c, HIPRZ_ERR_INVALID, "pick: null output");
    hiprz_raycast r;
    const int rc = hiprz_ray_cast(c, x, y, &r);
    *instance_out = rc == HIPRZ_OK ? r.instance : -1, *material_out = rc == HIPRZ_OK ? r.material : -1;
    return rc;
}

// Render stream: tone map, (peers' pushes,) present kernel + pick into the slot, `ready`.  Copy stream: waits for `ready`, one copy of the
// slot to its pinned twin, `copied`.  The render stream waits for a slot's previous `copied` before it writes that slot again.
int hiprz_present(hiprz_ctx* c, uint32_t x, uint32_t y) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (c->is_peer) return fail(c, HIPRZ_ERR_STATE, "present on a part of a multi-device context");
    if (!c->have_scene || !c->have_camera) return fail(c, HIPRZ_ERR_STATE, "present before scene and camera upload");
    if (!c->frame_slot[0].host || !c->copy_stream) return fail(c, HIPRZ_ERR_STATE, "present: the camera has no frame slots");
    if (c->denoise_on && c->user_world > 1u)  // refused before anything is enqueued: the slots and the sequence stay as they are
        return fail(c, HIPRZ_ERR_STATE, "present: hiprz_set_denoise is set, but this context renders shard " + std::to_string(c->user_rank) + " of " +
                                            std::to_string(c->user_world) + " and does not hold the frame (clear it, or gather and hiprz_denoise_image)");
    if (c->denoise_on && (c->denoise_params.flags & HIPRZ_DENOISE_VARIANCE) && !c->variance_on)  // likewise
        return fail(c, HIPRZ_ERR_STATE, "present: hiprz_set_denoise asks for HIPRZ_DENOISE_VARIANCE, but hiprz_set_variance is off");
    (void)hipSetDevice(c->device);
    for (const auto& s : c->frame_slot)  // a copy of an earlier present that failed on the device
        if (s.copy_enqueued) {
            const hipError_t e = hipEventQuery(s.copied);
            if (e != hipSuccess && e != hipErrorNotReady) return fail(c, HIPRZ_ERR_DEVICE, std::string("present: frame copy: ") + hipGetErrorString(e));
        }
    if (const int rc = hiprz_tonemap(c); rc != HIPRZ_OK) return rc;
    (void)hipSetDevice(c->device);
    const uint32_t sequence = c->presented + 1u;
    hiprz_frame_state::FrameSlot& slot = c->frame_slot[(sequence - 1u) & 1u];
    if (slot.copy_enqueued) RZ_HIP(c, hipStreamWaitEvent(c->stream, slot.copied, 0));
    const uint32_t W = c->camera.width, H = c->camera.height;
    const size_t n = size_t(W) * H;
    uint32_t* rgba8 = reinterpret_cast<uint32_t*>(slot.dev.ptr);
    float* depth = reinterpret_cast<float*>(rgba8 + n);
    int32_t* record = reinterpret_cast<int32_t*>(depth + n);
    // pixels of shards rendered elsewhere (hiprz_set_shard by the caller) stay zero, as in hiprz_read_*
    if (c->user_world > 1u) RZ_HIP(c, hipMemsetAsync(slot.dev.ptr, 0, n * (sizeof(uint32_t) + sizeof(float)), c->stream));
    const uint32_t n_tiles = c->tiles_x * c->tiles_y;
    if (c->peers.empty() || c->shard_mode == HIPRZ_SHARD_SAMPLES) {  // (sample mode: the head's summed tone map and its depth)
        if (c->n_local_tiles)
            RZ_LAUNCH((rz_present_kernel<false>), dim3(c->n_local_tiles), dim3(256), 0, c->stream, c->rgba8.ptr, c->depth.ptr, nullptr, nullptr,
                      size_t(0), rgba8, depth, W, H, c->tiles_x, n_tiles, c->world, c->rank);
    } else {
        // every peer pushes its tiles into its slices of present_gather, behind its own tone map and the previous present kernel
        const auto [n_parts, stride, cap] = part_geometry(c);
        if (c->present_gather.buf.count < stride * (n_parts - 1u) * (sizeof(uint32_t) + sizeof(float)))
            return fail(c, HIPRZ_ERR_STATE, "present: the staging of the parts' tiles is not sized for this shard");
        uint32_t* parts_rgba8 = reinterpret_cast<uint32_t*>(c->present_gather.buf.ptr);
        float* parts_depth = reinterpret_cast<float*>(parts_rgba8 + stride * (n_parts - 1u));
        for (uint32_t r = 1; r < n_parts; ++r) {
            hiprz_ctx* p = c->peers[r - 1u];
            const size_t local = size_t(p->n_local_tiles) * 256u, at = stride * (r - 1u);
            const int rc = push_part(c, p, &c->present_gather, {{parts_rgba8 + at, p->rgba8.ptr, local * sizeof(uint32_t)}, {parts_depth + at, p->depth.ptr, local * sizeof(float)}});
            if (rc != HIPRZ_OK) return rc;
        }
        if (c->n_local_tiles)
            RZ_LAUNCH((rz_present_kernel<true>), dim3(c->n_local_tiles, n_parts), dim3(256), 0, c->stream, c->rgba8.ptr, c->depth.ptr, parts_rgba8,
                      parts_depth, stride, rgba8, depth, W, H, c->tiles_x, n_tiles, c->world, c->rank);
        if (const int rc = mark_consumed(c, c->present_gather); rc != HIPRZ_OK) return rc;
    }
    if (c->denoise_on) {  // hiprz_set_denoise: the filter's tone map replaces the slot's image (the depth stays the first-hit depth)
        if (const int rc = denoise_frame(c, &c->denoise_params, rgba8); rc != HIPRZ_OK) return rc;
        (void)hipSetDevice(c->device);
    }
    // the ray cast of hiprz_ray_cast: clamped pixel (camera.cpp:159-165), answered where some part of this context rendered it
    if (x >= W) x = W - 1u;
    if (y >= H) y = H - 1u;
    uint32_t owner, lt;
    shard_of_tile(x / 32u, y / 8u, c->tiles_x, c->world, owner, lt);
    bool owned = owner == c->rank;
    for (hiprz_ctx* p : c->peers) owned = owned || (p->world == c->world && owner == p->rank);
    RZ_LAUNCH(rz_pick_slot_kernel, dim3(1), dim3(1), 0, c->stream, c->dscene, c->dcamera, x, y, uint32_t(owned), depth, record);
    RZ_HIP(c, hipGetLastError());
    RZ_HIP(c, hipEventRecord(slot.ready, c->stream));
    RZ_HIP(c, hipStreamWaitEvent(c->copy_stream, slot.ready, 0));
    RZ_HIP(c, hipMemcpyAsync(slot.host, slot.dev.ptr, n * (sizeof(uint32_t) + sizeof(float)) + 4u * sizeof(int32_t), hipMemcpyDeviceToHost, c->copy_stream));
    RZ_HIP(c, hipEventRecord(slot.copied, c->copy_stream));
    slot.copy_enqueued = true;
    slot.sequence = sequence, slot.passes = c->passes;
    slot.ray_count = total_ray_count(c);
    c->presented = sequence;
    return HIPRZ_OK;
}

int hiprz_read_frame(hiprz_ctx* c, uint32_t sequence, hiprz_frame* out) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!out) return fail(c, HIPRZ_ERR_INVALID, "read_frame: null output");
    if (c->presented == 0u) return fail(c, HIPRZ_ERR_STATE, "read_frame: nothing presented on this camera since it was sized");
    if (sequence == 0u) sequence = c->presented;
    if (sequence > c->presented || sequence + 1u < c->presented)
        return fail(c, HIPRZ_ERR_STATE, "read_frame: sequence " + std::to_string(sequence) + " is not one of the newest two (" +
                                            std::to_string(c->presented) + ")");
    const hiprz_frame_state::FrameSlot& slot = c->frame_slot[(sequence - 1u) & 1u];
    if (slot.sequence != sequence || !slot.copy_enqueued) return fail(c, HIPRZ_ERR_STATE, "read_frame: sequence not presented");
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipEventSynchronize(slot.copied));
    const size_t n = size_t(c->camera.width) * c->camera.height;
    const int32_t* record = reinterpret_cast<const int32_t*>(slot.host + n * (sizeof(uint32_t) + sizeof(float)));
    out->rgba8 = slot.host;
    out->depth = reinterpret_cast<const float*>(slot.host + n * sizeof(uint32_t));
    out->width = c->camera.width, out->height = c->camera.height;
    out->passes = slot.passes, out->sequence = slot.sequence, out->ray_count = slot.ray_count;
    out->hit = hiprz_raycast{record[0], record[1], record[2], uint32_t(record[3])};
    return HIPRZ_OK;
}

}  // extern "C"
