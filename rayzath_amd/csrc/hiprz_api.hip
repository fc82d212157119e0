// hiprz_api.hip — the device half of the C-ABI declared in include/hiprz.h: context life cycle, settings, render calls.
//
// Replaces, for the HIPGPU backend, what the reference's CUDA backend does in cuda_engine_core.cu (host<->device
// mirroring), cuda_engine_renderer.cu (launch sequence) and cuda_postprocess_kernel.cu (pass update).
// The pass kernels live in hiprz_kernels.hpp and are instantiated by hiprz_launch_*.hip; scene mirroring lives in hiprz_scene.hip (and,
// where it needs no device, hiprz_scene_host.cpp); what turns the parts' tiles into frames (tone map, assembly, reads, export, present)
// lives in hiprz_readback.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hiprz.h"
#include "hiprz_ctx.hpp"
#include "hiprz_device.hpp"

using namespace hiprz;

// =======================================================================================
// Small kernels: pass index, batch moments, self-test
// =======================================================================================

// resident kernels, heaviest first: sort keys from the units' measured costs (falling cost = rising key)
__global__ void __launch_bounds__(256) rz_order_keys_kernel(const uint32_t* cost, uint32_t* keys, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) keys[i] = 0x00FFFFFFu - (cost[i] < 0x00FFFFFFu ? cost[i] : 0x00FFFFFFu);
}

// passUpdate / segmentUpdate (cuda_postprocess_kernel.cu:95-104, cuda_render_kernel.cu:122-129):
// the pass index lives on the device so a captured graph replays without new arguments.
__global__ void rz_pass_update_kernel(uint32_t* pass) { *pass += 1u; }
__global__ void rz_pass_reset_kernel(uint32_t* pass) { *pass = 0u; }
__global__ void rz_pass_add_kernel(uint32_t* pass, uint32_t n) { *pass += n; }

// hiprz_set_variance (include/hiprz.h "VARIANCE"): one thread per local pixel behind the passes of a render call.  The call's batch closes
// for a pixel when at least one path finished in it since the pixel's last closed batch (the accumulator gains radiance in every segment,
// alpha only when a path ends: a batch without a finished path is a fragment of a sample and merges into the next one).  snap_only: the
// call restarted the frame from reprojected history, which is no sample.
__global__ void __launch_bounds__(256) rz_moments_kernel(const float4* accum, float4* snap, float4* m0, float4* m1, uint32_t n, uint32_t snap_only) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const float4 a = accum[i];
    if (snap_only) {
        snap[i] = a;
        return;
    }
    const float4 s = snap[i];
    const float dr = a.x - s.x, dg = a.y - s.y, db = a.z - s.z, dw = a.w - s.w;
    if (!(dw >= 1.0f)) return;
    float4 u = m0[i], v = m1[i];
    u.x = u.x + dr * dr, u.y = u.y + dg * dg, u.z = u.z + db * db, u.w = u.w + dw * dw;
    v.x = v.x + dr * dw, v.y = v.y + dg * dw, v.z = v.z + db * dw, v.w = v.w + 1.0f;
    m0[i] = u, m1[i] = v, snap[i] = a;
}

// Device self-test: div_shared() must equal the correctly rounded `/` bit for bit over its
// whole stated operand range.  out[0] = mismatches, out[1] = cases tested, out[2] = box tests the filter left undecided,
// out[3] = lobe cases in which roughness 2^-100 does not return the mirror's (+0, 1).
__global__ void __launch_bounds__(256) rz_selftest_div_kernel(uint32_t n_per_thread, uint32_t seed, unsigned long long* out) {
    uint32_t h = mix32(seed ^ (blockIdx.x * 256u + threadIdx.x) * 0x9E3779B9u);
    uint32_t bad = 0, tested = 0, undecided = 0, tiny_differs = 0;
    // a byte over 255 (hiprz_u8_div.hpp, RZ_U8_SHORT_DIV): the two-fma form against the division, bit for bit, for every byte — thread
    // t of each block takes byte t; called directly, whichever way the switch stands
    if (__float_as_uint(u8_over_255_short(float(threadIdx.x))) != __float_as_uint(float(threadIdx.x) / 255.0f)) bad += 1;
    for (uint32_t i = 0; i < n_per_thread; ++i) {
        h = mix32(h + i);
        // d: random sign/mantissa, exponent in [-40, 2); n: zero or exponent in [-84, 41)
        const uint32_t de = 127u - 40u + (h >> 8) % 42u;
        const float d = __uint_as_float((h & 0x80000000u) | (de << 23) | (mix32(h) & 0x7FFFFFu));
        const uint32_t g = mix32(h ^ 0xA5A5A5A5u);
        const uint32_t ne = 127u - 84u + (g >> 8) % 125u;
        float n = __uint_as_float((g & 0x80000000u) | (ne << 23) | (mix32(g) & 0x7FFFFFu));
        if ((g & 0xFFu) == 0u) n = 0.0f;
        const float y = refined_rcp(d);
        const float n2 = n == 0.0f ? 0.0f : __uint_as_float(__float_as_uint(n) ^ (mix32(g + 7u) & 0x007FFFFFu));  // second numerator, same exponent
        const f2 fast = div_shared2(f2{n, n2}, d, y);
        const float exact = n / d, exact2 = n2 / d;
        tested += 2;
        if (__float_as_uint(fast.x) != __float_as_uint(exact) && !(fast.x == 0.0f && exact == 0.0f)) bad += 1;
        if (__float_as_uint(fast.y) != __float_as_uint(exact2) && !(fast.y == 0.0f && exact2 == 0.0f)) bad += 1;
        if (__float_as_uint(div_shared(n, d, y)) != __float_as_uint(fast.x)) bad += 1;
        // sincosf must return what sinf and cosf return: the samplers' angles are in [0, 2*pi], test a wider range
        const float angle = __uint_as_float((g & 0x80000000u) | ((118u + (h >> 11) % 16u) << 23) | (mix32(h + 3u) & 0x7FFFFFu));
        float sn, cs;
        sincosf(angle, &sn, &cs);
        if (__float_as_uint(sn) != __float_as_uint(sinf(angle)) || __float_as_uint(cs) != __float_as_uint(cosf(angle))) bad += 1;
        // the glossy lobe of a mirror (RZ_MIRROR_LOBE_CONST, sample_direction): the general sequence — spelled here, so that it runs
        // whichever way the switch stands — must return (sin, cos) = (+0, 1) at roughness +0 and -0 for every draw u2 in [0, 1); every
        // sixteenth case takes an end of the range: 0, 2^-24, 1 - 2^-24.  Reports into `bad` only.  `tiny_differs` counts the cases in
        // which roughness 2^-100 — a value that takes the general path under either setting — does not return the same bits:
        // tests/test_mirror_lobe_gpu.py renders its twin worlds with it.
        {
            float u2 = float(mix32(h + 0x10BEu) >> 8) * (1.0f / 16777216.0f);
            if ((i & 15u) == 15u) {
                const uint32_t edge = (i >> 4) % 3u;
                u2 = edge == 0u ? 0.0f : edge == 1u ? 1.0f / 16777216.0f : 1.0f - 1.0f / 16777216.0f;
            }
            auto lobe = [&](float roughness, float& s_xy, float& c_z) {
                const float theta = RZ_ACOSF(1.0f - 2.0f * ((1.0f - RZ_POWF(u2 + 1.0e-5f, roughness)) * 0.5f));
                RZ_SINCOSF(theta, s_xy, c_z);
            };
            // the roughness comes out of a register the compiler cannot fold: +0 or -0 by a bit of the hash, the other sign second
            const float zero = __uint_as_float(h & 0x80000000u), other = __uint_as_float(~h & 0x80000000u);
            float s0, c0, s1, c1, st, ct;
            lobe(zero, s0, c0), lobe(other, s1, c1), lobe(__uint_as_float((127u - 100u) << 23), st, ct);
            if (__float_as_uint(s0) != 0x00000000u || __float_as_uint(c0) != 0x3F800000u) bad += 1;
            if (__float_as_uint(s1) != 0x00000000u || __float_as_uint(c1) != 0x3F800000u) bad += 1;
            if (__float_as_uint(st) != 0x00000000u || __float_as_uint(ct) != 0x3F800000u) tiny_differs += 1;
        }
        // the filtered box test (box_filter): whenever it claims to know, the exact test must agree.  A ray from a random point towards a
        // random direction against a random box around the origin region — every second case with a face of the box exactly ON the ray's
        // range end or through the ray's origin plane, where comparisons are decided by a rounding
        {
            auto unit = [&](uint32_t k) { return float(mix32(h + 0x9E37u * k) >> 8) * (1.0f / 16777216.0f); };
            WalkRay r;
            r.o = V3(unit(1) * 8.0f - 4.0f, unit(2) * 8.0f - 4.0f, unit(3) * 8.0f - 4.0f);
            v3 dir = V3(unit(4) * 2.0f - 1.0f, unit(5) * 2.0f - 1.0f, unit(6) * 2.0f - 1.0f);
            if ((h & 7u) == 0u) dir.x *= 1.0e-6f;  // nearly parallel to two faces
            dir = normalized(dir);
            r.d = dir, r.near_ = 0.0f, r.far_ = (h & 1u) ? unit(7) * 6.0f : RZ_FLT_MAX;
            prepare<true>(r, true);
            const float cx = unit(8) * 6.0f - 3.0f, cy = unit(9) * 6.0f - 3.0f, cz = unit(10) * 6.0f - 3.0f;
            float hx = unit(11) * 2.0f, hy = unit(12) * 2.0f, hz = unit(13) * 2.0f;
            if ((h & 48u) == 0u) hz = 0.0f;  // a flat box (an axis-aligned wall)
            float4 b0 = make_float4(cx - hx, cx + hx, cy - hy, cy + hy), b1 = make_float4(cz - hz, cz + hz, 0.0f, 0.0f);
            if (h & 2u) {  // put the far end of the range exactly where the ray crosses the box's lower x face (when it points that way)
                const float t = (b0.x - r.o.x) / r.d.x;
                if (t > 0.0f && t < 1.0e6f) r.far_ = t;
            }
            if (r.fast) {
                bool missed, hit;
                box_filter(b0, b1, r, missed, hit);
                const bool exact = box_hit_unpacked<false>(b0, b1, r);
                tested += 1;
                if ((hit && !exact) || (missed && exact) || (hit && missed)) bad += 1;
                if (!hit && !missed) undecided += 1;
            }
            // (The comparison below runs on every case and reports into `bad`; `tested` stays the count of quotients and filtered box
            // tests, which tests/test_parity_gpu.py bounds from both sides.)
            // the one-leaf walk's triangle loop: two triangles in one iteration (tri_pair_step: tri_hit2 + pair_pick) against the
            // one-by-one loop (tri_hit, the far end moving between the two) — far end, winner, b1, b2 and the facing bit.  Random pairs
            // in front of the ray, and by the bits of `kind`: the same triangle twice (equal distances: the first wins), a ray almost in
            // the triangle's plane (|det| < 1e-7: the nudge), an origin in the plane (t = 0), and a near or far end that IS a hit's t.
            {
                const uint32_t kind = (h >> 4) & 7u;
                float4 ta[3], tb[3];
                auto corner = [&](uint32_t k, float depth) { return V3(unit(k) * 6.0f - 3.0f, unit(k + 1u) * 6.0f - 3.0f, depth); };
                auto make = [&](float4 (&rec)[3], uint32_t k, float depth) {
                    const v3 p1 = corner(k, depth + unit(k + 6u)), p2 = corner(k + 2u, depth + unit(k + 7u)), p3 = corner(k + 4u, depth + unit(k + 8u));
                    const v3 e1 = p2 - p1, e2 = p3 - p1;
                    rec[0] = make_float4(p1.x, p1.y, p1.z, 0.0f), rec[1] = make_float4(e1.x, e1.y, e1.z, 0.0f), rec[2] = make_float4(e2.x, e2.y, e2.z, 0.0f);
                };
                make(ta, 20u, 2.0f), make(tb, 30u, (h & 0x100u) ? 2.0f : 3.0f);
                if (kind == 1u) tb[0] = ta[0], tb[1] = ta[1], tb[2] = ta[2];
                WalkRay q;
                q.o = V3(unit(40) * 2.0f - 1.0f, unit(41) * 2.0f - 1.0f, -1.0f);
                const v3 aim = V3(unit(42) * 4.0f - 2.0f, unit(43) * 4.0f - 2.0f, 2.5f);
                q.d = normalized(aim - q.o), q.near_ = 0.0f, q.far_ = (h & 0x200u) ? RZ_FLT_MAX : 8.0f;
                if (kind == 2u) {  // almost in a's plane: along edge1, tilted towards the normal by up to 2e-8
                    const v3 e1 = xyz(ta[1]), nrm = cross(xyz(ta[1]), xyz(ta[2]));
                    q.d = normalized(normalized(e1) + normalized(nrm) * ((unit(44) - 0.5f) * 4.0e-8f));
                }
                if (kind == 3u) q.o = xyz(ta[0]) + xyz(ta[1]) * (unit(45) * 0.5f) + xyz(ta[2]) * (unit(46) * 0.5f);  // in a's plane
                q.fast = false, q.y = V3(0.0f, 0.0f, 0.0f);
                if (kind >= 4u) {  // a range end on a hit's distance: a's (4, 5) or b's (6, 7), near (even) or far (odd)
                    const bool of_a = kind < 6u;
                    WalkRay probe = q;
                    probe.far_ = RZ_FLT_MAX;
                    float t = 0.0f, u, v, det;
                    if (tri_hit(xyz(of_a ? ta[0] : tb[0]), xyz(of_a ? ta[1] : tb[1]), xyz(of_a ? ta[2] : tb[2]), probe, t, u, v, det)) {
                        if (kind & 1u) q.far_ = t;
                        else q.near_ = t;
                    }
                }
                const bool has_b = (h & 0xC00u) != 0u;  // every fourth case: a lone triangle in the iteration
                // one by one
                WalkRay seq = q;
                uint32_t seq_tri = 0xFFFFFFFFu;
                float seq_b1 = 0.0f, seq_b2 = 0.0f;
                bool seq_external = false;
                {
                    float t, u, v, det;
                    if (tri_hit(xyz(ta[0]), xyz(ta[1]), xyz(ta[2]), seq, t, u, v, det)) {
                        seq.far_ = t;
                        seq_tri = 0u, seq_b1 = u, seq_b2 = v, seq_external = det > 0.0f;
                    }
                    if (has_b && tri_hit(xyz(tb[0]), xyz(tb[1]), xyz(tb[2]), seq, t, u, v, det)) {
                        seq.far_ = t;
                        seq_tri = 1u, seq_b1 = u, seq_b2 = v, seq_external = det > 0.0f;
                    }
                }
                // as a pair
                LeafBest best;
                best.far_ = q.far_, best.triangle = 0xFFFFFFFFu, best.b1 = best.b2 = 0.0f, best.external = false;
                tri_pair_step(pair3(ta[0], has_b ? tb[0] : ta[0]), pair3(ta[1], has_b ? tb[1] : ta[1]), pair3(ta[2], has_b ? tb[2] : ta[2]), 0u, has_b, q, best);
                if (__float_as_uint(best.far_) != __float_as_uint(seq.far_) || best.triangle != seq_tri || __float_as_uint(best.b1) != __float_as_uint(seq_b1) ||
                    __float_as_uint(best.b2) != __float_as_uint(seq_b2) || best.external != seq_external)
                    bad += 1;
            }
        }
    }
    atomicAdd(&out[0], (unsigned long long)bad);
    atomicAdd(&out[1], (unsigned long long)tested);
    atomicAdd(&out[2], (unsigned long long)undecided);
    atomicAdd(&out[3], (unsigned long long)tiny_differs);
}

// =======================================================================================
// Host side of the context
// =======================================================================================
namespace hiprz {
thread_local std::string g_create_error;
int fail(hiprz_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->error = msg;
    else g_create_error = msg;
    return code;
}
// the launch sites' kernel stubs (hiprz_ctx.hpp: RZ_LAUNCH); filled during static initialisation of the translation units
std::vector<KernelEntry>& kernel_table() {
    static std::vector<KernelEntry> table;
    return table;
}
void register_kernel(const void* stub, const char* name) { kernel_table().push_back(KernelEntry{stub, name}); }
// Every kernel a launcher can select must resolve in the code objects this process loaded, on the device a context is created for:
// checked once per device, at the first hiprz_create.  (What it costs: the runtime loads every code object of the library up front
// instead of at the first launch from it.)
int resolve_kernels(int device) {
    static std::vector<int> checked;
    for (int d : checked)
        if (d == device) return HIPRZ_OK;
    for (const KernelEntry& e : kernel_table()) {
        hipFuncAttributes attr;
        const hipError_t err = hipFuncGetAttributes(&attr, e.stub);
        if (err != hipSuccess) {
            (void)hipGetLastError();
            return fail(nullptr, HIPRZ_ERR_DEVICE, std::string("libhiprz.so is inconsistent: the loaded gfx950 code objects do not hold a kernel the host side can launch (") +
                                                       hipGetErrorString(err) + "): " + e.name + " — rebuild (make -C rayzath_amd/csrc; tools/check_kernels.py)");
        }
    }
    checked.push_back(device);
    return HIPRZ_OK;
}
// settings are shared by the cameras of a context: a change invalidates the graph of every one of them
void invalidate_graphs(hiprz_ctx* c) {
    c->graph_valid = false;
    for (auto& f : c->parked) f.graph_valid = false;
}
}  // namespace hiprz

namespace {

void release_variance(hiprz_frame_state* c) {
    c->var_snap.release(), c->var_m0.release(), c->var_m1.release(), c->var_tiles.release(), c->var_image.release(), c->sum_m0.release(), c->sum_m1.release();
}
void release_frame(hiprz_frame_state* c) {
    c->st0.release(), c->st1.release(), c->st2.release(), c->accum.release(), c->depth.release(), c->rgba8.release();
    c->hit0.release(), c->hit1.release();
    c->nee.release(), c->prev_accum.release(), c->prev_depth.release();
    c->unit_cost.release(), c->launch_order.release(), c->order_keys.release(), c->seg_ctl.release();
    c->order_sort.keys_out.release(), c->order_sort.vals_a.release(), c->order_sort.vals_b.release(), c->order_sort.counts.release(), c->order_sort.row_total.release();
    c->sort_keys.release(), c->sort_perm.release();
    for (auto& t : c->sort_temp) t.keys_out.release(), t.vals_a.release(), t.vals_b.release(), t.counts.release(), t.row_total.release();
    c->shadow_keys.release(), c->shadow_perm.release();
    c->image_f4.release(), c->state_md.release(), c->state_ray.release(), c->gather.release(), c->sum_accum.release();
    c->guides.release(), c->dn_out.release(), c->dn_rgba8.release();
    c->guides_valid = c->dn_valid = false;
    release_variance(c);
}
void release_parked(hiprz_ctx* c, hiprz_frame_state* f) {  // a camera that is not the selected one: its graph, frame slots and frame
    if (f->graph_exec) (void)hipGraphExecDestroy(f->graph_exec);
    release_present(c, f);
    release_frame(f);
    f->pass_dev.release();
}

// Camera::reproject (cuda_camera.cuh:390-426) for one pixel of the frame that has just had its first pass: the first hit point —
// the pixel-centre ray (generateSimpleRay) at the stored depth — seen from the previous camera; where that camera's depth buffer holds
// the same surface (within 1 % of the distance), its accumulator * blend is appended to this pixel's.
struct PrevCamera {
    float position[3], x_axis[3], y_axis[3], z_axis[3];
    float tan_half_fov, aspect_ratio;
};
__global__ void __launch_bounds__(256) rz_reproject_kernel(const DFrame f, const DCamera cam, const PrevCamera prev, const float4* prev_accum,
                                                           const float* prev_depth, float blend) {
    const PixelId p = pixel_of_thread(f, cam, blockIdx.x, threadIdx.x);
    if (!p.active) return;
    Ray ray;
    generate_simple_ray(cam, ray, p.x, p.y);
    const v3 space_p = ray.o + ray.d * f.depth[p.local];
    const v3 rel = space_p - ld3(prev.position);
    const v3 local_p = transform_backward(ld3(prev.x_axis), ld3(prev.y_axis), ld3(prev.z_axis), rel);
    if (local_p.z <= 0.0f) return;  // behind the previous camera
    const float fx = (((local_p.x / local_p.z) / prev.tan_half_fov) + 0.5f) * float(cam.width);
    const float fy = (((local_p.y / local_p.z) / (-prev.tan_half_fov / prev.aspect_ratio)) + 0.5f) * float(cam.height);
    if (fx < 0.0f || fx >= float(cam.width) || fy < 0.0f || fy >= float(cam.height)) return;  // outside the previous frustum
    const uint32_t sx = uint32_t(fx), sy = uint32_t(fy);
    // the history is a row-major image of the WHOLE previous frame (keep_history): the source pixel of a moved camera may have been
    // rendered by another device of the context.  Pixels no shard of this context owns hold depth 0 and never pass the test below.
    const size_t from = size_t(sy) * cam.width + sx;
    const float point_dist = magnitude(rel), buffer_dist = prev_depth[from];
    if (fabsf(point_dist - buffer_dist) < 0.01f * point_dist) {
        const float4 a = f.accum[p.local], h = prev_accum[from];
        f.accum[p.local] = make_float4(a.x + h.x * blend, a.y + h.y * blend, a.z + h.z * blend, a.w + h.w * blend);
    }
}

void reproject_after_first_pass(hiprz_ctx* c, const DFrame& f, const hiprz_camera& previous) {
    PrevCamera prev;
    std::memcpy(prev.position, previous.position, 12), std::memcpy(prev.x_axis, previous.x_axis, 12);
    std::memcpy(prev.y_axis, previous.y_axis, 12), std::memcpy(prev.z_axis, previous.z_axis, 12);
    prev.tan_half_fov = previous.tan_half_fov, prev.aspect_ratio = previous.aspect_ratio;
    RZ_LAUNCH(rz_reproject_kernel, dim3(c->plan.tile_grid), dim3(256), 0, c->stream, f, c->dcamera, prev, c->prev_accum.ptr, c->prev_depth.ptr, c->temporal_blend);
}

int allocate_frame(hiprz_ctx* c) {
    c->frame_started = false;  // whatever history there was belongs to other buffers
    c->guides_valid = c->dn_valid = false;
    const uint32_t W = c->camera.width, H = c->camera.height;
    c->tiles_x = (W + 31u) / 32u;
    c->tiles_y = (H + 7u) / 8u;
    c->n_local_tiles = shard_local_tiles(c->tiles_x, c->tiles_y, c->rank, c->world);
    // owned active pixels (ray counter of this shard)
    uint64_t owned = 0;
    for (uint32_t lt = 0; lt < c->n_local_tiles; ++lt) {
        uint32_t tx, ty;
        shard_tile(lt, c->tiles_x, c->rank, c->world, tx, ty);  // (hiprz_shard.hpp)
        const uint32_t w = std::min(32u, W - tx * 32u), h = std::min(8u, H - ty * 8u);
        owned += uint64_t(w) * h;
    }
    c->owned_pixels = owned;
    const size_t n = size_t(c->n_local_tiles) * 256u;
    RZ_HIP(c, c->st0.resize(n));
    RZ_HIP(c, c->st1.resize(n));
    RZ_HIP(c, c->st2.resize(n));
    RZ_HIP(c, c->accum.resize(n));
    RZ_HIP(c, c->hit0.resize(n));
    RZ_HIP(c, c->hit1.resize(n));
    RZ_HIP(c, c->sort_keys.resize(n));
    RZ_HIP(c, c->sort_perm.resize(n));
    RZ_HIP(c, c->shadow_keys.resize(n));
    RZ_HIP(c, c->shadow_perm.resize(n));
    if (n) {
        RZ_HIP(c, hipMemsetAsync(c->sort_keys.ptr, 0, n * sizeof(uint32_t), c->stream));
        RZ_HIP(c, hipMemsetAsync(c->shadow_keys.ptr, 0, n * sizeof(uint32_t), c->stream));
        const int src = sort_workspace(c, n);
        if (src != HIPRZ_OK) return src;
    }
    RZ_HIP(c, c->depth.resize(n));
    RZ_HIP(c, c->rgba8.resize(n));
    RZ_HIP(c, c->image_f4.resize(size_t(W) * H));
    {   // heaviest-first launch order of the resident kernels: at most one unit per wave of the shard
        const size_t units = size_t(c->n_local_tiles) * 4u;
        RZ_HIP(c, c->unit_cost.resize(units));
        RZ_HIP(c, c->launch_order.resize(units));
        RZ_HIP(c, c->order_keys.resize(units));
        if (units) {
            RZ_HIP(c, hipMemsetAsync(c->unit_cost.ptr, 0, units * sizeof(uint32_t), c->stream));
            const int orc = sort_temp_resize(c, c->order_sort, units);
            if (orc != HIPRZ_OK) return orc;
        }
        c->order_units = 0u, c->batches_since_order = 0u;
    }
    {   // the segmented batch kernel's control words + one word per unit of the (swizzle-padded) grid
        const size_t words = hiprz::kSegFlags + ((size_t(c->n_local_tiles) + 7u) / 8u) * 8u;
        RZ_HIP(c, c->seg_ctl.resize(words));
        RZ_HIP(c, hipMemsetAsync(c->seg_ctl.ptr, 0, c->seg_ctl.count * sizeof(uint32_t), c->stream));
    }
    if (n) {
        RZ_HIP(c, hipMemsetAsync(c->accum.ptr, 0, n * sizeof(float4), c->stream));
        RZ_HIP(c, hipMemsetAsync(c->depth.ptr, 0, n * sizeof(float), c->stream));
        RZ_HIP(c, hipMemsetAsync(c->rgba8.ptr, 0, n * sizeof(uint32_t), c->stream));
        RZ_HIP(c, hipMemsetAsync(c->st0.ptr, 0, n * sizeof(float4), c->stream));
        RZ_HIP(c, hipMemsetAsync(c->st1.ptr, 0, n * sizeof(float4), c->stream));
        RZ_HIP(c, hipMemsetAsync(c->st2.ptr, 0, n * sizeof(float2), c->stream));
    }
    return HIPRZ_OK;
}

}  // namespace

namespace hiprz {

// the only code that turns context fields into inputs of the launch plan (hiprz_plan.hpp)
PlanInputs plan_inputs(const hiprz_ctx* c) {
    PlanInputs in{};
    in.pipeline_setting = c->pipeline_setting, in.traversal_mode = c->traversal_mode, in.lds_scene_override = c->lds_scene_override;
    in.walk_order = c->walk_order, in.sort_rays = c->sort_rays, in.sort_bits = c->sort_bits, in.shadow_sort = c->shadow_sort;
    in.shadow_packet = c->shadow_packet, in.defer_shadow_rays = c->defer_shadow_rays, in.nolight_kernels = c->nolight_kernels;
    in.trace_waves = c->trace_waves, in.batch_waves = c->batch_waves, in.batch_segments = c->batch_segments;
    in.wave_resident_max = c->wave_resident_max, in.xcd_swizzle = c->xcd_swizzle, in.heavy_first = c->heavy_first != 0, in.mode_flags = c->mode_flags;
    in.spot_samples = c->config.spot_samples, in.direct_samples = c->config.direct_samples;
    in.have_scene = c->have_scene, in.scene_tree = c->scene_tree, in.lds_scene = c->lds_scene, in.hot_bytes = c->dscene.hot_bytes;
    in.stack_entries = c->stack_entries, in.world_stack_entries = c->dscene.world_stack_entries, in.mesh_stack_entries = c->dscene.mesh_stack_entries;
    in.n_instances = c->dscene.n_instances, in.n_lights = c->dscene.n_spot_lights + c->dscene.n_direct_lights, in.n_textures = c->n_textures;
    in.n_nodes = c->n_nodes, in.top_count = c->dscene.top_count, in.flat_world = c->flat_world;
    in.have_camera = c->have_camera, in.n_local_tiles = c->n_local_tiles;
    return in;
}

DFrame make_frame(hiprz_ctx* c, bool counted) {
    const LaunchPlan& p = c->plan;
    DFrame f{};
    f.st0 = c->st0.ptr, f.st1 = c->st1.ptr, f.st2 = c->st2.ptr;
    f.accum = c->accum.ptr, f.depth = c->depth.ptr, f.rgba8 = c->rgba8.ptr;
    f.hit0 = c->hit0.ptr, f.hit1 = c->hit1.ptr;
    f.pass = c->pass_dev.ptr;
    f.counters = counted ? c->counters_dev.ptr : nullptr;
    f.tiles_x = c->tiles_x, f.rank = c->rank, f.world = c->world, f.n_local_tiles = c->n_local_tiles;
    f.xcd_swizzle = c->xcd_swizzle ? 1u : 0u;
    f.nee = c->nee.ptr, f.nee_quads = p.nee_quads;
    f.sort_key = p.sort_enabled ? c->sort_keys.ptr : nullptr;
    f.perm = p.sort_enabled ? c->sort_perm.ptr : nullptr;
    f.shadow_key = p.shadow_sort ? c->shadow_keys.ptr : nullptr;
    f.shadow_perm = p.shadow_sort ? c->shadow_perm.ptr : nullptr;
    // resident kernels: units by falling cost once an order for THIS kind of unit exists; costs are always collected (not while counting)
    f.unit_cost = p.heavy_units ? c->unit_cost.ptr : nullptr;
    f.launch_order = p.heavy_units && c->order_units == p.heavy_units ? c->launch_order.ptr : nullptr;
    return f;
}

DConfig make_config(const hiprz_ctx* c) {
    return DConfig{c->config.max_depth, c->config.spot_samples, c->config.direct_samples, c->config.seed, c->mode_flags};
}

void resolve_pipeline(hiprz_ctx* c) {
    const int before = c->pipeline;
    c->pipeline = choose_pipeline(plan_inputs(c));
    if (c->pipeline != before) invalidate_graphs(c);
}

}  // namespace hiprz

namespace {

// one pass on the stream: trace + shade (split pipeline) or the fused kernel
void launch_pass(hiprz_ctx* c, const DFrame& f, bool first, bool counted, hipEvent_t between_trace_and_shade = nullptr) {
    c->sorted_this_pass = false;
    if (c->plan.shade.active) {  // split pipeline, and the first pass of a wave-resident frame
        launch_trace(c, f, first, counted);
        if (between_trace_and_shade) (void)hipEventRecord(between_trace_and_shade, c->stream);
        launch_shade(c, f, first, counted);
    } else {
        launch_fused(c, f, first, counted);
    }
}

// resident pipeline: all `n` cumulative passes of the batch in one launch (+ one launch that advances the pass index)
void launch_resident(hiprz_ctx* c, const DFrame& f, uint32_t n, bool counted, hipEvent_t before = nullptr, hipEvent_t after = nullptr) {
    launch_batch(c, f, n, counted, before, after);
    RZ_LAUNCH(rz_pass_add_kernel, dim3(1), dim3(1), 0, c->stream, c->pass_dev.ptr, n);
    c->rgba8_valid = true;
    // Heaviest first: the batch that just ran left every unit's cost behind.  The order is derived after the first batch that measured
    // (and whenever the kind of unit changed) and refreshed every 64th batch — per-tile costs of a fixed view are stable, paths
    // regenerate at the same pixels — by one key kernel + a 24-bit radix sort of a few thousand keys on the render stream.
    if (f.unit_cost && n >= 2u) {
        const uint32_t units = c->plan.heavy_units;
        c->batches_since_order += 1u;
        if (c->order_units != units || c->batches_since_order >= 64u) {
            RZ_LAUNCH(rz_order_keys_kernel, dim3((units + 255u) / 256u), dim3(256), 0, c->stream, c->unit_cost.ptr, c->order_keys.ptr, units);
            sort_u32(c->stream, c->order_keys.ptr, units, 24, c->launch_order.ptr, nullptr, c->order_sort);
            c->order_units = units, c->batches_since_order = 0u;
        }
    }
}

hipEvent_t take_event(hiprz_ctx* c) {
    if (!c->event_pool.empty()) {
        hipEvent_t e = c->event_pool.back();
        c->event_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

void drop_graph(hiprz_ctx* c) {
    // a replay of the old exec may still be in flight on the stream (an asynchronous caller that changes a setting between
    // two render calls): wait for it before the exec goes away
    if (c->graph_exec && c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->graph_exec) (void)hipGraphExecDestroy(c->graph_exec);
    c->graph_exec = nullptr;
    c->graph_valid = false;
}

// [cumulative pass, sort, pass update] x n on the stream — eagerly, or into a capture
void enqueue_cumulative(hiprz_ctx* c, const DFrame& f, uint32_t n) {
    for (uint32_t i = 0; i < n; ++i) {
        launch_pass(c, f, false, false);
        launch_sort(c);
        RZ_LAUNCH(rz_pass_update_kernel, dim3(1), dim3(1), 0, c->stream, c->pass_dev.ptr);
    }
}

int finish_batch(hiprz_ctx* c, hipEvent_t e0, hipEvent_t e1, uint32_t n_passes, const StageTimer& timer) {
    RZ_HIP(c, hipEventRecord(e1, c->stream));
    RZ_HIP(c, hipGetLastError());
    if (c->pending_events.size() >= 4096) {  // nobody is collecting timings: recycle the oldest pair
        c->event_pool.push_back(c->pending_events.front().first);
        c->event_pool.push_back(c->pending_events.front().second);
        c->pending_events.erase(c->pending_events.begin());
        c->pending_launches.erase(c->pending_launches.begin());
    }
    c->pending_events.emplace_back(e0, e1);
    c->pending_launches.push_back(n_passes);
    c->timings.set("render (enqueue)", timer.ms());
    return HIPRZ_OK;
}

// What a captured batch depends on, byte for byte: the arguments every kernel of the batch receives by value (scene, camera, config and
// frame views: raw pointers into buffers the context owns, sizes, sharding), the workspaces the sorts use, and the launch plan: every
// kernel instantiation, grid and LDS size the batch's launches select.  The graph holds kernel nodes and event fork / join nodes only — no memset, memcpy or
// library nodes, no host pointers — so "same key" means a replay does what an eager batch would do now.
std::vector<unsigned char> graph_key_of(hiprz_ctx* c, const DFrame& f, uint32_t n_passes) {
    std::vector<unsigned char> key;
    auto put = [&key](const void* p, size_t n) { key.insert(key.end(), static_cast<const unsigned char*>(p), static_cast<const unsigned char*>(p) + n); };
    const DConfig cfg = make_config(c);
    put(&c->dscene, sizeof(DScene)), put(&c->dcamera, sizeof(DCamera)), put(&cfg, sizeof cfg), put(&f, sizeof f);
    for (const auto& t : c->sort_temp) {
        const void* ptrs[5] = {t.keys_out.ptr, t.vals_a.ptr, t.vals_b.ptr, t.counts.ptr, t.row_total.ptr};
        put(ptrs, sizeof ptrs);
    }
    put(&c->plan, sizeof c->plan), put(&n_passes, sizeof n_passes);
    return key;
}

// the first pass of a restarted frame (renderFirstPass) with the reprojection of the frame it replaces; the caller advances the pass index
void first_pass(hiprz_ctx* c, const DFrame& f, bool counted) {
    const bool history = keep_history(c);
    const hiprz_camera previous = c->frame_camera;
    c->frame_camera = c->camera, c->frame_started = true;
    RZ_LAUNCH(rz_pass_reset_kernel, dim3(1), dim3(1), 0, c->stream, c->pass_dev.ptr);
    launch_pass(c, f, true, counted);
    if (history) reproject_after_first_pass(c, f, previous);
    c->reset_pending = false;
    c->passes = 0;
    c->ray_count = 0;
}

void grow_kernel_events(hiprz_ctx* c, size_t n) {
    while (c->kernel_events.size() < n) {
        hipEvent_t e = nullptr;
        (void)hipEventCreate(&e);
        c->kernel_events.push_back(e);
    }
}

int render_passes(hiprz_ctx* c, uint32_t n_passes, bool counted) {
    if (!c->have_scene || !c->have_camera) return fail(c, HIPRZ_ERR_STATE, "render before scene and camera upload");
    if (n_passes == 0) return HIPRZ_OK;
    if (c->n_local_tiles == 0) {  // a part that owns no tile of this frame traces nothing: its ray counter restarts with the frame all the same
        if (c->reset_pending) c->ray_count = 0;  // (it held the previous frame's rays, which hiprz_ray_count would go on adding to the other parts')
        return HIPRZ_OK;
    }
    resolve_pipeline(c);  // the choice depends on the selected camera's shard size too
    StageTimer timer;
    c->plan = plan_launches(plan_inputs(c), counted);
    c->have_plan = true;
    if (c->plan.defer_shadows) {  // hand-over buffers of the deferred shadow rays: (4 + 2 * samples) float4 per owned pixel
        const size_t n = size_t(c->n_local_tiles) * 256u * c->plan.nee_quads;
        if (c->nee.count < n) c->graph_valid = false;
        RZ_HIP(c, c->nee.resize(n));
    }
    const DFrame f = make_frame(c, counted);
    if (!f.perm) c->perm_valid = false;                                        // passes without reordering leave the order behind
    else if (!c->reset_pending && !c->perm_valid) launch_sort_identity(c);    // reordering was switched on between two batches
    hipEvent_t e0 = take_event(c), e1 = take_event(c);
    RZ_HIP(c, hipEventRecord(e0, c->stream));
    c->rgba8_valid = false;
    if (c->pipeline == 2) {
        uint32_t remaining = n_passes;
        if (c->reset_pending) {  // renderFirstPass: the fused kernel
            first_pass(c, f, counted);
            RZ_LAUNCH(rz_pass_update_kernel, dim3(1), dim3(1), 0, c->stream, c->pass_dev.ptr);
            c->passes += 1;
            c->ray_count += c->owned_pixels;
            remaining -= 1u;
        }
        if (remaining) {
            c->kernel_event_passes = 0;
            if (counted) launch_resident(c, f, remaining, true);
            else if (c->time_kernels) {  // bench.py's roofline: the batch kernel's own duration
                grow_kernel_events(c, 3u);
                launch_resident(c, f, remaining, false, c->kernel_events[0], c->kernel_events[1]);
                c->kernel_event_passes = remaining;
            } else launch_resident(c, f, remaining, false);
            c->passes += remaining;
            c->ray_count += uint64_t(remaining) * c->owned_pixels;
        }
        return finish_batch(c, e0, e1, n_passes, timer);
    }
    if (c->use_graph && !c->time_kernels && !counted && !c->reset_pending && n_passes >= 2) {
        // steady state: one graph launch instead of 2 * n_passes kernel launches
        std::vector<unsigned char> key = graph_key_of(c, f, n_passes);
#ifdef RZ_GRAPH_ASSERT  // debug builds: a key that changed under a graph still marked valid is a missed invalidation — say so loudly
        if (c->graph_valid && c->graph_passes == n_passes && key != c->graph_key) {
            std::fprintf(stderr, "hiprz: captured graph marked valid although its launch arguments changed (a buffer was reallocated or a setting changed without invalidate_graphs)\n");
            std::abort();
        }
#endif
        if (!c->graph_valid || c->graph_passes != n_passes || key != c->graph_key) {
            drop_graph(c);
            c->graph_key = std::move(key);
            hipGraph_t graph = nullptr;
            RZ_HIP(c, hipStreamBeginCapture(c->stream, hipStreamCaptureModeThreadLocal));
            enqueue_cumulative(c, f, n_passes);
            RZ_HIP(c, hipStreamEndCapture(c->stream, &graph));
            const hipError_t ie = hipGraphInstantiate(&c->graph_exec, graph, nullptr, nullptr, 0);
            (void)hipGraphDestroy(graph);
            if (ie != hipSuccess) return fail(c, HIPRZ_ERR_DEVICE, std::string("hipGraphInstantiate: ") + hipGetErrorString(ie));
            c->graph_passes = n_passes;
            c->graph_valid = true;
            c->graph_captures += 1;
        }
        RZ_HIP(c, hipGraphLaunch(c->graph_exec, c->stream));
        c->passes += n_passes;
        c->ray_count += uint64_t(n_passes) * c->owned_pixels;
        return finish_batch(c, e0, e1, n_passes, timer);
    }
    // kernel-level timing (bench.py's roofline): events before the trace kernel, between the two kernels and after the
    // shade kernel of every pass.  Event timing does not work from inside a captured graph, so a timed batch is launched
    // eagerly.
    const bool timed = c->time_kernels && c->pipeline == 1 && !counted && !c->reset_pending;
    if (timed) {
        grow_kernel_events(c, 3u * size_t(n_passes));
        c->kernel_event_passes = n_passes;
    }
    for (uint32_t i = 0; i < n_passes; ++i) {
        if (timed) {
            (void)hipEventRecord(c->kernel_events[3 * i], c->stream);
            launch_pass(c, f, false, false, c->kernel_events[3 * i + 1]);
            (void)hipEventRecord(c->kernel_events[3 * i + 2], c->stream);
            launch_sort(c);
            RZ_LAUNCH(rz_pass_update_kernel, dim3(1), dim3(1), 0, c->stream, c->pass_dev.ptr);
            c->passes += 1;
            c->ray_count += c->owned_pixels;
            continue;
        }
        if (c->reset_pending) first_pass(c, f, counted);
        else launch_pass(c, f, false, counted);
        launch_sort(c);
        RZ_LAUNCH(rz_pass_update_kernel, dim3(1), dim3(1), 0, c->stream, c->pass_dev.ptr);
        c->passes += 1;
        c->ray_count += c->owned_pixels;  // traced_rays += W*H per pass (cpu_engine_renderer.cpp:173), per shard
    }
    return finish_batch(c, e0, e1, n_passes, timer);
}

// A render call: its passes and, under hiprz_set_variance, the batch they form — the moments are zeroed before the passes of a call that
// restarts the frame, and rz_moments_kernel follows the passes eagerly on the same stream (behind the graph launch or the resident
// kernel: it is no part of the captured graph, and nothing the graph's key holds depends on it).
int render_impl(hiprz_ctx* c, uint32_t n_passes, bool counted) {
    const bool batch = c->variance_on && c->have_scene && c->have_camera && n_passes != 0u && c->n_local_tiles != 0u;
    const size_t n = size_t(c->n_local_tiles) * 256u;
    bool snap_only = false;
    if (batch) {
        // (a buffer that had to be allocated is zeroed too: hiprz_set_variance and whatever sizes a frame leave a restart pending)
        const bool fresh = c->reset_pending || c->var_snap.count < n || c->var_m0.count < n || c->var_m1.count < n;
        RZ_HIP(c, c->var_snap.resize(n));
        RZ_HIP(c, c->var_m0.resize(n));
        RZ_HIP(c, c->var_m1.resize(n));
        if (fresh) {
            RZ_HIP(c, hipMemsetAsync(c->var_snap.ptr, 0, n * sizeof(float4), c->stream));
            RZ_HIP(c, hipMemsetAsync(c->var_m0.ptr, 0, n * sizeof(float4), c->stream));
            RZ_HIP(c, hipMemsetAsync(c->var_m1.ptr, 0, n * sizeof(float4), c->stream));
        }
        // keep_history's own condition: the first pass of this call is followed by the reprojection of the previous frame
        snap_only = c->reset_pending && (c->mode_flags & HIPRZ_COMPAT_REPROJECTION) && c->frame_started;
    }
    const int rc = render_passes(c, n_passes, counted);
    if (rc != HIPRZ_OK || !batch) return rc;
    RZ_LAUNCH(rz_moments_kernel, dim3(c->n_local_tiles), dim3(256), 0, c->stream, c->accum.ptr, c->var_snap.ptr, c->var_m0.ptr, c->var_m1.ptr, uint32_t(n),
              snap_only ? 1u : 0u);
    RZ_HIP(c, hipGetLastError());
    return HIPRZ_OK;
}

// hiprz_select_camera on one context: the selected camera's frame state lives in the context itself, the others are parked
void select_camera_one(hiprz_ctx* c, uint32_t k) {
    if (k == c->active_camera || k >= c->parked.size()) return;
    hiprz_frame_state& self = *c;
    std::swap(c->parked[c->active_camera], self);  // park the active one (its slot held an empty state)
    std::swap(self, c->parked[k]);
    c->active_camera = k;
}
// A captured graph of a batch of passes stays valid while nothing its kernel arguments depend on has changed: the setters
// invalidate it only when a value really differs (both host sides call hiprz_set_config before every frame).
template <typename T>
void assign_setting(hiprz_ctx* c, T& field, const T& value) {
    if (std::memcmp(&field, &value, sizeof(T)) != 0) {
        field = value;
        invalidate_graphs(c);
    }
}
}  // namespace

extern "C" {

int hiprz_create(hiprz_ctx** out, int device_id) {
    if (!out) return fail(nullptr, HIPRZ_ERR_INVALID, "hiprz_create: out is null");
    *out = nullptr;
    int n_devices = 0;
    hipError_t e = hipGetDeviceCount(&n_devices);
    if (e != hipSuccess || n_devices == 0)
        return fail(nullptr, HIPRZ_ERR_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= n_devices) return fail(nullptr, HIPRZ_ERR_INVALID, "hiprz_create: device id out of range");
    e = hipSetDevice(device_id);
    if (e != hipSuccess) return fail(nullptr, HIPRZ_ERR_DEVICE, std::string("hipSetDevice: ") + hipGetErrorString(e));
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, device_id);
    if (e != hipSuccess) return fail(nullptr, HIPRZ_ERR_DEVICE, std::string("hipGetDeviceProperties: ") + hipGetErrorString(e));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(nullptr, HIPRZ_ERR_DEVICE, std::string("hiprz is built for gfx950 only, device is ") + prop.gcnArchName);
    if (const int rc = resolve_kernels(device_id); rc != HIPRZ_OK) return rc;
    auto* c = new hiprz_ctx();
    if (const char* w = std::getenv("HIPRZ_TRACE_WAVES")) c->trace_waves = std::atoi(w);
    if (const char* w = std::getenv("HIPRZ_DEFER_SHADOWS")) c->defer_shadow_rays = std::atoi(w) != 0;
    if (const char* w = std::getenv("HIPRZ_HEAVY_FIRST")) c->heavy_first = std::atoi(w) != 0;
    if (const char* w = std::getenv("HIPRZ_BATCH_WAVES")) c->batch_waves = std::atoi(w);
    if (const char* w = std::getenv("HIPRZ_BATCH_SEGMENTS")) c->batch_segments = std::max(0, std::atoi(w));
    if (const char* w = std::getenv("HIPRZ_NOLIGHT_KERNELS")) c->nolight_kernels = std::atoi(w) != 0;
    if (const char* w = std::getenv("HIPRZ_SORT_BITS")) c->sort_bits = std::min(24, std::max(0, std::atoi(w)));
    if (const char* w = std::getenv("HIPRZ_SHADOW_PACKET")) c->shadow_packet = std::atoi(w);
    if (const char* w = std::getenv("HIPRZ_SHADOW_TREE")) c->shadow_tree = std::atoi(w) != 0;
    if (const char* w = std::getenv("HIPRZ_SHADOW_SORT")) c->shadow_sort = std::atoi(w) != 0;
    if (const char* w = std::getenv("HIPRZ_WAVE_RESIDENT_MAX")) c->wave_resident_max = uint32_t(std::max(0, std::atoi(w)));
    c->device = device_id;
    c->n_cus = uint32_t(std::max(1, prop.multiProcessorCount));
    c->parked.resize(1);  // one camera; its state lives in the context itself
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->peer_done, hipEventDisableTiming);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->aux_fork, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->aux_join, hipEventDisableTiming);
    if (e == hipSuccess) e = c->pass_dev.resize(1);
    if (e == hipSuccess) e = c->counters_dev.resize(16);
    if (e == hipSuccess) e = c->pick_dev.resize(4);
    if (e == hipSuccess) e = hipMemsetAsync(c->pass_dev.ptr, 0, sizeof(uint32_t), c->stream);
    if (e != hipSuccess) {
        const std::string msg = std::string("context setup: ") + hipGetErrorString(e);
        hiprz_destroy(c);
        return fail(nullptr, HIPRZ_ERR_DEVICE, msg);
    }
    *out = c;
    return HIPRZ_OK;
}

int hiprz_create_multi(hiprz_ctx** out, const int* device_ids, int n_devices) {
    if (!out) return fail(nullptr, HIPRZ_ERR_INVALID, "hiprz_create_multi: out is null");
    *out = nullptr;
    if (!device_ids || n_devices < 1 || n_devices > 64) return fail(nullptr, HIPRZ_ERR_INVALID, "hiprz_create_multi: 1..64 device ids");
    hiprz_ctx* head = nullptr;
    int rc = hiprz_create(&head, device_ids[0]);
    if (rc != HIPRZ_OK) return rc;
    for (int r = 1; r < n_devices; ++r) {
        hiprz_ctx* peer = nullptr;
        rc = hiprz_create(&peer, device_ids[r]);
        if (rc != HIPRZ_OK) {
            const std::string msg = g_create_error;
            (void)hiprz_destroy(head);
            return fail(nullptr, rc, msg);
        }
        peer->is_peer = true;
        head->peers.push_back(peer);
        if (device_ids[r] != device_ids[0]) {  // direct copies between the two GPUs (xGMI); absent peer access hip stages them through the host
            int can = 0;
            (void)hipDeviceCanAccessPeer(&can, device_ids[0], device_ids[r]);
            if (can) {
                (void)hipSetDevice(device_ids[0]);
                (void)hipDeviceEnablePeerAccess(device_ids[r], 0);
                (void)hipGetLastError();  // "already enabled" is fine
            }
        }
    }
    rc = hiprz_set_shard(head, 0u, 1u);
    if (rc != HIPRZ_OK) {
        const std::string msg = head->error;
        (void)hiprz_destroy(head);
        return fail(nullptr, rc, msg);
    }
    *out = head;
    return HIPRZ_OK;
}

int hiprz_device_count(hiprz_ctx* c, uint32_t* out) {
    if (!c || !out) return HIPRZ_ERR_INVALID;
    *out = uint32_t(c->peers.size()) + 1u;
    return HIPRZ_OK;
}

// ---- cameras: the reference renders every enabled camera of the world per call (cpu_engine_renderer.cpp:97-117) ----
int hiprz_set_camera_count(hiprz_ctx* c, uint32_t n) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_camera_count(p, n));
    if (n == 0u || n > 4096u) return fail(c, HIPRZ_ERR_INVALID, "set_camera_count: 1..4096 cameras");
    (void)hipSetDevice(c->device);
    if (c->active_camera >= n) select_camera_one(c, 0u);
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    for (uint32_t k = n; k < uint32_t(c->parked.size()); ++k) release_parked(c, &c->parked[k]);
    c->parked.resize(n);
    return HIPRZ_OK;
}

int hiprz_camera_count(hiprz_ctx* c, uint32_t* out) {
    if (!c || !out) return HIPRZ_ERR_INVALID;
    *out = uint32_t(c->parked.size());
    return HIPRZ_OK;
}

int hiprz_select_camera(hiprz_ctx* c, uint32_t index) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_select_camera(p, index));
    if (index >= c->parked.size()) return fail(c, HIPRZ_ERR_INVALID, "select_camera: index beyond hiprz_set_camera_count");
    select_camera_one(c, index);
    if (!c->pass_dev.ptr) {  // a camera selected for the first time: its device-resident pass index
        (void)hipSetDevice(c->device);
        RZ_HIP(c, c->pass_dev.resize(1));
        RZ_HIP(c, hipMemsetAsync(c->pass_dev.ptr, 0, sizeof(uint32_t), c->stream));
    }
    return HIPRZ_OK;
}

int hiprz_destroy(hiprz_ctx* c) {
    if (!c) return HIPRZ_OK;
    for (hiprz_ctx* p : c->peers) (void)hiprz_destroy(p);
    c->peers.clear();
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (uint32_t k = 0; k < uint32_t(c->parked.size()); ++k)  // every camera's frame
        if (k != c->active_camera) release_parked(c, &c->parked[k]);
    if (c->peer_done) (void)hipEventDestroy(c->peer_done);
    if (c->history_done) (void)hipEventDestroy(c->history_done);
    if (c->aux_stream) (void)hipStreamSynchronize(c->aux_stream), (void)hipStreamDestroy(c->aux_stream);
    if (c->aux_fork) (void)hipEventDestroy(c->aux_fork);
    if (c->aux_join) (void)hipEventDestroy(c->aux_join);
    drop_graph(c);
    for (auto& p : c->pending_events) {
        (void)hipEventDestroy(p.first);
        (void)hipEventDestroy(p.second);
    }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    for (auto e : c->kernel_events) (void)hipEventDestroy(e);
    c->hot.release(), c->node_skip.release(), c->nodes64.release(), c->textures.release();
    c->dev_nodes.release(), c->has_mesh.release(), c->build_temp.release(), c->slot_parent.release(), c->ref_to_dev.release(), c->refit_visit.release();
    c->world_items.release(), c->update_tris.release(), c->update_attrs.release();
    c->shadow_nodes64.release(), c->shadow_order.release();
    c->build_sort.keys_out.release(), c->build_sort.vals_a.release(), c->build_sort.vals_b.release(), c->build_sort.counts.release(), c->build_sort.row_total.release();
    c->caller_sort.keys_out.release(), c->caller_sort.vals_a.release(), c->caller_sort.vals_b.release(), c->caller_sort.counts.release(), c->caller_sort.row_total.release();
    c->texels.release(), c->spot_lights.release(), c->direct_lights.release();
    release_present(c, c);
    release_frame(c);
    c->pass_dev.release(), c->counters_dev.release(), c->pick_dev.release(), c->present_gather.release();
    c->dn_tmp[0].release(), c->dn_tmp[1].release();
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
    return HIPRZ_OK;
}

const char* hiprz_last_error(const hiprz_ctx* c) { return c ? c->error.c_str() : g_create_error.c_str(); }

int hiprz_upload_camera(hiprz_ctx* c, const hiprz_camera* cam) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_upload_camera(p, cam));
    if (!cam) return fail(c, HIPRZ_ERR_INVALID, "upload_camera: camera is null");
    if (cam->width == 0 || cam->height == 0 || cam->width > 32768u || cam->height > 32768u)
        return fail(c, HIPRZ_ERR_INVALID, "upload_camera: resolution must be 1..32768");
    StageTimer timer;
    (void)hipSetDevice(c->device);
    const bool resized = !c->have_camera || cam->width != c->camera.width || cam->height != c->camera.height;
    if (!c->have_camera || std::memcmp(&c->camera, cam, sizeof(hiprz_camera)) != 0) c->graph_valid = false;
    c->camera = *cam;
    DCamera& d = c->dcamera;
    std::memcpy(d.position, cam->position, 12);
    std::memcpy(d.x_axis, cam->x_axis, 12);
    std::memcpy(d.y_axis, cam->y_axis, 12);
    std::memcpy(d.z_axis, cam->z_axis, 12);
    d.width = cam->width, d.height = cam->height;
    d.tan_half_fov = cam->tan_half_fov, d.aspect_ratio = cam->aspect_ratio;
    d.near_ = cam->near_far[0], d.far_ = cam->near_far[1];
    d.focal_distance = cam->focal_distance, d.aperture = cam->aperture, d.exposure_time = cam->exposure_time;
    c->have_camera = true;
    if (resized) {
        int rc = allocate_frame(c);
        if (rc == HIPRZ_OK) rc = allocate_present(c);
        if (rc != HIPRZ_OK) return rc;
    }
    c->reset_pending = true;  // camera changed => context.reset (cpu_engine_renderer.cpp:108-112)
    c->guides_valid = false;
    c->timings.set("upload camera", timer.ms());
    return HIPRZ_OK;
}

int hiprz_set_config(hiprz_ctx* c, const hiprz_config* cfg) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!cfg) return fail(c, HIPRZ_ERR_INVALID, "set_config: config is null");
    for (size_t r = 0; r < c->peers.size(); ++r) {  // HIPRZ_SHARD_SAMPLES: part k of the context draws from the seed stream seed + k
        hiprz_ctx* p = c->peers[r];
        hiprz_config part = *cfg;
        if (c->shard_mode == HIPRZ_SHARD_SAMPLES) part.seed += uint32_t(r) + 1u;
        const int rz_rc = hiprz_set_config(p, &part);
        if (rz_rc != HIPRZ_OK) return fail(c, rz_rc, "device " + std::to_string(p->device) + ": " + p->error);
    }
    if (cfg->max_depth == 0 || cfg->max_depth > 254u) return fail(c, HIPRZ_ERR_INVALID, "max_depth must be 1..254 (u8, 255 = path ended)");
    // The CPU kernel divides by sample_count/light_count and yields NaN for 0 samples
    // (cpu_engine_kernel.cpp:742-743, 789-790); the CUDA backend clamps to >= 1 (cuda_kernel_data.cu:23-31).
    if (cfg->spot_samples == 0 || cfg->direct_samples == 0 || cfg->spot_samples > 255u || cfg->direct_samples > 255u)
        return fail(c, HIPRZ_ERR_INVALID, "light sample counts must be 1..255");
    if (std::memcmp(&c->config, cfg, sizeof(hiprz_config)) != 0) stale_guides(c);
    assign_setting(c, c->config, *cfg);
    return HIPRZ_OK;
}

namespace {
int reset_all_cameras(hiprz_ctx* c) {
    for (hiprz_ctx* p : c->peers) (void)reset_all_cameras(p);
    c->reset_pending = true;
    for (auto& f : c->parked) f.reset_pending = true;
    stale_guides(c);
    return HIPRZ_OK;
}
int set_shard_one(hiprz_ctx* c, uint32_t rank, uint32_t world) {
    const bool changed = rank != c->rank || world != c->world;
    c->rank = rank, c->world = world;
    if (!changed) return HIPRZ_OK;
    invalidate_graphs(c);
    (void)hipSetDevice(c->device);
    const uint32_t active = c->active_camera;
    for (uint32_t k = 0; k < uint32_t(c->parked.size()); ++k) {  // every camera's frame is re-tiled for the new shard
        select_camera_one(c, k);
        if (c->have_camera) {
            int rc = allocate_frame(c);
            if (rc == HIPRZ_OK) rc = size_present_gather(c);
            if (rc != HIPRZ_OK) return rc;
            c->reset_pending = true;
        }
    }
    select_camera_one(c, active);
    return HIPRZ_OK;
}
}  // namespace

int hiprz_set_shard(hiprz_ctx* c, uint32_t rank, uint32_t world) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (world == 0 || rank >= world) return fail(c, HIPRZ_ERR_INVALID, "set_shard: need rank < world");
    // a multi-device context splits ITS shard once more over its devices: device r of n renders shard rank * n + r of world * n
    // (HIPRZ_SHARD_SAMPLES: every part renders the whole of the context's shard, on its own seed stream)
    const bool samples = c->shard_mode == HIPRZ_SHARD_SAMPLES;
    const uint32_t n = samples ? 1u : uint32_t(c->peers.size()) + 1u;
    c->user_rank = rank, c->user_world = world;
    for (uint32_t r = 1; r <= uint32_t(c->peers.size()); ++r) {
        const int rc = set_shard_one(c->peers[r - 1u], samples ? rank : rank * n + r, world * n);
        if (rc != HIPRZ_OK) return fail(c, rc, "device " + std::to_string(c->peers[r - 1u]->device) + ": " + c->peers[r - 1u]->error);
    }
    return set_shard_one(c, rank * n, world * n);
}

int hiprz_set_shard_mode(hiprz_ctx* c, uint32_t mode) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (mode > HIPRZ_SHARD_SAMPLES) return fail(c, HIPRZ_ERR_INVALID, "set_shard_mode: HIPRZ_SHARD_TILES or HIPRZ_SHARD_SAMPLES");
    if (mode == c->shard_mode) return HIPRZ_OK;
    c->shard_mode = mode;
    if (c->peers.empty()) return HIPRZ_OK;  // one part: both modes are the same thing
    // the parts' shards and seed streams follow the mode; whatever was accumulated under the other one does not mix with it
    int rc = hiprz_set_shard(c, c->user_rank, c->user_world);
    if (rc != HIPRZ_OK) return rc;
    const hiprz_config cfg = c->config;
    rc = hiprz_set_config(c, &cfg);
    if (rc != HIPRZ_OK) return rc;
    invalidate_graphs(c);
    for (hiprz_ctx* p : c->peers) invalidate_graphs(p);
    return reset_all_cameras(c);
}

int hiprz_shard_mode(hiprz_ctx* c, uint32_t* mode_out) {
    if (!c || !mode_out) return HIPRZ_ERR_INVALID;
    *mode_out = c->shard_mode;
    return HIPRZ_OK;
}

int hiprz_set_traversal_mode(hiprz_ctx* c, int mode) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_traversal_mode(p, mode));
    if (mode < -1 || mode == 0 || mode > 3) return fail(c, HIPRZ_ERR_INVALID, "traversal mode: -1 = per scene, 1 = LDS stack, 2 = workgroup-binned, 3 = skip links (single-wave workgroups)");
    assign_setting(c, c->traversal_mode, mode);
    resolve_pipeline(c);
    return HIPRZ_OK;
}

int hiprz_set_mode(hiprz_ctx* c, uint32_t compat_flags) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_mode(p, compat_flags));
    if (compat_flags & ~HIPRZ_MODE_CUDA_COMPAT) return fail(c, HIPRZ_ERR_INVALID, "set_mode: unknown HIPRZ_COMPAT_* flag");
    if (compat_flags != c->mode_flags) {
        const bool integrator_changed = ((compat_flags ^ c->mode_flags) & kIntegratorFlags) != 0u;
        c->mode_flags = compat_flags;
        if (integrator_changed) {
            stale_guides(c);
            invalidate_graphs(c);
            c->reset_pending = true;  // another integrator: what has been accumulated does not mix with it
            for (auto& f : c->parked) f.reset_pending = true;
            resolve_pipeline(c);
        }
    }
    return HIPRZ_OK;
}

int hiprz_set_temporal_blend(hiprz_ctx* c, float blend) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_temporal_blend(p, blend));
    c->temporal_blend = std::min(std::max(blend, 0.0f), 1.0f);  // camera.cpp:154-156
    return HIPRZ_OK;
}

int hiprz_set_tree(hiprz_ctx* c, uint32_t tree) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_tree(p, tree));
    if (tree > HIPRZ_TREE_AUTO) return fail(c, HIPRZ_ERR_INVALID, "set_tree: HIPRZ_TREE_REFERENCE, _SAH, _DEVICE, _DEVICE_SAH or _AUTO");
    c->tree_mode = tree == HIPRZ_TREE_DEVICE_SAH ? HIPRZ_TREE_DEVICE : tree;  // one kind of scene (device-built, refittable), two builders
    c->device_sah = tree == HIPRZ_TREE_DEVICE_SAH;
    return HIPRZ_OK;
}

int hiprz_tree(hiprz_ctx* c, uint32_t* tree_out) {
    if (!c || !tree_out) return HIPRZ_ERR_INVALID;
    if (!c->have_scene) return fail(c, HIPRZ_ERR_STATE, "tree: no scene uploaded");
    *tree_out = c->scene_tree == HIPRZ_TREE_DEVICE && c->build_sah ? HIPRZ_TREE_DEVICE_SAH : c->scene_tree;
    return HIPRZ_OK;
}

int hiprz_set_walk_order(hiprz_ctx* c, int order) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_walk_order(p, order));
    if (order < 0 || order > 2) return fail(c, HIPRZ_ERR_INVALID, "walk order: 0 = the reference's child order, 1 = front-to-back, 2 = front-to-back also in counted renders");
    assign_setting(c, c->walk_order, order);
    return HIPRZ_OK;
}

int hiprz_set_lds_scene(hiprz_ctx* c, int mode) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_lds_scene(p, mode));
    if (mode < -1 || mode > 1) return fail(c, HIPRZ_ERR_INVALID, "lds scene: -1 auto, 0 off, 1 on");
    assign_setting(c, c->lds_scene_override, mode);
    resolve_pipeline(c);
    return HIPRZ_OK;
}

int hiprz_set_pipeline(hiprz_ctx* c, int pipeline) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_pipeline(p, pipeline));
    if (pipeline < -1 || pipeline > 2) return fail(c, HIPRZ_ERR_INVALID, "pipeline: -1 = per scene, 0 = fused pass kernel, 1 = trace kernel + shade kernel, 2 = resident (one launch per batch of passes)");
    assign_setting(c, c->pipeline_setting, pipeline);
    resolve_pipeline(c);
    return HIPRZ_OK;
}

int hiprz_pipeline(hiprz_ctx* c, int* out) {
    if (!c || !out) return HIPRZ_ERR_INVALID;
    *out = c->pipeline;
    return HIPRZ_OK;
}

int hiprz_traversal_mode(hiprz_ctx* c, int* out) {
    if (!c || !out) return HIPRZ_ERR_INVALID;
    *out = int(plan_launches(plan_inputs(c), false).reported_mode);
    return HIPRZ_OK;
}

int hiprz_launch_plan(hiprz_ctx* c, uint32_t* words, uint32_t capacity, uint32_t* n_words_out) {
    constexpr uint32_t n = uint32_t(sizeof(LaunchPlan) / sizeof(uint32_t));
    static_assert(sizeof(LaunchPlan) == n * sizeof(uint32_t), "LaunchPlan is 32-bit words without padding");
    if (!c || !words || !n_words_out) return HIPRZ_ERR_INVALID;
    if (capacity < n) return fail(c, HIPRZ_ERR_INVALID, "launch_plan: the buffer holds fewer than " + std::to_string(n) + " words");
    if (!c->have_plan) return fail(c, HIPRZ_ERR_STATE, "launch_plan: no render call has planned its launches yet");
    std::memcpy(words, &c->plan, sizeof(LaunchPlan));
    *n_words_out = n;
    return HIPRZ_OK;
}

int hiprz_set_ray_sort(hiprz_ctx* c, int mode) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_ray_sort(p, mode));
    if (mode < -1 || mode > 1) return fail(c, HIPRZ_ERR_INVALID, "ray sort: -1 auto, 0 off, 1 on");
    assign_setting(c, c->sort_rays, mode);
    return HIPRZ_OK;
}

int hiprz_set_xcd_swizzle(hiprz_ctx* c, int enabled) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_xcd_swizzle(p, enabled));
    assign_setting(c, c->xcd_swizzle, enabled != 0);
    return HIPRZ_OK;
}

int hiprz_set_graph(hiprz_ctx* c, int enabled) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_graph(p, enabled));
    c->use_graph = enabled != 0;
    return HIPRZ_OK;
}

int hiprz_graph_captures(hiprz_ctx* c, uint32_t* out) {
    if (!c || !out) return HIPRZ_ERR_INVALID;
    *out = c->graph_captures;
    return HIPRZ_OK;
}

int hiprz_reset(hiprz_ctx* c) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_reset(p));
    c->reset_pending = true;
    c->guides_valid = false;
    return HIPRZ_OK;
}

int hiprz_set_variance(hiprz_ctx* c, int enabled) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_set_variance(p, enabled));
    const bool on = enabled != 0;
    if (on == c->variance_on) return HIPRZ_OK;
    c->variance_on = on;
    stale_guides(c);
    c->reset_pending = true;  // the moments belong to one accumulation, from its first batch on
    for (auto& f : c->parked) f.reset_pending = true;
    if (!on) {
        (void)hipSetDevice(c->device);
        (void)hipStreamSynchronize(c->stream);  // an enqueued batch may still write them
        release_variance(c);
        for (auto& f : c->parked) release_variance(&f);
    }
    return HIPRZ_OK;
}

int hiprz_render(hiprz_ctx* c, uint32_t n_passes) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!c->peers.empty() && n_passes) {
        const int rc = assemble_history(c);
        if (rc != HIPRZ_OK) return rc;
    }
    RZ_FANOUT(c, hiprz_render(p, n_passes));
    (void)hipSetDevice(c->device);
    return render_impl(c, n_passes, false);
}

int hiprz_render_counted(hiprz_ctx* c, uint32_t n_passes, hiprz_counters* out) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!out) return fail(c, HIPRZ_ERR_INVALID, "render_counted: out is null");
    hiprz_counters peers_total{};
    for (hiprz_ctx* p : c->peers) {
        hiprz_counters part{};
        const int rz_rc = hiprz_render_counted(p, n_passes, &part);
        if (rz_rc != HIPRZ_OK) return fail(c, rz_rc, "device " + std::to_string(p->device) + ": " + p->error);
        uint64_t* t = reinterpret_cast<uint64_t*>(&peers_total);
        const uint64_t* q = reinterpret_cast<const uint64_t*>(&part);
        for (size_t k = 0; k < sizeof(hiprz_counters) / sizeof(uint64_t); ++k) t[k] += q[k];
    }
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipMemsetAsync(c->counters_dev.ptr, 0, 16 * sizeof(unsigned long long), c->stream));
    const int rc = render_impl(c, n_passes, true);
    if (rc != HIPRZ_OK) return rc;
    unsigned long long v[10];
    RZ_HIP(c, hipMemcpyAsync(v, c->counters_dev.ptr, sizeof v, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    out->segments = v[0], out->box_tests = v[1], out->tri_tests = v[2], out->hits = v[3];
    out->shadow_rays = v[4], out->light_samples = v[5], out->texel_fetches = v[6], out->finished = v[7];
    out->shadow_box_tests = v[8], out->shadow_tri_tests = v[9];
    {
        uint64_t* t = reinterpret_cast<uint64_t*>(out);
        const uint64_t* q = reinterpret_cast<const uint64_t*>(&peers_total);
        for (size_t k = 0; k < sizeof(hiprz_counters) / sizeof(uint64_t); ++k) t[k] += q[k];
    }
    return HIPRZ_OK;
}

int hiprz_sync(hiprz_ctx* c) {
    if (!c) return HIPRZ_ERR_INVALID;
    RZ_FANOUT(c, hiprz_sync(p));
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    return HIPRZ_OK;
}

int hiprz_ray_count(hiprz_ctx* c, uint64_t* out) {
    if (!c || !out) return HIPRZ_ERR_INVALID;
    *out = total_ray_count(c);
    return HIPRZ_OK;
}
int hiprz_pass_count(hiprz_ctx* c, uint32_t* out) {
    if (!c || !out) return HIPRZ_ERR_INVALID;
    *out = c->passes;
    return HIPRZ_OK;
}

void* hiprz_stream(hiprz_ctx* c) { return c ? reinterpret_cast<void*>(c->stream) : nullptr; }

int hiprz_device_view(hiprz_ctx* c, void* dscene, size_t dscene_bytes, void* dcamera, size_t dcamera_bytes) {
    if (!c) return HIPRZ_ERR_INVALID;
    if (!dscene || dscene_bytes != sizeof(DScene) || dcamera_bytes != (dcamera ? sizeof(DCamera) : 0u))
        return fail(c, HIPRZ_ERR_INVALID, "device_view: the caller's device views are not this library's (built from other headers?)");
    if (c->is_peer) return fail(c, HIPRZ_ERR_STATE, "device_view on a part of a multi-device context");
    if (!c->have_scene) return fail(c, HIPRZ_ERR_STATE, "device_view before a scene upload");
    if (dcamera && !c->have_camera) return fail(c, HIPRZ_ERR_STATE, "device_view: no camera has been uploaded");
    (void)hipSetDevice(c->device);
    std::memcpy(dscene, &c->dscene, sizeof(DScene));
    if (dcamera) std::memcpy(dcamera, &c->dcamera, sizeof(DCamera));
    return HIPRZ_OK;
}

uint32_t hiprz_kernel_count(void) { return uint32_t(kernel_table().size()); }

int hiprz_selftest(hiprz_ctx* c, uint32_t cases_per_thread, uint32_t seed, uint64_t* mismatches, uint64_t* tested) {
    if (!c || !mismatches || !tested) return HIPRZ_ERR_INVALID;
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipMemsetAsync(c->counters_dev.ptr, 0, 8 * sizeof(unsigned long long), c->stream));
    RZ_LAUNCH(rz_selftest_div_kernel, dim3(1024), dim3(256), 0, c->stream, cases_per_thread, seed, c->counters_dev.ptr);
    unsigned long long v[4];
    RZ_HIP(c, hipMemcpyAsync(v, c->counters_dev.ptr, sizeof v, hipMemcpyDeviceToHost, c->stream));
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    *mismatches = v[0], *tested = v[1];
    // how often the filtered box test has to fall back to the exact sequence on these (adversarial: half of them put a face on a range end) cases
    c->timings.set("selftest: box tests the filter left undecided, per million", double(v[2]) * 1.0e6 / double(262144ull * cases_per_thread));
    // a count, not a time: 0 = a material of roughness 2^-100 samples the direction a mirror does, through the general sequence
    c->timings.set("selftest: lobe cases where roughness 2^-100 leaves (+0, 1)", double(v[3]));
    return HIPRZ_OK;
}

int hiprz_timings(hiprz_ctx* c, char* buf, size_t len) {
    if (!c || !buf || len == 0) return HIPRZ_ERR_INVALID;
    const std::string s = c->timings.str();
    std::snprintf(buf, len, "%s", s.c_str());
    return HIPRZ_OK;
}

int hiprz_time_kernels(hiprz_ctx* c, int enabled) {
    if (!c) return HIPRZ_ERR_INVALID;
    c->time_kernels = enabled != 0;  // timed batches are launched eagerly; a captured graph stays valid for the untimed ones
    return HIPRZ_OK;
}

int hiprz_kernel_breakdown_ms(hiprz_ctx* c, double* trace_ms, double* shade_ms, uint32_t* passes) {
    if (!c || !trace_ms || !shade_ms || !passes) return HIPRZ_ERR_INVALID;
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    *trace_ms = *shade_ms = 0.0;
    *passes = 0;
    if (c->pipeline == 2) {  // one launch for all the passes of the batch: reported as "trace"
        if (c->kernel_event_passes) {
            float a = 0;
            RZ_HIP(c, hipEventElapsedTime(&a, c->kernel_events[0], c->kernel_events[1]));
            *trace_ms = a;
            *passes = c->kernel_event_passes;
        }
        return HIPRZ_OK;
    }
    if (c->pipeline != 1) return HIPRZ_OK;
    for (uint32_t i = 0; i < c->kernel_event_passes; ++i) {
        float a = 0, b = 0;
        RZ_HIP(c, hipEventElapsedTime(&a, c->kernel_events[3 * i], c->kernel_events[3 * i + 1]));
        RZ_HIP(c, hipEventElapsedTime(&b, c->kernel_events[3 * i + 1], c->kernel_events[3 * i + 2]));
        *trace_ms += a, *shade_ms += b;
    }
    *passes = c->kernel_event_passes;
    return HIPRZ_OK;
}

int hiprz_kernel_time_ms(hiprz_ctx* c, double* total_ms, uint64_t* launches) {
    if (!c || !total_ms || !launches) return HIPRZ_ERR_INVALID;
    (void)hipSetDevice(c->device);
    RZ_HIP(c, hipStreamSynchronize(c->stream));
    double total = 0;
    uint64_t n = 0;
    for (size_t i = 0; i < c->pending_events.size(); ++i) {
        float ms = 0;
        RZ_HIP(c, hipEventElapsedTime(&ms, c->pending_events[i].first, c->pending_events[i].second));
        total += ms;
        n += c->pending_launches[i];
        c->event_pool.push_back(c->pending_events[i].first);
        c->event_pool.push_back(c->pending_events[i].second);
    }
    c->pending_events.clear();
    c->pending_launches.clear();
    *total_ms = total, *launches = n;
    if (n) c->timings.set("pass kernel (device)", total / double(n));
    return HIPRZ_OK;
}

}  // extern "C"
