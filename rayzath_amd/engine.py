"""Python host side of the HIPGPU backend, above the C-ABI.

`Engine` mirrors the reference's backend interface — `renderWorld(World&, const
RenderConfig&, bool block, bool sync)` and `timingsString()` (RayZath/cpu_engine.hpp:17-22,
RayZath/cuda_engine.cuh:34-39) — and `RenderConfig/LightSampling/Tracing` mirror
RayZath/engine_parts.hpp:76-128.  `Context` is a thin handle around `hiprz_ctx`.
All compute happens in libhiprz.so; there is no CPU path here.
"""
import ctypes as C

import numpy as np

from . import _abi, _lib
from ._lib import HiprzError
from .scene import HostBackend, camera_struct, flatten, flatten_motion


class LightSampling:
    def __init__(self, spot_light=1, direct_light=1):
        self.spot_light, self.direct_light = int(spot_light), int(direct_light)


class Tracing:
    def __init__(self, max_depth=16, rpp=8):
        self.max_depth, self.rpp = int(max_depth), int(rpp)


class RenderConfig:
    def __init__(self, light_sampling=None, tracing=None, seed=20240501):
        self.light_sampling = light_sampling or LightSampling()
        self.tracing = tracing or Tracing()
        self.seed = int(seed)

    def struct(self):
        return _abi.Config(self.tracing.max_depth, self.tracing.rpp, self.light_sampling.spot_light,
                           self.light_sampling.direct_light, self.seed & 0xFFFFFFFF)


COMPAT_BEER_LAMBERT, COMPAT_SCATTERING, COMPAT_SHADOW_COLOR, COMPAT_TEXTURE_MULT, COMPAT_FILTERING, COMPAT_REPROJECTION = 1, 2, 4, 8, 16, 32  # hiprz_set_mode


TREE_REFERENCE, TREE_SAH, TREE_DEVICE, TREE_DEVICE_SAH, TREE_AUTO = range(5)   # hiprz_set_tree (include/hiprz.h)
SHARD_TILES, SHARD_SAMPLES = 0, 1   # hiprz_set_shard_mode


def denoise_params(iterations=None, sigma_normal=None, sigma_depth=None, sigma_color=None, demodulate=None, variance=None):
    """hiprz_denoise_params: the library's defaults (hiprz_denoise_default_params) with the given fields replaced.  `variance`: the
    variance-guided filter (DENOISE_VARIANCE), whose sigma_color is a luminance tolerance in standard deviations."""
    p = _abi.DenoiseParams()
    _lib.load().hiprz_denoise_default_params(C.byref(p))
    if iterations is not None:
        p.iterations = int(iterations)
    for name, value in (("sigma_normal", sigma_normal), ("sigma_depth", sigma_depth), ("sigma_color", sigma_color)):
        if value is not None:
            setattr(p, name, float(value))
    if demodulate is not None:
        p.flags = (p.flags & ~_abi.DENOISE_DEMODULATE) | (_abi.DENOISE_DEMODULATE if demodulate else 0)
    if variance is not None:
        p.flags = (p.flags & ~_abi.DENOISE_VARIANCE) | (_abi.DENOISE_VARIANCE if variance else 0)
    return p


def _wants_variance(params):
    return params is not None and bool(params.flags & _abi.DENOISE_VARIANCE)


def default_streams(n_lights):
    """How many contexts-with-a-stream the hosts put on ONE GPU (hiprz_create_multi with the device named that often, tiles interleaved):
    two when the scene has no lights — one half's sorts, pass bookkeeping and kernel tails run beside the other half's walks (measured on
    MI355X: config B +6 %, C +12 %, D +5 %) — one when it has (the deferred shadow kernel and the two sorts of a pass already overlap on
    streams of their own, and halving their grids costs more than it hides: config E -10 %)."""
    return 1 if n_lights else 2


class Context:
    """Owns one hiprz_ctx: one GPU and one stream — or, given a list of device ids, one context over several GPUs
    (hiprz_create_multi: tiles interleaved over the devices, readbacks gather the peers' tiles over peer-to-peer copies)."""

    def __init__(self, device=0):
        self.lib = _lib.load()
        self._ctx = C.c_void_p()
        if isinstance(device, (list, tuple)):
            ids = (C.c_int * len(device))(*[int(d) for d in device])
            rc = self.lib.hiprz_create_multi(C.byref(self._ctx), ids, len(device))
        else:
            rc = self.lib.hiprz_create(C.byref(self._ctx), int(device))
        if rc != _abi.OK:
            raise HiprzError(rc, (self.lib.hiprz_last_error(None) or b"").decode())
        self.width = self.height = 0
        self._sizes = {}
        self._presented = {}  # camera -> sequence of its newest present
        self._head_device = int(device[0]) if isinstance(device, (list, tuple)) else int(device)
        self._meter = None    # noise(): a hiprz_noise_meter on the head device, created at the first measurement
        self._exposure = {}   # camera -> (aperture, exposure_time) as uploaded: the k of the tone curve noise() measures through

    def device_count(self):
        v = C.c_uint32()
        self._check(self.lib.hiprz_device_count(self._ctx, C.byref(v)))
        return v.value

    # --- cameras: one frame state each, the calls below address the selected one ---
    def set_camera_count(self, n):
        self._check(self.lib.hiprz_set_camera_count(self._ctx, n))
        self._presented = {k: v for k, v in self._presented.items() if k < n}

    def camera_count(self):
        v = C.c_uint32()
        self._check(self.lib.hiprz_camera_count(self._ctx, C.byref(v)))
        return v.value

    def select_camera(self, index):
        self._check(self.lib.hiprz_select_camera(self._ctx, index))
        self._sizes[getattr(self, "_camera", 0)] = (self.width, self.height)
        self._camera = index
        self.width, self.height = self._sizes.get(index, (0, 0))

    def update_shading(self, flat_scene):
        """Materials and lights of `flat_scene` replace those of the uploaded scene in place (same material count); no tree work.
        Map indices are positions in the UPLOADED scene's texture list: when `flat_scene` numbers other map objects, or the same ones in
        another order (a material re-pointed at another uploaded map changes the first-use order), the whole scene is uploaded instead."""
        f = flat_scene
        if getattr(f, "map_ids", None) != getattr(self, "_uploaded_map_ids", None) or f.map_ids is None:
            return self.upload_scene(f)
        self._check(self.lib.hiprz_update_shading(self._ctx, f.materials.ctypes.data, len(f.materials), f.spot_lights.ctypes.data, len(f.spot_lights),
                                                  f.direct_lights.ctypes.data, len(f.direct_lights)))

    def close(self):
        if getattr(self, "_meter", None) is not None:
            self._meter.close()
            self._meter = None
        if getattr(self, "_query", None) is not None:
            self._query.close()
            self._query = None
        if getattr(self, "_order", None) is not None:
            self._order.close()
            self._order = None
        if getattr(self, "_bake", None) is not None:
            self._bake.close()
            self._bake = None
        if getattr(self, "_atlas", None) is not None:
            self._atlas.close()
            self._atlas = None
        if getattr(self, "_light", None) is not None:
            self._light.close()
            self._light = None
        if getattr(self, "_gather", None) is not None:
            self._gather.close()
            self._gather = None
        if getattr(self, "_probe", None) is not None:
            self._probe.close()
            self._probe = None
        if getattr(self, "_smooth", None) is not None:
            self._smooth.close()
            self._smooth = None
        if getattr(self, "_field", None) is not None:
            self._field.close()
            self._field = None
        if getattr(self, "_place", None) is not None:
            self._place.close()
            self._place = None
        if getattr(self, "_view", None) is not None:
            self._view.close()
            self._view = None
        if self._ctx:
            self.lib.hiprz_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != _abi.OK:
            raise HiprzError(rc, (self.lib.hiprz_last_error(self._ctx) or b"").decode())

    # --- uploads ---
    def upload_scene(self, flat_scene):
        self._check(self.lib.hiprz_upload_scene(self._ctx, C.byref(flat_scene.struct)))
        self._uploaded_map_ids = getattr(flat_scene, "map_ids", None)
        self._n_instances = int(flat_scene.struct.n_instances)      # (update_instances takes all of them: the number stays)

    def upload_camera(self, camera_struct_):
        self._check(self.lib.hiprz_upload_camera(self._ctx, C.byref(camera_struct_)))
        if (self.width, self.height) != (camera_struct_.width, camera_struct_.height):
            self._presented[getattr(self, "_camera", 0)] = 0  # a resize restarts the camera's sequence
        self.width, self.height = camera_struct_.width, camera_struct_.height
        self._exposure[getattr(self, "_camera", 0)] = (float(camera_struct_.aperture), float(camera_struct_.exposure_time))

    def set_config(self, config_struct):
        self._check(self.lib.hiprz_set_config(self._ctx, C.byref(config_struct)))

    def set_shard(self, rank, world):
        self._check(self.lib.hiprz_set_shard(self._ctx, rank, world))
        self._shard_world = int(world)

    def set_shard_mode(self, mode):
        """How the parts of a context over several devices / streams divide its share (hiprz_set_shard_mode): SHARD_TILES (default) —
        interleaved tiles, the one-device frame bit for bit; SHARD_SAMPLES — every part renders the whole share on the seed stream
        seed + part and the accumulators are summed wherever the frame leaves the context."""
        self._check(self.lib.hiprz_set_shard_mode(self._ctx, mode))

    def shard_mode(self):
        v = C.c_uint32()
        self._check(self.lib.hiprz_shard_mode(self._ctx, C.byref(v)))
        return v.value

    def set_traversal_mode(self, mode):
        self._check(self.lib.hiprz_set_traversal_mode(self._ctx, mode))

    def set_walk_order(self, order):
        """0 = mesh children in the reference's order (counters equal the CPU kernel's), 1 = front to back (default)."""
        self._check(self.lib.hiprz_set_walk_order(self._ctx, order))

    def set_mode(self, compat_flags):
        """0 = the CPU kernel (default, parity-checked); COMPAT_* flags add behaviours of the reference's CUDA engine (include/hiprz.h)."""
        self._check(self.lib.hiprz_set_mode(self._ctx, compat_flags))

    def set_temporal_blend(self, blend):
        """Camera::temporalBlend of the selected camera: the weight of the previous frame's history at a restart (COMPAT_REPROJECTION)."""
        self._check(self.lib.hiprz_set_temporal_blend(self._ctx, blend))

    def tree(self):
        """The trees of the uploaded scene (hiprz_tree): TREE_REFERENCE .. TREE_DEVICE_SAH."""
        out = C.c_uint32(0)
        self._check(self.lib.hiprz_tree(self._ctx, C.byref(out)))
        return out.value

    def set_tree(self, tree):
        """0 = the uploaded (reference) mesh trees, 1 = rebuilt with a binned SAH at the next upload_scene (same frames, fewer tests),
        2 = all trees built on the device at upload (same frames; update_triangles / update_instances afterwards), 3 = as 2 with the
        device's binned surface-area builder for the mesh trees, 4 (TREE_AUTO) = 0 for scenes staged in LDS, 3 for all others."""
        self._check(self.lib.hiprz_set_tree(self._ctx, tree))

    def update_triangles(self, first, tris, attrs):
        """New records (numpy arrays of _abi.tri_dtype / tri_attr_dtype) for triangles [first, first + len) of the uploaded order; the device
        refits the mesh trees that hold them.  Scenes uploaded under set_tree(2) only."""
        tris, attrs = np.ascontiguousarray(tris), np.ascontiguousarray(attrs)
        assert len(tris) == len(attrs)
        self._check(self.lib.hiprz_update_triangles(self._ctx, first, len(tris), tris.ctypes.data, attrs.ctypes.data))

    def rebuild_trees(self, tree=TREE_DEVICE_SAH):
        """Every mesh tree built again by the device over the vertices it holds now (after update_triangles deformed a mesh far from the
        shape its tree was built for); TREE_DEVICE or TREE_DEVICE_SAH.  Scenes with device-built trees only."""
        self._check(self.lib.hiprz_rebuild_trees(self._ctx, tree))

    def update_instances(self, instances):
        """New transformations and world boxes of ALL instances (array of _abi.instance_dtype); the device rebuilds the world tree."""
        instances = np.ascontiguousarray(instances)
        self._check(self.lib.hiprz_update_instances(self._ctx, instances.ctypes.data, len(instances)))

    def download_trees(self, n_instances, n_tris, n_tlas_order):
        """(nodes, tlas_root, tlas_order, blas_roots, tri_refpos) of the trees the context walks now."""
        n = C.c_uint32()
        self._check(self.lib.hiprz_download_trees(self._ctx, None, 0, C.byref(n), None, None, None, None))
        nodes = np.zeros(n.value, dtype=_abi.node_dtype)
        root = C.c_uint32()
        order, roots, refpos = np.zeros(max(n_tlas_order, 1), np.uint32), np.zeros(max(n_instances, 1), np.uint32), np.zeros(max(n_tris, 1), np.uint32)
        self._check(self.lib.hiprz_download_trees(self._ctx, nodes.ctypes.data, len(nodes), C.byref(n), C.byref(root), order.ctypes.data, roots.ctypes.data, refpos.ctypes.data))
        return nodes, root.value, order[:n_tlas_order], roots[:n_instances], refpos[:n_tris]

    def set_pipeline(self, pipeline):
        self._check(self.lib.hiprz_set_pipeline(self._ctx, pipeline))

    def pipeline(self):
        v = C.c_int()
        self._check(self.lib.hiprz_pipeline(self._ctx, C.byref(v)))
        return v.value

    def launch_plan(self):
        """The launch plan of the most recent render call (hiprz_launch_plan) as its raw uint32 words."""
        words, n = np.zeros(256, dtype=np.uint32), C.c_uint32()
        self._check(self.lib.hiprz_launch_plan(self._ctx, words.ctypes.data_as(C.POINTER(C.c_uint32)), len(words), C.byref(n)))
        return words[:n.value].copy()

    def graph_captures(self):
        v = C.c_uint32()
        self._check(self.lib.hiprz_graph_captures(self._ctx, C.byref(v)))
        return v.value

    def traversal_mode(self):
        v = C.c_int()
        self._check(self.lib.hiprz_traversal_mode(self._ctx, C.byref(v)))
        return v.value

    def set_lds_scene(self, mode):
        self._check(self.lib.hiprz_set_lds_scene(self._ctx, mode))

    # --- rendering ---
    def reset(self):
        self._check(self.lib.hiprz_reset(self._ctx))

    def render(self, n_passes):
        self._check(self.lib.hiprz_render(self._ctx, n_passes))

    def render_counted(self, n_passes):
        out = _abi.Counters()
        self._check(self.lib.hiprz_render_counted(self._ctx, n_passes, C.byref(out)))
        return out.as_dict()

    def tonemap(self):
        self._check(self.lib.hiprz_tonemap(self._ctx))

    def sync(self):
        self._check(self.lib.hiprz_sync(self._ctx))

    # --- readback ---
    def read_rgba8(self):
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._check(self.lib.hiprz_read_rgba8(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def read_depth(self):
        out = np.zeros((self.height, self.width), dtype=np.float32)
        self._check(self.lib.hiprz_read_depth(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def read_accum(self):
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._check(self.lib.hiprz_read_accum(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def read_state(self):
        n = self.width * self.height
        ray = np.zeros((self.height, self.width, 9), dtype=np.float32)
        md = np.zeros((self.height, self.width, 2), dtype=np.uint32)
        self._check(self.lib.hiprz_read_state(self._ctx, ray.ctypes.data, md.ctypes.data, n))
        return dict(origin=ray[..., 0:3], direction=ray[..., 3:6], color=ray[..., 6:9], material=md[..., 0], depth=md[..., 1])

    def ray_count(self):
        v = C.c_uint64()
        self._check(self.lib.hiprz_ray_count(self._ctx, C.byref(v)))
        return v.value

    def pass_count(self):
        v = C.c_uint32()
        self._check(self.lib.hiprz_pass_count(self._ctx, C.byref(v)))
        return v.value

    def pick(self, x, y):
        i, m = C.c_int32(), C.c_int32()
        self._check(self.lib.hiprz_pick(self._ctx, x, y, C.byref(i), C.byref(m)))
        return i.value, m.value

    def ray_cast(self, x, y):
        """Kernel::rayCast through pixel (x, y) of the selected camera's current frame: (instance, material slot, material, triangle's
        index in its mesh), -1 where nothing was met / the slot is unset."""
        r = _abi.RayCast()
        self._check(self.lib.hiprz_ray_cast(self._ctx, x, y, C.byref(r)))
        return r.instance, r.material_slot, r.material, r.triangle

    # --- pipelined frame delivery ---
    def present(self, x=0, y=0):
        """hiprz_present: enqueue the selected camera's frame (tone map, rgba8 + depth + the ray cast through pixel (x, y)) for the copy to
        pinned host memory; never waits for the GPU.  Returns the frame's sequence number."""
        self._check(self.lib.hiprz_present(self._ctx, int(x), int(y)))
        cam = getattr(self, "_camera", 0)
        self._presented[cam] = self._presented.get(cam, 0) + 1  # as the context counts: 1, 2, ... per camera, from 1 again after a resize
        return self._presented[cam]

    def read_frame(self, seq=0, copy=False):
        """hiprz_read_frame: waits for that frame's copy.  Returns dict(rgba8 (H, W, 4) u8, depth (H, W) f32, width, height, passes,
        sequence, ray_count, hit=(instance, material slot, material, triangle)).  The arrays are views of the context's pinned memory, valid
        until the second present after this one on the camera (or a resize): copy=True returns arrays of their own."""
        f = _abi.Frame()
        self._check(self.lib.hiprz_read_frame(self._ctx, int(seq), C.byref(f)))
        h, w = f.height, f.width
        rgba8 = np.ctypeslib.as_array(f.rgba8, shape=(h, w, 4))
        depth = np.ctypeslib.as_array(f.depth, shape=(h, w))
        if copy:
            rgba8, depth = rgba8.copy(), depth.copy()
        return dict(rgba8=rgba8, depth=depth, width=w, height=h, passes=f.passes, sequence=f.sequence, ray_count=f.ray_count,
                    hit=(f.hit.instance, f.hit.material_slot, f.hit.material, f.hit.triangle))

    # --- denoising: first-hit guides and the a-trous filter (include/hiprz.h) ---
    @staticmethod
    def _params(params):
        return None if params is None else C.byref(params)

    def render_guides(self):
        self._check(self.lib.hiprz_render_guides(self._ctx))

    def read_guides(self):
        """(H, W) array of _abi.guide_dtype: normal, depth, albedo, instance of every pixel's first hit (rendered when stale)."""
        out = np.zeros((self.height, self.width), dtype=_abi.guide_dtype)
        self._check(self.lib.hiprz_read_guides(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def guides_device(self):
        v = C.c_void_p()
        self._check(self.lib.hiprz_guides_device(self._ctx, C.byref(v)))
        return v.value

    def denoise(self, params=None):
        """hiprz_denoise: guides (when stale), assembly, filter and tone map of the selected camera's frame, enqueued; None = the defaults."""
        self._check(self.lib.hiprz_denoise(self._ctx, self._params(params)))

    def read_denoised(self):
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._check(self.lib.hiprz_read_denoised(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def read_denoised_rgba8(self):
        out = np.zeros((self.height, self.width, 4), dtype=np.uint8)
        self._check(self.lib.hiprz_read_denoised_rgba8(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def denoise_image(self, accum_ptr, guides_ptr, params, dst_ptr, stream=None):
        """The filter on device images: W*H float4 accumulator, W*H guides (None = the context's), W*H float4 destination."""
        self._check(self.lib.hiprz_denoise_image(self._ctx, accum_ptr, guides_ptr, self._params(params), dst_ptr, stream))

    def set_denoise(self, params):
        """While set (params not None), present() delivers the denoised image in the frame's rgba8; None clears it."""
        self._check(self.lib.hiprz_set_denoise(self._ctx, self._params(params)))

    def denoise_image_variance(self, accum_ptr, guides_ptr, variance_ptr, params, dst_ptr, stream=None):
        """The variance-guided filter on device images: as denoise_image, plus a W*H float4 variance image (read_variance's layout)."""
        self._check(self.lib.hiprz_denoise_image_variance(self._ctx, accum_ptr, guides_ptr, variance_ptr, self._params(params), dst_ptr, stream))

    # --- variance: batch moments of the accumulator, one batch per render call (include/hiprz.h "VARIANCE") ---
    def set_variance(self, enabled):
        """hiprz_set_variance: a real change restarts accumulation."""
        self._check(self.lib.hiprz_set_variance(self._ctx, int(bool(enabled))))

    def read_variance(self):
        """(H, W, 4) float32: the variance of the mean radiance per channel and the number of closed batches K (0 variance where K < 2)."""
        out = np.zeros((self.height, self.width, 4), dtype=np.float32)
        self._check(self.lib.hiprz_read_variance(self._ctx, out.ctypes.data, out.nbytes))
        return out

    def variance_device(self):
        v = C.c_void_p()
        self._check(self.lib.hiprz_variance_device(self._ctx, C.byref(v)))
        return v.value

    def accum_device(self):
        """hiprz_accum_device: the accumulator image of read_accum() on the head device, enqueued on stream(); valid until the next call
        that reads back, denoises or presents."""
        v = C.c_void_p()
        self._check(self.lib.hiprz_accum_device(self._ctx, C.byref(v)))
        return v.value

    # --- noise level: a per-tile error map in display units and its summary (include/hiprz_noise.h) ---
    def noise(self, threshold=1.0 / 255.0, min_batches=8):
        """The noise level of the selected camera's frame: (noise.Summary, tiles (tiles_y, tiles_x, 4) float32 of (sum e^2, max e,
        n_estimated, n_above)), e the standard error of a pixel's displayed luminance.  Needs set_variance(1) (HIPRZ_ERR_STATE otherwise):
        a pixel has an estimate once `min_batches` render calls closed a batch for it — 8 is where the estimate's own relative error,
        sqrt(2 / (K - 1)), is about 0.5.  `threshold`: pixels with e above it are counted.  Waits for the stream; changes no frame."""
        from . import noise as _noise
        variance = self.variance_device()  # refuses first: off, or before scene and camera
        accum = self.accum_device()
        if self._meter is None:
            self._meter = _noise.Meter(self._head_device)
        aperture, exposure_time = self._exposure[getattr(self, "_camera", 0)]
        params = _noise.Params(aperture, exposure_time, float(threshold), int(min_batches))
        return self._meter.measure(accum, variance, self.width, self.height, params, self.stream())

    # --- ray queries: closest hit and occlusion for caller-supplied rays (include/hiprz_query.h) ---
    def query(self):
        """the context's query.Query, created at the first use (device-pointer calls: closest_device, occluded_device, pixel_rays_device)"""
        from . import query as _query
        if getattr(self, "_query", None) is None:
            self._query = _query.Query(self._ctx)
        return self._query

    def order(self):
        """the context's order.Order (include/hiprz_order.h), created at the first use: the queries above walked in sorted ray order"""
        from . import order as _order
        if getattr(self, "_order", None) is None:
            self._order = _order.Order(self._ctx)
        return self._order

    def trace(self, rays, normalize=False, ordered=False):
        """The closest hit of every ray of `rays` (an array of query.ray_dtype) in the uploaded world: an array of query.hit_dtype of the
        same shape.  normalize: the device's normalized() is applied to the directions first, t is then along the normalised direction;
        otherwise the directions must be of unit length.  An invalid ray reads HIT_INVALID.  Waits for the stream; changes no frame.
        ordered: the rays are walked in the renderer's sorted order (include/hiprz_order.h) — the same bytes, sooner for a large batch of
        rays in no particular order, later for rays that arrive coherent (a camera's pixels)."""
        return (self.order() if ordered else self.query()).closest(rays, normalize)

    def occluded(self, rays, normalize=False, ordered=False):
        """uint32 per ray: 1 = some triangle lies within (near, far) of the ray.  Waits for the stream; changes no frame.  ordered: as
        for trace."""
        return (self.order() if ordered else self.query()).occluded(rays, normalize)

    def ray_order(self, rays, normalize=False):
        """(perm, keys), uint32 arrays of rays.size: the order an ordered query walks `rays` in — perm[i] is the index (into the flattened
        rays) of the ray walked i-th, the stable order of keys — and every ray's 24-bit sort key, 0 for an invalid ray"""
        return self.order().permutation(rays, normalize, self.sync)

    # --- occlusion baking: the rays of surface points made, walked and counted on the device (include/hiprz_bake.h) ---
    def bake(self):
        """the context's bake.Bake, created at the first use (device-pointer calls: occlusion_device, rays_device)"""
        from . import bake as _bake
        if getattr(self, "_bake", None) is None:
            self._bake = _bake.Bake(self._ctx)
        return self._bake

    def _bake_with(self, directions):
        b = self.bake()
        if directions is not None and not (isinstance(directions, tuple) and directions == b.table):       # a cosine table already set is not set again
            b.set_directions(directions)
        return b

    def bake_occlusion(self, points, directions=(64, 4), seed=0):
        """Ambient occlusion of every surface point of `points` (an array of bake.point_dtype: position, near, normal, far) in the uploaded
        world: an array of bake.texel_dtype of the same shape — `occluded` of the K rays of the point are occluded (bake.INVALID for an
        invalid point), `bent` is the sum of the directions that are not.  directions: a (K, S) pair for the cosine table of S sets of K
        directions, an (S, K, 4) float32 array of unit vectors around +z, or None for the table set before.  Point i uses set
        bake.set_of(i, seed, S).  Waits for the stream; changes no frame."""
        return self._bake_with(directions).occlusion(points, seed)

    def bake_rays(self, points, seed=0, directions=None):
        """The rays bake_occlusion walks for `points` under the table set before (or `directions`): query.ray_dtype of shape
        points.shape + (K,), to feed to trace / occluded (closest-hit distances for distance-weighted occlusion)."""
        return self._bake_with(directions).rays(points, seed, self.sync)

    # --- bake atlases: UV charts rasterised into surface points on the device, gutters dilated (include/hiprz_atlas.h) ---
    def atlas(self):
        """the context's atlas.Atlas, created at the first use (begin, add, add_device, points_device, dilate_device, ...)"""
        from . import atlas as _atlas
        if getattr(self, "_atlas", None) is None:
            self._atlas = _atlas.Atlas(self._ctx)
        return self._atlas

    def atlas_points(self, parts, width, height, near=1.0e-3, far=3.0e38):
        """The surface points of a width x height atlas: `parts` is a list of (instance_index, charts) pairs, charts an array of
        atlas.tri_dtype (atlas.charts(mesh)) in the mesh's own space, placed as the instance is in the context now; triangle ids are
        numbered through the list.  (points, samples) of shape (height, width): bake.point_dtype and atlas.sample_dtype, a texel no chart
        covers reads zeros and atlas.NONE.  Waits for the stream; changes no frame."""
        from . import atlas as _atlas
        a = self.atlas()
        _atlas.build(a, parts, width, height, near, far)
        return a.read()

    def bake_atlas(self, parts, width, height, directions=(64, 4), seed=0, rings=2, near=1.0e-3, far=3.0e38):
        """atlas_points, bake_occlusion of the points where they lie on the device, and `rings` rings of gutter dilation:
        (texels, samples, ring) of shape (height, width) — bake.texel_dtype, atlas.sample_dtype and uint32 (0 covered, r filled in ring r,
        atlas.NONE still empty).  Texel (x, y) is point y * width + x of the bake.  Waits for the stream; changes no frame."""
        from . import atlas as _atlas
        a, b = self.atlas(), self._bake_with(directions)
        _atlas.build(a, parts, width, height, near, far)
        texels, ring = _atlas.bake(a, b, rings, seed)
        return texels, a.read(points=False)[1], ring

    # --- light baking: the shadowed direct light of the scene's own lights per surface point (include/hiprz_light.h) ---
    def light(self):
        """the context's light.Light, created at the first use (device-pointer calls: bake_device, rays_device)"""
        from . import light as _light
        if getattr(self, "_light", None) is None:
            self._light = _light.Light(self._ctx)
        return self._light

    def _light_with(self, samples):
        h = self.light()
        if samples is not None and not (isinstance(samples, tuple) and samples == h.table):       # a disk table already set is not set again
            h.set_samples(samples)
        return h

    def bake_light(self, points, samples=(16, 4), seed=0, lights=None):
        """The direct light of the uploaded scene's spot and direct lights at every surface point of `points` (an array of
        bake.point_dtype), with their shadows: an array of light.texel_dtype of the same shape — `light` is the RGB irradiance-like sum
        include/hiprz_light.h defines (multiply by the surface colour), `shadowed` the number of shadow rays found occluded
        (light.INVALID for an invalid point).  samples: a (K, S) pair for the library's disk table of S sets of K samples (K = 1: hard
        shadows), an (S, K, 2) float32 array of points of the unit disk, or None for the table set before.  lights: None for every light
        or (spot_first, spot_count, direct_first, direct_count), a count of None meaning "to the end" — one call per range gives
        per-light maps.  Waits for the stream; changes no frame."""
        return self._light_with(samples).bake(points, seed, lights)

    def light_rays(self, points, seed=0, samples=None, lights=None):
        """(rays, weights): the shadow rays bake_light walks for `points` under the table set before (or `samples`) and their weights —
        query.ray_dtype and float32 of shape points.shape + (L, K), spot lights first; a skipped sample reads direction 0 and weight 0."""
        return self._light_with(samples).rays(points, seed, lights, self.sync)

    def bake_light_atlas(self, parts, width, height, samples=(16, 4), seed=0, rings=2, near=1.0e-3, far=3.0e38, lights=None, smooth=None):
        """atlas_points, bake_light of the points where they lie on the device, and `rings` rings of gutter dilation: (texels, samples,
        ring) of shape (height, width) — light.texel_dtype, atlas.sample_dtype and uint32 (0 covered, r filled in ring r, atlas.NONE still
        empty).  Texel (x, y) is point y * width + x of the bake.  smooth: None, or smooth.params(...) (or a dict of its keywords) for
        smooth_texels of the baked light on the device before the dilation, so that the gutters take smoothed values.  Waits for the
        stream; changes no frame."""
        from . import atlas as _atlas
        a, h = self.atlas(), self._light_with(samples)
        _atlas.build(a, parts, width, height, near, far)
        texels, ring = _atlas.bake_light(a, h, rings, seed, lights, *self._smooth_with(smooth))
        return texels, a.read(points=False)[1], ring

    # --- bounce baking: the light an atlas holds, gathered over the hemisphere of a surface point (include/hiprz_gather.h) ---
    def gatherer(self):
        """the context's gather.Gather, created at the first use (device-pointer calls: texels_device, samples_device, compose_device)"""
        from . import gather as _gather
        if getattr(self, "_gather", None) is None:
            self._gather = _gather.Gather(self._ctx)
        return self._gather

    def _gather_with(self, directions, charts):
        g = self.gatherer()
        if directions is not None and not (isinstance(directions, tuple) and directions == g.table):       # a cosine table already set is not set again
            g.set_directions(directions)
        if charts is not None:
            g.set_charts(*charts)
        return g

    def gather(self, points, source, width, height, charts, directions=(64, 4), seed=0, sky=(0.0, 0.0, 0.0)):
        """The light that reaches every surface point of `points` (an array of bake.point_dtype) after one bounce: the mean over the K
        hemisphere rays of the point (the rays of bake_rays for the same table and seed) of what the width x height atlas `source` —
        16-byte records, RGB and a word that is gather.INVALID where a texel has no value — holds under each ray's closest hit, `sky` for
        a ray that hits nothing, 0 for a back face, an instance outside the atlas or a texel without a value.  charts: (base, uv) of
        gather.chart_tables(parts, n_instances), or None for the map set before.  An array of gather.texel_dtype of the same shape:
        `mean`, and `counts` = rays that read a texel | rays that missed << 16 (gather.INVALID for an invalid point).  Waits for the
        stream; changes no frame."""
        return self._gather_with(directions, charts).texels(points, source, width, height, seed, sky)

    def gather_samples(self, points, seed=0, directions=None, charts=None):
        """What gather walks for `points` under the table and the chart map set before (or `directions`, `charts`): gather.sample_dtype of
        shape points.shape + (K,) — the chart id under the closest hit of ray k or one of gather.MISS / UNMAPPED / BACK / INVALID_RAY,
        the hit's barycentric weights of vertices 2 and 3, and its distance."""
        return self._gather_with(directions, charts).samples(points, seed, self.sync)

    def bake_bounce_atlas(self, parts, width, height, albedo, emission=None, bounces=1, directions=(64, 4), samples=(16, 4), seed=0, rings=2, sky=(0.0, 0.0, 0.0),
                          near=1.0e-3, far=3.0e38, lights=None, smooth=None):
        """atlas_points, bake_light of the points and then `bounces` radiosity steps on the device: the source albedo * (direct + indirect)
        + emission per texel, `rings` rings of gutter dilation, and gather at the points.  albedo and emission: a colour (3,), an
        (height, width, 3) array or (height, width) 16-byte records; emission None is 0.  (direct, indirect, ring) of shape (height,
        width), both dilated — light.texel_dtype, gather.texel_dtype and the ring map of bake_light_atlas; albedo * (direct.light +
        indirect.mean) + emission is what a texel sends on.  smooth: None, or smooth.params(...) (or a dict of its keywords): direct is then
        smoothed once right after its bake, and every bounce's indirect right after its gather — before it is composed into the next
        source, the last before its dilation — so that no bounce feeds its noise into the next.  Points, sources and texels never visit
        the host between the steps.  Waits for the stream; changes no frame."""
        return self._bake_bounce(parts, width, height, albedo, emission, bounces, directions, samples, seed, rings, sky, near, far, lights, None, smooth)

    def _bake_bounce(self, parts, width, height, albedo, emission, bounces, directions, samples, seed, rings, sky, near, far, lights, then, smooth=None):
        """the one path of bake_bounce_atlas and bake_probe_field: atlas.bake_bounce on this context's handles, `then` handed through"""
        from . import atlas as _atlas
        from . import gather as _gather
        shape = (height, width)
        albedo = _gather.records(albedo, shape)
        emission = None if emission is None else _gather.records(emission, shape)
        a, h = self.atlas(), self._light_with(samples)
        _atlas.build(a, parts, width, height, near, far)
        g = self._gather_with(directions, _gather.chart_tables(parts, getattr(self, "_n_instances", 0)))
        return _atlas.bake_bounce(a, h, g, albedo, emission, bounces, rings, seed, lights, sky, self.sync, then, *self._smooth_with(smooth))

    # --- lightmap smoothing: an edge-stopping filter over an atlas's records, guided by its surface points (include/hiprz_smooth.h) ---
    def smoother(self):
        """the context's smooth.Smooth, created at the first use (device-pointer call: texels_device)"""
        from . import smooth as _smooth
        if getattr(self, "_smooth", None) is None:
            self._smooth = _smooth.Smooth(self._ctx)
        return self._smooth

    def _smooth_with(self, smooth):
        """(handle, params record) of a bake's `smooth` keyword; (None, None) for None, which loads and runs no smoothing code"""
        if smooth is None:
            return None, None
        from . import smooth as _smooth
        return self.smoother(), _smooth._params(smooth)

    def smooth_texels(self, points, records, params=None):
        """The records of an atlas smoothed along its surfaces: `points` (height, width) of bake.point_dtype (atlas_points), `records`
        (height, width) of a 16-byte dtype — three floats and a word, light.texel_dtype or gather.texel_dtype — and `params` a
        smooth.params(...) record, a dict of its keywords or None for its defaults.  A texel whose word is smooth.INVALID, whose point has
        no normal or whose floats are not finite keeps its 16 bytes and enters no mean; every word comes back unchanged.  An array like
        `records`.  Waits for the stream; changes no frame."""
        from . import smooth as _smooth
        return self.smoother().texels(points, records, _smooth.params() if params is None else params)

    # --- probe baking: the light arriving at points of free space as spherical-harmonic coefficients (include/hiprz_probe.h) ---
    def prober(self):
        """the context's probe.Probe, created at the first use (device-pointer calls: gather_device, light_device, samples_device)"""
        from . import probe as _probe
        if getattr(self, "_probe", None) is None:
            self._probe = _probe.Probe(self._ctx)
        return self._probe

    def _probe_with(self, directions, samples, charts):
        p = self.prober()
        if directions is not None and not (isinstance(directions, tuple) and directions == p.table):       # a sphere table already set is not set again
            p.set_directions(directions)
        if samples is not None and not (isinstance(samples, tuple) and samples == p.disk):
            p.set_samples(samples)
        if charts is not None:
            p.set_charts(*charts)
        return p

    def bake_probes(self, probes, source, width, height, charts, directions=(64, 4), samples=(16, 4), seed=0, sky=(0.0, 0.0, 0.0), lights=None, direct=True):
        """The light arriving at every probe of `probes` (an array of bake.point_dtype: position, near, frame axis, far) from all
        directions: an array of probe.sh_dtype of the same shape — nine spherical-harmonic coefficients per colour, the mean over the K
        rays of the probe of what the width x height atlas `source` holds under each ray's closest hit (the rule of gather) times the
        basis, plus, with `direct`, the scene's spot and direct lights with their shadows (the sampling of bake_light without its cosine).
        probe.irradiance(sh, n) then approximates bake_light(...).light + gather(...).mean of a surface point there with normal n.
        directions: a (K, S) pair for the sphere table, an (S, K, 4) array or None for the table set before; samples: as for bake_light;
        charts: (base, uv) of gather.chart_tables(parts, n_instances), or None for the map set before; lights: as for bake_light.
        sh[0].w is rays that read a texel | rays that missed << 16 (probe.INVALID for an invalid probe), sh[1].w the shadowed rays.  The
        records never visit the host between the two launches.  Waits for the stream; changes no frame."""
        p = self._probe_with(directions, samples if direct else None, charts)
        return p.bake(probes, source, width, height, seed, sky, lights, direct, self.sync)

    def probe_samples(self, probes, seed=0, directions=None, charts=None):
        """What bake_probes walks for `probes` under the table and the chart map set before (or `directions`, `charts`):
        gather.sample_dtype of shape probes.shape + (K,), the records gather_samples writes for the same points, table, seed and map."""
        return self._probe_with(directions, None, charts).samples(probes, seed, self.sync)

    def bake_probe_field(self, parts, width, height, albedo, emission, bounces, probes, directions=(64, 4), samples=(16, 4), seed=0, rings=2, sky=(0.0, 0.0, 0.0),
                         near=1.0e-3, far=3.0e38, lights=None, probe_directions=(64, 4), direct=True, smooth=None, visibility=None, place=None):
        """bake_bounce_atlas and, while the source of its last gather — albedo * (direct + indirect of the bounce before) + emission,
        dilated — is still on the device, bake_probes of `probes` from it: (direct, indirect, ring, sh), the first three what
        bake_bounce_atlas returns in every byte, sh of probe.sh_dtype in the shape of `probes`.  probe_directions: the probes' table, a
        (K, S) pair for the sphere table or an (S, K, 4) array.  smooth: as for bake_bounce_atlas.  visibility: None, or a reach — then
        bake_visibility of the probes (the table set on the fielder before, (256, 4) when none is, the same seed) is run while they are
        on the device and its records (field.vis_dtype, the shape of `probes`) come back as a fifth item.  place: None, or
        place.params(...) / place.params_for(grid, ...) (or a dict of params' keywords) — then place_probes (the table set on the
        placer before, (256, 4) when none is, the same seed) moves the probes where they lie on the device first, sh and the visibility
        records are baked at the moved positions, and the moved probes (the dtype and shape of `probes`) and their records
        (place.record_dtype) come back as two more trailing items.  Waits for the stream; changes no frame."""
        from . import _hiprt
        from . import gather as _gather
        from . import probe as _probe
        probes = _probe.Probe._probes(probes)
        p = self._probe_with(probe_directions, samples if direct else None, _gather.chart_tables(parts, getattr(self, "_n_instances", 0)))
        bufs = []
        if place is not None:
            return self._bake_placed_field(p, place, parts, width, height, albedo, emission, bounces, probes, directions, samples, seed, rings, sky, near, far, lights, direct,
                                           smooth, visibility)
        if visibility is None:
            def then(source_ptr):
                if probes.size == 0:
                    return np.zeros(probes.shape, _probe.sh_dtype)
                bufs.extend([_hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer(probes.size * _probe.sh_dtype.itemsize)])
                p.bake_device(bufs[0].ptr, probes.size, source_ptr, width, height, bufs[1].ptr, seed, sky, lights, direct)
                return lambda: bufs[1].download(probes.shape, _probe.sh_dtype)
        else:
            from . import field as _field
            f = self._field_with(None if self.fielder().K else (256, 4))
            seen = []

            def then(source_ptr):
                if probes.size == 0:
                    seen.append(np.zeros(probes.shape, _field.vis_dtype))
                    return np.zeros(probes.shape, _probe.sh_dtype)
                bufs.extend([_hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer(probes.size * _probe.sh_dtype.itemsize), _hiprt.DeviceBuffer(probes.size * _field.vis_dtype.itemsize)])
                p.bake_device(bufs[0].ptr, probes.size, source_ptr, width, height, bufs[1].ptr, seed, sky, lights, direct)
                f.visibility_device(bufs[0].ptr, probes.size, bufs[2].ptr, seed, visibility)

                def after():
                    seen.append(bufs[2].download(probes.shape, _field.vis_dtype))
                    return bufs[1].download(probes.shape, _probe.sh_dtype)
                return after

        try:
            baked = self._bake_bounce(parts, width, height, albedo, emission, bounces, directions, samples, seed, rings, sky, near, far, lights, then, smooth)
            return baked if visibility is None else baked + (seen[0],)
        finally:
            for b in bufs:
                b.free()

    def _bake_placed_field(self, p, place, parts, width, height, albedo, emission, bounces, probes, directions, samples, seed, rings, sky, near, far, lights, direct, smooth,
                           visibility):
        """bake_probe_field(place=): the probes are moved in their device buffer before the two bakes read it"""
        from . import _hiprt
        from . import field as _field
        from . import place as _place
        from . import probe as _probe
        placer = self._place_with(None if self.placer().K else (256, 4))
        f = None if visibility is None else self._field_with(None if self.fielder().K else (256, 4))
        bufs, extra = [], []

        def then(source_ptr):
            if probes.size == 0:
                extra.extend(([] if f is None else [np.zeros(probes.shape, _field.vis_dtype)]) + [probes.copy(), np.zeros(probes.shape, _place.record_dtype)])
                return np.zeros(probes.shape, _probe.sh_dtype)
            sizes = [_probe.sh_dtype.itemsize, _place.record_dtype.itemsize] + ([] if f is None else [_field.vis_dtype.itemsize])
            bufs.extend([_hiprt.DeviceBuffer.of(probes)] + [_hiprt.DeviceBuffer(probes.size * size) for size in sizes])
            placer.probes_device(bufs[0].ptr, probes.size, bufs[0].ptr, bufs[2].ptr, seed, place)
            p.bake_device(bufs[0].ptr, probes.size, source_ptr, width, height, bufs[1].ptr, seed, sky, lights, direct)
            if f is not None:
                f.visibility_device(bufs[0].ptr, probes.size, bufs[3].ptr, seed, visibility)

            def after():
                if f is not None:
                    extra.append(bufs[3].download(probes.shape, _field.vis_dtype))
                extra.extend([bufs[0].download(probes.shape, probes.dtype), bufs[2].download(probes.shape, _place.record_dtype)])
                return bufs[1].download(probes.shape, _probe.sh_dtype)
            return after

        try:
            return self._bake_bounce(parts, width, height, albedo, emission, bounces, directions, samples, seed, rings, sky, near, far, lights, then, smooth) + tuple(extra)
        finally:
            for b in bufs:
                b.free()

    # --- probe placement: the probes of a grid moved out of geometry and away from the surface they hug (include/hiprz_place.h) ---
    def placer(self):
        """the context's place.Placer, created at the first use (device-pointer call: probes_device)"""
        from . import place as _place
        if getattr(self, "_place", None) is None:
            self._place = _place.Placer(self._ctx)
        return self._place

    def _place_with(self, directions):
        pl = self.placer()
        if directions is not None and not (isinstance(directions, tuple) and directions == pl.table):       # a sphere table already set is not set again
            pl.set_directions(directions)
        return pl

    def place_probes(self, probes, directions=(256, 4), seed=0, params=None):
        """The probes of `probes` (an array of bake.point_dtype, as for bake_probes) moved out of geometry: (moved, records) — `moved` like
        `probes` with new positions, `records` of place.record_dtype in the same shape: the offset, place.state(records) at the final
        position (place.CLEAR, NEAR — a front face nearer than min_front — or INSIDE — more than max_back rays hit back faces), the
        place.STUCK bit when a wanted move was not made, the moves made, the nearest front and back face and the counts of rays that hit
        either; word = place.INVALID for an invalid probe, which is copied unchanged.  A probe INSIDE steps through the nearest back face
        and half of min_front beyond, a probe NEAR steps along its most open ray; the offset never exceeds max_offset on any axis.
        directions: a (K, S) pair for the sphere table, an (S, K, 4) array or None for the table set before; K >= 64.  The rays are
        bake_rays's for the same table and seed from wherever the probe is.  params: place.params(...) or place.params_for(grid, ...), or a
        dict of params' keywords.  Waits for the stream; changes no frame."""
        if params is None:
            raise TypeError("place_probes needs params: place.params(min_front, reach, max_offset) or place.params_for(grid, min_front, reach)")
        return self._place_with(directions).probes(probes, seed, params)

    # --- probe fields: a visibility map per probe and the leak-free lookup of a grid of probes on the device (include/hiprz_field.h) ---
    def fielder(self):
        """the context's field.Fielder, created at the first use (device-pointer calls: visibility_device, lookup_device)"""
        from . import field as _field
        if getattr(self, "_field", None) is None:
            self._field = _field.Fielder(self._ctx)
        return self._field

    def _field_with(self, directions):
        f = self.fielder()
        if directions is not None and not (isinstance(directions, tuple) and directions == f.table):       # a sphere table already set is not set again
            f.set_directions(directions)
        return f

    def bake_visibility(self, probes, directions=(256, 4), seed=0, reach=3.0e38):
        """How far every probe of `probes` (an array of bake.point_dtype, as for bake_probes) sees in each direction: an array of
        field.vis_dtype of the same shape — per texel of an 8 x 8 octahedral map in world axes the mean and the mean square of
        min(distance to the closest hit, reach) over the probe's K rays, each ray weighted by the 32nd power of its cosine to the texel's
        direction; `words` = (front-face hits, back-face hits, misses, K), words[3] = field.INVALID for an invalid probe.  directions: a
        (K, S) pair for the sphere table, an (S, K, 4) array or None for the table set before; K >= 64.  The rays are bake_rays's for the
        same table and seed.  reach: what a ray that hits nothing sees, and the cap of every distance — a few grid steps.  Waits for the
        stream; changes no frame."""
        return self._field_with(directions).visibility(probes, seed, reach)

    def lookup_field(self, grid, probes, sh, points, vis=None, params=None):
        """The irradiance a grid of baked probes gives every point of `points` (an array of bake.point_dtype: position and unit normal;
        near and far are ignored), evaluated on the device: an array of field.result_dtype of the same shape — `rgb` in the units of a
        lightmap texel, `word` the number of probes that took part (field.INVALID, and rgb 0, for an invalid point or when none did).
        grid: field.grid_of(lo, hi, shape); probes and sh: the grid's probes (probe.grid) and their records in its C order; vis: their
        bake_visibility records — each of the eight probes around a point is then weighted by a Chebyshev test of the point's distance
        against what the probe saw in its direction, so that a probe behind a wall does not leak — or None for the plain trilinear
        blend; params: field.params(bias=..., max_back=...), a dict of its keywords or None for its defaults.  Needs no uploaded scene.
        Waits for the stream; changes no frame."""
        return self.fielder().lookup(grid, probes, sh, points, vis, params)

    # --- baked view: a frame of the selected camera shaded from a lit atlas and a probe field (include/hiprz_view.h) ---
    def viewer(self):
        """the context's view.View, created at the first use (device-pointer calls: pixels_device, samples_device)"""
        from . import view as _view
        if getattr(self, "_view", None) is None:
            self._view = _view.View(self._ctx)
        return self._view

    def _view_with(self, charts):
        v = self.viewer()
        if charts is not None:
            v.set_charts(*charts)
        return v

    def view(self, source, width, height, charts, field=None, sky=(0.0, 0.0, 0.0), params=None, rgba8=False):
        """The selected camera's frame of the baked scene: an (H_c, W_c) array of view.pixel_dtype — `rgb`, and `word` = kind << 28 |
        count.  Every pixel casts its pixel-centre ray (pixel_rays) to its closest hit (trace).  A front-face hit on an object of the
        chart map reads the width x height atlas `source` — 16-byte records, what a texel sends on (lit_source) — at the hit: kind
        view.ATLAS, count the taps used; params: view.params(filter="nearest" | "bilinear"), the filter's name or None for nearest, the
        texel gather reads.  A front-face hit on an object outside the atlas reads the probe field `field` = (grid, probes, sh,
        vis_or_None, field_params_or_None), the arguments of lookup_field, at the hit for the hit's normal, times the surface's colour,
        plus colour x emission on an emitter: kind view.FIELD, count the probes.  view.NONE (rgb 0) where neither has a value, view.SKY
        (`sky`) where the ray hits nothing, view.BACK (rgb 0) on a back face.  charts: (base, uv) of gather.chart_tables(parts,
        n_instances), or None for the map set before (a map equal to the one set is not uploaded again).  rgba8: also return the (H_c, W_c, 4) uint8 frame tonemap_image makes of the
        float image under the selected camera's exposure.  Waits for the stream; changes no frame."""
        from . import _hiprt
        from . import view as _view
        v = self._view_with(charts)
        source = np.ascontiguousarray(source)
        if source.dtype.itemsize != 16 or source.size != width * height:
            raise TypeError("source must be width*height records of 16 bytes")
        arrays = None if field is None else _view.field_arrays(field)
        shape, n = (self.height, self.width), max(self.width * self.height, 1)
        self.sync()  # (makes the head device the current one: the buffers below are allocated there)
        bufs = [_hiprt.DeviceBuffer.of(source), _hiprt.DeviceBuffer(n * 16)]
        try:
            image = rgba = None
            if rgba8:
                image, rgba = _hiprt.DeviceBuffer(n * 16), _hiprt.DeviceBuffer(n * 4)
                bufs += [image, rgba]
            on_device = None
            if arrays is not None:
                grid, probes, sh, vis, fp = arrays
                held = [_hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer.of(sh)] + ([] if vis is None else [_hiprt.DeviceBuffer.of(vis)])
                bufs += held
                on_device = (grid, held[0].ptr, held[1].ptr, None if vis is None else held[2].ptr, probes.size, fp)
            v.pixels_device(bufs[0].ptr, width, height, bufs[1].ptr, None if image is None else image.ptr, on_device, sky, params)
            if rgba8:
                self.tonemap_image(image.ptr, rgba.ptr)
            self.sync()
            pixels = bufs[1].download(shape, _view.pixel_dtype)
            return (pixels, rgba.download(shape + (4,), np.uint8)) if rgba8 else pixels
        finally:
            for b in bufs:
                b.free()

    def view_samples(self, charts=None):
        """What view walks for the selected camera's pixels under the chart map set before (or `charts`): gather.sample_dtype of shape
        (H_c, W_c) — the chart id under the pixel's closest hit or one of gather.MISS / UNMAPPED / BACK / INVALID_RAY, the hit's
        barycentric weights of vertices 2 and 3, and its distance."""
        return self._view_with(charts).samples((self.height, self.width), self.sync)

    def lit_source(self, direct, indirect, albedo, emission=None, rings=2):
        """The source of view from what bake_bounce_atlas returns: albedo * (direct + indirect) + emission per texel (the gather's
        compose) and `rings` rings of gutter dilation on the atlas built last.  direct and indirect: (H, W) 16-byte records (indirect may
        be None); albedo and emission as for bake_bounce_atlas.  (H, W) records of gather.record_dtype."""
        from . import gather as _gather
        direct = np.ascontiguousarray(direct)
        albedo = _gather.records(albedo, direct.shape)
        emission = None if emission is None else _gather.records(emission, direct.shape)
        composed = self.gatherer().compose(direct, indirect, albedo, emission, self.sync)
        return self.atlas().dilate(composed, rings)[0].view(_gather.record_dtype)

    def pixel_rays(self):
        """(H, W) array of query.ray_dtype: the selected camera's pixel-centre rays, the ones the first pass, the guides and ray_cast walk"""
        from . import _hiprt
        from . import query as _query
        q = self.query()
        self.sync()  # (makes the head device the current one: the buffer below is allocated there)
        buf = _hiprt.DeviceBuffer(self.width * self.height * _query.ray_dtype.itemsize)
        try:
            q.pixel_rays_device(buf.ptr)
            self.sync()
            return buf.download((self.height, self.width), _query.ray_dtype)
        finally:
            buf.free()

    def selftest(self, cases_per_thread=64, seed=1):
        bad, n = C.c_uint64(), C.c_uint64()
        self._check(self.lib.hiprz_selftest(self._ctx, cases_per_thread, seed, C.byref(bad), C.byref(n)))
        return bad.value, n.value

    def selftest_sort(self, keys, key_bits=24, repeats=1):
        """The ray-order radix sort on `keys` (uint32 array): (violations of "stable permutation in key order", device microseconds)."""
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        bad, us = C.c_uint64(), C.c_double()
        self._check(self.lib.hiprz_selftest_sort(self._ctx, keys.ctypes.data_as(C.POINTER(C.c_uint32)), keys.size, int(key_bits), int(repeats),
                                                 C.byref(bad), C.byref(us)))
        return bad.value, us.value

    def selftest_math(self, op, inputs):
        """hiprz_selftest_math: one call of the device's shading arithmetic per row of `inputs`.  `op`: a name of _abi.MATH_OPS or its
        HIPRZ_MATH_* value; `inputs`: float32, (n, width) or (n,) for an op of one argument (uint32 fields as float bit patterns; the row
        layouts are in include/hiprz.h).  Returns the (n, width_out) float32 results."""
        from . import _abi
        op = _abi.MATH_OPS.index(op) if isinstance(op, str) else int(op)
        w_in, w_out = C.c_uint32(), C.c_uint32()
        self._check(self.lib.hiprz_selftest_math_widths(op, C.byref(w_in), C.byref(w_out)))
        inputs = np.ascontiguousarray(inputs, dtype=np.float32)
        if inputs.ndim == 1:
            inputs = inputs.reshape(-1, 1)
        if inputs.ndim != 2 or inputs.shape[1] != w_in.value:
            raise ValueError(f"op {op} takes rows of {w_in.value} floats, got an array of shape {inputs.shape}")
        out = np.zeros((inputs.shape[0], w_out.value), dtype=np.float32)
        self._check(self.lib.hiprz_selftest_math(self._ctx, op, inputs.ctypes.data, w_in.value, inputs.shape[0], out.ctypes.data, w_out.value))
        return out

    def timings(self):
        buf = C.create_string_buffer(4096)
        self._check(self.lib.hiprz_timings(self._ctx, buf, len(buf)))
        return buf.value.decode()

    def time_kernels(self, enabled=True):
        self._check(self.lib.hiprz_time_kernels(self._ctx, int(enabled)))

    def kernel_breakdown_ms(self):
        """(trace kernel ms, shade kernel ms, passes) of the last batch of cumulative passes (split pipeline)."""
        t, s_, n = C.c_double(), C.c_double(), C.c_uint32()
        self._check(self.lib.hiprz_kernel_breakdown_ms(self._ctx, C.byref(t), C.byref(s_), C.byref(n)))
        return t.value, s_.value, n.value

    def kernel_time_ms(self):
        """(total device ms, passes) of the pass kernel since the last call (hip events on the ctx stream)."""
        t, n = C.c_double(), C.c_uint64()
        self._check(self.lib.hiprz_kernel_time_ms(self._ctx, C.byref(t), C.byref(n)))
        return t.value, n.value

    # --- multi-GPU hand-off (device pointers) ---
    def local_pixel_capacity(self):
        v = C.c_size_t()
        self._check(self.lib.hiprz_local_pixel_capacity(self._ctx, C.byref(v)))
        return v.value

    def export_accum_tiles(self, dst_ptr, nbytes):
        self._check(self.lib.hiprz_export_accum_tiles(self._ctx, dst_ptr, nbytes))

    def export_rgba8_tiles(self, dst_ptr, nbytes):
        self._check(self.lib.hiprz_export_rgba8_tiles(self._ctx, dst_ptr, nbytes))

    def untile_gathered(self, src_ptr, world, part_stride_bytes, element_bytes, dst_ptr, stream=None):
        self._check(self.lib.hiprz_untile_gathered(self._ctx, src_ptr, world, part_stride_bytes, element_bytes, dst_ptr, stream))

    def untile_rgba8(self, src_ptr, rank, world, dst_ptr):
        self._check(self.lib.hiprz_untile_rgba8(self._ctx, src_ptr, rank, world, dst_ptr))

    def set_ray_sort(self, mode):
        self._check(self.lib.hiprz_set_ray_sort(self._ctx, mode))

    def set_xcd_swizzle(self, enabled):
        self._check(self.lib.hiprz_set_xcd_swizzle(self._ctx, int(enabled)))

    def set_graph(self, enabled):
        self._check(self.lib.hiprz_set_graph(self._ctx, int(enabled)))

    def untile_accum(self, src_ptr, rank, world, dst_ptr):
        self._check(self.lib.hiprz_untile_accum(self._ctx, src_ptr, rank, world, dst_ptr))

    def tonemap_image(self, src_ptr, dst_ptr, stream=None):
        self._check(self.lib.hiprz_tonemap_image_on(self._ctx, src_ptr, dst_ptr, stream))

    def stream(self):
        return self.lib.hiprz_stream(self._ctx)


class Engine:
    """HIPGPU peer of CPU::Engine / Cuda::Engine.  Writes its results into the world's camera
    like the reference backends do (imageBuffer / depthBuffer / rayCount, camera.hpp:50-56,113-119)."""

    REBUILD_EVERY = 16   # moved frames (World.mark_moved) between two device rebuilds of the refitted trees

    def __init__(self, device=0, streams=None, pipelined=False, denoise=None):
        """`device`: a GPU id, or a list of ids (one context over several GPUs).  `streams` (single GPU only): how many contexts share
        the GPU, None = default_streams() of the first world rendered; asking for `engine.context` before that settles for one.
        `pipelined`: frames leave through Context.present / read_frame, and renderWorld(sync=False) hands out the PREVIOUS call's frame
        while this call's renders (the C++ engine's sync=false); the default reads every frame synchronously and ignores `sync`.
        `denoise`: None, or _abi.DenoiseParams (denoise_params()): the cameras' image buffers receive the denoised frame, on both paths
        (with variance=True the context's variance estimate is switched on: every renderWorld call is one batch)."""
        self._device, self._streams, self._context = device, streams, None
        self._denoise = denoise
        self._measuring = False  # render_until() was called: the variance estimate stays on for its measurements
        self._pipelined = pipelined
        self._pending = []  # pipelined, sync=False: (camera slot, camera, sequence) presented by the previous call, not yet handed out
        self._tree = TREE_AUTO   # the hosts' default: the snapshot's trees for scenes staged in LDS, the device's surface-area trees otherwise
        self.backend = HostBackend(_lib.load())
        self._world_key = None
        self._camera_key, self._camera_ids = {}, None

    @property
    def context(self):
        if self._context is None:
            self._context = Context(self._device)
            self._context.set_tree(self._tree)
            self._apply_denoise()
        return self._context

    def set_denoise(self, params):
        """None, or the parameters of the filter whose output the cameras' image buffers receive from the next frame on."""
        self._denoise = params
        if self._context is not None:
            self._apply_denoise()

    def _apply_denoise(self):
        """the context's filter parameters, and its variance estimate on exactly while they ask for the variance-guided filter or
        render_until() measures the noise level with it"""
        self._context.set_variance(_wants_variance(self._denoise) or self._measuring)
        self._context.set_denoise(self._denoise)

    def set_tree(self, tree):
        """Context.set_tree for the engine's context (default TREE_AUTO); takes effect at the next scene upload, which this forces."""
        self._tree, self._world_key = tree, None
        if self._context is not None:
            self._context.set_tree(tree)

    def set_mode(self, compat_flags):
        """Context.set_mode for the engine's context (COMPAT_REPROJECTION works over several streams / devices too: the context assembles
        the whole previous frame at a restart)."""
        self._mode = compat_flags
        if self._context is not None:
            self._context.set_mode(compat_flags)

    def renderWorld(self, world, render_config, block=True, sync=True):
        if self._context is None and not isinstance(self._device, (list, tuple)):
            k = self._streams or default_streams(len(world.spot_lights) + len(world.direct_lights))
            self._context = Context([self._device] * k) if k > 1 else Context(self._device)
            self._context.set_tree(self._tree)
            self._apply_denoise()
            if getattr(self, "_mode", 0):
                self._context.set_mode(self._mode)
        ctx = self.context
        # the backend re-mirrors what changed and restarts accumulation then (cpu_engine_renderer.cpp:108-112)
        world_key = getattr(world, "_version", None), id(world)
        if getattr(world, "_moved", False):  # World.mark_moved(): an animation frame
            world._moved = False
            moved = None
            if self._world_key == world_key and not getattr(world, "_dirty", True) and ctx.tree() in (TREE_DEVICE, TREE_DEVICE_SAH) \
                    and len(world.instances) == len(self._flat.instances):
                moved = flatten_motion(world, self._flat.tris["source_index"], self.backend)
            if moved is None:
                world._dirty = True       # no device trees (or another topology): an ordinary modification
            else:                         # the device refits its trees and rebuilds the world tree; nothing is built on the host
                tris, attrs, instances = moved
                if len(tris):
                    ctx.update_triangles(0, tris, attrs)
                if len(instances):
                    ctx.update_instances(instances)
                # a refitted tree keeps the topology it was built with: every REBUILD_EVERY-th moved frame the device builds the trees
                # again over the vertices it holds
                self._moved_frames = getattr(self, "_moved_frames", 0) + 1
                if self._moved_frames % self.REBUILD_EVERY == 0:
                    ctx.rebuild_trees(ctx.tree())
        if self._world_key != world_key or getattr(world, "_dirty", True):
            self._flat = flatten(world, self.backend)
            self._moved_frames = 0
            ctx.upload_scene(self._flat)
            self._world_key = world_key
            world._dirty = False
        ctx.set_config(render_config.struct())
        cameras = [c for c in [world.camera] + list(getattr(world, "cameras", [])) if getattr(c, "enabled", True)]
        pending, self._pending = self._pending, []
        if [id(c) for c in cameras] != self._camera_ids:  # one frame state per enabled camera, in the reference's order
            for k, cam, seq in pending:  # the previous call's frames go out before their camera slots are rearranged
                if any(cam is c for c in cameras):
                    ctx.select_camera(k)
                    self._deliver(ctx, cam, world, ctx.read_frame(seq))
            pending = []
            ctx.set_camera_count(max(len(cameras), 1))
            self._camera_ids, self._camera_key = [id(c) for c in cameras], {}
        for k, cam in enumerate(cameras):
            ctx.select_camera(k)
            cam_key = (cam.width, cam.height, cam.position.tobytes(), cam.rotation.tobytes(), cam.fov, cam.near_far,
                       cam.focal_distance, cam.aperture, cam.exposure_time)
            if self._camera_key.get(k) != cam_key:
                resized = self._camera_key.get(k, (None, None))[:2] != cam_key[:2]
                for item in [q for q in pending if q[0] == k and resized]:  # a resize frees the camera's frame slots: its frame goes out first
                    pending.remove(item)
                    if item[1] is cam:
                        self._deliver(ctx, cam, world, ctx.read_frame(item[2]))
                ctx.upload_camera(camera_struct(cam, self.backend))
                ctx.set_temporal_blend(cam.temporal_blend)
                self._camera_key[k] = cam_key
            ctx.render(max(render_config.tracing.rpp, 1))
            if self._pipelined:
                px, py = getattr(cam, "ray_cast_pixel", (0, 0))
                seq = ctx.present(int(px), int(py))  # enqueue only
                if sync:
                    self._deliver(ctx, cam, world, ctx.read_frame(seq))
                else:
                    self._pending.append((k, cam, seq))
                continue
            if self._denoise is not None:
                ctx.denoise(self._denoise)
                cam.image_buffer = ctx.read_denoised_rgba8()  # synchronises
            else:
                ctx.tonemap()
                cam.image_buffer = ctx.read_rgba8()  # synchronises
            cam.depth_buffer = ctx.read_depth()
            cam.ray_count = ctx.ray_count()
            # Kernel::rayCast after every frame (cpu_engine_renderer.cpp:176): what the camera's ray-cast pixel looks at
            px, py = getattr(cam, "ray_cast_pixel", (0, 0))
            inst, slot, _, _ = ctx.ray_cast(int(px), int(py))
            cam.raycasted_instance = world.instances[inst] if 0 <= inst < len(world.instances) else None
            materials = getattr(cam.raycasted_instance, "materials", None) or []
            cam.raycasted_material = materials[slot] if cam.raycasted_instance is not None and 0 <= slot < len(materials) else None
        if self._pipelined and not sync:  # every camera's render is enqueued: hand out the previous call's frames (the first call has none)
            for k, cam, seq in pending:
                if any(cam is c for c in cameras):
                    ctx.select_camera(k)
                    self._deliver(ctx, cam, world, ctx.read_frame(seq))
            if pending and cameras:
                ctx.select_camera(len(cameras) - 1)

    def render_until(self, world, render_config, target, max_passes, min_batches=8):
        """Render to a noise target: renderWorld calls (each one batch of tracing.rpp passes) until EVERY pixel of the frame has an
        estimate and the worst tile's rms error is at most `target` (display units: 1/255 is one step of RGBA8), or until `max_passes`
        passes were rendered.  From the `min_batches`-th call on the frame is measured after every call (Context.noise).  The rule reads
        tile_rms_max, not rms: noise concentrated in one region is not averaged away by a clean background.  Returns (noise.Summary of the
        last measurement, passes rendered by this call, met).
        The variance estimate is switched on if it was off — a real change, which restarts accumulation — and stays on afterwards.  The
        world's first camera is the one measured.  Refused (HIPRZ_ERR_STATE) on a context that renders one shard of a frame
        (Context.set_shard with world > 1): it does not hold the frame."""
        rpp = max(int(render_config.tracing.rpp), 1)
        if int(max_passes) < 1 or int(min_batches) < 2:
            raise ValueError("render_until: max_passes must be at least 1 and min_batches at least 2")

        def refuse_shards():
            if getattr(self._context, "_shard_world", 1) > 1:
                raise HiprzError(_abi.ERR_STATE, "render_until: this context renders one shard of the frame (set_shard) and does not hold it")

        if self._context is not None:
            refuse_shards()
        if not self._measuring:
            self._measuring = True
            if self._context is not None:
                self._apply_denoise()

        def rule(s):
            return s.estimated == s.pixels and s.tile_rms_max <= target

        summary, passes, calls, met = None, 0, 0, False
        while passes < max_passes and not met:
            self.renderWorld(world, render_config)
            refuse_shards()
            calls, passes, summary = calls + 1, passes + rpp, None
            if calls >= min_batches:
                summary = self._measure(min_batches)
                met = rule(summary)
        if summary is None:  # fewer calls than min_batches: the frame as it stands (it may have been accumulating before this call)
            summary = self._measure(min_batches)
            met = rule(summary)
        return summary, passes, met

    def _measure(self, min_batches):
        ctx = self._context
        if ctx.camera_count() > 1:
            ctx.select_camera(0)
        return ctx.noise(min_batches=min_batches)[0]

    @staticmethod
    def _deliver(ctx, cam, world, frame):
        """a frame of Context.read_frame into the camera, as the synchronous path fills it"""
        cam.image_buffer = frame["rgba8"].copy()
        cam.depth_buffer = frame["depth"].copy()
        cam.ray_count = frame["ray_count"]
        inst, slot, _, _ = frame["hit"]
        cam.raycasted_instance = world.instances[inst] if 0 <= inst < len(world.instances) else None
        materials = getattr(cam.raycasted_instance, "materials", None) or []
        cam.raycasted_material = materials[slot] if cam.raycasted_instance is not None and 0 <= slot < len(materials) else None

    def timingsString(self):
        return self.context.timings()
