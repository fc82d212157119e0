"""ctypes binding of the CPU oracle (oracle/librz_oracle.so) — TEST INFRASTRUCTURE ONLY.

Imported by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg, never by the
rayzath_amd package.
"""
import ctypes as C
import os

import numpy as np

from rayzath_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "oracle", "librz_oracle.so")


class _Ctx(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("image", C.POINTER(C.c_float)),
                ("path_depth", C.POINTER(C.c_uint8)), ("ray_origin", C.POINTER(C.c_float)),
                ("ray_direction", C.POINTER(C.c_float)), ("ray_material", C.POINTER(C.c_uint32)),
                ("ray_color", C.POINTER(C.c_float)), ("depth", C.POINTER(C.c_float)),
                ("rgba8", C.POINTER(C.c_uint8)), ("passes", C.c_uint32), ("traced_rays", C.c_uint64)]


# rzo_first_hit_record: the pixel's hiprz_guide (_abi.guide_dtype, 32 bytes) and what classifies the hit
first_hit_dtype = np.dtype([("normal", "<f4", 3), ("depth", "<f4"), ("albedo", "<f4", 3), ("instance", "<u4"), ("triangle", "<i4"),
                            ("source_index", "<u4"), ("material_slot", "<i4"), ("material", "<i4"), ("external", "<u4"), ("u", "<f4"),
                            ("v", "<f4"), ("emission", "<f4")])
assert first_hit_dtype.itemsize == 64

_lib = None
_variants = {}


def variant(name):
    """oracle/librz_oracle_<name>.so: a libm stand-in (lo, hi, mix, lo2, hi2, mix2) or a mutant (mut_<bug>), see oracle/Makefile."""
    if name not in _variants:
        _variants[name] = load(os.path.join(ROOT, "oracle", f"librz_oracle_{name}.so"))
    return _variants[name]


def load(path=LIB_PATH):
    global _lib
    if _lib is not None and path == LIB_PATH:
        return _lib
    lib = C.CDLL(path)
    P, U32, F = C.c_void_p, C.c_uint32, C.c_float
    lib.rzo_context_create.restype, lib.rzo_context_create.argtypes = C.POINTER(_Ctx), [U32, U32]
    lib.rzo_context_destroy.restype, lib.rzo_context_destroy.argtypes = None, [C.POINTER(_Ctx)]
    lib.rzo_context_reset.restype, lib.rzo_context_reset.argtypes = None, [C.POINTER(_Ctx)]
    lib.rzo_render_pass.restype = None
    lib.rzo_render_pass.argtypes = [C.POINTER(_abi.Scene), C.POINTER(_abi.Camera), C.POINTER(_abi.Config), C.POINTER(_Ctx),
                                    C.c_int, C.POINTER(_abi.Counters)]
    lib.rzo_render_pass_mode.restype = None
    lib.rzo_render_pass_mode.argtypes = lib.rzo_render_pass.argtypes + [U32]
    lib.rzo_compat_fetch.restype, lib.rzo_compat_fetch.argtypes = None, [C.POINTER(_abi.Scene), C.c_int32, F, F, P, P]
    lib.rzo_pick.restype = None
    lib.rzo_pick.argtypes = [C.POINTER(_abi.Scene), C.POINTER(_abi.Camera), C.POINTER(_Ctx), U32, U32,
                             C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.rzo_ray_cast.restype = None
    lib.rzo_ray_cast.argtypes = [C.POINTER(_abi.Scene), C.POINTER(_abi.Camera), C.POINTER(_Ctx), U32, U32, C.POINTER(_abi.RayCast)]
    lib.rzo_first_hit.restype, lib.rzo_first_hit.argtypes = None, [C.POINTER(_abi.Scene), C.POINTER(_abi.Camera), U32, U32, U32, P]
    lib.rzo_first_hit_frame.restype, lib.rzo_first_hit_frame.argtypes = None, [C.POINTER(_abi.Scene), C.POINTER(_abi.Camera), U32, P, C.c_int]
    lib.rzo_seed_value.restype, lib.rzo_seed_value.argtypes = F, [U32, U32, U32]
    lib.rzo_rng_sequence.restype, lib.rzo_rng_sequence.argtypes = None, [F, F, F, U32, P]
    lib.rzo_box_test.restype, lib.rzo_box_test.argtypes = C.c_int, [P, P, P, P, F, F]
    lib.rzo_triangle_test.restype, lib.rzo_triangle_test.argtypes = C.c_int, [P, P, P, P, P, F, F, P]
    lib.rzo_fresnel.restype, lib.rzo_fresnel.argtypes = F, [P, P, F, F, P]
    lib.rzo_cosine_sample_hemisphere.restype, lib.rzo_cosine_sample_hemisphere.argtypes = None, [F, F, P, P]
    lib.rzo_sample_sphere.restype, lib.rzo_sample_sphere.argtypes = None, [F, F, P, P]
    lib.rzo_sample_disk.restype, lib.rzo_sample_disk.argtypes = None, [F, F, P, F, P]
    lib.rzo_sample_hemisphere.restype, lib.rzo_sample_hemisphere.argtypes = None, [F, F, P, P]
    lib.rzo_glossy_lobe.restype, lib.rzo_glossy_lobe.argtypes = None, [F, F, P]
    lib.rzo_tonemap_pixel.restype, lib.rzo_tonemap_pixel.argtypes = None, [P, F, F, P]
    lib.rzo_math_mode.restype, lib.rzo_math_mode.argtypes = C.c_char_p, []
    if path == LIB_PATH:
        _lib = lib
    return lib


class OracleRenderer:
    """CPU::Renderer + CPU::Kernel of the reference, restated (oracle/rz_oracle.c).  mode: HIPRZ_COMPAT_* flags, the CUDA engine's
    behaviours (rzo_render_pass_mode); 0 = the CPU engine."""

    def __init__(self, flat_scene, camera, config, lib=None, mode=0):
        self.lib = lib or load()
        self.scene, self.camera, self.config, self.mode = flat_scene, camera, config, int(mode)
        self.ctx = self.lib.rzo_context_create(camera.width, camera.height)
        self.w, self.h = camera.width, camera.height

    def close(self):
        if self.ctx:
            self.lib.rzo_context_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self.lib.rzo_context_reset(self.ctx)

    def render(self, n_passes=1, threads=0, counted=False):
        total = {n: 0 for n, _ in _abi.Counters._fields_}
        cnt = _abi.Counters()
        for _ in range(n_passes):
            self.lib.rzo_render_pass_mode(C.byref(self.scene.struct), C.byref(self.camera), C.byref(self.config), self.ctx,
                                          threads, C.byref(cnt) if counted else None, self.mode)
            if counted:
                for k, v in cnt.as_dict().items():
                    total[k] += v
        return total

    def adopt(self, accum, state, passes):
        """Continue from another renderer's frame: its accumulator (H, W, 4), its path state (the dict of `state` / Context.read_state)
        and its pass count replace this context's.  The ray colour's alpha is not part of the exported state and is never read: 1."""
        c, n = self.ctx.contents, self.w * self.h

        def put(ptr, values, dtype, width):
            flat = np.ascontiguousarray(values, dtype=dtype).reshape(n * width)
            C.memmove(ptr, flat.ctypes.data, flat.nbytes)

        put(c.image, accum, np.float32, 4)
        put(c.ray_origin, state["origin"], np.float32, 3)
        put(c.ray_direction, state["direction"], np.float32, 3)
        color = np.ones((self.h, self.w, 4), np.float32)
        color[..., :3] = state["color"]
        put(c.ray_color, color, np.float32, 4)
        put(c.ray_material, state["material"], np.uint32, 1)
        put(c.path_depth, state["depth"], np.uint8, 1)
        c.passes = int(passes)

    def _arr(self, ptr, shape, dtype):
        n = int(np.prod(shape))
        return np.ctypeslib.as_array(ptr, shape=(n,)).view(dtype).reshape(shape).copy()

    @property
    def accum(self):
        return self._arr(self.ctx.contents.image, (self.h, self.w, 4), np.float32)

    @property
    def depth(self):
        return self._arr(self.ctx.contents.depth, (self.h, self.w), np.float32)

    @property
    def rgba8(self):
        return self._arr(self.ctx.contents.rgba8, (self.h, self.w, 4), np.uint8)

    @property
    def state(self):
        c = self.ctx.contents
        return dict(origin=self._arr(c.ray_origin, (self.h, self.w, 3), np.float32),
                    direction=self._arr(c.ray_direction, (self.h, self.w, 3), np.float32),
                    color=self._arr(c.ray_color, (self.h, self.w, 4), np.float32)[..., :3],
                    material=self._arr(c.ray_material, (self.h, self.w), np.uint32),
                    depth=self._arr(c.path_depth, (self.h, self.w), np.uint8).astype(np.uint32))

    @property
    def passes(self):
        return int(self.ctx.contents.passes)

    @property
    def traced_rays(self):
        return int(self.ctx.contents.traced_rays)

    def pick(self, x, y):
        i, m = C.c_int32(), C.c_int32()
        self.lib.rzo_pick(C.byref(self.scene.struct), C.byref(self.camera), self.ctx, x, y, C.byref(i), C.byref(m))
        return i.value, m.value

    def ray_cast(self, x, y):
        """(instance, material slot, material, the triangle's index in its mesh) as Context.ray_cast returns them"""
        r = _abi.RayCast()
        self.lib.rzo_ray_cast(C.byref(self.scene.struct), C.byref(self.camera), self.ctx, x, y, C.byref(r))
        return r.instance, r.material_slot, r.material, r.triangle


def first_hits(flat_scene, camera, mode=0, lib=None, threads=1):
    """(H, W) array of first_hit_dtype: rzo_first_hit of every pixel under the HIPRZ_COMPAT_* flags `mode`.  The view
    guides(records) is what Context.read_guides must return."""
    lib = lib or load()
    out = np.zeros((camera.height, camera.width), first_hit_dtype)
    lib.rzo_first_hit_frame(C.byref(flat_scene.struct), C.byref(camera), int(mode), out.ctypes.data, threads)
    return out


def first_hit(flat_scene, camera, x, y, mode=0, lib=None):
    """one pixel's record, by the per-pixel entry point"""
    lib = lib or load()
    out = np.zeros(1, first_hit_dtype)
    lib.rzo_first_hit(C.byref(flat_scene.struct), C.byref(camera), int(mode), x, y, out.ctypes.data)
    return out[0]


def guides(records):
    """the hiprz_guide part of first-hit records as an array of _abi.guide_dtype"""
    out = np.zeros(records.shape, _abi.guide_dtype)
    for name in _abi.guide_dtype.names:
        out[name] = records[name]
    return out


def compat_fetch(flat_scene, texture, u, v, lib=None):
    """TextureBuffer::fetch of the CUDA engine on flat_scene's texture `texture` at each (u, v): (..., 4) float32 and the texel-fetch count."""
    lib = lib or load()
    u, v = np.broadcast_arrays(np.asarray(u, np.float32), np.asarray(v, np.float32))
    out = np.zeros(u.shape + (4,), np.float32)
    flat_out = out.reshape(-1, 4)
    fetches, n = C.c_uint64(), 0
    for i, (a, b) in enumerate(zip(u.ravel(), v.ravel())):
        lib.rzo_compat_fetch(C.byref(flat_scene.struct), texture, float(a), float(b), flat_out[i].ctypes.data, C.byref(fetches))
        n += fetches.value
    return out, n
