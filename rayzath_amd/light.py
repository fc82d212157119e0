"""Loader and ctypes mirror of light baking (include/hiprz_light.h, rayzath_amd/csrc/libhiprz_light.so): per surface point, K shadow rays per
light of the scene made from a table of disk samples, weighted, walked and summed on the device — the direct light that arrives and how
many rays were shadowed.  As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _abi, _hiprt, _satellite
from .bake import point_dtype
from .query import ray_dtype

LIB_PATH = _satellite.lib_path("HIPRZ_LIGHT_LIB", "libhiprz_light.so")
INVALID = 0x80000000                              # HIPRZ_LIGHT_INVALID
TO_END = 0xFFFFFFFF                               # HIPRZ_LIGHT_TO_END

texel_dtype = np.dtype([("light", "<f4", 3), ("shadowed", "<u4")])                                            # hiprz_light_texel
range_dtype = np.dtype([("spot_first", "<u4"), ("spot_count", "<u4"), ("direct_first", "<u4"), ("direct_count", "<u4")])  # hiprz_light_range
assert texel_dtype.itemsize == 16 and range_dtype.itemsize == 16

P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t
ENTRY_POINTS = {
    "hiprz_light_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_light_destroy": (C.c_int, [P]),
    "hiprz_light_last_error": (C.c_char_p, [P]),
    "hiprz_light_set_samples": (C.c_int, [P, P, U32, U32]),
    "hiprz_light_set_of": (U32, [U32, U32, U32]),
    "hiprz_light_disk_samples": (C.c_int, [U32, U32, P]),
    "hiprz_light_count": (C.c_int, [P, P, C.POINTER(U32), C.POINTER(U32)]),
    "hiprz_light_bake": (C.c_int, [P, P, SZ, U32, P, P, P]),
    "hiprz_light_rays": (C.c_int, [P, P, SZ, U32, P, P, P, P]),
    "hiprz_light_bake_host": (C.c_int, [P, P, SZ, U32, P, P]),
    "hiprz_light_layout": (None, [P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


def disk_samples(K, S):
    """the library's disk table: (S, K, 2) float32, (r cos phi, r sin phi) with r = sqrt((k + 0.5) / K)"""
    out = np.zeros((S, K, 2), np.float32)
    if load().hiprz_light_disk_samples(K, S, out.ctypes.data) != _abi.OK:
        raise ValueError(f"K = {K} is not a power of two in 1..1024 or S = {S} is not in 1..64")
    return out


def set_of(i, seed, S):
    """the set of samples point i uses under `seed`"""
    return int(load().hiprz_light_set_of(i, seed, S))


def light_range(lights):
    """a one-record array of range_dtype from None (every light: None) or (spot_first, spot_count, direct_first, direct_count), a count of
    None or TO_END meaning "to the end" """
    if lights is None:
        return None
    sf, sc, df, dc = lights
    out = np.zeros(1, range_dtype)
    out[0] = (sf, TO_END if sc is None else sc, df, TO_END if dc is None else dc)
    return out


class Light(_satellite.Handle):
    """Owns one hiprz_light bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _light = property(lambda self: self._handle)

    def __init__(self, ctx_ptr):
        self.K = self.S = 0
        self.table = None         # the (K, S) of a disk table set through set_samples, None for a caller's array or none
        super().__init__(load(), "light", ctx_ptr)

    def set_samples(self, samples):
        """samples: an (S, K, 2) float32 array of points of the unit disk, or a (K, S) pair for the library's disk table"""
        pair = tuple(samples) if isinstance(samples, tuple) else None
        if pair is not None:
            samples = disk_samples(*pair)
        table = np.ascontiguousarray(samples, np.float32)
        if table.ndim != 3 or table.shape[2] != 2:
            raise TypeError("samples must be an (S, K, 2) float32 array or a (K, S) pair")
        self._check(self.lib.hiprz_light_set_samples(self._light, table.ctypes.data, table.shape[1], table.shape[0]))
        self.S, self.K = table.shape[:2]
        self.table = pair

    @staticmethod
    def _points(points):
        points = np.ascontiguousarray(points)
        if points.dtype not in (point_dtype, ray_dtype):      # a point is the ray along its normal: the same 32 bytes
            raise TypeError("points must be an array of rayzath_amd.bake.point_dtype")
        return points

    @staticmethod
    def _range_ptr(rng):
        return None if rng is None else rng.ctypes.data

    def count(self, lights=None):
        """(spots, directs): the lights `lights` selects in the context's scene as it is now (the library's own rule, asked of the device view)"""
        rng, spots, directs = light_range(lights), U32(), U32()
        self._check(self.lib.hiprz_light_count(self._light, self._range_ptr(rng), C.byref(spots), C.byref(directs)))
        return spots.value, directs.value

    def bake(self, points, seed=0, lights=None):
        """texels (texel_dtype, the shape of `points`) of host points; waits for the context's stream"""
        points, rng = self._points(points), light_range(lights)
        out = np.zeros(points.shape, texel_dtype)
        self._check(self.lib.hiprz_light_bake_host(self._light, points.ctypes.data, points.size, seed, self._range_ptr(rng), out.ctypes.data))
        return out

    def bake_device(self, points_ptr, n, out_ptr, seed=0, lights=None, stream=None):
        """enqueue only: n points at the device address points_ptr -> n texels at out_ptr"""
        rng = light_range(lights)
        self._check(self.lib.hiprz_light_bake(self._light, points_ptr, n, seed, self._range_ptr(rng), out_ptr, stream))

    def rays_device(self, points_ptr, n, rays_ptr, weights_ptr, seed=0, lights=None, stream=None):
        """enqueue only: the n * L * K rays the bake walks for n device points, ray (i * L + l) * K + k of (point i, light l, sample k),
        to rays_ptr and their weights to weights_ptr"""
        rng = light_range(lights)
        self._check(self.lib.hiprz_light_rays(self._light, points_ptr, n, seed, self._range_ptr(rng), rays_ptr, weights_ptr, stream))

    def rays(self, points, seed, lights, sync):
        """(rays, weights) of host points: query.ray_dtype and float32 of shape points.shape + (L, K), L the number of lights `lights`
        selects now (count()).  `sync` waits for the context's stream (Context.sync: it also makes the head device current for the buffers)."""
        points = self._points(points)
        if not self.K:
            dummy = (C.c_uint8 * 32)()
            self._check(self.lib.hiprz_light_rays(self._light, dummy, 0, seed, None, dummy, dummy, None))  # without a table: refused
        n_lights = sum(self.count(lights))                  # refuses what the rays call would: no scene, a bad range
        n, shape = points.size, points.shape + (n_lights, self.K)
        total = n * n_lights * self.K
        if total == 0:
            return np.zeros(shape, ray_dtype), np.zeros(shape, np.float32)
        sync()
        d_points, d_rays, d_weights = _hiprt.DeviceBuffer.of(points), _hiprt.DeviceBuffer(total * ray_dtype.itemsize), _hiprt.DeviceBuffer(total * 4)
        try:
            self.rays_device(d_points.ptr, n, d_rays.ptr, d_weights.ptr, seed, lights)
            sync()
            return d_rays.download(shape, ray_dtype), d_weights.download(shape, np.float32)
        finally:
            d_points.free(), d_rays.free(), d_weights.free()
