"""Loader and ctypes mirror of occlusion baking (include/hiprz_bake.h, rayzath_amd/csrc/libhiprz_bake.so): per surface point, K rays made
from a table of directions, walked and counted on the device — how many are occluded and the sum of the directions that are not.  As with
_lib.py there is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _abi, _hiprt, _satellite
from .query import ray_dtype

LIB_PATH = _satellite.lib_path("HIPRZ_BAKE_LIB", "libhiprz_bake.so")
INVALID = 0x80000000                              # HIPRZ_BAKE_INVALID

point_dtype = np.dtype([("position", "<f4", 3), ("near", "<f4"), ("normal", "<f4", 3), ("far", "<f4")])      # hiprz_bake_point
texel_dtype = np.dtype([("bent", "<f4", 3), ("occluded", "<u4")])                                            # hiprz_bake_texel
assert point_dtype.itemsize == 32 and texel_dtype.itemsize == 16

P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t
ENTRY_POINTS = {
    "hiprz_bake_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_bake_destroy": (C.c_int, [P]),
    "hiprz_bake_last_error": (C.c_char_p, [P]),
    "hiprz_bake_set_directions": (C.c_int, [P, P, U32, U32]),
    "hiprz_bake_set_of": (U32, [U32, U32, U32]),
    "hiprz_bake_cosine_directions": (C.c_int, [U32, U32, P]),
    "hiprz_bake_occlusion": (C.c_int, [P, P, SZ, U32, P, P]),
    "hiprz_bake_rays": (C.c_int, [P, P, SZ, U32, P, P]),
    "hiprz_bake_occlusion_host": (C.c_int, [P, P, SZ, U32, P]),
    "hiprz_bake_layout": (None, [P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


def points(position, normal, near=1.0e-3, far=3.0e38):
    """an array of point_dtype from (n, 3) positions and normals (broadcast against each other) and scalar or (n,) ranges"""
    position, normal = np.broadcast_arrays(np.asarray(position, np.float32), np.asarray(normal, np.float32))
    out = np.zeros(position.shape[:-1], point_dtype)
    out["position"], out["normal"], out["near"], out["far"] = position, normal, near, far
    return out


def cosine_directions(K, S):
    """the library's cosine-weighted Fibonacci table: (S, K, 4) float32, (x, y, z, 0), z along the normal"""
    out = np.zeros((S, K, 4), np.float32)
    if load().hiprz_bake_cosine_directions(K, S, out.ctypes.data) != _abi.OK:
        raise ValueError(f"K = {K} is not one of 16, 32, 64, 128, 256, 512, 1024 or S = {S} is not in 1..64")
    return out


def set_of(i, seed, S):
    """the set of directions point i uses under `seed`"""
    return int(load().hiprz_bake_set_of(i, seed, S))


class Bake(_satellite.Handle):
    """Owns one hiprz_bake bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _bake = property(lambda self: self._handle)

    def __init__(self, ctx_ptr):
        self.K = self.S = 0
        self.table = None         # the (K, S) of a cosine table set through set_directions, None for a caller's array or none
        super().__init__(load(), "bake", ctx_ptr)

    def set_directions(self, directions):
        """directions: an (S, K, 4) float32 array of unit vectors in the local frame (z along the normal), or a (K, S) pair for the cosine table"""
        pair = tuple(directions) if isinstance(directions, tuple) else None
        if pair is not None:
            directions = cosine_directions(*pair)
        table = np.ascontiguousarray(directions, np.float32)
        if table.ndim != 3 or table.shape[2] != 4:
            raise TypeError("directions must be an (S, K, 4) float32 array or a (K, S) pair")
        self._check(self.lib.hiprz_bake_set_directions(self._bake, table.ctypes.data, table.shape[1], table.shape[0]))
        self.S, self.K = table.shape[:2]
        self.table = pair

    @staticmethod
    def _points(points):
        points = np.ascontiguousarray(points)
        if points.dtype not in (point_dtype, ray_dtype):      # a point is the ray along its normal: the same 32 bytes
            raise TypeError("points must be an array of rayzath_amd.bake.point_dtype")
        return points

    def occlusion(self, points, seed=0):
        """texels (texel_dtype, the shape of `points`) of host points; waits for the context's stream"""
        points = self._points(points)
        out = np.zeros(points.shape, texel_dtype)
        self._check(self.lib.hiprz_bake_occlusion_host(self._bake, points.ctypes.data, points.size, seed, out.ctypes.data))
        return out

    def occlusion_device(self, points_ptr, n, out_ptr, seed=0, stream=None):
        """enqueue only: n points at the device address points_ptr -> n texels at out_ptr"""
        self._check(self.lib.hiprz_bake_occlusion(self._bake, points_ptr, n, seed, out_ptr, stream))

    def rays_device(self, points_ptr, n, rays_ptr, seed=0, stream=None):
        """enqueue only: the n * K rays the bake walks for n device points, ray i * K + k of (point i, direction k), to rays_ptr"""
        self._check(self.lib.hiprz_bake_rays(self._bake, points_ptr, n, seed, rays_ptr, stream))

    def rays(self, points, seed, sync):
        """the rays of host points as an array of query.ray_dtype of shape points.shape + (K,).  `sync` waits for the context's stream
        (Context.sync: it also makes the head device current for the buffers)."""
        points = self._points(points)
        n = points.size
        if n == 0 or not self.K:
            dummy = (C.c_uint8 * 32)()
            self._check(self.lib.hiprz_bake_rays(self._bake, dummy, 0, seed, dummy, None))  # without a table: refused; else nothing to do
            return np.zeros(points.shape + (self.K,), ray_dtype)
        sync()
        d_points, d_rays = _hiprt.DeviceBuffer.of(points), _hiprt.DeviceBuffer(n * self.K * ray_dtype.itemsize)
        try:
            self.rays_device(d_points.ptr, n, d_rays.ptr, seed)
            sync()
            return d_rays.download(points.shape + (self.K,), ray_dtype)
        finally:
            d_points.free(), d_rays.free()
