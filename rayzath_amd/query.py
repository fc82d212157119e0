"""Loader and ctypes mirror of the ray queries (include/hiprz_query.h, rayzath_amd/csrc/libhiprz_query.so): closest hit and occlusion for
caller-supplied rays in the world a context holds.  As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _satellite

LIB_PATH = _satellite.lib_path("HIPRZ_QUERY_LIB", "libhiprz_query.so")
NORMALIZE = 1                                     # HIPRZ_QUERY_NORMALIZE
HIT_FOUND, HIT_EXTERNAL, HIT_INVALID = 1, 2, 4    # hiprz_hit::flags

ray_dtype = np.dtype([("origin", "<f4", 3), ("near", "<f4"), ("direction", "<f4", 3), ("far", "<f4")])      # hiprz_ray
hit_dtype = np.dtype([("t", "<f4"), ("u", "<f4"), ("v", "<f4"), ("flags", "<u4"), ("instance", "<i4"), ("material_slot", "<i4"),
                      ("material", "<i4"), ("triangle", "<u4"), ("normal", "<f4", 3), ("scene_triangle", "<i4")])  # hiprz_hit
assert ray_dtype.itemsize == 32 and hit_dtype.itemsize == 48

P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t
ENTRY_POINTS = {
    "hiprz_query_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_query_destroy": (C.c_int, [P]),
    "hiprz_query_last_error": (C.c_char_p, [P]),
    "hiprz_query_closest": (C.c_int, [P, P, SZ, U32, P, P]),
    "hiprz_query_occluded": (C.c_int, [P, P, SZ, U32, P, P]),
    "hiprz_query_closest_host": (C.c_int, [P, P, SZ, U32, P]),
    "hiprz_query_occluded_host": (C.c_int, [P, P, SZ, U32, P]),
    "hiprz_query_pixel_rays": (C.c_int, [P, P, P]),
    "hiprz_query_layout": (None, [P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


def rays(origin, direction, near=0.0, far=3.0e38):
    """an array of ray_dtype from (n, 3) origins and directions (broadcast against each other) and scalar or (n,) ranges"""
    origin, direction = np.broadcast_arrays(np.asarray(origin, np.float32), np.asarray(direction, np.float32))
    out = np.zeros(origin.shape[:-1], ray_dtype)
    out["origin"], out["direction"], out["near"], out["far"] = origin, direction, near, far
    return out


def ray_records(rays):
    """`rays` as a contiguous array of ray_dtype, for a call that takes its address"""
    rays = np.ascontiguousarray(rays)
    if rays.dtype != ray_dtype:
        raise TypeError("rays must be an array of rayzath_amd.query.ray_dtype")
    return rays


class Query(_satellite.Handle):
    """Owns one hiprz_query bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _query = property(lambda self: self._handle)
    _rays = staticmethod(ray_records)

    def __init__(self, ctx_ptr):
        super().__init__(load(), "query", ctx_ptr)

    def closest(self, rays, normalize=False):
        """hits (hit_dtype, the shape of `rays`) of host rays; waits for the context's stream"""
        rays = self._rays(rays)
        hits = np.zeros(rays.shape, hit_dtype)
        self._check(self.lib.hiprz_query_closest_host(self._query, rays.ctypes.data, rays.size, NORMALIZE if normalize else 0, hits.ctypes.data))
        return hits

    def occluded(self, rays, normalize=False):
        """uint32 per host ray: 1 = something lies within its range; waits for the context's stream"""
        rays = self._rays(rays)
        out = np.zeros(rays.shape, np.uint32)
        self._check(self.lib.hiprz_query_occluded_host(self._query, rays.ctypes.data, rays.size, NORMALIZE if normalize else 0, out.ctypes.data))
        return out

    def closest_device(self, rays_ptr, n, hits_ptr, normalize=False, stream=None):
        """enqueue only: n rays at the device address rays_ptr -> n hits at hits_ptr"""
        self._check(self.lib.hiprz_query_closest(self._query, rays_ptr, n, NORMALIZE if normalize else 0, hits_ptr, stream))

    def occluded_device(self, rays_ptr, n, out_ptr, normalize=False, stream=None):
        self._check(self.lib.hiprz_query_occluded(self._query, rays_ptr, n, NORMALIZE if normalize else 0, out_ptr, stream))

    def pixel_rays_device(self, rays_ptr, stream=None):
        """enqueue only: the selected camera's W*H pixel-centre rays, row-major, to the device address rays_ptr"""
        self._check(self.lib.hiprz_query_pixel_rays(self._query, rays_ptr, stream))
