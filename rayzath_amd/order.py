"""Loader and ctypes mirror of the ordered ray queries (include/hiprz_order.h, rayzath_amd/csrc/libhiprz_order.so): the queries of query.py
for incoherent batches, walked in the renderer's sorted ray order; the result bytes are query.py's.  As with _lib.py there is no fallback:
a missing library raises."""
import ctypes as C

import numpy as np

from . import _hiprt, _satellite
from .query import NORMALIZE, hit_dtype, ray_dtype, ray_records

LIB_PATH = _satellite.lib_path("HIPRZ_ORDER_LIB", "libhiprz_order.so")

P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t
ENTRY_POINTS = {
    "hiprz_order_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_order_destroy": (C.c_int, [P]),
    "hiprz_order_last_error": (C.c_char_p, [P]),
    "hiprz_order_permutation": (C.c_int, [P, P, SZ, U32, P, P, P]),
    "hiprz_order_closest": (C.c_int, [P, P, SZ, U32, P, P]),
    "hiprz_order_occluded": (C.c_int, [P, P, SZ, U32, P, P]),
    "hiprz_order_closest_by": (C.c_int, [P, P, P, SZ, U32, P, P]),
    "hiprz_order_occluded_by": (C.c_int, [P, P, P, SZ, U32, P, P]),
    "hiprz_order_closest_host": (C.c_int, [P, P, SZ, U32, P]),
    "hiprz_order_occluded_host": (C.c_int, [P, P, SZ, U32, P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


class Order(_satellite.Handle):
    """Owns one hiprz_order bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _order = property(lambda self: self._handle)
    _rays = staticmethod(ray_records)

    def __init__(self, ctx_ptr):
        super().__init__(load(), "order", ctx_ptr)

    def closest(self, rays, normalize=False):
        """query.Query.closest's hits of host rays, walked in sorted order; waits for the context's stream"""
        rays = self._rays(rays)
        hits = np.zeros(rays.shape, hit_dtype)
        self._check(self.lib.hiprz_order_closest_host(self._order, rays.ctypes.data, rays.size, NORMALIZE if normalize else 0, hits.ctypes.data))
        return hits

    def occluded(self, rays, normalize=False):
        """query.Query.occluded's words of host rays, walked in sorted order; waits for the context's stream"""
        rays = self._rays(rays)
        out = np.zeros(rays.shape, np.uint32)
        self._check(self.lib.hiprz_order_occluded_host(self._order, rays.ctypes.data, rays.size, NORMALIZE if normalize else 0, out.ctypes.data))
        return out

    def permutation(self, rays, normalize=False, sync=None):
        """(perm, keys) of host rays as uint32 arrays of rays.size: perm[i] is the index of the ray walked i-th, keys[k] ray k's sort key.
        `sync` waits for the context's stream (Context.sync: it also makes the head device current for the buffers)."""
        rays = self._rays(rays).reshape(-1)
        n = rays.size
        if n == 0:
            return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
        sync()
        d_rays, d_keys, d_perm = _hiprt.DeviceBuffer.of(rays), _hiprt.DeviceBuffer(4 * n), _hiprt.DeviceBuffer(4 * n)
        try:
            self.permutation_device(d_rays.ptr, n, d_perm.ptr, d_keys.ptr, normalize)
            sync()
            return d_perm.download((n,), np.uint32), d_keys.download((n,), np.uint32)
        finally:
            d_rays.free(), d_keys.free(), d_perm.free()

    def permutation_device(self, rays_ptr, n, perm_ptr, keys_ptr=None, normalize=False, stream=None):
        """enqueue only: the sorted order of n device rays to perm_ptr, their keys in caller order to keys_ptr unless None"""
        self._check(self.lib.hiprz_order_permutation(self._order, rays_ptr, n, NORMALIZE if normalize else 0, keys_ptr, perm_ptr, stream))

    def closest_device(self, rays_ptr, n, hits_ptr, normalize=False, stream=None, perm_ptr=None):
        """enqueue only: n rays at the device address rays_ptr -> n hits at hits_ptr; perm_ptr: a kept order (hiprz_order_closest_by)"""
        flags = NORMALIZE if normalize else 0
        if perm_ptr is None:
            self._check(self.lib.hiprz_order_closest(self._order, rays_ptr, n, flags, hits_ptr, stream))
        else:
            self._check(self.lib.hiprz_order_closest_by(self._order, rays_ptr, perm_ptr, n, flags, hits_ptr, stream))

    def occluded_device(self, rays_ptr, n, out_ptr, normalize=False, stream=None, perm_ptr=None):
        flags = NORMALIZE if normalize else 0
        if perm_ptr is None:
            self._check(self.lib.hiprz_order_occluded(self._order, rays_ptr, n, flags, out_ptr, stream))
        else:
            self._check(self.lib.hiprz_order_occluded_by(self._order, rays_ptr, perm_ptr, n, flags, out_ptr, stream))
