"""Loader and ctypes mirror of the ordered ray queries (include/hiprz_order.h, rayzath_amd/csrc/libhiprz_order.so): the queries of query.py
for incoherent batches, walked in the renderer's sorted ray order; the result bytes are query.py's.  As with _lib.py there is no fallback:
a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _abi, _hiprt, _lib
from ._lib import HiprzError
from .query import NORMALIZE, hit_dtype, ray_dtype

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("HIPRZ_ORDER_LIB") or os.path.join(_HERE, "csrc", "libhiprz_order.so")
_lib_order = None

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
    global _lib_order
    if _lib_order is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
                "rayzath_amd has no CPU fallback.")
        _lib.load()  # libhiprz.so first: the order library reads contexts through hiprz_device_view and sorts through hiprz_sort_u32_device
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in ENTRY_POINTS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib_order = lib
    return _lib_order


class Order:
    """Owns one hiprz_order bound to the hiprz_ctx `ctx_ptr`; close it before the context."""

    def __init__(self, ctx_ptr):
        self.lib = load()
        self._order = C.c_void_p()
        rc = self.lib.hiprz_order_create(C.byref(self._order), ctx_ptr)
        if rc != _abi.OK:
            raise HiprzError(rc, (self.lib.hiprz_order_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc != _abi.OK:
            raise HiprzError(rc, (self.lib.hiprz_order_last_error(self._order) or b"").decode())

    @staticmethod
    def _rays(rays):
        rays = np.ascontiguousarray(rays)
        if rays.dtype != ray_dtype:
            raise TypeError("rays must be an array of rayzath_amd.query.ray_dtype")
        return rays

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

    def close(self):
        if self._order:
            self.lib.hiprz_order_destroy(self._order)
            self._order = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
