"""Loader and ctypes mirror of lightmap smoothing (include/hiprz_smooth.h, rayzath_amd/csrc/libhiprz_smooth.so): an edge-stopping a-trous
filter over the 16-byte records of a bake atlas, guided by the surface point under each texel — a texel is a weighted mean of its
neighbours on the same surface, never of a neighbour in the atlas alone.  As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _abi, _satellite
from .bake import point_dtype

LIB_PATH = _satellite.lib_path("HIPRZ_SMOOTH_LIB", "libhiprz_smooth.so")
INVALID = 0x80000000                              # HIPRZ_SMOOTH_INVALID: the word of a texel that has no value
MAX_SIZE, MAX_ITERATIONS = 16384, 8

params_dtype = np.dtype([("iterations", "<u4"), ("radius", "<f4"), ("plane", "<f4"), ("sigma_colour", "<f4")])      # hiprz_smooth_params
assert params_dtype.itemsize == 16

P, U32 = C.c_void_p, C.c_uint32
ENTRY_POINTS = {
    "hiprz_smooth_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_smooth_destroy": (C.c_int, [P]),
    "hiprz_smooth_last_error": (C.c_char_p, [P]),
    "hiprz_smooth_check_params": (C.c_int, [P]),
    "hiprz_smooth_texels": (C.c_int, [P, P, P, U32, U32, P, P, P]),
    "hiprz_smooth_texels_host": (C.c_int, [P, P, P, U32, U32, P, P]),
    "hiprz_smooth_layout": (None, [P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


def params(iterations=3, radius=0.0, plane=0.05, sigma_colour=2.0):
    """a hiprz_smooth_params record (params_dtype, shape ()): `iterations` a-trous steps 1, 2, 4, ... (1 .. 8); `radius` and `plane` in
    world units — no tap further than `radius` from the texel's point, none further than `plane` from its tangent plane; `sigma_colour`
    in the units of the records, halved with every iteration; 0 switches a stop off.  The defaults smooth over three iterations
    (a footprint of 29 texels), keep to the texel's own plane within 0.05, stop at a colour difference of 2 (light of the order of 1: a
    K = 4 penumbra's steps of 0.25 blend, a shadow's edge survives the later, narrower iterations) and leave the world-sized stop, whose
    right value depends on the scene's scale, off.  ValueError for what hiprz_smooth_check_params refuses."""
    p = np.zeros((), params_dtype)
    if not 1 <= int(iterations) <= MAX_ITERATIONS:
        raise ValueError(f"iterations = {iterations} is not in 1..{MAX_ITERATIONS}")
    p["iterations"], p["radius"], p["plane"], p["sigma_colour"] = int(iterations), radius, plane, sigma_colour
    if load().hiprz_smooth_check_params(p.ctypes.data) != _abi.OK:
        raise ValueError(f"radius = {radius}, plane = {plane} and sigma_colour = {sigma_colour} must be finite and >= 0")
    return p


def _params(p):
    """the record of `p`: a params() record, or a mapping of params()'s keywords"""
    if isinstance(p, dict):
        return params(**p)
    p = np.ascontiguousarray(p)
    if p.dtype != params_dtype or p.size != 1:
        raise TypeError("smooth must be a rayzath_amd.smooth.params() record or a dict of its keywords")
    return p.reshape(())


def layout():
    out = (U32 * 8)()
    load().hiprz_smooth_layout(out)
    return list(out)


class Smooth(_satellite.Handle):
    """Owns one hiprz_smooth bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _smooth = property(lambda self: self._handle)

    def __init__(self, ctx_ptr):
        super().__init__(load(), "smooth", ctx_ptr)

    def texels(self, points, records, smooth):
        """the smoothed records of a host atlas: `points` (H, W) of bake.point_dtype, `records` (H, W) of a 16-byte dtype (RGB and a word);
        an array like `records`, which is not changed.  Waits for the context's stream."""
        points, records, p = np.ascontiguousarray(points), np.ascontiguousarray(records), _params(smooth)
        if points.dtype != point_dtype or points.ndim != 2:
            raise TypeError("points must be an (H, W) array of rayzath_amd.bake.point_dtype")
        if records.dtype.itemsize != 16 or records.shape != points.shape:
            raise TypeError("records must be an (H, W) array of 16-byte records, the shape of points")
        out = np.zeros_like(records)
        H, W = points.shape
        self._check(self.lib.hiprz_smooth_texels_host(self._smooth, points.ctypes.data, records.ctypes.data, W, H, p.ctypes.data, out.ctypes.data))
        return out

    def texels_device(self, points_ptr, records_ptr, width, height, smooth, out_ptr=None, stream=None):
        """enqueue only: the width x height points at the device address points_ptr and the records at records_ptr -> records at out_ptr
        (None: in place, at records_ptr)"""
        p = _params(smooth)
        self._check(self.lib.hiprz_smooth_texels(self._smooth, points_ptr, records_ptr, width, height, p.ctypes.data, records_ptr if out_ptr is None else out_ptr, stream))
