"""Loader and ctypes mirror of the noise meter (include/hiprz_noise.h, rayzath_amd/csrc/libhiprz_noise.so): a per-tile error map of a
frame in display units and its summary.  As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._lib import HiprzError

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libhiprz_noise.so")
TILE_W, TILE_H = 32, 8
_lib = None


class Params(C.Structure):  # hiprz_noise_params
    _fields_ = [("aperture", C.c_float), ("exposure_time", C.c_float), ("threshold", C.c_float), ("min_batches", C.c_uint32)]


class Summary(C.Structure):  # hiprz_noise_summary
    _fields_ = [("rms", C.c_double), ("tile_rms_max", C.c_double), ("max", C.c_float), ("worst_tile", C.c_uint32),
                ("estimated", C.c_uint64), ("above", C.c_uint64), ("pixels", C.c_uint64), ("tiles_x", C.c_uint32), ("tiles_y", C.c_uint32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


P, U32 = C.c_void_p, C.c_uint32
ENTRY_POINTS = {
    "hiprz_noise_create": (C.c_int, [C.POINTER(P), C.c_int]),
    "hiprz_noise_destroy": (C.c_int, [P]),
    "hiprz_noise_last_error": (C.c_char_p, [P]),
    "hiprz_noise_tiles": (C.c_int, [P, P, P, U32, U32, C.POINTER(Params), P, P]),
    "hiprz_noise_measure": (C.c_int, [P, P, P, U32, U32, C.POINTER(Params), P, C.POINTER(Summary), P]),
    "hiprz_noise_summarise": (C.c_int, [P, U32, U32, U32, U32, C.POINTER(Summary)]),
    "hiprz_noise_layout": (None, [P]),
}


def load():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it first (python -c 'import __graft_entry__ as g; g.build()'). "
                "rayzath_amd has no CPU fallback.")
        lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in ENTRY_POINTS.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
    return _lib


def tile_grid(width, height):
    """(tiles_x, tiles_y) of a width x height frame"""
    return (width + TILE_W - 1) // TILE_W, (height + TILE_H - 1) // TILE_H


def summarise(tiles, width, height):
    """hiprz_noise_summarise (pure host) on a (tiles_y, tiles_x, 4) float32 array of tile records"""
    tiles = np.ascontiguousarray(tiles, dtype=np.float32)
    out = Summary()
    rc = load().hiprz_noise_summarise(tiles.ctypes.data, tiles.shape[1], tiles.shape[0], width, height, C.byref(out))
    if rc != _abi.OK:
        raise HiprzError(rc, "noise_summarise: bad arguments")
    return out


class Meter:
    """Owns one hiprz_noise_meter on one device."""

    def __init__(self, device=0):
        self.lib = load()
        self._meter = C.c_void_p()
        rc = self.lib.hiprz_noise_create(C.byref(self._meter), int(device))
        if rc != _abi.OK:
            raise HiprzError(rc, (self.lib.hiprz_noise_last_error(None) or b"").decode())

    def _check(self, rc):
        if rc != _abi.OK:
            raise HiprzError(rc, (self.lib.hiprz_noise_last_error(self._meter) or b"").decode())

    def tiles(self, accum_ptr, variance_ptr, width, height, params, tiles_out_ptr, stream=None):
        """enqueue only: tile records into device memory at tiles_out_ptr"""
        self._check(self.lib.hiprz_noise_tiles(self._meter, accum_ptr, variance_ptr, width, height, C.byref(params), tiles_out_ptr, stream))

    def measure(self, accum_ptr, variance_ptr, width, height, params, stream=None):
        """(Summary, tiles (tiles_y, tiles_x, 4) float32) of the two W*H float4 device images; waits for `stream`"""
        tx, ty = tile_grid(max(int(width), 1), max(int(height), 1))
        tiles = np.zeros((ty, tx, 4), dtype=np.float32)
        out = Summary()
        self._check(self.lib.hiprz_noise_measure(self._meter, accum_ptr, variance_ptr, width, height, C.byref(params), stream, C.byref(out), tiles.ctypes.data))
        return out, tiles

    def close(self):
        if self._meter:
            self.lib.hiprz_noise_destroy(self._meter)
            self._meter = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
