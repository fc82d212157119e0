"""Loader and ctypes mirror of probe placement (include/hiprz_place.h, rayzath_amd/csrc/libhiprz_place.so): the probes of a grid moved out
of geometry and away from the surface they hug, on the device — every probe evaluated by its K rays and nudged, up to `iterations` times,
through the nearest back face when it sits inside geometry and towards its most open direction when a front face is nearer than a margin.
As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _abi, _hiprt, _satellite
from .bake import point_dtype
from .probe import sphere_directions
from .query import ray_dtype

LIB_PATH = _satellite.lib_path("HIPRZ_PLACE_LIB", "libhiprz_place.so")
CLEAR, NEAR, INSIDE = 0, 1, 2                     # state(records)
STATE_MASK = 0xFF
STUCK = 0x100                                     # HIPRZ_PLACE_STUCK: the loop stopped without a move it wanted to make
INVALID = 0x80000000                              # HIPRZ_PLACE_INVALID: the word of an invalid probe
MAX_ITERATIONS = 16

params_dtype = np.dtype([("min_front", "<f4"), ("reach", "<f4"), ("max_offset", "<f4", (3,)), ("iterations", "<u4"), ("max_back", "<u4"), ("reserved", "<u4")])  # hiprz_place_params
record_dtype = np.dtype([("offset", "<f4", (3,)), ("word", "<u4"), ("front", "<f4"), ("back", "<f4"), ("n_back", "<u4"), ("n_front", "<u4")])                # hiprz_place_record
assert (params_dtype.itemsize, record_dtype.itemsize) == (32, 32)

P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t
ENTRY_POINTS = {
    "hiprz_place_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_place_destroy": (C.c_int, [P]),
    "hiprz_place_last_error": (C.c_char_p, [P]),
    "hiprz_place_set_directions": (C.c_int, [P, P, U32, U32]),
    "hiprz_place_check_params": (C.c_int, [P]),
    "hiprz_place_probes": (C.c_int, [P, P, SZ, U32, P, P, P, P]),
    "hiprz_place_probes_host": (C.c_int, [P, P, SZ, U32, P, P, P]),
    "hiprz_place_layout": (None, [P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


def params(min_front, reach, max_offset, iterations=4, max_back=None):
    """a hiprz_place_params record (params_dtype, shape ()): a probe with a front face nearer than `min_front` is moved away from it, one
    more than `max_back` of whose rays hit back faces is moved out through the nearest of them; distances are capped at `reach`; the
    offset stays within `max_offset` (a number, or one per axis) on every axis; at most `iterations` moves.  max_back None: a quarter of
    the table's K, filled in by the call that places.  ValueError for what hiprz_place_check_params refuses."""
    p = np.zeros((), params_dtype)
    offset = np.broadcast_to(np.asarray(max_offset, np.float64), (3,))
    if not 0 <= int(iterations) < 2 ** 32 or (max_back is not None and not 0 <= int(max_back) < 2 ** 32):
        raise ValueError(f"iterations = {iterations} or max_back = {max_back} is not a uint32")
    p["min_front"], p["reach"], p["max_offset"], p["iterations"] = min_front, reach, offset, int(iterations)
    p["max_back"] = 0 if max_back is None else int(max_back)
    if load().hiprz_place_check_params(p.ctypes.data) != _abi.OK:
        raise ValueError(f"min_front = {min_front} and reach = {reach} must be finite and > 0, max_offset = {max_offset} finite and >= 0, iterations = {iterations} at most {MAX_ITERATIONS}")
    return p if max_back is not None else _Unset(p)


class _Unset:
    """params() without a max_back: the record, to be completed with K // 4 by the call that places"""

    def __init__(self, record):
        self.record = record


def params_for(grid, min_front, reach, iterations=4, max_back=None, share=0.45):
    """params() for the probes of `grid` (field.grid_of): max_offset = `share` of the grid's step per axis, so that a probe stays in its
    own cell"""
    return params(min_front, reach, np.float32(share) * np.asarray(grid["step"], np.float32).reshape(3), iterations, max_back)


def _params(p, K):
    """the record of `p` for a table of K directions: a params() record (max_back K // 4 where it was left open) or a dict of params()'s
    keywords"""
    if isinstance(p, dict):
        p = params(**p)
    if isinstance(p, _Unset):
        p = p.record.copy()
        p["max_back"] = K // 4
        return p
    p = np.ascontiguousarray(p)
    if p.dtype != params_dtype or p.size != 1:
        raise TypeError("params must be a rayzath_amd.place.params() record or a dict of its keywords")
    return p.reshape(())


def state(records):
    """CLEAR, NEAR or INSIDE per record (INVALID for the record of an invalid probe)"""
    word = np.asarray(records)["word"]
    return np.where(word == INVALID, np.uint32(INVALID), word & np.uint32(STATE_MASK))


def moves(records):
    """the moves made per record (0 for an invalid probe)"""
    word = np.asarray(records)["word"]
    return np.where(word == INVALID, np.uint32(0), (word >> np.uint32(16)) & np.uint32(0x7FFF))


def layout():
    out = (U32 * 8)()
    load().hiprz_place_layout(out)
    return list(out)


def _probes(probes):
    probes = np.ascontiguousarray(probes)
    if probes.dtype not in (point_dtype, ray_dtype):      # a probe is the ray along its axis: the same 32 bytes
        raise TypeError("probes must be an array of rayzath_amd.bake.point_dtype")
    return probes


class Placer(_satellite.Handle):
    """Owns one hiprz_place bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _place = property(lambda self: self._handle)

    def __init__(self, ctx_ptr):
        self.K = self.S = 0
        self.table = None         # the (K, S) of a sphere table set through set_directions, None for a caller's array or none
        super().__init__(load(), "place", ctx_ptr)

    def set_directions(self, directions):
        """directions: an (S, K, 4) float32 array of unit vectors in the probe's frame, or a (K, S) pair for the probe library's sphere
        table; K is one of 64 .. 1024"""
        pair = tuple(directions) if isinstance(directions, tuple) else None
        if pair is not None:
            if pair[0] < 64:
                raise ValueError(f"K = {pair[0]} is below 64: a placement wants at least a ray per lane")
            directions = sphere_directions(*pair)
        table = np.ascontiguousarray(directions, np.float32)
        if table.ndim != 3 or table.shape[2] != 4:
            raise TypeError("directions must be an (S, K, 4) float32 array or a (K, S) pair")
        self._check(self.lib.hiprz_place_set_directions(self._place, table.ctypes.data, table.shape[1], table.shape[0]))
        self.S, self.K = table.shape[:2]
        self.table = pair

    def probes(self, probes, seed, params, records=True):
        """(moved probes, records) of host probes — the dtype and shape of `probes`, record_dtype of the same shape (None without
        `records`); waits for the context's stream"""
        probes, p = _probes(probes), _params(params, self.K)
        moved = np.zeros(probes.shape, probes.dtype)
        out = np.zeros(probes.shape, record_dtype) if records else None
        self._check(self.lib.hiprz_place_probes_host(self._place, probes.ctypes.data, probes.size, seed, p.ctypes.data, moved.ctypes.data, None if out is None else out.ctypes.data))
        return moved, out

    def probes_device(self, probes_ptr, n, out_probes_ptr, out_records_ptr, seed, params, stream=None):
        """enqueue only: n probes at the device address probes_ptr -> n moved probes at out_probes_ptr (which may be probes_ptr) and, unless
        out_records_ptr is None, n records of 32 bytes there"""
        p = _params(params, self.K)
        self._check(self.lib.hiprz_place_probes(self._place, probes_ptr, n, seed, p.ctypes.data, out_probes_ptr, out_records_ptr, stream))

    def probes_through_device(self, probes, seed, params, sync, in_place=False, records=True):
        """probes() by the device-pointer call on buffers of this call's own: `in_place` moves the probes where they lie, `records` False
        passes no record array.  `sync` waits for the context's stream (Context.sync: it also makes the head device current)."""
        probes = _probes(probes)
        if probes.size == 0:
            return np.zeros(probes.shape, probes.dtype), (np.zeros(probes.shape, record_dtype) if records else None)
        sync()
        bufs = [_hiprt.DeviceBuffer.of(probes)]
        if not in_place:
            bufs.append(_hiprt.DeviceBuffer(probes.size * 32))
        if records:
            bufs.append(_hiprt.DeviceBuffer(probes.size * 32))
        try:
            self.probes_device(bufs[0].ptr, probes.size, bufs[0 if in_place else 1].ptr, bufs[-1].ptr if records else None, seed, params)
            sync()
            return bufs[0 if in_place else 1].download(probes.shape, probes.dtype), (bufs[-1].download(probes.shape, record_dtype) if records else None)
        finally:
            for b in bufs:
                b.free()
