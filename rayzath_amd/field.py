"""Loader and ctypes mirror of probe fields (include/hiprz_field.h, rayzath_amd/csrc/libhiprz_field.so): a visibility map per probe — the
first two moments of the distance its rays see, per texel of an 8 x 8 octahedral map — and the lookup of a grid of baked probes for shaded
points on the device, each probe weighted by a Chebyshev test against its map so that a probe behind a wall does not leak through the
blend.  As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _abi, _hiprt, _satellite
from .bake import point_dtype
from .probe import sh_dtype, sphere_directions
from .query import ray_dtype

LIB_PATH = _satellite.lib_path("HIPRZ_FIELD_LIB", "libhiprz_field.so")
INVALID = 0x80000000                              # HIPRZ_FIELD_INVALID: words[3] of an invalid probe, the word of an invalid result
TEXELS = 64

vis_dtype = np.dtype([("moments", "<f4", (64, 2)), ("words", "<u4", (4,))])                                # hiprz_field_vis
grid_dtype = np.dtype([("lo", "<f4", (3,)), ("step", "<f4", (3,)), ("n", "<u4", (3,)), ("reserved", "<u4")])  # hiprz_field_grid
params_dtype = np.dtype([("bias", "<f4"), ("max_back", "<u4"), ("reserved", "<u4", (2,))])                  # hiprz_field_params
result_dtype = np.dtype([("rgb", "<f4", (3,)), ("word", "<u4")])                                            # hiprz_field_result
assert (vis_dtype.itemsize, grid_dtype.itemsize, params_dtype.itemsize, result_dtype.itemsize) == (528, 40, 16, 16)

P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t
ENTRY_POINTS = {
    "hiprz_field_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_field_destroy": (C.c_int, [P]),
    "hiprz_field_last_error": (C.c_char_p, [P]),
    "hiprz_field_set_directions": (C.c_int, [P, P, U32, U32]),
    "hiprz_field_texel_directions": (C.c_int, [P]),
    "hiprz_field_check_grid": (C.c_int, [P, SZ]),
    "hiprz_field_check_params": (C.c_int, [P]),
    "hiprz_field_visibility": (C.c_int, [P, P, SZ, U32, C.c_float, P, P]),
    "hiprz_field_visibility_host": (C.c_int, [P, P, SZ, U32, C.c_float, P]),
    "hiprz_field_lookup": (C.c_int, [P, P, P, P, P, SZ, P, P, SZ, P, P]),
    "hiprz_field_lookup_host": (C.c_int, [P, P, P, P, P, SZ, P, P, SZ, P]),
    "hiprz_field_layout": (None, [P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


def texel_directions():
    """the library's 64 texel directions, world axes: (64, 4) float32, w = 0; texel j = 8 * iy + ix"""
    out = np.zeros((64, 4), np.float32)
    load().hiprz_field_texel_directions(out.ctypes.data)
    return out


def params(bias=0.0, max_back=0):
    """a hiprz_field_params record (params_dtype, shape ()): the shaded point is moved `bias` along its normal before it is held against a
    visibility map; a probe more than `max_back` of whose rays hit back faces sits inside geometry and is left out.  ValueError for what
    hiprz_field_check_params refuses."""
    p = np.zeros((), params_dtype)
    if not 0 <= int(max_back) < 2 ** 32:
        raise ValueError(f"max_back = {max_back} is not a uint32")
    p["bias"], p["max_back"] = bias, int(max_back)
    if load().hiprz_field_check_params(p.ctypes.data) != _abi.OK:
        raise ValueError(f"bias = {bias} must be finite and >= 0")
    return p


def _params(p):
    """the record of `p`: None for the defaults, a params() record, or a mapping of params()'s keywords"""
    if p is None:
        return params()
    if isinstance(p, dict):
        return params(**p)
    p = np.ascontiguousarray(p)
    if p.dtype != params_dtype or p.size != 1:
        raise TypeError("params must be a rayzath_amd.field.params() record or a dict of its keywords")
    return p.reshape(())


def grid_of(lo, hi, shape):
    """the hiprz_field_grid record (grid_dtype, shape ()) of probe.grid(lo, hi, shape): counts `shape` = (nx, ny, nz), corner `lo`, the
    float32 step (hi - lo) / (shape - 1) per axis (0 where the count is 1).  ValueError for what hiprz_field_check_grid refuses."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("shape must be three counts of at least 1")
    g = np.zeros((), grid_dtype)
    g["lo"], g["n"] = lo, shape
    g["step"] = [(hi[a] - lo[a]) / (shape[a] - 1) if shape[a] > 1 else 0.0 for a in range(3)]
    if load().hiprz_field_check_grid(g.ctypes.data, int(np.prod(shape, dtype=np.int64))) != _abi.OK:
        raise ValueError(f"no grid from {lo} to {hi} of shape {shape}: every step must be finite and > 0, the count below 2^31")
    return g


def _grid(g):
    g = np.ascontiguousarray(g)
    if g.dtype != grid_dtype or g.size != 1:
        raise TypeError("grid must be a rayzath_amd.field.grid_of() record")
    return g.reshape(())


def layout():
    out = (U32 * 8)()
    load().hiprz_field_layout(out)
    return list(out)


def _points(points, what="points"):
    points = np.ascontiguousarray(points)
    if points.dtype not in (point_dtype, ray_dtype):      # a probe is the ray along its axis: the same 32 bytes
        raise TypeError(f"{what} must be an array of rayzath_amd.bake.point_dtype")
    return points


class Fielder(_satellite.Handle):
    """Owns one hiprz_field bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _field = property(lambda self: self._handle)

    def __init__(self, ctx_ptr):
        self.K = self.S = 0
        self.table = None         # the (K, S) of a sphere table set through set_directions, None for a caller's array or none
        super().__init__(load(), "field", ctx_ptr)

    def set_directions(self, directions):
        """directions: an (S, K, 4) float32 array of unit vectors in the probe's frame, or a (K, S) pair for the probe library's sphere
        table; K is one of 64 .. 1024"""
        pair = tuple(directions) if isinstance(directions, tuple) else None
        if pair is not None:
            if pair[0] < 64:
                raise ValueError(f"K = {pair[0]} is below 64: a 64-texel map needs at least a ray per texel")
            directions = sphere_directions(*pair)
        table = np.ascontiguousarray(directions, np.float32)
        if table.ndim != 3 or table.shape[2] != 4:
            raise TypeError("directions must be an (S, K, 4) float32 array or a (K, S) pair")
        self._check(self.lib.hiprz_field_set_directions(self._field, table.ctypes.data, table.shape[1], table.shape[0]))
        self.S, self.K = table.shape[:2]
        self.table = pair

    def visibility(self, probes, seed, reach):
        """the visibility records (vis_dtype, the shape of `probes`) of host probes; waits for the context's stream"""
        probes = _points(probes, "probes")
        out = np.zeros(probes.shape, vis_dtype)
        self._check(self.lib.hiprz_field_visibility_host(self._field, probes.ctypes.data, probes.size, seed, reach, out.ctypes.data))
        return out

    def visibility_device(self, probes_ptr, n, out_ptr, seed, reach, stream=None):
        """enqueue only: n probes at the device address probes_ptr -> n records of 528 bytes at out_ptr"""
        self._check(self.lib.hiprz_field_visibility(self._field, probes_ptr, n, seed, reach, out_ptr, stream))

    @staticmethod
    def _field_arrays(grid, probes, sh, vis):
        grid, probes, sh = _grid(grid), _points(probes, "probes").reshape(-1), np.ascontiguousarray(sh).reshape(-1)
        if sh.dtype != sh_dtype or sh.size != probes.size:
            raise TypeError("sh must be records of rayzath_amd.probe.sh_dtype, one per probe")
        if vis is not None:
            vis = np.ascontiguousarray(vis).reshape(-1)
            if vis.dtype != vis_dtype or vis.size != probes.size:
                raise TypeError("vis must be records of rayzath_amd.field.vis_dtype, one per probe")
        return grid, probes, sh, vis

    def lookup(self, grid, probes, sh, points, vis=None, params=None):
        """the results (result_dtype, the shape of `points`) of host points in a host field; waits for the context's stream"""
        grid, probes, sh, vis = self._field_arrays(grid, probes, sh, vis)
        points, p = _points(points), _params(params)
        out = np.zeros(points.shape, result_dtype)
        self._check(self.lib.hiprz_field_lookup_host(self._field, grid.ctypes.data, probes.ctypes.data, sh.ctypes.data, None if vis is None else vis.ctypes.data, probes.size,
                                                     p.ctypes.data, points.ctypes.data, points.size, out.ctypes.data))
        return out

    def lookup_device(self, grid, probes_ptr, sh_ptr, vis_ptr, n_probes, points_ptr, m, out_ptr, params=None, stream=None):
        """enqueue only: m points at points_ptr against the n_probes probes, records and (vis_ptr None: no) visibility records at their
        device addresses -> m results of 16 bytes at out_ptr"""
        grid, p = _grid(grid), _params(params)
        self._check(self.lib.hiprz_field_lookup(self._field, grid.ctypes.data, probes_ptr, sh_ptr, vis_ptr, n_probes, p.ctypes.data, points_ptr, m, out_ptr, stream))

    def lookup_through_device(self, grid, probes, sh, points, vis, params, sync):
        """lookup() by the device-pointer call on buffers of this call's own.  `sync` waits for the context's stream (Context.sync: it also
        makes the head device current for the buffers)."""
        grid, probes, sh, vis = self._field_arrays(grid, probes, sh, vis)
        points = _points(points)
        if points.size == 0:
            return np.zeros(points.shape, result_dtype)
        sync()
        bufs = [_hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer.of(sh), _hiprt.DeviceBuffer.of(points), _hiprt.DeviceBuffer(points.size * 16)]
        if vis is not None:
            bufs.append(_hiprt.DeviceBuffer.of(vis))
        try:
            self.lookup_device(grid, bufs[0].ptr, bufs[1].ptr, None if vis is None else bufs[4].ptr, probes.size, bufs[2].ptr, points.size, bufs[3].ptr, params)
            sync()
            return bufs[3].download(points.shape, result_dtype)
        finally:
            for b in bufs:
                b.free()
