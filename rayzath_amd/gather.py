"""Loader and ctypes mirror of bounce baking (include/hiprz_gather.h, rayzath_amd/csrc/libhiprz_gather.so): per surface point, K hemisphere
rays made from a table of directions, walked to their closest hits and looked up in an atlas that already holds light — the mean of what
the point sees, and how many rays read a texel or missed.  As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _abi, _hiprt, _satellite
from .bake import cosine_directions, point_dtype
from .query import ray_dtype

LIB_PATH = _satellite.lib_path("HIPRZ_GATHER_LIB", "libhiprz_gather.so")
INVALID = 0x80000000                              # HIPRZ_GATHER_INVALID: a texel without a value, the counts of an invalid point
NONE = 0xFFFFFFFF                                 # HIPRZ_GATHER_NONE: the base of an instance that is not in the atlas
MISS, UNMAPPED, BACK, INVALID_RAY = 0xFFFFFFFF, 0xFFFFFFFE, 0xFFFFFFFD, 0xFFFFFFFC      # the codes of hiprz_gather_sample::id
MAX_CHARTS, MAX_SIZE = 0xFFFFFFFC, 16384

texel_dtype = np.dtype([("mean", "<f4", 3), ("counts", "<u4")])                                               # hiprz_gather_texel
sample_dtype = np.dtype([("id", "<u4"), ("bx", "<f4"), ("by", "<f4"), ("t", "<f4")])                          # hiprz_gather_sample
chart_dtype = np.dtype([("u1", "<f4"), ("v1", "<f4"), ("u2", "<f4"), ("v2", "<f4"), ("u3", "<f4"), ("v3", "<f4"), ("zero", "<f4", 2)])  # hiprz_gather_chart
record_dtype = np.dtype([("rgb", "<f4", 3), ("word", "<u4")])                                                 # a source, albedo or emission record
assert texel_dtype.itemsize == 16 and sample_dtype.itemsize == 16 and chart_dtype.itemsize == 32 and record_dtype.itemsize == 16

P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t
ENTRY_POINTS = {
    "hiprz_gather_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_gather_destroy": (C.c_int, [P]),
    "hiprz_gather_last_error": (C.c_char_p, [P]),
    "hiprz_gather_set_directions": (C.c_int, [P, P, U32, U32]),
    "hiprz_gather_set_charts": (C.c_int, [P, P, U32, P, U32]),
    "hiprz_gather_texels": (C.c_int, [P, P, SZ, U32, P, U32, U32, P, P, P]),
    "hiprz_gather_samples": (C.c_int, [P, P, SZ, U32, P, P]),
    "hiprz_gather_texels_host": (C.c_int, [P, P, SZ, U32, P, U32, U32, P, P]),
    "hiprz_gather_compose": (C.c_int, [P, P, P, P, P, P, SZ, P]),
    "hiprz_gather_compose_host": (C.c_int, [P, P, P, P, P, P, SZ]),
    "hiprz_gather_layout": (None, [P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


def chart_tables(parts, n_instances):
    """(base, uv) for Gather.set_charts from the `parts` list of an atlas — (instance_index, charts) pairs, charts an array of
    atlas.tri_dtype in the mesh's own triangle order, numbered through in list order as atlas.build numbers them: base[i] is the id of the
    first triangle of instance i (NONE for an instance no part names), uv the chart_dtype record of every id"""
    from .atlas import tri_dtype
    base = np.full(n_instances, NONE, np.uint32)
    chunks, at = [], 0
    for instance, tris in parts:
        tris = np.ascontiguousarray(tris).reshape(-1)
        if tris.dtype != tri_dtype:
            raise TypeError("charts must be an array of rayzath_amd.atlas.tri_dtype")
        if not 0 <= instance < n_instances:
            raise ValueError(f"instance {instance} of a part is not one of the scene's {n_instances}")
        if base[instance] != NONE:
            raise ValueError(f"instance {instance} is in two parts: a hit on it has one chart id")
        base[instance] = at
        uv = np.zeros(tris.size, chart_dtype)
        for name in ("u1", "v1", "u2", "v2", "u3", "v3"):
            uv[name] = tris[name]
        chunks.append(uv)
        at += tris.size
    return base, (np.concatenate(chunks) if chunks else np.zeros(0, chart_dtype))


def records(rgb, shape, word=0):
    """an array of record_dtype of `shape` from a colour (3,) or an array shape + (3,); an array of 16-byte records passes through"""
    rgb = np.asarray(rgb)
    if rgb.dtype.itemsize == 16 and rgb.dtype.fields:
        if rgb.shape != tuple(shape):
            raise ValueError(f"records of shape {rgb.shape} for {tuple(shape)}")
        return np.ascontiguousarray(rgb)
    out = np.zeros(shape, record_dtype)
    out["rgb"], out["word"] = np.asarray(rgb, np.float32), word
    return out


def _sky(sky):
    sky = np.ascontiguousarray(sky, np.float32)
    if sky.shape != (3,):
        raise TypeError("sky must be three floats")
    return sky


class Gather(_satellite.Handle):
    """Owns one hiprz_gather bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _gather = property(lambda self: self._handle)

    def __init__(self, ctx_ptr):
        self.K = self.S = 0
        self.table = None         # the (K, S) of a cosine table set through set_directions, None for a caller's array or none
        super().__init__(load(), "gather", ctx_ptr)

    def set_directions(self, directions):
        """directions: an (S, K, 4) float32 array of unit vectors in the local frame (z along the normal), or a (K, S) pair for the bake's
        cosine table"""
        pair = tuple(directions) if isinstance(directions, tuple) else None
        if pair is not None:
            directions = cosine_directions(*pair)
        table = np.ascontiguousarray(directions, np.float32)
        if table.ndim != 3 or table.shape[2] != 4:
            raise TypeError("directions must be an (S, K, 4) float32 array or a (K, S) pair")
        self._check(self.lib.hiprz_gather_set_directions(self._gather, table.ctypes.data, table.shape[1], table.shape[0]))
        self.S, self.K = table.shape[:2]
        self.table = pair

    def set_charts(self, base, uv):
        """the chart map: base (n_instances,) uint32 and uv (n_charts,) chart_dtype — chart_tables(parts, n_instances)"""
        base, uv = np.ascontiguousarray(base, np.uint32).reshape(-1), np.ascontiguousarray(uv).reshape(-1)
        if uv.dtype != chart_dtype:
            raise TypeError("uv must be an array of rayzath_amd.gather.chart_dtype")
        self._check(self.lib.hiprz_gather_set_charts(self._gather, base.ctypes.data if base.size else None, base.size, uv.ctypes.data if uv.size else None, uv.size))

    @staticmethod
    def _points(points):
        points = np.ascontiguousarray(points)
        if points.dtype not in (point_dtype, ray_dtype):      # a point is the ray along its normal: the same 32 bytes
            raise TypeError("points must be an array of rayzath_amd.bake.point_dtype")
        return points

    def texels(self, points, source, W, H, seed=0, sky=(0.0, 0.0, 0.0)):
        """texels (texel_dtype, the shape of `points`) of host points over a host source of W*H 16-byte records; waits for the context's stream"""
        points, source, sky = self._points(points), np.ascontiguousarray(source), _sky(sky)
        if source.dtype.itemsize != 16 or source.size != W * H:
            raise TypeError("source must be W*H records of 16 bytes")
        out = np.zeros(points.shape, texel_dtype)
        self._check(self.lib.hiprz_gather_texels_host(self._gather, points.ctypes.data, points.size, seed, source.ctypes.data, W, H, sky.ctypes.data, out.ctypes.data))
        return out

    def texels_device(self, points_ptr, n, source_ptr, W, H, out_ptr, seed=0, sky=(0.0, 0.0, 0.0), stream=None):
        """enqueue only: n points at the device address points_ptr, the W*H records at source_ptr -> n texels at out_ptr"""
        sky = _sky(sky)
        self._check(self.lib.hiprz_gather_texels(self._gather, points_ptr, n, seed, source_ptr, W, H, sky.ctypes.data, out_ptr, stream))

    def samples_device(self, points_ptr, n, samples_ptr, seed=0, stream=None):
        """enqueue only: the n * K samples the gather walks for n device points, sample i * K + k of (point i, direction k), to samples_ptr"""
        self._check(self.lib.hiprz_gather_samples(self._gather, points_ptr, n, seed, samples_ptr, stream))

    def samples(self, points, seed, sync):
        """the samples of host points as an array of sample_dtype of shape points.shape + (K,).  `sync` waits for the context's stream
        (Context.sync: it also makes the head device current for the buffers)."""
        points = self._points(points)
        n = points.size
        if n == 0 or not self.K:
            dummy = (C.c_uint8 * 32)()
            self._check(self.lib.hiprz_gather_samples(self._gather, dummy, 0, seed, dummy, None))  # without a table or a map: refused; else nothing to do
            return np.zeros(points.shape + (self.K,), sample_dtype)
        sync()
        d_points, d_samples = _hiprt.DeviceBuffer.of(points), _hiprt.DeviceBuffer(n * self.K * sample_dtype.itemsize)
        try:
            self.samples_device(d_points.ptr, n, d_samples.ptr, seed)
            sync()
            return d_samples.download(points.shape + (self.K,), sample_dtype)
        finally:
            d_points.free(), d_samples.free()

    def compose_device(self, direct_ptr, indirect_ptr, albedo_ptr, emission_ptr, out_ptr, n_texels, stream=None):
        """enqueue only: out = albedo * (direct + indirect) + emission per texel, the word of `direct`; indirect_ptr and emission_ptr may be None"""
        self._check(self.lib.hiprz_gather_compose(self._gather, direct_ptr, indirect_ptr, albedo_ptr, emission_ptr, out_ptr, n_texels, stream))

    def compose(self, direct, indirect, albedo, emission, sync):
        """compose_device for host arrays of 16-byte records of one shape (indirect and emission may be None): record_dtype of that shape"""
        direct = np.ascontiguousarray(direct)
        arrays = [direct] + [None if a is None else np.ascontiguousarray(a) for a in (indirect, albedo, emission)]
        for a in arrays:
            if a is not None and (a.dtype.itemsize != 16 or a.shape != direct.shape):
                raise TypeError("compose takes arrays of 16-byte records of one shape")
        sync()
        bufs = [None if a is None else _hiprt.DeviceBuffer.of(a) for a in arrays] + [_hiprt.DeviceBuffer(max(direct.nbytes, 16))]
        try:
            self.compose_device(*[None if b is None else b.ptr for b in bufs], direct.size)
            sync()
            return bufs[-1].download(direct.shape, record_dtype)
        finally:
            for b in bufs:
                if b is not None:
                    b.free()
