"""Loader and ctypes mirror of probe baking (include/hiprz_probe.h, rayzath_amd/csrc/libhiprz_probe.so): per probe — a point of free space —
K rays over the whole sphere walked to their closest hits and looked up in an atlas that already holds light, plus the scene's own lights
with their shadows, projected onto nine spherical-harmonic coefficients per colour; the evaluation of such a record for a normal, and a
regular grid of probes with its trilinear blend.  As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _abi, _hiprt, _satellite
from .bake import point_dtype
from .gather import _sky, chart_dtype, sample_dtype
from .light import disk_samples, light_range
from .query import ray_dtype

LIB_PATH = _satellite.lib_path("HIPRZ_PROBE_LIB", "libhiprz_probe.so")
INVALID = 0x80000000                              # HIPRZ_PROBE_INVALID: sh[0].w of an invalid probe
MAX_SIZE = 16384

sh_dtype = np.dtype([("sh", "<f4", (9, 4))])      # hiprz_probe_sh: [b] = (r, g, b, word)
assert sh_dtype.itemsize == 144
WEIGHTS = np.array([1.0, 2.0, 2.0, 2.0, 3.75, 3.75, 0.3125, 3.75, 0.9375], np.float32)      # include/hiprz_probe.h "THE EVALUATION"

P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t
ENTRY_POINTS = {
    "hiprz_probe_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_probe_destroy": (C.c_int, [P]),
    "hiprz_probe_last_error": (C.c_char_p, [P]),
    "hiprz_probe_set_directions": (C.c_int, [P, P, U32, U32]),
    "hiprz_probe_set_samples": (C.c_int, [P, P, U32, U32]),
    "hiprz_probe_set_charts": (C.c_int, [P, P, U32, P, U32]),
    "hiprz_probe_sphere_directions": (C.c_int, [U32, U32, P]),
    "hiprz_probe_irradiance": (None, [P, P, P]),
    "hiprz_probe_gather": (C.c_int, [P, P, SZ, U32, P, U32, U32, P, P, P]),
    "hiprz_probe_samples": (C.c_int, [P, P, SZ, U32, P, P]),
    "hiprz_probe_light": (C.c_int, [P, P, SZ, U32, P, P, P, P]),
    "hiprz_probe_gather_host": (C.c_int, [P, P, SZ, U32, P, U32, U32, P, P]),
    "hiprz_probe_light_host": (C.c_int, [P, P, SZ, U32, P, P, P]),
    "hiprz_probe_layout": (None, [P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


def sphere_directions(K, S):
    """the library's table of S sets of K directions uniform on the whole sphere: (S, K, 4) float32, w = 0"""
    out = np.zeros((S, K, 4), np.float32)
    if load().hiprz_probe_sphere_directions(K, S, out.ctypes.data) != _abi.OK:
        raise ValueError(f"K = {K} is not one of 16, 32, ..., 1024 or S = {S} is not in 1..64")
    return out


def words(sh):
    """(counts, shadowed) of records: sh[0].w and sh[1].w as uint32"""
    w = np.ascontiguousarray(sh).view(sh_dtype)["sh"][..., 3].view(np.uint32)
    return w[..., 0], w[..., 1]


def basis(d):
    """include/hiprz_probe.h "THE BASIS" on directions (..., 3), in their dtype, one rounding per operation: (..., 9)"""
    d = np.asarray(d)
    T = d.dtype.type
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.ones_like(x), y, z, x, x * y, y * z, (T(3.0) * (z * z)) - T(1.0), x * z, (x * x) - (y * y)], -1)


def irradiance(sh, normals):
    """E(n) of records `sh` (sh_dtype, any shape) for unit normals of shape sh.shape + (3,) (or (3,) for all): float32 of shape
    sh.shape + (3,), by the header's float32 rule — e = +0, then e = e + ((w_b * sh[b].c) * B_b(n)) for b = 0 .. 8.  An invalid record
    reads 0.  Host numpy."""
    rec = np.ascontiguousarray(sh).view(sh_dtype)
    coeff = rec["sh"][..., :3]                                                       # (..., 9, 3)
    B = basis(np.broadcast_to(np.asarray(normals, np.float32), rec.shape + (3,)))    # (..., 9)
    e = np.zeros(rec.shape + (3,), np.float32)
    with np.errstate(all="ignore"):
        for b in range(9):
            e = e + ((WEIGHTS[b] * coeff[..., b, :]) * B[..., b, None])
    e[words(rec)[0] == INVALID] = 0.0
    return e


def grid(lo, hi, shape, axis=(0.0, 1.0, 0.0), near=1.0e-3, far=3.0e38):
    """probes (bake.point_dtype) of shape `shape` = (nx, ny, nz) on the regular grid from corner `lo` to corner `hi` inclusive (a count of
    1 along an axis sits at lo); `axis` is every probe's frame axis.  Probe [i, j, k] is at lo + (i, j, k) * (hi - lo) / (shape - 1)."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError("shape must be three counts of at least 1")
    axes = [lo[a] + (hi[a] - lo[a]) * (np.arange(shape[a]) / max(shape[a] - 1, 1)) for a in range(3)]
    out = np.zeros(shape, point_dtype)
    out["position"] = np.stack(np.meshgrid(*axes, indexing="ij"), -1).astype(np.float32)
    out["normal"], out["near"], out["far"] = np.asarray(axis, np.float32), near, far
    return out


class Field:
    """The records `sh` (sh_dtype of shape (nx, ny, nz)) of the probes of grid(lo, hi, shape).  Host numpy: there is no device-side evaluation."""

    def __init__(self, lo, hi, shape, sh):
        self.lo, self.hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
        self.shape = tuple(int(v) for v in shape)
        self.sh = np.ascontiguousarray(sh).view(sh_dtype).reshape(self.shape)

    def blend(self, positions):
        """the records at `positions` (..., 3): the coefficients of the eight surrounding probes blended trilinearly in float32 (positions
        outside the grid clamp to it), invalid probes left out and the weights renormalised; a position all of whose probes are invalid
        reads the invalid record.  The words of a blended record are 0."""
        pos = np.asarray(positions, np.float64)
        cell, frac = [], []
        for a in range(3):
            n = self.shape[a]
            span = self.hi[a] - self.lo[a]
            g = np.clip((pos[..., a] - self.lo[a]) / span * (n - 1), 0.0, n - 1.0) if n > 1 and span != 0 else np.zeros(pos.shape[:-1])
            i = np.minimum(np.floor(g).astype(np.int64), max(n - 2, 0))
            cell.append(i), frac.append((g - i).astype(np.float32))
        ok = words(self.sh)[0] != INVALID
        total = np.zeros(pos.shape[:-1] + (9, 3), np.float32)
        weight = np.zeros(pos.shape[:-1], np.float32)
        one = np.float32(1.0)
        for corner in range(8):
            idx, w = [], one
            for a in range(3):
                up = (corner >> a) & 1
                idx.append(np.minimum(cell[a] + up, self.shape[a] - 1))
                w = w * (frac[a] if up else one - frac[a])
            w = np.where(ok[tuple(idx)], w, np.float32(0.0)).astype(np.float32)
            total = total + w[..., None, None] * self.sh["sh"][tuple(idx)][..., :3]
            weight = weight + w
        out = np.zeros(pos.shape[:-1], sh_dtype)
        with np.errstate(all="ignore"):
            out["sh"][..., :3] = np.where(weight[..., None, None] > 0, total / weight[..., None, None], np.float32(0.0))
        out["sh"][..., 0, 3] = np.where(weight > 0, np.uint32(0), np.uint32(INVALID)).astype(np.uint32).view(np.float32)
        return out

    def irradiance(self, positions, normals):
        """E(n) at `positions` (..., 3) for unit `normals` (..., 3): blend(), then irradiance()"""
        return irradiance(self.blend(positions), normals)


class Probe(_satellite.Handle):
    """Owns one hiprz_probe bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _probe = property(lambda self: self._handle)

    def __init__(self, ctx_ptr):
        self.K = self.S = self.LK = self.LS = 0
        self.table = None         # the (K, S) of a sphere table set through set_directions, None for a caller's array or none
        self.disk = None          # the (K, S) of a disk table set through set_samples
        super().__init__(load(), "probe", ctx_ptr)

    def set_directions(self, directions):
        """directions: an (S, K, 4) float32 array of unit vectors in the probe's frame, or a (K, S) pair for the library's sphere table"""
        pair = tuple(directions) if isinstance(directions, tuple) else None
        if pair is not None:
            directions = sphere_directions(*pair)
        table = np.ascontiguousarray(directions, np.float32)
        if table.ndim != 3 or table.shape[2] != 4:
            raise TypeError("directions must be an (S, K, 4) float32 array or a (K, S) pair")
        self._check(self.lib.hiprz_probe_set_directions(self._probe, table.ctypes.data, table.shape[1], table.shape[0]))
        self.S, self.K = table.shape[:2]
        self.table = pair

    def set_samples(self, samples):
        """samples: an (S, K, 2) float32 array of points of the unit disk, or a (K, S) pair for the light library's disk table"""
        pair = tuple(samples) if isinstance(samples, tuple) else None
        if pair is not None:
            samples = disk_samples(*pair)
        table = np.ascontiguousarray(samples, np.float32)
        if table.ndim != 3 or table.shape[2] != 2:
            raise TypeError("samples must be an (S, K, 2) float32 array or a (K, S) pair")
        self._check(self.lib.hiprz_probe_set_samples(self._probe, table.ctypes.data, table.shape[1], table.shape[0]))
        self.LS, self.LK = table.shape[:2]
        self.disk = pair

    def set_charts(self, base, uv):
        """the chart map: base (n_instances,) uint32 and uv (n_charts,) gather.chart_dtype — gather.chart_tables(parts, n_instances)"""
        base, uv = np.ascontiguousarray(base, np.uint32).reshape(-1), np.ascontiguousarray(uv).reshape(-1)
        if uv.dtype != chart_dtype:
            raise TypeError("uv must be an array of rayzath_amd.gather.chart_dtype")
        self._check(self.lib.hiprz_probe_set_charts(self._probe, base.ctypes.data if base.size else None, base.size, uv.ctypes.data if uv.size else None, uv.size))

    @staticmethod
    def _probes(probes):
        probes = np.ascontiguousarray(probes)
        if probes.dtype not in (point_dtype, ray_dtype):      # a probe is the ray along its axis: the same 32 bytes
            raise TypeError("probes must be an array of rayzath_amd.bake.point_dtype")
        return probes

    @staticmethod
    def _range_ptr(rng):
        return None if rng is None else rng.ctypes.data

    def gather(self, probes, source, W, H, seed=0, sky=(0.0, 0.0, 0.0)):
        """records (sh_dtype, the shape of `probes`) of host probes over a host source of W*H 16-byte records; waits for the context's stream"""
        probes, source, sky = self._probes(probes), np.ascontiguousarray(source), _sky(sky)
        if source.dtype.itemsize != 16 or source.size != W * H:
            raise TypeError("source must be W*H records of 16 bytes")
        out = np.zeros(probes.shape, sh_dtype)
        self._check(self.lib.hiprz_probe_gather_host(self._probe, probes.ctypes.data, probes.size, seed, source.ctypes.data, W, H, sky.ctypes.data, out.ctypes.data))
        return out

    def light(self, probes, seed=0, lights=None, base=None):
        """the light term of host probes added to the records `base` (None: to +0): sh_dtype of the shape of `probes`; waits for the
        context's stream"""
        probes, rng = self._probes(probes), light_range(lights)
        out = np.zeros(probes.shape, sh_dtype)
        if base is not None:
            base = np.ascontiguousarray(base)
            if base.dtype != sh_dtype or base.shape != probes.shape:
                raise TypeError("base must be records of rayzath_amd.probe.sh_dtype of the probes' shape")
        self._check(self.lib.hiprz_probe_light_host(self._probe, probes.ctypes.data, probes.size, seed, self._range_ptr(rng), None if base is None else base.ctypes.data,
                                                    out.ctypes.data))
        return out

    def gather_device(self, probes_ptr, n, source_ptr, W, H, out_ptr, seed=0, sky=(0.0, 0.0, 0.0), stream=None):
        """enqueue only: n probes at the device address probes_ptr, the W*H records at source_ptr -> n records at out_ptr"""
        sky = _sky(sky)
        self._check(self.lib.hiprz_probe_gather(self._probe, probes_ptr, n, seed, source_ptr, W, H, sky.ctypes.data, out_ptr, stream))

    def light_device(self, probes_ptr, n, out_ptr, seed=0, lights=None, base_ptr=None, stream=None):
        """enqueue only: the light term of n device probes added to the records at base_ptr (None: to +0) -> n records at out_ptr, which
        may be base_ptr"""
        rng = light_range(lights)
        self._check(self.lib.hiprz_probe_light(self._probe, probes_ptr, n, seed, self._range_ptr(rng), base_ptr, out_ptr, stream))

    def samples_device(self, probes_ptr, n, samples_ptr, seed=0, stream=None):
        """enqueue only: the n * K samples the gather walks for n device probes, sample i * K + k of (probe i, direction k), to samples_ptr"""
        self._check(self.lib.hiprz_probe_samples(self._probe, probes_ptr, n, seed, samples_ptr, stream))

    def samples(self, probes, seed, sync):
        """the samples of host probes as an array of gather.sample_dtype of shape probes.shape + (K,).  `sync` waits for the context's
        stream (Context.sync: it also makes the head device current for the buffers)."""
        probes = self._probes(probes)
        n = probes.size
        if n == 0 or not self.K:
            dummy = (C.c_uint8 * 32)()
            self._check(self.lib.hiprz_probe_samples(self._probe, dummy, 0, seed, dummy, None))  # without a table or a map: refused; else nothing to do
            return np.zeros(probes.shape + (self.K,), sample_dtype)
        sync()
        d_probes, d_samples = _hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer(n * self.K * sample_dtype.itemsize)
        try:
            self.samples_device(d_probes.ptr, n, d_samples.ptr, seed)
            sync()
            return d_samples.download(probes.shape + (self.K,), sample_dtype)
        finally:
            d_probes.free(), d_samples.free()

    def bake_device(self, probes_ptr, n, source_ptr, W, H, out_ptr, seed=0, sky=(0.0, 0.0, 0.0), lights=None, direct=True, stream=None):
        """enqueue only: the gathered term of n device probes and, with `direct`, the light term on top of it in place — two launches, the
        records never visit the host between them"""
        self.gather_device(probes_ptr, n, source_ptr, W, H, out_ptr, seed, sky, stream)
        if direct:
            self.light_device(probes_ptr, n, out_ptr, seed, lights, out_ptr, stream)

    def bake(self, probes, source, W, H, seed, sky, lights, direct, sync):
        """bake_device for host probes and a host source: sh_dtype of the probes' shape"""
        probes, source = self._probes(probes), np.ascontiguousarray(source)
        if source.dtype.itemsize != 16 or source.size != W * H:
            raise TypeError("source must be W*H records of 16 bytes")
        n = probes.size
        if n == 0:
            return np.zeros(probes.shape, sh_dtype)
        sync()
        bufs = [_hiprt.DeviceBuffer.of(probes), _hiprt.DeviceBuffer.of(source), _hiprt.DeviceBuffer(n * sh_dtype.itemsize)]
        try:
            self.bake_device(bufs[0].ptr, n, bufs[1].ptr, W, H, bufs[2].ptr, seed, sky, lights, direct)
            sync()
            return bufs[2].download(probes.shape, sh_dtype)
        finally:
            for b in bufs:
                b.free()
