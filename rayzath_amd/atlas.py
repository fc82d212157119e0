"""Loader and ctypes mirror of bake atlases (include/hiprz_atlas.h, rayzath_amd/csrc/libhiprz_atlas.so): UV charts rasterised on the device
into one surface point per texel of a W x H atlas (bake.point_dtype, ready for hiprz_bake_occlusion) and the dilation that fills the
gutters of what was baked.  As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _abi, _satellite
from .bake import point_dtype

LIB_PATH = _satellite.lib_path("HIPRZ_ATLAS_LIB", "libhiprz_atlas.so")
NONE = 0xFFFFFFFF                                 # HIPRZ_ATLAS_NONE
MAX_SIZE, MAX_RINGS = 16384, 64

# hiprz_atlas_tri: (p1.xyz, u1) (p2.xyz, u2) (p3.xyz, u3) (n1.xyz, v1) (n2.xyz, v2) (n3.xyz, v3)
tri_dtype = np.dtype([("p1", "<f4", 3), ("u1", "<f4"), ("p2", "<f4", 3), ("u2", "<f4"), ("p3", "<f4", 3), ("u3", "<f4"),
                      ("n1", "<f4", 3), ("v1", "<f4"), ("n2", "<f4", 3), ("v2", "<f4"), ("n3", "<f4", 3), ("v3", "<f4")])
sample_dtype = np.dtype([("triangle", "<u4"), ("bx", "<f4"), ("by", "<f4"), ("zero", "<u4")])                  # hiprz_atlas_sample
assert tri_dtype.itemsize == 96 and sample_dtype.itemsize == 16

P, U32, SZ, F32 = C.c_void_p, C.c_uint32, C.c_size_t, C.c_float
ENTRY_POINTS = {
    "hiprz_atlas_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_atlas_destroy": (C.c_int, [P]),
    "hiprz_atlas_last_error": (C.c_char_p, [P]),
    "hiprz_atlas_layout": (None, [P]),
    "hiprz_atlas_begin": (C.c_int, [P, U32, U32]),
    "hiprz_atlas_add": (C.c_int, [P, P, SZ, U32, U32, F32, F32, P]),
    "hiprz_atlas_add_host": (C.c_int, [P, P, SZ, U32, U32, F32, F32]),
    "hiprz_atlas_points_device": (P, [P]),
    "hiprz_atlas_samples_device": (P, [P]),
    "hiprz_atlas_read_host": (C.c_int, [P, P, P]),
    "hiprz_atlas_records_device": (P, [P]),
    "hiprz_atlas_read_records_host": (C.c_int, [P, P, P]),
    "hiprz_atlas_dilate": (C.c_int, [P, P, U32, P, P]),
    "hiprz_atlas_dilate_host": (C.c_int, [P, P, U32, P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


def charts(mesh, texcrds=None, tri_texcrds=None):
    """an array of tri_dtype, one record per triangle of the scene.Mesh `mesh` in its own order: the mesh's positions and normals (zeros
    where a triangle has none: the face normal is used) and, as atlas coordinates, the mesh's own UVs or a second set — `texcrds` (n, 2)
    with `tri_texcrds` (T, 3) indices into it (the mesh's own indices when only `texcrds` is given)"""
    uv = mesh.texcrds if texcrds is None else np.ascontiguousarray(texcrds, np.float32).reshape(-1, 2)
    ids = mesh.tri_texcrds if tri_texcrds is None else np.ascontiguousarray(tri_texcrds, np.uint32).reshape(-1, 3)
    T = len(mesh.tri_vertices)
    if len(ids) != T:
        raise ValueError(f"{len(ids)} texture-coordinate triples for {T} triangles")
    if T and (ids == _abi.IDS_UNUSED).all(-1).any():
        raise ValueError("a triangle has no texture coordinates: an atlas needs a UV for every vertex")
    if T and int(ids.max()) >= len(uv):
        raise ValueError("a texture-coordinate index is out of range")
    out = np.zeros(T, tri_dtype)
    has_normals = ~(mesh.tri_normals == _abi.IDS_UNUSED).all(-1)
    for k in range(3):
        out[f"p{k + 1}"] = mesh.vertices[mesh.tri_vertices[:, k]]
        out[f"u{k + 1}"], out[f"v{k + 1}"] = uv[ids[:, k], 0], uv[ids[:, k], 1]
        if has_normals.any():
            out[f"n{k + 1}"][has_normals] = mesh.normals[mesh.tri_normals[has_normals, k]]
    return out


def _tris(tris):
    tris = np.ascontiguousarray(tris)
    if tris.dtype != tri_dtype:
        raise TypeError("charts must be an array of rayzath_amd.atlas.tri_dtype")
    return tris.reshape(-1)


class Atlas(_satellite.Handle):
    """Owns one hiprz_atlas bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _atlas = property(lambda self: self._handle)

    def __init__(self, ctx_ptr):
        self.width = self.height = 0
        super().__init__(load(), "atlas", ctx_ptr)

    def begin(self, width, height):
        """a new atlas of width x height texels; the next add clears it"""
        self._check(self.lib.hiprz_atlas_begin(self._atlas, width, height))
        self.width, self.height = int(width), int(height)

    def add(self, tris, triangle_base=0, instance=0, near=1.0e-3, far=3.0e38):
        """host triangles (tri_dtype) with the ids triangle_base + i, placed as instance `instance` is in the context now"""
        tris = _tris(tris)
        self._check(self.lib.hiprz_atlas_add_host(self._atlas, tris.ctypes.data, tris.size, triangle_base, instance, near, far))

    def add_device(self, tris_ptr, n, triangle_base=0, instance=0, near=1.0e-3, far=3.0e38, stream=None):
        """enqueue only: n hiprz_atlas_tri at the device address tris_ptr"""
        self._check(self.lib.hiprz_atlas_add(self._atlas, tris_ptr, n, triangle_base, instance, near, far, stream))

    def points_device(self):
        """the device address of the W*H points (bake.point_dtype), valid until the next begin or close; None before the first add"""
        return self.lib.hiprz_atlas_points_device(self._atlas)

    def samples_device(self):
        return self.lib.hiprz_atlas_samples_device(self._atlas)

    def read(self, points=True, samples=True):
        """(points, samples) of shape (H, W) from the device (None for the one not asked for); waits for the context's stream"""
        shape = (self.height, self.width)
        p = np.zeros(shape, point_dtype) if points else None
        s = np.zeros(shape, sample_dtype) if samples else None
        self._check(self.lib.hiprz_atlas_read_host(self._atlas, p.ctypes.data if points else None, s.ctypes.data if samples else None))
        return p, s

    def records_device(self):
        """the device address of the handle's own W*H 16-byte records (for what is baked per texel), valid as points_device"""
        return self.lib.hiprz_atlas_records_device(self._atlas)

    def read_records(self, dtype, ring=True):
        """(the handle's records as (H, W) of the 16-byte `dtype`, the ring map of the last dilation or None); waits for the context's stream"""
        records = np.zeros((self.height, self.width), dtype)
        assert records.dtype.itemsize == 16
        rings = np.zeros((self.height, self.width), np.uint32) if ring else None
        self._check(self.lib.hiprz_atlas_read_records_host(self._atlas, records.ctypes.data, rings.ctypes.data if ring else None))
        return records, rings

    def dilate_device(self, records_ptr, rings, ring_out_ptr=None, stream=None):
        """enqueue only: `rings` rings of dilation in place on the W*H 16-byte records at the device address records_ptr"""
        self._check(self.lib.hiprz_atlas_dilate(self._atlas, records_ptr, rings, ring_out_ptr, stream))

    def dilate(self, records, rings):
        """(records dilated by `rings` rings, the ring map (H, W) uint32) of a host array of W*H 16-byte records; `records` is not changed"""
        records = np.ascontiguousarray(records)
        if records.dtype.itemsize != 16 or records.size != self.width * self.height:
            raise TypeError("records must be W*H records of 16 bytes")
        out, ring = records.copy(), np.zeros((self.height, self.width), np.uint32)
        self._check(self.lib.hiprz_atlas_dilate_host(self._atlas, out.ctypes.data, rings, ring.ctypes.data))
        return out, ring


def build(atlas, parts, width, height, near, far):
    """begin + one add per (instance_index, charts) pair of `parts`, ids numbered through in the order of the list"""
    atlas.begin(width, height)
    base = 0
    for instance, tris in parts:
        tris = _tris(tris)
        atlas.add(tris, base, instance, near, far)
        base += tris.size
    if not parts:
        raise ValueError("an atlas needs at least one (instance, charts) pair")


def bake(atlas, baker, rings, seed):
    """the atlas's points baked where they lie, into the handle's own records, and those dilated by `rings` rings: (texels, ring) of shape
    (H, W).  Waits for the context's stream."""
    from .bake import texel_dtype
    baker.occlusion_device(atlas.points_device(), atlas.width * atlas.height, atlas.records_device(), seed)
    atlas.dilate_device(atlas.records_device(), rings)
    return atlas.read_records(texel_dtype)


def bake_light(atlas, lighter, rings, seed, lights=None, smoother=None, smooth=None):
    """the atlas's points light-baked (light.Light `lighter`) where they lie, into the handle's own records, and those dilated by `rings`
    rings: (texels, ring) of shape (H, W).  smooth: None, or the params of smooth.Smooth `smoother`, which then smooths the records in
    place between the bake and the dilation.  Waits for the context's stream."""
    from .light import texel_dtype
    lighter.bake_device(atlas.points_device(), atlas.width * atlas.height, atlas.records_device(), seed, lights)
    if smooth is not None:
        smoother.texels_device(atlas.points_device(), atlas.records_device(), atlas.width, atlas.height, smooth)
    atlas.dilate_device(atlas.records_device(), rings)
    return atlas.read_records(texel_dtype)


def bake_bounce(atlas, lighter, gatherer, albedo, emission, bounces, rings, seed, lights, sky, sync, then=None, smoother=None, smooth=None):
    """the atlas's points light-baked (light.Light `lighter`) and then, `bounces` times: the source albedo * (direct + indirect) + emission
    composed per texel, dilated by `rings` rings and gathered (gather.Gather `gatherer`, its chart map set for this atlas) back at the
    points.  Points, sources and texels stay on the device; albedo and emission are (H, W) arrays of 16-byte records (emission may be
    None).  (direct, indirect, ring) of shape (H, W), both dilated: light.texel_dtype, gather.texel_dtype and the ring map.  `sync` waits
    for the context's stream.  then: called as then(source_ptr) once the last bounce is gathered, with the source that gather read — composed,
    dilated and still on the device; what it enqueues is waited for with the rest and the value it returns (a function of no arguments
    is called after the wait) is returned as a fourth item.  smooth: None, or the params of smooth.Smooth `smoother`, which then smooths
    in place, where they lie: direct once, right after its bake (before any source is composed from it, and so before its dilation), and
    every bounce's indirect right after its gather (before it is composed into the next source; the last before its dilation)."""
    from . import _hiprt
    from .gather import texel_dtype as gathered_dtype
    from .light import texel_dtype as light_dtype
    if bounces < 1:
        raise ValueError("a bounce bake takes at least one bounce")
    shape, n = (atlas.height, atlas.width), atlas.width * atlas.height
    for a in (albedo, emission):
        if a is not None and (a.dtype.itemsize != 16 or a.shape != shape):
            raise TypeError("albedo and emission must be (H, W) arrays of 16-byte records")
    sync()
    bufs = []
    try:
        direct, indirect, source, ring = (_hiprt.DeviceBuffer(n * size) for size in (16, 16, 16, 4))
        bufs += [direct, indirect, source, ring]
        d_albedo = _hiprt.DeviceBuffer.of(albedo)
        bufs.append(d_albedo)
        d_emission = None if emission is None else _hiprt.DeviceBuffer.of(emission)
        bufs.append(d_emission)
        points = atlas.points_device()
        lighter.bake_device(points, n, direct.ptr, seed, lights)
        if smooth is not None:
            smoother.texels_device(points, direct.ptr, atlas.width, atlas.height, smooth)
        gathered = None
        for _ in range(bounces):
            gatherer.compose_device(direct.ptr, gathered, d_albedo.ptr, None if d_emission is None else d_emission.ptr, source.ptr, n)
            atlas.dilate_device(source.ptr, rings)
            gatherer.texels_device(points, n, source.ptr, atlas.width, atlas.height, indirect.ptr, seed, sky)
            if smooth is not None:
                smoother.texels_device(points, indirect.ptr, atlas.width, atlas.height, smooth)
            gathered = indirect.ptr
        after = None if then is None else then(source.ptr)
        atlas.dilate_device(direct.ptr, rings)
        atlas.dilate_device(indirect.ptr, rings, ring.ptr)
        sync()
        baked = direct.download(shape, light_dtype), indirect.download(shape, gathered_dtype), ring.download(shape, np.uint32)
        return baked if then is None else baked + (after() if callable(after) else after,)
    finally:
        for b in bufs:
            if b is not None:
                b.free()
