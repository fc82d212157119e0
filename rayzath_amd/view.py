"""Loader and ctypes mirror of the baked view (include/hiprz_view.h, rayzath_amd/csrc/libhiprz_view.so): a frame of the selected camera
shaded on the device from a lit atlas — through the gather's chart map — and, for objects outside the atlas, from a probe field and the
surface's colour.  As with _lib.py there is no fallback: a missing library raises."""
import ctypes as C

import numpy as np

from . import _abi, _hiprt, _satellite
from .field import _grid, _points
from .field import _params as _field_params
from .field import vis_dtype
from .gather import _sky, chart_dtype, sample_dtype
from .probe import sh_dtype

LIB_PATH = _satellite.lib_path("HIPRZ_VIEW_LIB", "libhiprz_view.so")
NEAREST, BILINEAR = 0, 1                          # HIPRZ_VIEW_NEAREST, _BILINEAR
NONE, ATLAS, FIELD, SKY, BACK = 0, 1, 2, 3, 4     # the kinds of hiprz_view_pixel::word
KIND_SHIFT, COUNT_MASK = 28, 0x0FFFFFFF
FILTERS = {"nearest": NEAREST, "bilinear": BILINEAR}

pixel_dtype = np.dtype([("rgb", "<f4", (3,)), ("word", "<u4")])                     # hiprz_view_pixel
params_dtype = np.dtype([("filter", "<u4"), ("reserved", "<u4", (3,))])             # hiprz_view_params
assert pixel_dtype.itemsize == 16 and params_dtype.itemsize == 16


class FieldStruct(C.Structure):                                                    # hiprz_view_field
    _fields_ = [("grid", C.c_void_p), ("probes", C.c_void_p), ("sh", C.c_void_p), ("vis", C.c_void_p), ("n_probes", C.c_size_t), ("params", C.c_void_p)]


P, U32, SZ = C.c_void_p, C.c_uint32, C.c_size_t
ENTRY_POINTS = {
    "hiprz_view_create": (C.c_int, [C.POINTER(P), P]),
    "hiprz_view_destroy": (C.c_int, [P]),
    "hiprz_view_last_error": (C.c_char_p, [P]),
    "hiprz_view_set_charts": (C.c_int, [P, P, U32, P, U32]),
    "hiprz_view_check_params": (C.c_int, [P]),
    "hiprz_view_pixels": (C.c_int, [P, P, U32, U32, P, P, P, P, P, P]),
    "hiprz_view_samples": (C.c_int, [P, P, P]),
    "hiprz_view_pixels_host": (C.c_int, [P, P, U32, U32, P, P, P, P, P]),
    "hiprz_view_layout": (None, [P]),
}


def load():
    return _satellite.load(LIB_PATH, ENTRY_POINTS)


def params(filter="nearest"):
    """a hiprz_view_params record (params_dtype, shape ()): filter "nearest" (the gather's texel) or "bilinear" (four taps around the hit,
    taps without a value left out), or the code.  ValueError for what hiprz_view_check_params refuses."""
    p = np.zeros((), params_dtype)
    code = FILTERS.get(filter, filter)
    if isinstance(code, str) or not 0 <= int(code) < 2 ** 32:
        raise ValueError(f"filter = {filter!r} is neither 'nearest' nor 'bilinear'")
    p["filter"] = int(code)
    if load().hiprz_view_check_params(p.ctypes.data) != _abi.OK:
        raise ValueError(f"filter = {filter!r} is neither 'nearest' nor 'bilinear'")
    return p


def _params(p):
    """the record of `p`: None for the defaults, a params() record, a filter's name, or a mapping of params()'s keywords"""
    if p is None:
        return params()
    if isinstance(p, str):
        return params(p)
    if isinstance(p, dict):
        return params(**p)
    p = np.ascontiguousarray(p)
    if p.dtype != params_dtype or p.size != 1:
        raise TypeError("params must be a rayzath_amd.view.params() record, a filter's name or a dict of its keywords")
    return p.reshape(())


def kind(pixels):
    return np.asarray(pixels)["word"] >> np.uint32(KIND_SHIFT)


def count(pixels):
    return np.asarray(pixels)["word"] & np.uint32(COUNT_MASK)


def layout():
    out = (U32 * 8)()
    load().hiprz_view_layout(out)
    return list(out)


def field_arrays(field):
    """(grid, probes, sh, vis or None, field params) of a view's `field` = (grid, probes, sh, vis_or_None, field_params_or_None), checked"""
    if len(field) != 5:
        raise TypeError("field must be (grid, probes, sh, vis_or_None, field_params_or_None)")
    grid, probes, sh, vis, fp = field
    grid, probes, sh = _grid(grid), _points(probes, "probes").reshape(-1), np.ascontiguousarray(sh).reshape(-1)
    if sh.dtype != sh_dtype or sh.size != probes.size:
        raise TypeError("sh must be records of rayzath_amd.probe.sh_dtype, one per probe")
    if vis is not None:
        vis = np.ascontiguousarray(vis).reshape(-1)
        if vis.dtype != vis_dtype or vis.size != probes.size:
            raise TypeError("vis must be records of rayzath_amd.field.vis_dtype, one per probe")
    return grid, probes, sh, vis, _field_params(fp)


class View(_satellite.Handle):
    """Owns one hiprz_view bound to the hiprz_ctx `ctx_ptr`; close it before the context."""
    _view = property(lambda self: self._handle)

    def __init__(self, ctx_ptr):
        super().__init__(load(), "view", ctx_ptr)

    def set_charts(self, base, uv):
        """the chart map: base (n_instances,) uint32 and uv (n_charts,) gather.chart_dtype — gather.chart_tables(parts, n_instances)"""
        base, uv = np.ascontiguousarray(base, np.uint32).reshape(-1), np.ascontiguousarray(uv).reshape(-1)
        if uv.dtype != chart_dtype:
            raise TypeError("uv must be an array of rayzath_amd.gather.chart_dtype")
        self._check(self.lib.hiprz_view_set_charts(self._view, base.ctypes.data if base.size else None, base.size, uv.ctypes.data if uv.size else None, uv.size))

    def pixels_device(self, source_ptr, W, H, pixels_ptr, image_ptr=None, field=None, sky=(0.0, 0.0, 0.0), params=None, stream=None):
        """enqueue only: the frame of the selected camera from the W*H records at source_ptr -> one 16-byte record per pixel at pixels_ptr
        and / or a float4 (r, g, b, 1) per pixel at image_ptr.  field: None or (grid record, probes_ptr, sh_ptr, vis_ptr or None,
        n_probes, field params record or None), the three arrays on the device."""
        sky, p = _sky(sky), _params(params)
        f, keep = None, None
        if field is not None:
            grid, probes_ptr, sh_ptr, vis_ptr, n_probes, fp = field
            keep = (_grid(grid), _field_params(fp))
            f = FieldStruct(keep[0].ctypes.data, probes_ptr, sh_ptr, vis_ptr, n_probes, keep[1].ctypes.data)
        self._check(self.lib.hiprz_view_pixels(self._view, source_ptr, W, H, None if f is None else C.addressof(f), sky.ctypes.data, p.ctypes.data, pixels_ptr, image_ptr, stream))

    def samples_device(self, samples_ptr, stream=None):
        """enqueue only: what the view walks, one gather.sample_dtype record per pixel of the selected camera, to samples_ptr"""
        self._check(self.lib.hiprz_view_samples(self._view, samples_ptr, stream))

    def pixels(self, source, W, H, shape, field=None, sky=(0.0, 0.0, 0.0), params=None, image=False):
        """the host-pointer call: the pixel records (pixel_dtype, `shape` = (height, width) of the selected camera) of a host source and a
        host field; with `image` also the float4 image, shape + (4,).  Waits for the context's stream."""
        source, sky, p = np.ascontiguousarray(source), _sky(sky), _params(params)
        if source.dtype.itemsize != 16 or source.size != W * H:
            raise TypeError("source must be W*H records of 16 bytes")
        f = keep = None
        if field is not None:
            keep = field_arrays(field)
            grid, probes, sh, vis, fp = keep
            f = FieldStruct(grid.ctypes.data, probes.ctypes.data, sh.ctypes.data, None if vis is None else vis.ctypes.data, probes.size, fp.ctypes.data)
        out = np.zeros(shape, pixel_dtype)
        img = np.zeros(tuple(shape) + (4,), np.float32) if image else None
        self._check(self.lib.hiprz_view_pixels_host(self._view, source.ctypes.data, W, H, None if f is None else C.addressof(f), sky.ctypes.data, p.ctypes.data,
                                                    out.ctypes.data, None if img is None else img.ctypes.data))
        return (out, img) if image else out

    def samples(self, shape, sync):
        """the samples of the selected camera's pixels as an array of gather.sample_dtype of `shape` = (height, width).  `sync` waits for
        the context's stream (Context.sync: it also makes the head device current for the buffer)."""
        n = int(np.prod(shape))
        sync()
        buf = _hiprt.DeviceBuffer(max(n, 1) * sample_dtype.itemsize)
        try:
            self.samples_device(buf.ptr)
            sync()
            return buf.download(tuple(shape), sample_dtype)
        finally:
            buf.free()
