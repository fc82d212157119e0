"""The baked view (include/hiprz_view.h) restated in numpy float32, one rounding per operation like the device build (-ffp-contract=off):
the nearest and the bilinear tap of the atlas under a sample, the field's irradiance at a hit times the surface's colour, the sky and the
back face, and the 16-byte record with its kind and count.  The samples are the device's own (hiprz_view_samples) or generated ones, the
chart lookup is hiprz_gather.h's (tests/gather_reference.py), the field's is hiprz_field.h's (tests/field_reference.py: lookup).  For
tests/test_view_reference.py (CPU), which holds it to the same rule in float64 and shows that its mutants differ, and
tests/test_view_gpu.py, which holds the device's pixels to pixels() in every byte.

MUTANTS, each a wrong reading of the header that the tests must tell from the right one:
  nohalf      the -0.5 of the bilinear texel space dropped (texel centres at the integers)
  swapxy      x and y swapped: the bilinear column taken from v * H and the row from u * W
  zero        a tap without a value counted as zero instead of being left out
  noemission  the colour x emission term of an emitting hit left out
  unflipped   the field evaluated for the normal turned away from the ray (-n) instead of the one facing it

THE CAMERAS of the GPU tests (cameras()): tests/gather_world.py's at 32 x 24, the same at 33 x 19 (partial blocks on both axes) and at
1 x 1.  tests/test_view_reference.py shows in float64 that at most 1 % of their mapped pixels lie within 1e-4 texel of a texel boundary."""
import numpy as np

import field_reference as FR
import gather_reference as GR
import gather_world as GW
from rayzath_amd import bake, gather, view
from rayzath_amd.scene import Camera

F = np.float32
MUTANTS = ("nohalf", "swapxy", "zero", "noemission", "unflipped")
ATLAS_MUTANTS, FIELD_MUTANTS = MUTANTS[:3], MUTANTS[3:]
RESOLUTIONS = ((32, 24), (33, 19), (1, 1))
SOURCES = ((64, 48), (4, 3))
CAP, MARGIN = 0.01, 1e-4


def cameras():
    """the cameras of the GPU tests, one per resolution of RESOLUTIONS"""
    out = []
    for resolution in RESOLUTIONS:
        cam = Camera(position=(0.5, 3.5, -6.0), resolution=resolution, fov=1.0, near_far=(1e-2, 1e3))
        cam.look_at((0.0, 0.5, 0.0))
        out.append(cam)
    return out


def source_of(W, H, seed=3, holes=True):
    """a W x H source whose values differ per texel; with `holes` one texel in nine has no value (and holds a value that must not be read)"""
    rng = np.random.default_rng(seed + W)
    source = np.zeros((H, W), gather.record_dtype)
    source["rgb"] = rng.uniform(0.25, 4.0, (H, W, 3))
    source["word"] = rng.integers(0, 100, (H, W))
    if holes:
        source["word"][rng.random((H, W)) < 1.0 / 9.0] = gather.INVALID
    return source


def on_a_boundary(u, v, W, H, margin=MARGIN):
    """the float64 UV lies within `margin` texel of a texel boundary of a W x H atlas"""
    near = lambda a: np.abs(a - np.rint(a)) < margin
    return near(u * W) | near(v * H)


def atlas_taps(samples, charts, source, W, H, filter, dtype=F, mutant=None):
    """(rgb (..., 3), count) of every sample in `dtype`: "A FRONT-FACE HIT ON A MAPPED ID"; count 0: kind NONE (a code included), rgb 0"""
    s = np.asarray(samples)
    src = np.ascontiguousarray(source).reshape(-1).view(gather.record_dtype)
    u, v, mapped = GR.uv(s, charts, dtype)
    with np.errstate(all="ignore"):
        finite = mapped & np.isfinite(u) & np.isfinite(v)
        if filter == view.NEAREST:
            x, y, _ = GR.texel_of(u, v, W, H)
            texel = src[y * W + x]
            used = finite & (texel["word"] != gather.INVALID)
            rgb = np.where(used[..., None], texel["rgb"].astype(dtype), dtype(0.0))
            return rgb.astype(dtype), used.astype(np.uint32)
        half = dtype(0.0 if mutant == "nohalf" else 0.5)
        gx, gy = u * dtype(W) - half, v * dtype(H) - half
        if mutant == "swapxy":
            gx, gy = v * dtype(H) - half, u * dtype(W) - half
        flx, fly = np.floor(gx), np.floor(gy)
        fx, fy = gx - flx, gy - fly
        x0 = np.clip(np.where(finite, flx, 0), -1, W).astype(np.int64)
        y0 = np.clip(np.where(finite, fly, 0), -1, H).astype(np.int64)
        one = dtype(1.0)
        acc, sw, count = np.zeros(s.shape + (3,), dtype), np.zeros(s.shape, dtype), np.zeros(s.shape, np.uint32)
        for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
            x, y = x0 + dx, y0 + dy
            w = (fx if dx else one - fx) * (fy if dy else one - fy)
            inside = finite & (x >= 0) & (x < W) & (y >= 0) & (y < H)
            texel = src[np.clip(y, 0, H - 1) * W + np.clip(x, 0, W - 1)]
            has = texel["word"] != gather.INVALID
            used = inside if mutant == "zero" else inside & has
            value = np.where(has[..., None], texel["rgb"].astype(dtype), dtype(0.0))
            acc = np.where(used[..., None], acc + (w[..., None] * value), acc)
            sw = np.where(used, sw + w, sw)
            count = count + used
        ok = sw > 0
        rgb = np.where(ok[..., None], acc / sw[..., None], dtype(0.0))
    return rgb.astype(dtype), np.where(ok, count, 0).astype(np.uint32)


def hit_points(origin, direction, t):
    """p.c = o.c + (t * d.c) in float32"""
    o, d, t = np.asarray(origin, F), np.asarray(direction, F), np.asarray(t, F)
    with np.errstate(all="ignore"):
        return (o + (t[..., None] * d)).astype(F)


def field_light(samples, origin, direction, normal, color, emission, field, mutant=None):
    """(rgb (..., 3) float32, count) of every sample: "A FRONT-FACE HIT ON AN UNMAPPED INSTANCE OR ID" where the sample is UNMAPPED, (0, 0)
    elsewhere.  origin, direction: the pixel's ray; normal: hiprz_hit::normal; color (..., 3) and emission (...): the surface's; field: None
    or (grid, probes, sh, vis_or_None, field params record)."""
    s = np.asarray(samples)
    rgb, count = np.zeros(s.shape + (3,), F), np.zeros(s.shape, np.uint32)
    at = s["id"] == gather.UNMAPPED
    if field is None or not at.any():
        return rgb, count
    grid, probes, sh, vis, params = field
    n = np.asarray(normal, F)[at]
    points = bake.points(hit_points(origin, direction, s["t"])[at], -n if mutant == "unflipped" else n)
    got = FR.lookup(grid, probes, sh, vis, params, points)
    counted = np.where(got["word"] == FR.INVALID, 0, got["word"]).astype(np.uint32)
    c, e = np.asarray(color, F)[at], np.asarray(emission, F)[at]
    with np.errstate(all="ignore"):
        lit = c * got["rgb"]
        if mutant != "noemission":
            lit = np.where((e > 0)[:, None], lit + (c * e[:, None]), lit)
    rgb[at] = np.where((counted > 0)[:, None], lit, F(0.0))
    count[at] = counted
    return rgb, count


def pixels(samples, charts, source, W, H, sky, filter=view.NEAREST, origin=None, direction=None, normal=None, color=None, emission=None, field=None, mutant=None):
    """the records hiprz_view_pixels writes for the samples (any shape) of the device: view.pixel_dtype of that shape"""
    s = np.asarray(samples)
    out = np.zeros(s.shape, view.pixel_dtype)
    rgb, count = atlas_taps(s, charts, source, W, H, filter, F, mutant)
    kind = np.where(count > 0, view.ATLAS, view.NONE).astype(np.uint32)
    if field is not None:
        lit, counted = field_light(s, origin, direction, normal, color, emission, field, mutant)
        at = s["id"] == gather.UNMAPPED
        rgb, count = np.where(at[..., None], lit, rgb), np.where(at, counted, count)
        kind = np.where(at & (counted > 0), view.FIELD, kind)
    missed = (s["id"] == gather.MISS) | (s["id"] == gather.INVALID_RAY)
    rgb = np.where(missed[..., None], np.asarray(sky, F), rgb)
    kind = np.where(missed, view.SKY, np.where(s["id"] == gather.BACK, view.BACK, kind)).astype(np.uint32)
    out["rgb"] = rgb
    out["word"] = (kind << np.uint32(view.KIND_SHIFT)) | count.astype(np.uint32)
    return out


def image_of(records):
    """the float4 image of the records: (r, g, b, 1.0f)"""
    r = np.asarray(records)
    out = np.ones(r.shape + (4,), F)
    out[..., :3] = r["rgb"]
    return out


def float64_uv(world, flat, cam_struct, base, charts):
    """(mapped (H_c, W_c), u, v, instance, front) of a camera's pixels in float64: tests/gather_world.py's closest hit over
    tests/query_reference.py's pixel rays, and the chart's UV at the hit"""
    import query_reference as QR
    rays = QR.pixel_rays_d0(cam_struct)
    shape = rays.shape
    d = rays["direction"].reshape(-1, 3).astype(np.float64)
    d = d / np.sqrt((d * d).sum(-1, keepdims=True))
    o = rays["origin"].reshape(-1, 3).astype(np.float64)
    inst, tri, bx, by, front = GW.closest_hits(GW.world_triangles(world, flat), o, d, float(cam_struct.near_far[0]))
    b = np.asarray(base)[np.maximum(inst, 0)]
    mapped = (inst >= 0) & front & (b != gather.NONE)
    c = charts[np.where(mapped, b + tri, 0)]
    b1 = (1.0 - bx) - by
    u = c["u1"] * b1 + c["u2"] * bx + c["u3"] * by
    v = c["v1"] * b1 + c["v2"] * bx + c["v3"] * by
    return tuple(a.reshape(shape) for a in (mapped, u, v, inst, front))
