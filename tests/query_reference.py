"""The reference and the rays for the ray queries (include/hiprz_query.h), for tests/test_query_oracle.py (CPU) and
tests/test_query_gpu.py.

THE REFERENCE is the CPU oracle's first hit, rzo_first_hit, which answers for an ARBITRARY ray: under a 1x1 camera with position = o,
z_axis = d0 and any finite x_axis / y_axis, screen_direction gives dx = dy = 0 and rzo_first_hit(..., 0, 0) walks exactly the ray
(o, normalized(d0)) between near_far[0] and near_far[1] (oracle_ray).  For pixel (x, y) of a camera, pixel_d0 is the direction
generate_simple_ray normalises, x_axis * dx + y_axis * dy + z_axis in float32 in the device's operation order; tests/test_query_oracle.py
proves that the 1x1 record of (position, pixel_d0) equals rzo_first_hit_frame's on every pixel of the 118 scenes of tests/guide_scenes.py.

THE RAYS of a scene (scene_rays), seeded by a CRC of the scene's key (no dependence on Python's hash salt): for a scene with at least two
hit pixels in guide_scenes.records(key, 0), 32 "surface point to surface point" rays — two distinct random hit pixels a, b, their surface
points P = position + depth * normalized(d0) in float64, the origin O = P_a + N_a * 0.01 * max(1, |P_a|_inf) as float32 (N_a: the record's
normal, which faces the camera), even rays towards float32(P_b) (d0 = float32(P_b) - O), odd rays in a uniform direction of N_a's
hemisphere, near 1e-3, far 1e3; a ray with a zero direction component is dropped.  For the other scenes (empty worlds and the like): 8
random rays through the camera's frustum from its position, between its near and far.  All directions are un-normalised: they are walked
under HIPRZ_QUERY_NORMALIZE.

compare() follows guide_scenes.compare: `discrete` = a geometric field differs (found, t bits, instance, scene_triangle, triangle, slot,
material, external — no libm call precedes them), `far` = not discrete and a component of normal, u or v is beyond lockstep.REL *
max(|reference|, 1), `exact` = all 48 bytes equal."""
import ctypes as C
import os
import re
import zlib

import numpy as np

import guide_scenes as GS
import lockstep
import oracle
from rayzath_amd import _abi, query
from rayzath_amd.query import HIT_EXTERNAL, HIT_FOUND, hit_dtype, ray_dtype

F32 = np.float32
GEOMETRIC = ("flags", "instance", "scene_triangle", "triangle", "material_slot", "material")  # and the bits of t
RAYS_PER_SCENE, RAYS_PER_SPARSE_SCENE = 32, 8
NEAR, FAR = 1e-3, 1e3


def _axes(cam):
    return (np.array(cam.x_axis[:], F32), np.array(cam.y_axis[:], F32), np.array(cam.z_axis[:], F32))


def screen_direction(cam, x, y):
    """dx, dy of pixel centres (arrays or scalars) in float32, as screen_direction computes them"""
    tana = F32(cam.tan_half_fov)
    dx = (((np.asarray(x, F32) + F32(0.5)) / F32(cam.width)) - F32(0.5)) * tana
    dy = (((np.asarray(y, F32) + F32(0.5)) / F32(cam.height)) - F32(0.5)) * (-tana / F32(cam.aspect_ratio))
    return dx, dy


def _d0(cam, dx, dy):
    xa, ya, za = _axes(cam)
    dx, dy = np.asarray(dx, F32)[..., None], np.asarray(dy, F32)[..., None]
    return (xa * dx + ya * dy) + za * F32(1.0)


def pixel_d0(cam, x, y):
    """the direction generate_simple_ray normalises for pixel (x, y): (..., 3) float32"""
    return _d0(cam, *screen_direction(cam, x, y))


def frame_d0(cam):
    """(H, W, 3) pixel_d0 of every pixel"""
    ys, xs = np.mgrid[0:cam.height, 0:cam.width]
    return pixel_d0(cam, xs, ys)


def as_hits(records):
    """oracle.first_hit_dtype records as hit_dtype rows: t = depth, scene_triangle = triangle, triangle = source_index, ..."""
    records = np.asarray(records)
    out = np.zeros(records.shape, hit_dtype)
    found = records["instance"] != _abi.GUIDE_MISS
    out["t"], out["u"], out["v"], out["normal"] = records["depth"], records["u"], records["v"], records["normal"]
    out["flags"] = np.where(found, HIT_FOUND | np.where(records["external"] != 0, HIT_EXTERNAL, 0), 0)
    out["instance"] = np.where(found, records["instance"].astype(np.int64), -1)
    out["material_slot"], out["material"] = records["material_slot"], records["material"]
    out["triangle"], out["scene_triangle"] = records["source_index"], records["triangle"]
    return out


def oracle_ray(flat, cam, o, d0, near, far, lib=None):
    """the oracle's first hit of the ray (o, normalized(d0)) between near and far, as a hit_dtype row: rzo_first_hit through a 1x1 camera"""
    one = _abi.Camera.from_buffer_copy(cam)
    one.position[:] = [float(v) for v in o]
    one.z_axis[:] = [float(v) for v in d0]
    one.width = one.height = 1
    one.near_far[:] = [float(near), float(far)]
    return as_hits(oracle.first_hit(flat, one, 0, 0, 0, lib=lib))


def oracle_rays(flat, cam, rays, lib=None):
    """oracle_ray of every ray of a 1-d array of ray_dtype (directions un-normalised)"""
    out = np.zeros(len(rays), hit_dtype)
    for k, r in enumerate(rays):
        out[k] = oracle_ray(flat, cam, r["origin"], r["direction"], r["near"], r["far"], lib)
    return out


make_rays = query.rays


def device_view_sizes():
    """(sizeof(DScene), sizeof(DCamera)) as rayzath_amd/csrc/hiprz_device.hpp declares them: DScene's is pinned there by a static_assert,
    DCamera holds 4-byte fields only (float and uint32_t, arrays included), so its size is four times their number"""
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rayzath_amd", "csrc", "hiprz_device.hpp")).read()
    scene = int(re.search(r"static_assert\(sizeof\(DScene\) == (\d+)", text).group(1))
    body = re.search(r"struct DCamera \{(.*?)\n\};", text, flags=re.S).group(1)
    words = 0
    for ctype, names in re.findall(r"^\s*(float|uint32_t)\s+([^;]+);", body, flags=re.M):
        for name in names.split(","):
            m = re.fullmatch(r"\s*\w+(?:\[(\d+)\])?\s*", name)
            words += int(m.group(1) or 1)
    assert len(re.findall(r";", re.sub(r"//.*", "", body))) == len(re.findall(r"^\s*(?:float|uint32_t)\s+[^;]+;", body, flags=re.M)), "a field of another type"
    return scene, 4 * words


def pixel_rays_d0(cam):
    """(H, W) rays (position, pixel_d0, near, far) of a camera: the pixel rays before normalisation"""
    return make_rays(np.array(cam.position[:], F32), frame_d0(cam), cam.near_far[0], cam.near_far[1])


def seed_of(key):
    return zlib.crc32(repr(key).encode())


_RAYS = {}


def scene_rays(key):
    """(rays, dense): the scene's rays by the recipe above (1-d ray_dtype, never written to) and whether they start on hit pixels"""
    if key not in _RAYS:
        flat, cam = GS.flat_scene(key)[:2]
        rec = GS.records(key, 0)
        rng = np.random.default_rng([20261019, seed_of(key)])
        position = np.array(cam.position[:], np.float64)
        ys, xs = np.nonzero(rec["instance"] != _abi.GUIDE_MISS)
        dense = len(xs) >= 2
        origins, directions = [], []
        if dense:
            d0 = pixel_d0(cam, xs, ys).astype(np.float64)
            points = position + rec["depth"][ys, xs].astype(np.float64)[:, None] * (d0 / np.linalg.norm(d0, axis=-1, keepdims=True))
            normals = rec["normal"][ys, xs].astype(np.float64)
            for k in range(RAYS_PER_SCENE):
                a, b = rng.choice(len(xs), 2, replace=False)
                o = (points[a] + normals[a] * 0.01 * max(1.0, float(np.abs(points[a]).max()))).astype(F32)
                v = rng.normal(size=3)
                v /= np.linalg.norm(v)
                if np.dot(v, normals[a]) < 0:
                    v = -v
                d = points[b].astype(F32) - o if k % 2 == 0 else v.astype(F32)
                if (d == 0).any():
                    continue
                origins.append(o), directions.append(d)
            near, far = NEAR, FAR
        else:
            half_x = abs(float(cam.tan_half_fov)) * 0.5
            half_y = abs(float(cam.tan_half_fov) / float(cam.aspect_ratio)) * 0.5
            for k in range(RAYS_PER_SPARSE_SCENE):
                d = _d0(cam, F32(rng.uniform(-half_x, half_x)), F32(rng.uniform(-half_y, half_y)))
                if (d == 0).any():
                    continue
                origins.append(position.astype(F32)), directions.append(d)
            near, far = cam.near_far[0], cam.near_far[1]
        rays = make_rays(np.array(origins, F32).reshape(-1, 3), np.array(directions, F32).reshape(-1, 3), near, far)
        rays.setflags(write=False)
        _RAYS[key] = (rays, dense)
    return _RAYS[key]


_REFERENCE = {}


def scene_reference(key, variant=None):
    """oracle_rays of scene_rays(key), of the plain oracle or of the library `variant`; computed once, never written to"""
    at = (key, variant)
    if at not in _REFERENCE:
        flat, cam = GS.flat_scene(key)[:2]
        out = oracle_rays(flat, cam, scene_rays(key)[0], lib=oracle.variant(variant) if variant else None)
        out.setflags(write=False)
        _REFERENCE[at] = out
    return _REFERENCE[at]


def geometric_differs(got, ref):
    """per ray: a geometric field differs"""
    out = got["t"].view(np.uint32) != ref["t"].view(np.uint32)
    for name in GEOMETRIC:
        out = out | (got[name] != ref[name])
    return out


def compare(got, ref, records_kept=6):
    """hits `got` against the reference `ref` (both hit_dtype, same shape): dict(rays, exact, far, discrete, worst)"""
    got, ref = np.ascontiguousarray(got).reshape(-1), np.ascontiguousarray(ref).reshape(-1)
    assert got.shape == ref.shape and got.dtype == ref.dtype == hit_dtype
    discrete = geometric_differs(got, ref)
    far = (lockstep._beyond(got["normal"], ref["normal"]).any(-1) | lockstep._beyond(got["u"], ref["u"]) | lockstep._beyond(got["v"], ref["v"])) & ~discrete
    exact = (got.view(np.uint8).reshape(-1, 48) == ref.view(np.uint8).reshape(-1, 48)).all(-1)
    worst = []
    for kind, mask in (("discrete", discrete), ("far", far)):
        for i in np.flatnonzero(mask)[:records_kept - len(worst)]:
            worst.append(f"ray {i} {kind}: got {got[i]}, reference {ref[i]}")
    return dict(rays=int(got.size), exact=int(exact.sum()), far=int(far.sum()), discrete=int(discrete.sum()), worst=worst)


def bad(result):
    return result["far"] + result["discrete"]


def misses_read_as_specified(hits, rays):
    """every ray of `hits` without HIT_FOUND reads t = the ray's far (its bits), +0 in u, v and normal, -1 / -1 / -1 / 0 / -1"""
    hits, rays = np.ascontiguousarray(hits).reshape(-1), np.ascontiguousarray(rays).reshape(-1)
    miss = (hits["flags"] & HIT_FOUND) == 0
    h, r = hits[miss], rays[miss]
    return bool((h["t"].view(np.uint32) == r["far"].view(np.uint32)).all() and (h["u"].view(np.uint32) == 0).all() and (h["v"].view(np.uint32) == 0).all()
                and (h["normal"].view(np.uint32) == 0).all() and (h["instance"] == -1).all() and (h["material_slot"] == -1).all()
                and (h["material"] == -1).all() and (h["triangle"] == 0).all() and (h["scene_triangle"] == -1).all())
