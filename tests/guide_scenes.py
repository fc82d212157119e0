"""Scenes and the comparison for the first-hit guide buffers (hiprz_guide) and the ray cast, for tests/test_guides_oracle.py (CPU) and
tests/test_guides_oracle_gpu.py.

SCENES = the 60 scenes of generated_scenes.SEEDS + the 48 of tree_shape_scenes.NAMES + the scenes of NEW below, which make the hard
cases of a guide kernel certain instead of lucky.  Same interface as the two older modules: `world(name)` -> (World, RenderConfig),
deterministic; `flat_scene(key)` takes a key of any of the three sets and builds once.

NEW (all 48x32 or smaller, no lights, an emitting sky):
  normal_map_a / _b / _c   two quads WITH texcrds and a normal map each, one met from the front and one from behind (every hit on it is
                           internal), under mirrored, strongly non-uniform scales (largest axis > 8 x smallest) and turned about all
                           three axes; _b's map is linear-filtered with clamp, _c's point-filtered with mirror
  inside_sphere            the camera inside a sphere with interpolated normals and a texture: every hit is internal
  address_modes_a / _b / _c  eight quads, one texture per address mode (wrap / clamp / mirror / border) x filter (point / linear), with
                           map scale, rotation and translation and texcrds that leave [0, 1] on every side; the material colours are
                           not white, so a texture that replaces the colour is not a texture that multiplies it
  emission_maps            emission maps with zero and non-zero texels (point and linear) on materials with emission > 0: the albedo
                           is the colour on the zero texels and 1 elsewhere, and which texels emit depends on the mode
  no_texcrds               textured, emission-mapped and normal-mapped materials on triangles WITHOUT texcrds: fetched at (0, 0), the
                           normal map not applied
  slots                    material ids 0, 1, 2, 63, 70 and 200 on an instance with 64 slots (slot 63 set: 70 and 200 clamp to it), on
                           one with 3 slots of which one is unset, and on one with none

COVERAGE classifies every pixel by the oracle's first-hit record (the material of the first hit, the triangle's flags); FLOOR is the
floor of generated_scenes.FEATURES: each kind on at least 20 pixels of at least 3 scenes.

THE COMPARISON (compare) follows lockstep's rule.  Per pixel:
  discrete  hit / miss differs, the instance differs, or the depth is not bit-equal;
  far       not discrete, and a normal or albedo component differs by more than lockstep.REL * max(|reference|, 1);
  exact     all 32 bytes of the hiprz_guide are equal.
The bar comes from the oracle, never from the device: `standin_counts` compares rzo_first_hit of each one-ulp libm stand-in (lo, hi,
mix) with the plain oracle's; a scene's cap is 2 x the largest stand-in count + 2, a sweep's 2 x the largest stand-in total + one pixel
per 100 000.  No libm call precedes a first hit's record (the sky's texcrd is not part of it), so the stand-ins show 0 everywhere: the
caps are 2 pixels per scene and mode, and 1 pixel over the sweep of one mode.
"""
import math

import numpy as np

import generated_scenes
import lockstep
import oracle
import tree_shape_scenes
from rayzath_amd import _abi
from rayzath_amd.engine import LightSampling, RenderConfig, Tracing
from rayzath_amd.scene import Camera, Instance, Material, Mesh, TextureBuffer, World, generate_sphere

MODES = (0, 8, 16, 24, 31, 63)        # set_mode flags the guides are compared under: 8 = TEXTURE_MULT, 16 = FILTERING
NEW = ("normal_map_a", "normal_map_b", "normal_map_c", "inside_sphere", "address_modes_a", "address_modes_b", "address_modes_c",
       "emission_maps", "no_texcrds", "slots")
SCENES = tuple(generated_scenes.SEEDS) + tuple(tree_shape_scenes.NAMES) + NEW
FLOOR = (20, 3)                       # pixels, scenes
ADDRESS = ("wrap", "clamp", "mirror", "border")
FILTER = ("point", "linear")
HP = math.pi / 2


def _quad(uv=((0, 0), (1, 0), (1, 1), (0, 1)), materials=(0, 0), texcrds=True, normals=None):
    """a unit square in the plane z = 0, two triangles; uv: the four corners' texcrds"""
    vertices = [(-0.5, -0.5, 0.0), (0.5, -0.5, 0.0), (0.5, 0.5, 0.0), (-0.5, 0.5, 0.0)]
    tris = [(0, 1, 2), (0, 2, 3)]
    extra = dict(texcrds=uv, tri_texcrds=tris) if texcrds else {}
    if normals is not None:
        extra.update(normals=normals, tri_normals=tris)
    return Mesh(vertices, tris, tri_materials=list(materials), name="quad", **extra)


def _rgba(rng, h, w, lo=0):
    bitmap = rng.integers(lo, 256, size=(h, w, 4), dtype=np.uint8)
    bitmap[..., 3] = 255
    return bitmap


def _normal_bitmap(rng, h, w):
    bitmap = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    bitmap[..., 2] = rng.integers(150, 256, size=(h, w))
    return bitmap


def _world(rng_key):
    w = World()
    w.material = Material((200, 220, 255, 0), 0.0, 0.0, 1.0, 1.0, 0.0, name="sky")
    return w, np.random.default_rng([20261101, rng_key])


def _camera(w, position=(0.0, 0.0, -6.4), resolution=(48, 32), fov=1.3):
    w.camera = Camera(position=position, rotation=(0, 0, 0), resolution=resolution, fov=fov, near_far=(1e-2, 1e3), focal_distance=6.4,
                      aperture=0.01, exposure_time=1.0 / 60.0)


def _normal_map_world(index):
    w, rng = _world(index)
    sampling = (("point", "wrap"), ("linear", "clamp"), ("point", "mirror"))[index]
    # the quads lie in their z = 0 plane: the z scale acts on the normals alone.  Facing away = not turned, unless the z scale is negative
    scales = (((-2.4, 1.7, 0.2), (2.2, -1.8, 0.25)), ((1.8, 1.9, -0.2), (-2.0, 1.6, -17.0)), ((-2.1, -1.9, -0.2), (1.9, 1.5, -0.18)))[index]
    tilt = ((0.25, 0.3, 0.2), (0.2, 0.35, 0.3), (-0.3, 0.2, -0.4))[index]
    for side, (x, turn) in enumerate(((-1.15, 0.0), (1.15, math.pi))):      # turned by pi about y
        nmap = TextureBuffer(_normal_bitmap(rng, 5, 7), scale=(2.0, -1.5), rotation=0.4 + index, translation=(0.3, -0.2),
                             filter_mode=sampling[0], address_mode=sampling[1])
        m = w.add(Material(tuple(int(c) for c in rng.integers(60, 250, size=3)) + (255,), 0.0, 0.8, normal_map=nmap, name=f"mapped {side}"))
        uv = [(float(u), float(v)) for u, v in rng.uniform(-0.6, 1.7, size=(4, 2))]
        w.add(Instance(w.add(_quad(uv)), [m], position=(x, 0.0, 0.0), rotation=(tilt[0], tilt[1] + turn, tilt[2]), scale=scales[side],
                       name=f"mapped quad {side}"))
    _camera(w)
    return w


def _inside_sphere_world():
    w, rng = _world(10)
    tex = TextureBuffer(_rgba(rng, 6, 6, 40), scale=(3.0, 2.0), rotation=0.3, translation=(0.1, 0.2), filter_mode="linear", address_mode="mirror")
    m = w.add(Material((230, 180, 140, 255), 0.0, 0.7, texture=tex, name="shell"))
    w.add(Instance(w.add(generate_sphere(8, normals=True, texture_coordinates=True)), [m], position=(0, 0, 0), rotation=(0.3, 0.2, 0.1),
                   scale=(2.0, 1.2, 1.6), name="shell"))
    _camera(w, position=(0.2, 0.1, -0.3), resolution=(33, 33), fov=1.5)
    return w


def _address_modes_world(index):
    w, rng = _world(20 + index)
    bitmaps = [_rgba(rng, *size, 20) for size in ((4, 4), (3, 5), (7, 2))]
    for k, (address, filt) in enumerate((a, f) for f in FILTER for a in ADDRESS):
        tex = TextureBuffer(bitmaps[(k + index) % 3], scale=((1.3, -0.8), (0.7, 1.9), (-2.2, 0.6))[index], rotation=(0.35, -1.1, 2.6)[index],
                            translation=((0.15, -0.4), (-0.7, 0.2), (1.3, 0.45))[index], filter_mode=filt, address_mode=address)
        color = tuple(int(c) for c in rng.integers(90, 230, size=3)) + (255,)
        m = w.add(Material(color, 0.0, 0.9, texture=tex, name=f"{filt} {address}"))
        lo, hi = (-0.8, 1.9) if index != 2 else (-2.5, 3.5)
        uv = [(lo, lo), (hi, lo + 0.1), (hi - 0.2, hi), (lo + 0.3, hi)]
        x, y = -1.8 + 1.2 * (k % 4), 0.8 - 1.6 * (k // 4)
        w.add(Instance(w.add(_quad(uv)), [m], position=(x, y, 0.1 * (k % 3)), rotation=((0.1, -0.2, 0.15)[index], (0.2, 0.1, -0.25)[index], 0.1 * k),
                       scale=((1.05, 1.4, 1.0), (-1.05, 1.35, 1.0), (1.0, -1.4, 0.7))[index], name=f"{filt} {address}"))
    _camera(w)
    return w


def _emission_maps_world():
    w, rng = _world(30)
    values = np.array([[0.0, 2.0, 0.0, 0.5], [1.5, 0.0, 0.0, 3.0], [0.0, 0.0, 1.0, 0.0]], np.float32)
    for k, (filt, address) in enumerate((("point", "wrap"), ("linear", "clamp"), ("linear", "border"))):
        emap = TextureBuffer(values, scale=(1.4, 1.2), rotation=0.5 * k, translation=(0.1 * k, 0.3), filter_mode=filt, address_mode=address)
        m = w.add(Material(tuple(int(c) for c in rng.integers(80, 240, size=3)) + (255,), 0.0, 0.9, emission=(4.0, 0.5, 2.0)[k], emission_map=emap,
                           name=f"emitting {filt}"))
        w.add(Instance(w.add(_quad([(-0.3, -0.2), (1.4, 0.0), (1.3, 1.5), (-0.1, 1.2)])), [m], position=(-1.6 + 1.6 * k, 0.0, 0.0),
                       rotation=(0.1, 0.2 - 0.2 * k, 0.1), scale=(1.5, 2.6, 1.0), name=f"emitting {filt}"))
    _camera(w)
    return w


def _no_texcrds_world():
    w, rng = _world(40)
    tex = TextureBuffer(_rgba(rng, 4, 5, 30), scale=(1.7, 1.3), rotation=0.6, translation=(0.37, 0.81), filter_mode="linear", address_mode="clamp")
    nmap = TextureBuffer(_normal_bitmap(rng, 3, 3), translation=(0.2, 0.6))
    emap = TextureBuffer(np.array([[0.0, 1.0], [2.0, 0.0]], np.float32), translation=(0.1, 0.1), filter_mode="linear", address_mode="mirror")
    textured = w.add(Material((200, 150, 100, 255), 0.0, 0.9, texture=tex, normal_map=nmap, name="textured"))
    emitting = w.add(Material((120, 200, 160, 255), 0.0, 0.9, emission=3.0, texture=tex, emission_map=emap, name="emitting"))
    normals = [(0.2, 0.1, -1.0), (-0.3, 0.2, -1.0), (0.1, -0.4, -1.0), (0.0, 0.3, -1.0)]
    normals = [tuple(np.asarray(n) / np.linalg.norm(n)) for n in normals]
    for k, (m, mesh) in enumerate(((textured, _quad(texcrds=False)), (emitting, _quad(texcrds=False)), (textured, _quad(texcrds=False, normals=normals)))):
        w.add(Instance(w.add(mesh), [m], position=(-1.6 + 1.6 * k, 0.0, 0.0), rotation=(0.15, -0.2 + 0.2 * k, 0.0), scale=(1.4, 2.5, -0.6), name=f"bare {k}"))
    _camera(w)
    return w


def _slots_world():
    w, rng = _world(50)
    ids = (0, 1, 2, 63, 70, 200)
    vertices, tris = [], []
    for k in range(len(ids)):       # six vertical strips
        x0, x1 = -0.5 + k / 6.0, -0.5 + (k + 1) / 6.0
        a = len(vertices)
        vertices += [(x0, -0.5, 0.0), (x1, -0.5, 0.0), (x1, 0.5, 0.0), (x0, 0.5, 0.0)]
        tris += [(a, a + 1, a + 2), (a, a + 2, a + 3)]
    mesh = w.add(Mesh(vertices, tris, tri_materials=[i for i in ids for _ in range(2)], name="strips"))
    mats = [w.add(Material(tuple(int(c) for c in rng.integers(40, 250, size=3)) + (255,), 0.0, 0.9, emission=2.0 if k == 1 else 0.0, name=f"m{k}"))
            for k in range(5)]
    full = [mats[k % 4] if k % 5 else None for k in range(63)] + [mats[4]]
    for k, slots in enumerate((full, [mats[0], None, mats[2]], [])):
        w.add(Instance(mesh, slots, position=(0.0, 1.05 - 1.05 * k, 0.0), rotation=(0.1, 0.1 * k, 0.0), scale=(4.4, 0.95, 1.0), name=f"strips {k}"))
    _camera(w)
    return w


def world(name):
    """(World, RenderConfig) of the scene `name` of NEW"""
    assert name in NEW, name
    base, _, letter = name.rpartition("_")
    if base == "normal_map":
        w = _normal_map_world("abc".index(letter))
    elif base == "address_modes":
        w = _address_modes_world("abc".index(letter))
    else:
        w = dict(inside_sphere=_inside_sphere_world, emission_maps=_emission_maps_world, no_texcrds=_no_texcrds_world, slots=_slots_world)[name]()
    return w, RenderConfig(LightSampling(1, 1), Tracing(2, 8), seed=20261101 + NEW.index(name))


_CACHE = {}


def flat_scene(key):
    """(FlatScene, hiprz_camera, hiprz_config, World, RenderConfig) of a scene of SCENES, built once"""
    if key not in NEW:
        return lockstep.flat_scene(key)
    if key not in _CACHE:
        from rayzath_amd.scene import camera_struct, flatten
        w, config = world(key)
        _CACHE[key] = (flatten(w), camera_struct(w.camera), config.struct(), w, config)
    return _CACHE[key]


# --- the oracle's records, once per (scene, mode, library) ---
_RECORDS = {}


def records(key, mode=0, variant=None, threads=1):
    """(H, W) oracle.first_hit_dtype of scene `key` in `mode`, of the plain oracle or of the library `variant` (a stand-in or a mutant);
    shared by every test that needs it and never written to"""
    at = (key, mode, variant)
    if at not in _RECORDS:
        flat, cam = flat_scene(key)[:2]
        out = oracle.first_hits(flat, cam, mode, lib=oracle.variant(variant) if variant else None, threads=threads)
        out.setflags(write=False)
        _RECORDS[at] = out
    return _RECORDS[at]


# --- coverage ---
def _sampling_kind(address, filt):
    return f"{ADDRESS[address]} address under a {FILTER[filt]} filter"


KINDS = ("textured albedo", "emission map", "normal map on a triangle that has texcrds", "interpolated normals", "internal hit", "unset slot",
         "emissive") + tuple(_sampling_kind(a, f) for f in range(2) for a in range(4))


def coverage(key, mode=0):
    """{kind: pixels} of the first hits of scene `key`: each hit pixel classed by the material of its first hit and its triangle's flags"""
    flat, rec = flat_scene(key)[0], records(key, mode)
    hit = rec["instance"] != _abi.GUIDE_MISS
    out = {kind: 0 for kind in KINDS}
    out["hit"] = int(hit.sum())
    if not out["hit"]:
        return out
    r = rec[hit]
    material = flat.materials[np.where(r["material"] < 0, _abi.MATERIAL_DEFAULT, r["material"])]
    flags = flat.tris["material_flags"][r["triangle"]]
    textured = material["texture"] >= 0
    out["textured albedo"] = int(textured.sum())
    out["emission map"] = int((material["emission_map"] >= 0).sum())
    out["normal map on a triangle that has texcrds"] = int(((material["normal_map"] >= 0) & ((flags & _abi.TRI_HAS_TEXCRDS) != 0)).sum())
    out["interpolated normals"] = int(((flags & _abi.TRI_HAS_NORMALS) != 0).sum())
    out["internal hit"] = int((r["external"] == 0).sum())
    out["unset slot"] = int((r["material"] < 0).sum())
    out["emissive"] = int((r["emission"] > 0).sum())
    if textured.any():
        sampling = flat.textures["sampling"][material["texture"][textured]]
        for f in range(2):
            for a in range(4):
                out[_sampling_kind(a, f)] = int((((sampling & 0xFF) == f) & ((sampling >> 8) == a)).sum())
    return out


# --- the comparison ---
def as_guides(a):
    """an array of _abi.guide_dtype from guides or from first-hit records"""
    return a if a.dtype == _abi.guide_dtype else oracle.guides(a)


def compare(got, ref, records_kept=6):
    """guides `got` against the reference `ref` (guides, or first-hit records): dict(pixels, exact, far, discrete, worst)"""
    got, ref = np.ascontiguousarray(as_guides(got)), np.ascontiguousarray(as_guides(ref))
    assert got.shape == ref.shape
    hit, rhit = got["instance"] != _abi.GUIDE_MISS, ref["instance"] != _abi.GUIDE_MISS
    discrete = (hit != rhit) | (got["instance"] != ref["instance"]) | (got["depth"].view(np.uint32) != ref["depth"].view(np.uint32))
    far = (lockstep._beyond(got["normal"], ref["normal"]).any(-1) | lockstep._beyond(got["albedo"], ref["albedo"]).any(-1)) & ~discrete
    exact = (got.view(np.uint8).reshape(got.shape + (32,)) == ref.view(np.uint8).reshape(ref.shape + (32,))).all(-1)
    worst = []
    for kind, mask in (("discrete", discrete), ("far", far)):
        for y, x in list(zip(*np.nonzero(mask)))[:records_kept - len(worst)]:
            worst.append(f"pixel ({x}, {y}) {kind}: got {got[y, x]}, reference {ref[y, x]}")
    return dict(pixels=int(got.size), exact=int(exact.sum()), far=int(far.sum()), discrete=int(discrete.sum()), worst=worst)


def bad(result):
    return result["far"] + result["discrete"]


def misses_read_as_specified(got):
    """every miss of `got` reads exactly normal 0 / albedo 1 / GUIDE_MISS (bit patterns: +0.0 and 1.0)"""
    miss = got[got["instance"] == _abi.GUIDE_MISS]
    return bool((miss["normal"].view(np.uint32) == 0).all() and (miss["albedo"].view(np.uint32) == np.float32(1).view(np.uint32)).all())


def standin_counts(key, mode):
    """{stand-in: comparison result} of rzo_first_hit of each one-ulp libm stand-in against the plain oracle's on scene `key` in `mode`"""
    return {name: compare(records(key, mode, name), records(key, mode), records_kept=0) for name in lockstep.STANDINS}


def scene_cap(key, mode):
    """discrete + far pixels a device may show on one scene in one mode: 2 x the largest count of a one-ulp stand-in, plus 2"""
    return 2 * max(bad(r) for r in standin_counts(key, mode).values()) + 2


def sweep_cap(keys, mode):
    """... and over a sweep: 2 x the largest sweep total of a one-ulp stand-in, plus one pixel per 100 000"""
    totals, pixels = {name: 0 for name in lockstep.STANDINS}, 0
    for key in keys:
        counts = standin_counts(key, mode)
        for name in lockstep.STANDINS:
            totals[name] += bad(counts[name])
        pixels += counts[lockstep.STANDINS[0]]["pixels"]
    return 2 * max(totals.values()) + pixels // 100000
