"""Generated scenes for the lockstep comparison (tests/lockstep.py): `generated_world(seed)` draws a small world from the corners of the
parameter space that no hand-built scene reaches — mirrored and strongly non-uniform instances, cameras turned about all three axes or
standing inside geometry, near / far ranges that clip, portrait / 1x1 / 64x3 frames, ior exactly 1, roughness and metalness exactly 0 and
1, partial alpha, 1x1 maps and maps with negative scale, lights of size / angle / emission 0 or at their upper clamp, an empty world,
instances with 0, 1, 3 or 64 material slots of which some are unset, meshes with degenerate and duplicate triangles.

Deterministic from the seed alone (numpy's PCG64 and float arithmetic that does not depend on the process).  FEATURES names what the sweep
must contain; tests/test_lockstep_oracle.py asserts every entry on at least 3 scenes of SEEDS, that the validator accepts every scene and
that the oracle's frames stay finite.

What the generator leaves out, and why:
  * duplicate triangles always carry the same material and attributes: which of two coincident triangles is "the closest" depends on the
    order a tree hands them out, and the trees (reference, surface-area, device-built) legitimately differ in it;
  * degenerate triangles have zero area by a repeated vertex or three collinear vertices, never NaN / inf coordinates;
  * scales are never 0 (the ray's local direction would be inf) and a light's direction never the zero vector;
  * the sky's colour map is point-filtered.  Under HIPRZ_COMPAT_FILTERING a linear fetch weights four texels with float products that sum
    to 1 only to rounding: four opaque texels give alpha 1 or 0.99999994 (1.3 % of coordinates), and the integrator's opacity test
    `1 - alpha > 0` then picks another sampling branch with another number of random draws.  A map on a triangle takes its texcrd from
    barycentrics, the same bits on both sides; the sky's comes from atan2f / asinf, and it is read as a surface where the medium
    scattered the ray (HIPRZ_COMPAT_SCATTERING), so one libm ulp tipped that test on 0.7 % of such a scene's segments (Oracle).
The validator (hiprz_validate_scene) refused none of the drawn scenes.
"""
import math

import numpy as np

from rayzath_amd.engine import LightSampling, RenderConfig, Tracing
from rayzath_amd.scene import (Camera, DirectLight, Instance, Material, Mesh, SpotLight, TextureBuffer, World, generate_cube,
                               generate_plane, generate_sphere)

SEEDS = tuple(range(60))
SIZES = ((48, 32), (17, 41), (33, 33), (64, 3), (1, 1))
DEPTHS = (1, 2, 6, 16)
PASSES = 8


def _pick(rng, extremes, lo, hi, p_extreme=0.5):
    """A parameter from its extremes or from the interior."""
    if rng.random() < p_extreme:
        return float(extremes[rng.integers(len(extremes))])
    return float(rng.uniform(lo, hi))


def _map(rng, kind, tiny=False, linear=True):
    h, w = (1, 1) if tiny else (int(rng.integers(1, 9)), int(rng.integers(1, 9)))
    if kind == "rgba":
        bitmap = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        bitmap[..., 3] = rng.choice(np.array([0, 255, 255, 255, 128, 40], np.uint8), size=(h, w))   # texture alpha: opaque, clear, partial
    elif kind == "normal":
        bitmap = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
        bitmap[..., 2] = rng.integers(160, 256, size=(h, w))                                        # mostly along the surface normal
    elif kind == "r8":
        bitmap = rng.choice(np.array([0, 255, 17, 128, 200], np.uint8), size=(h, w))
    else:
        bitmap = rng.choice(np.array([0.0, 0.5, 1.0, 3.0], np.float32), size=(h, w)).astype(np.float32)
    scale = (float(rng.uniform(0.3, 4.0)) * (-1.0 if rng.random() < 0.4 else 1.0), float(rng.uniform(0.3, 4.0)) * (-1.0 if rng.random() < 0.4 else 1.0))
    return TextureBuffer(bitmap, scale=scale, rotation=float(rng.uniform(-3.2, 3.2)), translation=(float(rng.uniform(-2, 2)), float(rng.uniform(-2, 2))),
                         filter_mode=("point", "linear")[int(rng.integers(2)) * int(linear)], address_mode=("wrap", "clamp", "mirror", "border")[int(rng.integers(4))])


def _material(rng, name):
    alpha = int(rng.choice([255, 255, 255, 0, 128, 30]))
    color = tuple(int(c) for c in rng.integers(30, 256, size=3)) + (alpha,)
    maps = {}
    for field, kind, p in (("texture", "rgba", 0.3), ("normal_map", "normal", 0.15), ("metalness_map", "r8", 0.15), ("roughness_map", "r8", 0.15),
                           ("emission_map", "r32", 0.15)):
        if rng.random() < p:
            maps[field] = _map(rng, kind, tiny=rng.random() < 0.25)
    return Material(color, metalness=_pick(rng, (0.0, 1.0), 0.0, 1.0), roughness=_pick(rng, (0.0, 1.0), 0.0, 1.0),
                    emission=_pick(rng, (0.0, 0.0, 0.0, 4.0), 0.1, 8.0, 0.7), ior=_pick(rng, (1.0,), 1.0, 2.5, 0.4),
                    scattering=_pick(rng, (0.0,), 0.1, 2.0, 0.85), name=name, **maps)


def _irregular_mesh(rng):
    """A triangle soup with per-triangle texcrds / normals on some triangles, material ids 0 .. 2 and one beyond 63, two degenerate
    triangles (a repeated vertex; three collinear vertices) and two duplicates of earlier triangles."""
    n_v, n_t = 14, 18
    vertices = rng.uniform(-1.5, 1.5, size=(n_v, 3)).astype(np.float32)
    vertices[n_v - 1] = (vertices[0] + vertices[1]) * np.float32(0.5)                 # collinear with 0 and 1
    tri = np.array([rng.choice(n_v - 1, size=3, replace=False) for _ in range(n_t)], dtype=np.uint32)
    tri[n_t - 4] = (tri[0][0], tri[0][0], tri[0][1])                                  # repeated vertex
    tri[n_t - 3] = (0, 1, n_v - 1)                                                    # collinear
    tri[n_t - 2], tri[n_t - 1] = tri[1], tri[2]                                       # duplicates
    materials = rng.choice(np.array([0, 1, 2, 70, 70], np.uint32), size=n_t)
    texcrds = rng.uniform(-1.5, 2.5, size=(n_v, 2)).astype(np.float32)
    normals = rng.normal(size=(n_v, 3)).astype(np.float32)
    normals /= np.sqrt((normals * normals).sum(-1, keepdims=True)).astype(np.float32)
    unused = np.uint32(0xFFFFFFFF)
    tri_t = np.where(rng.random(n_t)[:, None] < 0.6, tri, unused).astype(np.uint32)
    tri_n = np.where(rng.random(n_t)[:, None] < 0.4, tri, unused).astype(np.uint32)
    for dup, src in ((n_t - 2, 1), (n_t - 1, 2)):
        materials[dup], tri_t[dup], tri_n[dup] = materials[src], tri_t[src], tri_n[src]
    return Mesh(vertices, tri, texcrds=texcrds, tri_texcrds=tri_t, normals=normals, tri_normals=tri_n, tri_materials=materials, name="irregular")


def _scale(rng):
    r = rng.random()
    if r < 0.2:                                                                        # strongly non-uniform
        s = np.array([rng.uniform(0.05, 0.2), rng.uniform(0.8, 1.5), rng.uniform(2.0, 4.0)])[rng.permutation(3)]
    else:
        s = rng.uniform(0.4, 1.6, size=3)
    if rng.random() < 0.3:                                                             # mirrored: one or three negative axes
        s = s * (np.array([-1.0, 1.0, 1.0])[rng.permutation(3)] if rng.random() < 0.7 else -1.0)
    return tuple(float(x) for x in s)


def generated_world(seed):
    """(World, RenderConfig) of sweep scene `seed`."""
    rng = np.random.default_rng([20240917, int(seed)])
    world = World()
    width, height = SIZES[seed % len(SIZES)]
    max_depth = DEPTHS[(seed // len(SIZES)) % len(DEPTHS)]

    sky = {}
    if rng.random() < 0.4:
        sky["texture"] = _map(rng, "rgba", linear=False)
    if rng.random() < 0.25:
        sky["emission_map"] = _map(rng, "r32")
    world.material = Material(tuple(int(c) for c in rng.integers(100, 256, size=3)) + (0,), 0.0, 0.0, _pick(rng, (0.0, 1.0), 0.2, 3.0), 1.0,
                              _pick(rng, (0.0,), 0.02, 0.3, 0.7), name="generated sky", **sky)

    materials = [world.add(_material(rng, f"m{i}")) for i in range(int(rng.integers(1, 7)))]
    n_instances = 0 if seed % 20 == 7 else int(rng.integers(1, 13))
    factories = (generate_cube, lambda: generate_plane(int(rng.integers(3, 7)), float(rng.uniform(0.5, 2.0)), float(rng.uniform(0.5, 2.0))),
                 lambda: generate_sphere(8, normals=True, texture_coordinates=True), lambda: generate_sphere(8, normals=False, texture_coordinates=False),
                 lambda: generate_sphere(16, normals=True, texture_coordinates=False), lambda: _irregular_mesh(rng))
    meshes = {}
    for i in range(n_instances):
        kind = int(rng.integers(len(factories)))
        if kind not in meshes or rng.random() < 0.3:
            meshes[kind] = world.add(factories[kind]())
        n_slots = int(rng.choice([0, 1, 1, 3, 3, 64])) if kind == 5 else int(rng.choice([0, 1, 1, 1, 3]))
        slots = [None if rng.random() < 0.2 else materials[int(rng.integers(len(materials)))] for _ in range(n_slots)]
        world.add(Instance(meshes[kind], slots, position=tuple(rng.uniform(-2.0, 2.0, size=3)), rotation=tuple(rng.uniform(-math.pi, math.pi, size=3)),
                           scale=_scale(rng), name=f"i{i}"))

    centre = np.mean([i.position for i in world.instances], axis=0) if world.instances else np.zeros(3, np.float32)
    n_spot, n_direct = (0, 0) if seed % 12 == 5 else (int(rng.integers(0, 3)), int(rng.integers(0, 3)))
    for _ in range(n_spot):
        position = centre + rng.uniform(-3.0, 3.0, size=3)
        world.add(SpotLight(position=position, direction=(centre - position) + rng.uniform(-0.5, 0.5, size=3) + 1e-3,
                            color=tuple(int(c) for c in rng.integers(60, 256, size=4)), size=_pick(rng, (0.0,), 0.02, 0.6, 0.3),
                            emission=_pick(rng, (0.0,), 10.0, 300.0, 0.2), beam_angle=_pick(rng, (0.0, math.pi), 0.2, 2.5, 0.35)))
    for _ in range(n_direct):
        world.add(DirectLight(direction=rng.uniform(-1.0, 1.0, size=3) + 1e-3, color=tuple(int(c) for c in rng.integers(60, 256, size=4)),
                              emission=_pick(rng, (0.0,), 1.0, 30.0, 0.2), angular_size=_pick(rng, (0.0, math.pi), 0.01, 1.0, 0.35)))

    # a random camera mostly sees nothing: stand back from the objects and look at one of them
    target = world.instances[int(rng.integers(len(world.instances)))].position if world.instances else centre
    many_slots = [i for i in world.instances if len(i.materials) == Instance.MATERIAL_CAPACITY]
    if many_slots and rng.random() < 0.7:                                              # ... by preference at one whose slots reach 63
        target = many_slots[0].position
    inside = bool(world.instances) and rng.random() < 0.15
    solids = [i for i in world.instances if i.mesh.name in ("default cube", "generated sphere")]
    reach = 0.3
    if inside and solids:                                                              # a camera inside a cube or a sphere: within 0.3 of its smallest half-extent
        solid = solids[int(rng.integers(len(solids)))]
        target, reach = solid.position, 0.3 * float(np.abs(solid.scale).min()) * 0.5
    offset = rng.normal(size=3)
    offset = offset / np.linalg.norm(offset) * (rng.uniform(0.0, reach) if inside else rng.uniform(2.5, 6.0))
    position = (target + offset).astype(np.float32)
    distance = float(np.linalg.norm(target - position))
    near_far = (1e-2, 1e3)
    if rng.random() < 0.25 and not inside:                                             # a range that clips the geometry
        near_far = (distance * float(rng.uniform(0.7, 1.0)), distance * float(rng.uniform(1.0, 1.4)))
    camera = Camera(position=position, resolution=(width, height), fov=float(rng.uniform(0.5, 1.7)), near_far=near_far,
                    focal_distance=max(distance, 0.5), aperture=_pick(rng, (1e-6,), 1e-3, 0.05), exposure_time=1.0 / 60.0)
    camera.look_at(target + rng.uniform(-0.3, 0.3, size=3).astype(np.float32))
    if rng.random() < 0.6:                                                             # ... and roll: all three rotations
        camera.rotation[2] = np.float32(rng.uniform(-math.pi, math.pi))
    world.camera = camera
    config = RenderConfig(LightSampling(int(rng.integers(1, 4)), int(rng.integers(1, 4))), Tracing(max_depth, 8), seed=20240501 + int(seed))
    return world, config


def _used_materials(world):
    return [m for i in world.instances for m in i.materials if m is not None]


def _camera_in_a_box(world):
    """the camera stands inside the world-space bounding box of an instance (the box the flattened scene carries)"""
    from rayzath_amd.scene import flatten
    if not world.instances:
        return False
    boxes, p = flatten(world).instances, np.asarray(world.camera.position, np.float32)
    return bool(((boxes["bb_min"] < p) & (p < boxes["bb_max"])).all(-1).any())


def _maps_of(world):
    out = []
    for m in [world.material] + list(world.materials):
        out += [t for t in (m.texture, m.normal_map, m.metalness_map, m.roughness_map, m.emission_map) if t is not None]
    return out


# name -> predicate(world, config): what the sweep must contain (each on at least 3 scenes)
FEATURES = {
    "negative scale": lambda w, c: any((i.scale < 0).any() for i in w.instances),
    "strongly non-uniform scale": lambda w, c: any(np.abs(i.scale).max() > 8 * np.abs(i.scale).min() for i in w.instances),
    "camera with three rotations": lambda w, c: all(abs(float(r)) > 0.05 for r in w.camera.rotation),
    "camera inside an instance's bounding box": lambda w, c: _camera_in_a_box(w),
    "clipping near / far range": lambda w, c: w.camera.near_far[0] > 0.1,
    "portrait frame": lambda w, c: w.camera.height > w.camera.width,
    "1x1 frame": lambda w, c: (w.camera.width, w.camera.height) == (1, 1),
    "64x3 frame": lambda w, c: (w.camera.width, w.camera.height) == (64, 3),
    "ior exactly 1": lambda w, c: any(m.ior == 1.0 and m.color[3] < 255 for m in _used_materials(w)),
    "roughness exactly 0": lambda w, c: any(m.roughness == 0.0 for m in _used_materials(w)),
    "roughness exactly 1": lambda w, c: any(m.roughness == 1.0 for m in _used_materials(w)),
    "metalness exactly 0": lambda w, c: any(m.metalness == 0.0 for m in _used_materials(w)),
    "metalness exactly 1": lambda w, c: any(m.metalness == 1.0 for m in _used_materials(w)),
    "partial alpha": lambda w, c: any(0 < m.color[3] < 255 for m in _used_materials(w)),
    "scattering material": lambda w, c: any(m.scattering > 0 for m in _used_materials(w)),
    "1x1 map": lambda w, c: any(t.bitmap.shape[:2] == (1, 1) for t in _maps_of(w)),
    "map with negative scale": lambda w, c: any(min(t.scale) < 0 for t in _maps_of(w)),
    "texture": lambda w, c: any(m.texture is not None for m in _used_materials(w)),
    "normal map": lambda w, c: any(m.normal_map is not None for m in _used_materials(w)),
    "metalness map": lambda w, c: any(m.metalness_map is not None for m in _used_materials(w)),
    "roughness map": lambda w, c: any(m.roughness_map is not None for m in _used_materials(w)),
    "emission map": lambda w, c: any(m.emission_map is not None for m in _used_materials(w)),
    "emissive sky": lambda w, c: w.material.emission > 0,
    "textured sky": lambda w, c: w.material.texture is not None,
    "spot light of size 0": lambda w, c: any(l.size < 1e-30 for l in w.spot_lights),
    "spot light with beam angle 0": lambda w, c: any(l.beam_angle == 0.0 for l in w.spot_lights),
    "spot light with beam angle pi": lambda w, c: any(l.beam_angle == 3.14159 for l in w.spot_lights),
    "direct light of angular size 0": lambda w, c: any(l.angular_size == 0.0 for l in w.direct_lights),
    "direct light of angular size pi": lambda w, c: any(l.angular_size > 3.14 for l in w.direct_lights),
    "light with emission 0": lambda w, c: any(l.emission == 0.0 for l in w.spot_lights + w.direct_lights),
    "no light": lambda w, c: not w.spot_lights and not w.direct_lights,
    "two spot lights": lambda w, c: len(w.spot_lights) == 2,
    "two direct lights": lambda w, c: len(w.direct_lights) == 2,
    "three light samples": lambda w, c: 3 in (c.light_sampling.spot_light, c.light_sampling.direct_light),
    "empty world": lambda w, c: not w.instances,
    "instance without material slots": lambda w, c: any(len(i.materials) == 0 for i in w.instances),
    "instance with one slot": lambda w, c: any(len(i.materials) == 1 for i in w.instances),
    "instance with three slots": lambda w, c: any(len(i.materials) == 3 for i in w.instances),
    "instance with 64 slots": lambda w, c: any(len(i.materials) == 64 for i in w.instances),
    "unset material slot": lambda w, c: any(m is None for i in w.instances for m in i.materials),
    "degenerate and duplicate triangles": lambda w, c: any(i.mesh.name == "irregular" for i in w.instances),
    "material id beyond 63": lambda w, c: any((i.mesh.tri_materials > 63).any() for i in w.instances),
    "sphere without normals and texcrds": lambda w, c: any(i.mesh.name == "generated sphere" and not len(i.mesh.normals) for i in w.instances),
    "cube": lambda w, c: any(i.mesh.name == "default cube" for i in w.instances),
    "plane": lambda w, c: any(i.mesh.name == "generated plane" for i in w.instances),
    "twelve instances": lambda w, c: len(w.instances) == 12,
    "max_depth 1": lambda w, c: c.tracing.max_depth == 1,
    "max_depth 16": lambda w, c: c.tracing.max_depth == 16,
}

# Scenes derived from sweep scenes, addressed as (kind, seed) wherever a seed is: "dark" is scene `seed` without its lights, "bare" without
# lights and without any map.  No scene of SEEDS is both (the six without lights all carry a map), and the library has instantiations
# for exactly these: shading without next-event estimation (RZ_SHADOW_NONE) and without texture fetches as well (RZ_SHADOW_PLAIN).
# tests/test_packaging_sweep_gpu.py needs them on one-leaf worlds (1, 3, 5, 9), on deeper world trees (0, 2, 8, 10) and on the empty
# world (7) to reach every kernel instantiation; tests/test_lockstep_gpu.py holds the default packaging on them to the oracle.
DERIVED = tuple(("bare", s) for s in (0, 1, 2, 3, 5, 7, 8, 9)) + tuple(("dark", s) for s in (0, 2, 10))
_MAPS = ("texture", "normal_map", "metalness_map", "roughness_map", "emission_map")


def derived_world(kind, seed):
    """(World, RenderConfig) of the derived scene (kind, seed)"""
    assert kind in ("dark", "bare"), kind
    world, config = generated_world(seed)
    world.spot_lights.clear(), world.direct_lights.clear()
    if kind == "bare":
        for m in [world.material] + list(world.materials):
            for field in _MAPS:
                setattr(m, field, None)
    return world, config


_CACHE = {}


def flat_scene(seed):
    """(FlatScene, hiprz_camera, hiprz_config, World, RenderConfig) of sweep scene `seed` (or of the derived scene (kind, seed)), built once."""
    if seed not in _CACHE:
        from rayzath_amd.scene import camera_struct, flatten
        world, config = derived_world(*seed) if isinstance(seed, tuple) else generated_world(seed)
        _CACHE[seed] = (flatten(world), camera_struct(world.camera), config.struct(), world, config)
    return _CACHE[seed]
