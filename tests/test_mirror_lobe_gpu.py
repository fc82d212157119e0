"""The glossy lobe at roughness 0 (RZ_MIRROR_LOBE_CONST: sample_direction takes (sin, cos) = (+0, 1) for a lane of roughness +-0 instead of
running powf, acosf and sincosf) and a byte over 255 in two fmas (RZ_U8_SHORT_DIV: from_u8, fetch_r8).

hiprz_selftest: its kernel runs the general sequence — spelled in the kernel, whichever way the switch stands — at roughness +0 and -0 on
draws in [0, 1) with the ends of the range among them and wants the bits (0x00000000, 0x3f800000); it compares the two-fma byte division
with `/` for all 256 bytes; and it counts the cases in which roughness 2^-100 does NOT return the same bits (hiprz_timings carries the
count).  That count must be 0, because the frames below are compared against twins built on it.

Frames: every world is rendered 1 + 8 passes at 64 x 48 (the living room at 96 x 64) through the three launch forms of
tests/test_surface_records_gpu.py — the resident pipeline, the split pipeline, nine render(1) calls on the default pipeline — and each
form's accumulator must equal, with np.array_equal, that of a twin world in which every material of roughness 0 has roughness 2^-100: a
value that is not zero, so its lanes run the general sequence, and that returns the mirror's (+0, 1).  Then render_counted(2): all ten
counters.

  cornell        config B's room: the mirror box among diffuse walls
  negative_zero  the same room with the mirror's roughness -0.0
  roughness_map  three metal panels of ONE mesh under one material whose roughness comes from a roughness_map of the texels 0, 1 and 255,
                 one texel per panel, so the lanes of a wave take the shortcut and the general sequence side by side.  A byte cannot hold
                 2^-100: in the twin the panel of texel 0 has a material of its own with roughness 2^-100 and no roughness map — and, so
                 that it fetches one texel per hit like the other (the counters are compared), its metalness 230 / 255 from a
                 metalness_map of one texel instead of the constant.  The other two panels are the same in both worlds.
  all_mirrors    the room with every material at metalness 1, roughness 0: every lane that samples a direction takes the shortcut
  living_room    96 x 64, three spot lights and a direct light, glass, scattering, gold: the general shading variant and brdf(), which
                 read the roughness themselves (roughness - 1, roughness + 1e-5, 1 - roughness: 2^-100 rounds away in each of them)
"""
import math
import re

import numpy as np
import pytest

from rayzath_amd import scenes
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.scene import Instance, Material, Mesh, TextureBuffer, World, camera_struct, flatten

pytestmark = pytest.mark.gpu

TINY = 2.0 ** -100
FORMS = (("resident pipeline", 2, False), ("split pipeline", 1, False), ("one render(1) at a time", None, True))


def _tiny_for_zero(world):
    for m in world.materials:
        if m.roughness == 0.0 and m.roughness_map is None:
            m.roughness = TINY
    return world


def cornell(twin):
    world = scenes.cornell_box(64, 48)
    return _tiny_for_zero(world) if twin else world


def negative_zero(twin):
    world = scenes.cornell_box(64, 48)
    mirrors = [m for m in world.materials if m.roughness == 0.0]
    assert len(mirrors) == 1
    mirrors[0].roughness = TINY if twin else -0.0
    return world


def _panels():
    """three upright quads side by side, facing the camera; all corners of panel k carry the texture coordinate of texel k of a 3 x 1 map"""
    vertices, tri_vertices, tri_texcrds, slots = [], [], [], []
    for k in range(3):
        x0, x1 = -1.5 + 1.02 * k, -1.5 + 1.02 * k + 0.95
        vertices += [(x0, -0.9, 0.9), (x1, -0.9, 0.9), (x1, 1.6, 1.1), (x0, 1.6, 1.1)]
        tri_vertices += [(4 * k, 4 * k + 1, 4 * k + 2), (4 * k, 4 * k + 2, 4 * k + 3)]
        tri_texcrds += [(k, k, k), (k, k, k)]
        slots += [0 if k == 0 else 1] * 2
    texcrds = [((k + 0.5) / 3.0, 0.5) for k in range(3)]
    return Mesh(vertices, tri_vertices, texcrds=texcrds, tri_texcrds=tri_texcrds, tri_materials=slots, name="three panels")


def roughness_map(twin):
    world = World()
    scenes._room(world, with_boxes=False)
    metalness = float(np.float32(230.0) / np.float32(255.0))
    metal = world.add(Material((240, 240, 240, 255), metalness, 0.5, 0.0, 1.0, 0.0,
                               roughness_map=TextureBuffer(np.array([[0, 1, 255]], dtype=np.uint8)), name="mapped metal"))
    first = metal
    if twin:
        first = world.add(Material((240, 240, 240, 255), 0.0, TINY, 0.0, 1.0, 0.0,
                                   metalness_map=TextureBuffer(np.array([[230]], dtype=np.uint8)), name="panel of texel 0"))
    world.add(Instance(world.add(_panels()), [first, metal], name="panels"))
    world.camera = scenes._camera(64, 48)
    return world


def all_mirrors(twin):
    world = scenes.cornell_box(64, 48)
    for m in world.materials:
        m.metalness, m.roughness = 1.0, 0.0
    return _tiny_for_zero(world) if twin else world


def living_room(twin):
    world = scenes.living_room(96, 64)
    assert sum(m.roughness == 0.0 for m in world.materials) >= 2 and world.spot_lights and world.direct_lights
    return _tiny_for_zero(world) if twin else world


CASES = {"cornell": cornell, "negative_zero": negative_zero, "roughness_map": roughness_map, "all_mirrors": all_mirrors,
         "living_room": living_room}


def _context(world, pipeline=None):
    ctx = Context(0)
    if pipeline is not None:
        ctx.set_pipeline(pipeline)
    ctx.upload_scene(flatten(world)), ctx.upload_camera(camera_struct(world.camera))
    ctx.set_config(RenderConfig(tracing=Tracing(6, 8)).struct())
    return ctx


@pytest.mark.parametrize("seed", [1, 20261])
def test_selftest_finds_no_mismatch(seed):
    ctx = _context(scenes.cornell_box(64, 48))
    bad, n = ctx.selftest(64, seed)
    line = [l for l in ctx.timings().splitlines() if "roughness 2^-100" in l]
    ctx.close()
    assert n > 0 and bad == 0, f"{bad} mismatches"
    assert len(line) == 1, "hiprz_timings carries the count of the lobe cases"
    differs = float(re.search(r"\)\s+([0-9.]+)ms", line[0]).group(1))
    print(f"seed {seed}: {n} cases, {bad} mismatches, lobe cases in which roughness 2^-100 leaves (+0, 1): {differs}")
    assert differs == 0.0, "roughness 2^-100 does not sample what a mirror samples on this device: the twins below need another value"


@pytest.mark.parametrize("name", list(CASES))
def test_frames_equal_the_twin_of_tiny_roughness(name):
    twin_world = CASES[name](True)
    twin = _context(twin_world)
    twin.render(1), twin.render(8)
    want_accum = twin.read_accum()
    want_counted = twin.render_counted(2)
    twin.close()
    assert np.isfinite(want_accum).all() and want_counted["hits"] > 0
    world = CASES[name](False)
    for label, pipeline, one_at_a_time in FORMS:
        ctx = _context(world, pipeline)
        if one_at_a_time:
            for _ in range(9):
                ctx.render(1)
        else:
            ctx.render(1), ctx.render(8)
        accum = ctx.read_accum()
        differ = int((accum != want_accum).any(-1).sum())
        assert np.array_equal(accum, want_accum), f"{name}, {label}: {differ} pixels of the accumulator differ from the twin's after 1 + 8 passes"
        counted = ctx.render_counted(2)
        print(f"{name}, {label} (pipeline {ctx.pipeline()}): {counted}")
        assert counted == want_counted, f"{name}, {label}: counters {counted} != {want_counted} (twin)"
        ctx.close()
