"""The binned walk on one-leaf worlds (closest_hit_flat, MODE 4: what the default traversal runs on a scene staged in LDS whose world
tree is one leaf of at most 8 instances) against the LDS-stack walk (set_traversal_mode(1)), which shares none of its candidate pick,
scan or early exit.  Per scene: the default traversal on pipelines 2, 0 and 1 and a twin on the stack walk; after render(1), render(3)
and render(5) accumulator, path state and first-hit depth of every pipeline equal the twin's bit for bit; then render_counted(4): every
counter equals the twin's, and the CPU oracle's for the fields the parity tests compare exactly (everything of the closest-hit walk and
the shading; these scenes have no lights).

Scenes, the smallest that reach each place the walk can go wrong (a tile is 32x8 pixels):
  cornell 40x12 / 1x1   partial tiles in both directions, two tiles; a single pixel
  quads n = 1, 2, 7, 8  leaves of fewer than 8 slots (bits of the missing slots, ids packed 4 bits each); n = 9: a world tree with inner
                        nodes, the general binned walk, which must be unaffected
  slabs                 eight parallel quads along the view axis, staggered so that pixels look through 1..8 of them, with a rotation and
                        non-unit scales (length factor != 1: the near end moves by a rounding, the boxes are tested again).  Listed far
                        to near every slab a ray crosses is accepted (up to 8 visits of one ray); listed near to far the first is
                        accepted and every later one culled by tm[k] > far, at every position
  cubes                 eight 12-triangle single-leaf meshes over the whole tile: 256 wide visits in a round want 2 048 lanes, the
                        one-lane-per-visit fallback; two cubes behind six quads: wide visits in rounds with few items, the octet path
  away / gap            a camera turned away from the world (root box missed: the walk returns 0), and one that looks between two quads
                        (root box hit, no instance: returns 1)

The scenes' counters on the CPU oracle (what each case is for: all 256 pixels of cubes hit a cube, the far-to-near slabs test 11 378
triangles in 4 096 segments, `away` tests 1 024 root boxes and nothing else) were checked when the test was written; the test itself
has not run on a GPU yet (profiles/r12/INDEX.md).
"""
import math

import numpy as np
import pytest

import oracle
from rayzath_amd import _abi, scenes
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.scene import Camera, Instance, Material, World, camera_struct, flatten, generate_cube, generate_plane

pytestmark = pytest.mark.gpu

HP = math.pi / 2
ORACLE_EXACT = ("segments", "hits", "light_samples", "texel_fetches", "finished")


def _camera(width, height, rotation=(0, 0, 0)):
    return Camera(position=(0, 1, -3.5), rotation=rotation, resolution=(width, height), fov=HP, near_far=(1.0e-2, 1.0e3),
                  focal_distance=4.0, aperture=0.02, exposure_time=1.0 / 60.0)


def _materials(world):
    return [world.add(Material((230, 230, 230, 255), 0.0, 1.0, name="white")),
            world.add(Material((255, 255, 255, 255), 0.0, 1.0, emission=20.0, name="light")),
            world.add(Material.mirror())]


def quads(n, width=64, height=16, spread=None, rotation=(0, 0, 0)):
    """n quads side by side, facing the camera"""
    world = World()
    mats = _materials(world)
    quad = world.add(generate_plane(4, 0.5, 0.5))
    step = spread if spread is not None else 9.0 / max(n, 1)
    for k in range(n):
        world.add(Instance(quad, [mats[k % 3]], position=((k - (n - 1) / 2) * step, 1, 1.0), rotation=(HP, 0, 0), name=f"quad {k}"))
    world.camera = _camera(width, height, rotation)
    return world


def slabs(far_to_near):
    world = World()
    mats = _materials(world)
    quad = world.add(generate_plane(4, 1.0, 1.0))
    order = range(7, -1, -1) if far_to_near else range(8)
    for k in order:   # slab k: 0.45 behind slab k - 1 and 0.5 to its right: the columns of the frame look through different sets
        world.add(Instance(quad, [mats[1] if k == 7 else mats[0] if k % 2 else mats[2]], position=(-2.2 + 0.5 * k, 1, -1.0 + 0.45 * k),
                           rotation=(HP + 0.05, 0.1, 0), scale=(1.7, 1.0, 0.6), name=f"slab {k}"))
    world.camera = _camera(64, 16)
    return world


def cubes(mixed):
    world = World()
    mats = _materials(world)
    cube = world.add(generate_cube())
    if not mixed:
        for k in range(8):
            world.add(Instance(cube, [mats[k % 3]], position=(-3.5 + k, 1, 0.5), rotation=(0, 0.1 * k, 0), scale=(1.0, 2.5, 1.0), name=f"cube {k}"))
    else:
        quad = world.add(generate_plane(4, 0.8, 0.8))
        for k in range(6):
            world.add(Instance(quad, [mats[k % 2]], position=(-3.0 + 1.2 * k, 1 + 0.2 * (k % 2), 0.2 * k), rotation=(HP, 0, 0), name=f"quad {k}"))
        for k in range(2):
            world.add(Instance(cube, [mats[2 - k]], position=(-1.0 + 2.0 * k, 1, 2.0), rotation=(0, 0.3, 0), scale=(0.8, 0.8, 0.8), name=f"cube {k}"))
    world.camera = _camera(32, 8)
    return world


CASES = {
    "cornell_40x12": lambda: scenes.cornell_box(40, 12),
    "cornell_1x1": lambda: scenes.cornell_box(1, 1),
    "quads_1": lambda: quads(1), "quads_2": lambda: quads(2), "quads_7": lambda: quads(7), "quads_8": lambda: quads(8),
    "quads_9": lambda: quads(9),
    "slabs_far_to_near": lambda: slabs(True), "slabs_near_to_far": lambda: slabs(False),
    "cubes_8": lambda: cubes(False), "cubes_2_quads_6": lambda: cubes(True),
    "away": lambda: quads(4, 32, 8, rotation=(0, math.pi, 0)),
    "gap": lambda: quads(2, 32, 8, spread=5.0),
}


def one_leaf(flat):
    meta = int(flat.nodes[flat.tlas_root]["meta"])
    return bool(meta & _abi.NODE_LEAF) and (meta & _abi.NODE_COUNT_MASK) <= 8


def frames(ctx):
    return dict(accum=ctx.read_accum(), depth=ctx.read_depth(), **{"state." + k: v for k, v in ctx.read_state().items()})


@pytest.mark.parametrize("name", list(CASES))
def test_one_leaf_walk_equals_the_stack_walk_and_the_oracle(name):
    world = CASES[name]()
    flat, cam = flatten(world), camera_struct(world.camera)
    assert one_leaf(flat) == (name != "quads_9")
    cfg = RenderConfig(tracing=Tracing(6, 8)).struct()
    contexts = {}
    for label, mode, pipeline in (("stack walk", 1, None), ("pipeline 2", None, 2), ("pipeline 0", None, 0), ("pipeline 1", None, 1)):
        ctx = Context(0)
        if mode is not None:
            ctx.set_traversal_mode(mode)
        if pipeline is not None:
            ctx.set_pipeline(pipeline)
        ctx.upload_scene(flat), ctx.upload_camera(cam), ctx.set_config(cfg)
        contexts[label] = ctx
    twin = contexts.pop("stack walk")
    for passes in (1, 3, 5):
        twin.render(passes)
        want = frames(twin)
        for label, ctx in contexts.items():
            ctx.render(passes)
            assert ctx.pipeline() == int(label[-1])
            for key, value in frames(ctx).items():
                assert np.array_equal(value, want[key]), f"{name}, {label}, after render({passes}): {key} differs from the stack walk"
    counted = twin.render_counted(4)
    for label, ctx in contexts.items():
        got = ctx.render_counted(4)
        for key in counted:
            assert got[key] == counted[key], f"{name}, {label}: counter {key} {got[key]} != {counted[key]} (stack walk)"
        for key, value in frames(ctx).items():
            assert np.array_equal(value, frames(twin)[key]), f"{name}, {label}, after the counted passes: {key}"
    ref = oracle.OracleRenderer(flat, cam, cfg)
    ref.render(1), ref.render(3), ref.render(5)
    ref_counted = ref.render(4, counted=True)
    print(name, "counted:", counted, "oracle:", ref_counted)
    for key in ORACLE_EXACT:
        assert counted[key] == ref_counted[key], f"{name}: counter {key} {counted[key]} != {ref_counted[key]} (oracle)"
    for total, shadow in (("box_tests", "shadow_box_tests"), ("tri_tests", "shadow_tri_tests")):
        assert counted[total] - counted[shadow] == ref_counted[total] - ref_counted[shadow], f"{name}: {total} (oracle)"
    # the scene is what the case is for
    pixels = 4 * cam.width * cam.height
    assert counted["segments"] == pixels
    if name == "slabs_far_to_near":   # a quad's visit tests its 2 triangles: more than 2 per segment = some ray made more than one visit
        assert counted["tri_tests"] > 2 * counted["segments"]
    if name == "away":
        assert counted["hits"] == 0 and counted["box_tests"] == pixels and counted["tri_tests"] == 0   # the root box and nothing else
    if name == "gap":
        assert 0 < counted["hits"] < pixels and counted["box_tests"] > pixels
    for ctx in list(contexts.values()) + [twin]:
        ctx.close()
    ref.close()
