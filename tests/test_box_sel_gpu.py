"""The one-leaf walk's up-front box tests (closest_hit_flat, MODE 4): the root box, the instance boxes tested before the rounds
(pretest_leaf_instances, its re-test included) and the visit's mesh box.  pretest_leaf_instances has two loops, and the cases below put
a world on either side of the choice: a leaf of eight instances under a wave of fast rays takes its eight tests as one straight run
(box_range_fast, no `k < count`); every other leaf and every wave with one ray that is not fast takes the general loop
(box_range_unpacked, which itself runs the shared-reciprocal form for a wave of fast rays and true divisions otherwise).

Self-test: ctx.selftest(256, seed) for three seeds.  Its kernel holds div_shared, which both loops divide with, to the correctly rounded
quotient bit for bit, the filtered box test to the exact one (flat boxes, range ends on a face, nearly parallel rays), and the triangle
pair step to the one-by-one loop.  Every mismatch lands in the one counter, which must be zero.

Scenes, by the method of tests/test_packed_pairs_gpu.py: the default traversal on pipelines 2, 0 and 1 against a twin on the LDS-stack
walk (set_traversal_mode(1): box_hit / div_shared2, another spelling of the same tests).  After render(1) and render(3): accumulator,
first-hit depth and path state equal the twin's bit for bit; then render_counted(2): every counter equals the twin's.  One case
(`flat_and_thick`) is also held to the CPU oracle: segments, hits and finished exact, box and triangle tests net of shadow tests.
Every frame is 32x8 pixels or smaller.

  quads_1, quads_2, quads_8   one-leaf worlds of 1, 2 and 8 instances: the root box, each unrolled slot of the pretest, `k < count` at
                              both ends
  flat_and_thick              axis-aligned walls (their boxes are flat: the two quotients of an axis are equal) and a rotated cube under
                              non-unit scales (all six differ)
  not_fast                    one instance placed beyond 2^40: the scene's fast_div is 0, every wave takes box_range_unpacked<false>
                              (asserted on the flattened scene: a box coordinate at or above 2^40)
  down_the_axis               a scene in the fast range seen by a camera that looks exactly down +z with a closed aperture.  A direction
                              component that is exactly zero makes its lane not fast; with the pixel jitter that is a rare draw, so
                              this case alone does not guarantee a wave of both kinds
  tiny_origin                 the same with the camera's x at 2^-66: below the fast range and not zero, so every ray that starts at the
                              camera is not fast and every ray that starts at a surface is — waves of new paths take the slow form, waves
                              of continued paths the fast one, and where a tile holds both kinds in one wave (the resident kernel restarts
                              finished paths) the wave takes the slow form for all its lanes
  partial_5x3                 one partial tile: inactive lanes in the pretest
  mixed                       the `mixed` world of tests/test_packed_pairs_gpu.py, rebuilt here: eight one-leaf meshes under a rotation and
                              non-unit scales, meant to move the near end by a rounding (the instance boxes are then tested again: the
                              re-test path) and to test the visit's mesh box on a rotated, scaled local ray
  not_fast_full_leaf, tiny_origin_full_leaf
                              the two above with the leaf filled to eight instances.  A leaf of eight under a wave of fast rays has its
                              up-front tests as one straight run (quads_8 and mixed take it in every wave); these two reach the general
                              loop behind it with a full leaf: in every wave, and in the waves that hold a ray from the camera
The tests cannot see which form ran: the library has no counter for it.
"""
import math

import numpy as np
import pytest

import oracle
from rayzath_amd import _abi
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.scene import Camera, Instance, Material, Mesh, World, camera_struct, flatten, generate_cube, generate_plane

pytestmark = pytest.mark.gpu

HP = math.pi / 2
ORACLE_EXACT = ("segments", "hits", "finished")


def _camera(width, height, position=(0, 1, -3.5), aperture=0.02):
    return Camera(position=position, rotation=(0, 0, 0), resolution=(width, height), fov=HP, near_far=(1.0e-2, 1.0e3),
                  focal_distance=4.0, aperture=aperture, exposure_time=1.0 / 60.0)


def _materials(world):
    return [world.add(Material((230, 230, 230, 255), 0.0, 1.0, name="white")),
            world.add(Material((255, 255, 255, 255), 0.0, 1.0, emission=20.0, name="light")),
            world.add(Material.mirror())]


def quads(n, width=32, height=8):
    """n quads side by side, facing the camera"""
    world = World()
    mats = _materials(world)
    quad = world.add(generate_plane(4, 0.5, 0.5))
    step = 9.0 / max(n, 2)
    for k in range(n):
        world.add(Instance(quad, [mats[k % 3]], position=((k - (n - 1) / 2) * step, 1, 1.0), rotation=(HP, 0, 0), name=f"quad {k}"))
    world.camera = _camera(width, height)
    return world


def room(width=32, height=8, cube=True, far_instance=False, camera=None, posts=0):
    """a floor, a back wall and two side walls, axis-aligned (the plane lies in xz: no rotation, or quarter turns), a lamp, and a cube
    under a rotation and non-unit scales; `posts` small quads more, to fill the leaf"""
    world = World()
    mats = _materials(world)
    wall = world.add(generate_plane(4, 3.0, 3.0))
    world.add(Instance(wall, [mats[0]], position=(0, -0.5, 1.0), rotation=(0, 0, 0), name="floor"))
    world.add(Instance(wall, [mats[2]], position=(0, 1.0, 2.5), rotation=(HP, 0, 0), name="back"))
    world.add(Instance(wall, [mats[0]], position=(-1.5, 1.0, 1.0), rotation=(0, 0, HP), name="left"))
    world.add(Instance(wall, [mats[0]], position=(1.5, 1.0, 1.0), rotation=(0, 0, -HP), name="right"))
    world.add(Instance(world.add(generate_plane(4, 1.0, 1.0)), [mats[1]], position=(0, 2.4, 1.0), rotation=(math.pi, 0, 0), name="lamp"))
    if cube:
        world.add(Instance(world.add(generate_cube()), [mats[0]], position=(0.3, 0.2, 0.8), rotation=(0.2, 0.5, 0.1), scale=(0.7, 1.3, 0.45), name="cube"))
    for k in range(posts):
        world.add(Instance(world.add(generate_plane(4, 0.4, 0.8)), [mats[2 * (k % 2)]], position=(-0.9 + 0.6 * k, 0.3, 0.4), rotation=(HP, 0.3, 0), name=f"post {k}"))
    if far_instance:
        world.add(Instance(world.add(generate_plane(4, 1.0, 1.0)), [mats[0]], position=(2.0 ** 41, 1.0, 1.0), rotation=(HP, 0, 0), name="far away"))
    world.camera = camera if camera is not None else _camera(width, height)
    return world


def fan(triangles, width=1.0, height=1.0):
    """a polygon of `triangles` triangles"""
    return generate_plane(triangles + 2, width, height)


def repeated_quad(times, width=1.0, height=1.0):
    """the quad's two triangles listed `times` times"""
    quad = generate_plane(4, width, height)
    return Mesh(quad.vertices, np.tile(quad.tri_vertices, (times, 1)), texcrds=quad.texcrds, tri_texcrds=np.tile(quad.tri_texcrds, (times, 1)),
                name="quad listed %d times" % times)


def mixed():
    world = World()
    mats = _materials(world)
    meshes = [fan(1, 1.5, 1.5), fan(2, 1.5, 1.5), fan(3, 1.5, 1.5), fan(5, 1.5, 1.5), fan(9, 1.5, 1.5), fan(12, 1.5, 1.5), fan(17, 1.5, 1.5),
              repeated_quad(2, 1.5, 1.5)]
    for k, mesh in enumerate(meshes):   # staggered in depth and overlapping: a ray visits several of them, nearer ones listed later
        world.add(Instance(world.add(mesh), [mats[1] if k == 0 else mats[0] if k % 2 else mats[2]],
                           position=(-2.4 + 0.7 * k, 1 + 0.15 * (k % 3), 2.5 - 0.3 * k), rotation=(HP + 0.05, 0.1, 0.02 * k), scale=(1.7, 1.0, 0.8),
                           name=f"polygon {k}"))
    world.camera = _camera(32, 8)
    return world


# name -> (world, instances in the world's one leaf)
CASES = {
    "quads_1": lambda: (quads(1), 1), "quads_2": lambda: (quads(2), 2), "quads_8": lambda: (quads(8), 8),
    "flat_and_thick": lambda: (room(), 6),
    "not_fast": lambda: (room(far_instance=True), 7), "not_fast_full_leaf": lambda: (room(far_instance=True, posts=1), 8),
    "down_the_axis": lambda: (room(camera=_camera(32, 8, aperture=0.0)), 6),
    "tiny_origin": lambda: (room(camera=_camera(32, 8, position=(2.0 ** -66, 1, -3.5), aperture=0.0)), 6),
    "tiny_origin_full_leaf": lambda: (room(camera=_camera(32, 8, position=(2.0 ** -66, 1, -3.5), aperture=0.0), posts=2), 8),
    "partial_5x3": lambda: (room(5, 3), 6),
    "mixed": lambda: (mixed(), 8),
}
WITH_ORACLE = ("flat_and_thick",)


def frames(ctx):
    return dict(accum=ctx.read_accum(), depth=ctx.read_depth(), **{"state." + k: v for k, v in ctx.read_state().items()})


@pytest.mark.parametrize("seed", [3, 20271, 0xB0C5E1])
def test_selftest_finds_no_mismatch(seed):
    ctx = Context(0)
    bad, n = ctx.selftest(256, seed)
    ctx.close()
    assert n >= 2 * 1024 * 256 * 256
    assert bad == 0, f"seed {seed}: {bad} mismatches in {n} cases"


@pytest.mark.parametrize("name", list(CASES))
def test_box_sel_equals_the_stack_walk(name):
    world, want_instances = CASES[name]()
    flat, cam = flatten(world), camera_struct(world.camera)
    root = int(flat.nodes[flat.tlas_root]["meta"])
    assert root & _abi.NODE_LEAF and (root & _abi.NODE_COUNT_MASK) == want_instances <= 8
    assert cam.width <= 32 and cam.height <= 8
    extent = max(float(np.abs(flat.instances["bb_min"]).max()), float(np.abs(flat.instances["bb_max"]).max()))
    assert (extent >= 2.0 ** 40) == name.startswith("not_fast")   # what decides the scene's fast_div (hiprz_scene_host.cpp: coord_ok)
    if name == "flat_and_thick":   # flat boxes and a thick one in one leaf
        size = flat.instances["bb_max"] - flat.instances["bb_min"]
        assert (size.min(axis=1) == 0.0).sum() >= 3 and (size.min(axis=1) > 0.1).sum() >= 1
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
    for passes in (1, 3):
        twin.render(passes)
        want = frames(twin)
        for label, ctx in contexts.items():
            ctx.render(passes)
            assert ctx.pipeline() == int(label[-1])
            for key, value in frames(ctx).items():
                assert np.array_equal(value, want[key]), f"{name}, {label}, after render({passes}): {key} differs from the stack walk"
    counted = twin.render_counted(2)
    want = frames(twin)
    for label, ctx in contexts.items():
        got = ctx.render_counted(2)
        for key in counted:
            assert got[key] == counted[key], f"{name}, {label}: counter {key} {got[key]} != {counted[key]} (stack walk)"
        for key, value in frames(ctx).items():
            assert np.array_equal(value, want[key]), f"{name}, {label}, after the counted passes: {key}"
    print(name, "counted:", counted)
    # the scene is what the case is for: every pixel's two segments, rays that hit, boxes beyond the root's
    assert counted["segments"] == 2 * cam.width * cam.height
    assert counted["hits"] > 0 and counted["tri_tests"] > 0 and counted["box_tests"] > counted["segments"]
    if name in WITH_ORACLE:
        ref = oracle.OracleRenderer(flat, cam, cfg)
        ref.render(1), ref.render(3)
        ref_counted = ref.render(2, counted=True)
        print(name, "oracle:", ref_counted)
        for key in ORACLE_EXACT:
            assert counted[key] == ref_counted[key], f"{name}: counter {key} {counted[key]} != {ref_counted[key]} (oracle)"
        for total, shadow in (("box_tests", "shadow_box_tests"), ("tri_tests", "shadow_tri_tests")):
            assert counted[total] - counted[shadow] == ref_counted[total] - ref_counted[shadow], f"{name}: {total} (oracle)"
        ref.close()
    for ctx in list(contexts.values()) + [twin]:
        ctx.close()
