"""The packed form of the one-leaf walk (closest_hit_flat, MODE 4): the triangles of a leaf tested two at a time (tri_hit2,
tri_pair_step, hiprz_pair_pick.hpp), behind box tests that stay one float per lane (box_range_unpacked).

Self-test: ctx.selftest(256, seed) for three seeds.  Its kernel compares the pair loop with the one-by-one loop on random and
adversarial triangle pairs (identical triangles, |det| < 1e-7, an origin in the triangle's plane, t on the near or the far end): far end,
winner, b1, b2 and the facing bit.  Every mismatch lands in the one counter, which must be zero.  (That comparison is not added to the
kernel's count of cases: tests/test_parity_gpu.py bounds that count by what the quotient and filtered-box cases alone give.)

Scenes, by the method of tests/test_flat_walk_gpu.py: the default traversal on pipelines 2, 0 and 1 against a twin on the LDS-stack walk
(set_traversal_mode(1)), which tests triangles one by one.  After render(1) and render(3): accumulator, first-hit depth and path state
equal the twin's bit for bit; then render_counted(2): every counter equals the twin's, and segments, hits, finished and the box and
triangle tests net of shadow tests equal the CPU oracle's.  The worlds are one leaf; every mesh is one leaf of a chosen triangle count
(asserted on the flattened scene): an n-gon of generate_plane has n - 2 triangles, the host builder keeps up to 32 in a root leaf.

  1, 2, 3, 4     one lane per visit: a lone triangle, one pair, a pair and a lone one, two pairs
  5, 8, 9        eight lanes per visit: no lane holds a pair (5, 8), lane 0 alone does (9)
  12, 16         four lanes and all eight hold a pair
  17, 25, 32     a second iteration in steps of 16, with a lone triangle (17), with pairs in lane 0 alone and lone ones elsewhere (25), full
  twice          a mesh that lists the same quad twice: triangles 2 and 3 coincide with 0 and 1, every hit is a tie of two distances and
                 the first in leaf order must win, within a pair (4 triangles, one lane) and across lanes and pairs (the quad four times
                 over: 8 triangles on eight lanes; five times: 10 triangles, lanes 0 and 1 hold pairs of coinciding triangles)
  mixed          eight such meshes (1, 2, 3, 5, 9, 12, 17 triangles and the doubled quad) under a rotation and non-unit scales over the whole
                 tile: meant to move the near end by a rounding (the instance boxes are then tested again) and to have more wide visits
                 than fit the workgroup, so that the one-lane-per-visit fallback runs the pair loop over 5 to 17 triangles.  The test
                 cannot see which path ran (the library has no counter for it); the phase counters of a -DRZ_PHASE_STATS build on
                 this scene are in profiles/r13/phase_stats_test_scenes.txt (60 of 80 rounds on the fallback, 245 pair iterations) —
                 to be read again with such a build if the scene is changed.  The re-test has no counter at all.
  partial        one partial tile, 5x3 pixels
"""
import math

import numpy as np
import pytest

import oracle
from rayzath_amd import _abi
from rayzath_amd.engine import Context, RenderConfig, Tracing
from rayzath_amd.scene import Camera, Instance, Material, Mesh, World, camera_struct, flatten, generate_plane

pytestmark = pytest.mark.gpu

HP = math.pi / 2
ORACLE_EXACT = ("segments", "hits", "finished")
COUNTS = (1, 2, 3, 4, 5, 8, 9, 12, 16, 17, 25, 32)


def _camera(width, height):
    return Camera(position=(0, 1, -3.5), rotation=(0, 0, 0), resolution=(width, height), fov=HP, near_far=(1.0e-2, 1.0e3),
                  focal_distance=4.0, aperture=0.02, exposure_time=1.0 / 60.0)


def _materials(world):
    return [world.add(Material((230, 230, 230, 255), 0.0, 1.0, name="white")),
            world.add(Material((255, 255, 255, 255), 0.0, 1.0, emission=20.0, name="light")),
            world.add(Material.mirror())]


def fan(triangles, width=1.0, height=1.0):
    """a polygon of `triangles` triangles"""
    return generate_plane(triangles + 2, width, height)


def repeated_quad(times, width=1.0, height=1.0):
    """the quad's two triangles listed `times` times: triangles 2k and 2k + 1 coincide with 0 and 1"""
    quad = generate_plane(4, width, height)
    return Mesh(quad.vertices, np.tile(quad.tri_vertices, (times, 1)), texcrds=quad.texcrds, tri_texcrds=np.tile(quad.tri_texcrds, (times, 1)),
                name="quad listed %d times" % times)


def polygons(meshes, width, height):
    """the meshes side by side, facing the camera, a mirror and an emitter among them so that paths go on"""
    world = World()
    mats = _materials(world)
    n = len(meshes)
    for k, mesh in enumerate(meshes):
        world.add(Instance(world.add(mesh), [mats[k % 3]], position=((k - (n - 1) / 2) * 2.2, 1, 1.0), rotation=(HP, 0, 0), name=f"polygon {k}"))
    world.camera = _camera(width, height)
    return world


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
    return world, [1, 2, 3, 5, 9, 12, 17, 4]


CASES = {f"fan_{n}": (lambda n=n: (polygons([fan(n), fan(n, 0.8, 1.1)], 32, 8), [n, n])) for n in COUNTS}
CASES["fans_64x16"] = lambda: (polygons([fan(2), fan(3), fan(9), fan(16), fan(25), fan(32)], 64, 16), [2, 3, 9, 16, 25, 32])
CASES["twice_pair"] = lambda: (polygons([repeated_quad(2), repeated_quad(1)], 32, 8), [4, 2])
CASES["twice_octet"] = lambda: (polygons([repeated_quad(4), repeated_quad(5)], 32, 8), [8, 10])
CASES["mixed"] = mixed
CASES["partial_5x3"] = lambda: (polygons([fan(3), fan(12)], 5, 3), [3, 12])


def leaf_counts(flat):
    """triangle count of every instance's mesh root, which must be a leaf"""
    out = []
    for inst in flat.instances:
        meta = int(flat.nodes[int(inst["blas_root"])]["meta"])
        assert meta & _abi.NODE_LEAF, "the mesh root is not a leaf"
        out.append(meta & _abi.NODE_COUNT_MASK)
    return out


def frames(ctx):
    return dict(accum=ctx.read_accum(), depth=ctx.read_depth(), **{"state." + k: v for k, v in ctx.read_state().items()})


@pytest.mark.parametrize("seed", [1, 20261, 0xC0FFEE])
def test_selftest_finds_no_mismatch(seed):
    ctx = Context(0)
    bad, n = ctx.selftest(256, seed)
    ctx.close()
    assert n >= 2 * 1024 * 256 * 256
    assert bad == 0, f"seed {seed}: {bad} mismatches in {n} cases"


@pytest.mark.parametrize("name", list(CASES))
def test_pairs_equal_the_stack_walk_and_the_oracle(name):
    world, want_counts = CASES[name]()
    flat, cam = flatten(world), camera_struct(world.camera)
    root = int(flat.nodes[flat.tlas_root]["meta"])
    assert root & _abi.NODE_LEAF and (root & _abi.NODE_COUNT_MASK) == len(want_counts) <= 8
    assert sorted(leaf_counts(flat)) == sorted(want_counts)
    compare_with_the_stack_walk(name, flat, cam, RenderConfig(tracing=Tracing(6, 8)).struct())


def compare_with_the_stack_walk(name, flat, cam, cfg):
    """the comparison of this file on one uploaded scene (tests/test_tree_shapes_gpu.py runs it on meshes of one leaf above 32 triangles)"""
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
    ref = oracle.OracleRenderer(flat, cam, cfg)
    ref.render(1), ref.render(3)
    ref_counted = ref.render(2, counted=True)
    print(name, "counted:", counted, "oracle:", ref_counted)
    for key in ORACLE_EXACT:
        assert counted[key] == ref_counted[key], f"{name}: counter {key} {counted[key]} != {ref_counted[key]} (oracle)"
    for total, shadow in (("box_tests", "shadow_box_tests"), ("tri_tests", "shadow_tri_tests")):
        assert counted[total] - counted[shadow] == ref_counted[total] - ref_counted[shadow], f"{name}: {total} (oracle)"
    # the scene is what the case is for: rays hit the polygons and test their triangles
    assert counted["segments"] == 2 * cam.width * cam.height
    assert counted["hits"] > 0 and counted["tri_tests"] > 0
    for ctx in list(contexts.values()) + [twin]:
        ctx.close()
    ref.close()
