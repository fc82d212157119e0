"""Dealing a leaf's later triangle pairs over the wave's lanes (dealt_visit in hiprz_device.hpp, hiprz_deal_pick.hpp): in a round of the
one-leaf walk that has one lane per visit, a lane that holds a visit of a one-leaf mesh tests pair 0 itself, and the pairs the wave's
visits have left are dealt over all 64 lanes when they fit one trip and some visit has three or more left (deal_taken); a wave takes
that path when it holds 1 to 21 visits of meshes of one leaf above 4 triangles.

Every case goes through test_packed_pairs_gpu.compare_with_the_stack_walk: the default traversal on pipelines 2, 0 and 1 against a twin
on the LDS-stack walk, accumulator, depth and path state bit for bit after render(1) and render(3), every counter after
render_counted(2), and the CPU oracle's exact fields.  A tile is 32x8 pixels, four waves of 8x8; a round falls back to one lane per
visit when the octets of its wide visits (meshes of one leaf above 4 triangles) do not fit the tile's 256 lanes, i.e. above 32 of them
less the narrow visits.  The scenes, with what the CPU oracle's first hits say of them (asserted below before anything runs on the
GPU; "cube pixels" = pixels whose first hit is a mesh of more than two pairs):

  cube_small       one cube among seven quads over the whole tile, small on screen: 4 cube pixels, all in one 8x8 block — a few owners
                   in a wave of quad visits, one dealt trip (T = 20)
  cube_column      the cube stretched over one pixel column: 8 cube pixels in one block, T = 40, one trip with every owner's five pairs
                   on neighbouring lanes
  cube_columns     over two to three pixel columns: 16 to 24 cube pixels in one block, T = 80 to 120: more than one trip, the decline path
  cubes_8          test_flat_walk_gpu's eight cubes over the whole tile: every lane a cube visit, T = 320, the decline path
  fans             fans of 3, 9, 16 and 25 triangles beside a wall-sized fan of 9 that forces the fallback: non-uniform rem (1, 4, 7
                   and 12 pairs left), odd leaves, has_b
  fans_big         the four fans large on screen: waves full of owners, declined, and the waves at the seams between two bins
  twice            repeated_quad(4) and repeated_quad(5) beside the wall-sized fan of 9: coinciding triangles, so equal distances found by
                   different lanes — the first in leaf order must win
  partial_5x3,     a cube and quads in a frame of 5x3 pixels and of one pixel: helpers that carry no pixel, rounds with fewer items
  partial_1x1      than lanes (and with at most 15 visits no fallback round: the octet path, which must be as it was)
  slabs_cubes      cubes with a rotation and non-unit scales behind test_flat_walk_gpu's kind of slabs: the near end moves by a rounding
                   and the boxes are tested again (the slabs hide the cubes from the first hits: no pixel count is asked)
  nine             nine instances, a cube among them: a world tree with inner nodes, the general binned walk, which must be unaffected

Which path a wave took cannot be seen from here; the phase counters of a -DRZ_PHASE_STATS build on these scenes are in
profiles/r28/phase_test_scenes.txt, to be read again with such a build if a scene is changed.
"""
import math

import numpy as np
import pytest

import oracle
from rayzath_amd import _abi
from rayzath_amd.engine import RenderConfig, Tracing
from rayzath_amd.scene import Camera, Instance, Material, World, camera_struct, flatten, generate_cube, generate_plane
from test_flat_walk_gpu import cubes
from test_packed_pairs_gpu import compare_with_the_stack_walk, fan, repeated_quad

pytestmark = pytest.mark.gpu

HP = math.pi / 2


def _camera(width, height):
    return Camera(position=(0, 1, -3.5), rotation=(0, 0, 0), resolution=(width, height), fov=HP, near_far=(1.0e-2, 1.0e3),
                  focal_distance=4.0, aperture=0.02, exposure_time=1.0 / 60.0)


def _materials(world):
    return [world.add(Material((230, 230, 230, 255), 0.0, 1.0, name="white")),
            world.add(Material((255, 255, 255, 255), 0.0, 1.0, emission=20.0, name="light")),
            world.add(Material.mirror())]


def cube_among_quads(cube_scale, n_quads=7, width=32, height=8, cube_x=-1.3):
    """a wall of quads over the whole frame and one cube in front of it, listed first"""
    world = World()
    mats = _materials(world)
    world.add(Instance(world.add(generate_cube()), [mats[2]], position=(cube_x, 1, 0.0), rotation=(0, 0.3, 0), scale=cube_scale, name="cube"))
    quad = world.add(generate_plane(4, 4.8 / n_quads, 3.0))
    for k in range(n_quads):
        world.add(Instance(quad, [mats[k % 2]], position=((k - (n_quads - 1) / 2) * 4.8 / n_quads, 1, 1.0), rotation=(HP, 0, 0), name=f"quad {k}"))
    world.camera = _camera(width, height)
    return world


def beside_a_wall_of_nine(meshes, sizes):
    """a fan of 9 triangles over the left of the tile (above 32 wide visits: every first round is on the fallback), a quad wall, and the
    small meshes in front of the wall, listed behind it"""
    world = World()
    mats = _materials(world)
    world.add(Instance(world.add(fan(9, 1.6, 3.0)), [mats[0]], position=(-1.5, 1, 1.0), rotation=(HP, 0, 0), name="wall of nine"))
    world.add(Instance(world.add(generate_plane(4, 3.2, 3.0)), [mats[1]], position=(0.9, 1, 1.0), rotation=(HP, 0, 0), name="quad wall"))
    for k, (mesh, size) in enumerate(zip(meshes, sizes)):
        world.add(Instance(world.add(mesh), [mats[2 - k % 2]], position=(-0.4 + 0.6 * k, 1 + 0.05 * k, 0.4), rotation=(HP, 0, 0), scale=(size, 1.0, size),
                           name=f"small {k}"))
    world.camera = _camera(32, 8)
    return world


def fans_big():
    world = World()
    mats = _materials(world)
    for k, n in enumerate((3, 9, 16, 25)):
        world.add(Instance(world.add(fan(n, 1.0, 2.6)), [mats[k % 3]], position=((k - 1.5) * 1.1, 1, 1.0), rotation=(HP, 0, 0), name=f"fan {n}"))
    world.camera = _camera(32, 8)
    return world


def slabs_cubes():
    world = World()
    mats = _materials(world)
    quad = world.add(generate_plane(4, 1.0, 1.0))
    for k in range(5, -1, -1):   # far to near, staggered: the columns of the frame look through different sets
        world.add(Instance(quad, [mats[0] if k % 2 else mats[2]], position=(-1.2 + 0.45 * k, 1, -1.0 + 0.45 * k), rotation=(HP + 0.05, 0.1, 0),
                           scale=(1.7, 1.0, 0.6), name=f"slab {k}"))
    cube = world.add(generate_cube())
    for k in range(2):
        world.add(Instance(cube, [mats[1 + k]], position=(-0.7 + 1.4 * k, 1.1, 2.2), rotation=(0.2, 0.4 + k, 0.1), scale=(0.5 + 0.9 * k, 1.7, 0.6),
                           name=f"cube {k}"))
    world.camera = _camera(32, 8)
    return world


def nine():
    return cube_among_quads((0.2, 0.2, 0.2), n_quads=8)


# name: (scene, least and most pixels of one 8x8 block whose first hit is a mesh of more than two pairs — the fullest block)
CASES = {
    "cube_small": (lambda: cube_among_quads((0.2, 0.2, 0.2)), 1, 12),
    "cube_column": (lambda: cube_among_quads((0.08, 4.0, 0.08)), 6, 12),
    "cube_columns": (lambda: cube_among_quads((0.2, 4.0, 0.1)), 13, 25),
    "cubes_8": (lambda: cubes(False), 64, 64),
    "fans": (lambda: beside_a_wall_of_nine([fan(3), fan(9), fan(16), fan(25)], [0.4, 0.25, 0.25, 0.25]), 26, 64),
    "fans_big": (fans_big, 26, 64),
    "twice": (lambda: beside_a_wall_of_nine([repeated_quad(4), repeated_quad(5), repeated_quad(4)], [0.35, 0.3, 0.55]), 26, 64),
    "partial_5x3": (lambda: cube_among_quads((1.5, 1.0, 0.5), width=5, height=3, cube_x=-1.0), 1, 15),
    "partial_1x1": (lambda: cube_among_quads((1.5, 1.0, 0.5), width=1, height=1, cube_x=0.0), 1, 1),
    "slabs_cubes": (slabs_cubes, 0, 64),
    "nine": (nine, 1, 12),
}


def multi_pair_pixels_per_block(flat, cam):
    """per 8x8 block: the pixels whose first hit (CPU oracle) is an instance whose mesh root is a leaf of more than 4 triangles"""
    long_leaf = []
    for inst in flat.instances:
        meta = int(flat.nodes[int(inst["blas_root"])]["meta"])
        long_leaf.append(bool(meta & _abi.NODE_LEAF) and (meta & _abi.NODE_COUNT_MASK) > 4)
    hits = oracle.first_hits(flat, cam)
    inst = hits["instance"].astype(np.int64)
    on = np.zeros(inst.shape, bool)
    for k, is_long in enumerate(long_leaf):
        if is_long:
            on |= (inst == k) & (hits["triangle"] >= 0)
    out = []
    for y in range(0, cam.height, 8):
        for x in range(0, cam.width, 8):
            out.append(int(on[y:y + 8, x:x + 8].sum()))
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_dealt_pairs_equal_the_stack_walk_and_the_oracle(name):
    build, least, most = CASES[name]
    world = build()
    flat, cam = flatten(world), camera_struct(world.camera)
    root = int(flat.nodes[flat.tlas_root]["meta"])
    assert bool(root & _abi.NODE_LEAF) == (name != "nine")
    blocks = multi_pair_pixels_per_block(flat, cam)
    print(name, "pixels per 8x8 block whose first hit is a leaf of more than two pairs:", blocks)
    assert least <= max(blocks) <= most, f"{name}: the scene is not what the case is for: {blocks}"
    compare_with_the_stack_walk(name, flat, cam, RenderConfig(tracing=Tracing(6, 8)).struct())
